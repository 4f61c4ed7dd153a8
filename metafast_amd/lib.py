"""ctypes binding of libmetafast_hip.so (the C-ABI in include/metafast_hip.h).

This is the host-side mirror of the reference's seams for the hot path
(IOUtils.loadReads / printKmers / loadKmers, SequencesFinders.thresholdStrategy,
ComponentsBuilder.splitStrategy, FeaturesCalculatorMain.buildAndPrintVector,
DistanceMatrixCalculatorMain.brayCurtisDistance).  There is no CPU fallback: if the
HIP library is missing or no GPU is present, calls fail loudly.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("METAFAST_HIP_LIB") or os.path.join(_HERE, "lib", "libmetafast_hip.so")     # (override: A/B runs of two builds)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "metafast_hip.h")
_lib = None

u64, i64, i32, vp, cp = C.c_uint64, C.c_int64, C.c_int, C.c_void_p, C.c_char_p
pu64, pvp = C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)

_SIGS = {
    "mf_last_error": (cp, []),
    "mf_version": (cp, []),
    "mf_ctx_create": (i32, [i32, i32, pvp]),
    "mf_ctx_destroy": (None, [vp]),
    "mf_ctx_set_stream": (i32, [vp, vp]),
    "mf_ctx_set_option": (i32, [vp, cp, i64]),
    "mf_ctx_synchronize": (i32, [vp]),
    "mf_ctx_trim": (i32, [vp]),
    "mf_ctx_trim_bytes": (i32, [vp, u64, C.POINTER(C.c_uint64)]),
    "mf_ctx_kernel_time": (i64, [vp, cp, C.POINTER(C.c_double)]),
    "mf_ctx_kernel_report": (i32, [vp, cp, u64]),
    "mf_ctx_reset_timers": (i32, [vp]),
    "mf_count_reads": (i32, [vp, C.POINTER(cp), i32, i32, i32, pvp]),
    "mf_table_drop_index": (i32, [vp]),
    "mf_count_wide_device": (i32, [vp, vp, vp, u64, u64, i32, i32, pvp]),
    "mf_wtable_destroy": (None, [vp]),
    "mf_wtable_stats": (i32, [vp, pu64, pu64, C.POINTER(C.c_int)]),
    "mf_wtable_export": (i32, [vp, vp, vp, vp, u64, pu64]),
    "mf_wtable_pieces": (i32, [vp, C.POINTER(C.c_uint32)]),
    "mf_wtable_piece_view": (i32, [vp, C.c_uint32, pvp, pvp, pvp, pu64]),
    "mf_count_wide_device_above": (i32, [vp, vp, vp, u64, u64, i32, i32, i32, pvp, pu64]),
    "mf_wtable_filter": (i32, [vp, i32, pvp]),
    "mf_wtable_drop_index": (i32, [vp]),
    "mf_wtable_lookup": (i32, [vp, vp, vp, u64, vp]),
    "mf_build_unitigs_wide_device": (i32, [vp, vp, i32, i32, pvp]),
    "mf_cut_components_wide_device": (i32, [vp, vp, i32, i32, pvp]),
    "mf_wcomps_destroy": (None, [vp]),
    "mf_wcomps_stats": (i32, [vp, pu64, pu64]),
    "mf_wcomps_export": (i32, [vp, vp, vp, vp, vp, vp, vp]),
    "mf_features_wide_device": (i32, [vp, vp, vp, i32, vp, vp]),
    "mf_count_reads_wide": (i32, [vp, C.POINTER(cp), i32, i32, i32, pvp]),
    "mf_wtable_write_kmers": (i32, [vp, i32, cp, cp, pu64]),
    "mf_wtable_load_kmers": (i32, [vp, C.POINTER(cp), i32, i32, i32, pvp]),
    "mf_wtable_write_kmers_filtered": (i32, [vp, i32, vp, i32, cp, pu64]),
    "mf_unique_kmers_multi_wide_tables": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp, C.POINTER(C.c_int), pu64, vp]),
    "mf_unique_kmers_multi_wide": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, i32, i32, cp, C.POINTER(C.c_int), pu64, vp]),
    "mf_kmers_per_sample_wide_tables": (i32, [vp, vp, i32, i32, i32, i32, pvp]),
    "mf_kmers_per_sample_wide": (i32, [vp, C.POINTER(cp), i32, i32, i32, i32, cp, pu64]),
    "mf_stats_kmers_wide_tables": (i32, [vp, vp, i32, vp, i32, i32, C.c_double, C.c_double, pvp, pvp, pvp, vp]),
    "mf_stats_kmers_wide": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, C.c_double, C.c_double, cp, vp]),
    "mf_kmers_samples_count_wide_tables": (i32, [vp, vp, i32, i32, pvp]),
    "mf_kmers_samples_count_wide": (i32, [vp, C.POINTER(cp), i32, i32, i32, cp, cp, pu64]),
    "mf_stats_kmers3_wide_tables": (i32, [vp, vp, i32, vp, i32, vp, i32, i32, C.c_double, C.c_double, pvp, pvp, pvp, pvp, vp]),
    "mf_stats_kmers3_wide": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, C.c_double, C.c_double, cp, vp]),
    "mf_kmers_grouped_count_wide_tables": (i32, [vp, vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, u64, pu64]),
    "mf_kmers_grouped_count_wide": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, cp, pu64]),
    "mf_kps_device_view_wide": (i32, [vp, pvp, pvp, pvp, pvp]),
    "mf_kps_export_wide": (i32, [vp, vp, vp, vp, vp]),
    "mf_wcomps_write": (i32, [vp, cp, cp]),
    "mf_wcomps_load": (i32, [vp, cp, i32, pvp]),
    "mf_features_wide": (i32, [vp, cp, cp, i32, i32, cp, cp]),
    "mf_features_wide_device_selected": (i32, [vp, vp, vp, vp, i32, vp, vp]),
    "mf_features_reads_wide_device": (i32, [vp, vp, vp, vp, u64, u64, i32, vp, vp]),
    "mf_features_reads_wide_device_selected": (i32, [vp, vp, vp, vp, u64, u64, vp, i32, vp, vp]),
    "mf_features_wide_selected": (i32, [vp, cp, cp, i32, i32, vp, cp, cp]),
    "mf_features_reads_wide": (i32, [vp, cp, C.POINTER(cp), i32, i32, i32, cp, cp]),
    "mf_features_reads_wide_selected": (i32, [vp, cp, C.POINTER(cp), i32, i32, i32, vp, cp, cp]),
    "mf_wcomps_unitigs_device": (i32, [vp, vp, i32, pvp]),
    "mf_comp2seq_wide": (i32, [vp, cp, i32, i32, cp, pu64, pu64]),
    "mf_wcomps_graph_device": (i32, [vp, vp, vp, i32, i32, pvp]),
    "mf_wcomps_from_sequences_device": (i32, [vp, vp, vp, u64, u64, i32, pvp]),
    "mf_seq2comp_wide": (i32, [vp, C.POINTER(cp), i32, i32, cp, cp, pu64, vp]),
    "mf_comp2graph_wide": (i32, [vp, cp, i32, C.POINTER(cp), i32, i32, cp, pu64, pu64, pu64]),
    "mf_comm_create_local": (i32, [vp, i32, vp]),
    "mf_comm_rccl_id": (i32, [vp]),
    "mf_comm_create_rccl": (i32, [vp, vp, i32, i32, pvp]),
    "mf_comm_create_external": (i32, [vp, i32, i32, vp, vp, pvp]),
    "mf_comm_destroy": (None, [vp]),
    "mf_comm_rank": (i32, [vp]),
    "mf_comm_world": (i32, [vp]),
    "mf_comm_kind": (cp, [vp]),
    "mf_comm_stat": (i64, [vp, cp]),
    "mf_comm_reset_stats": (i32, [vp]),
    "mf_comm_gather_ints": (i32, [vp, vp, i32, vp]),
    "mf_comm_all_gather": (i32, [vp, vp, vp, vp]),
    "mf_comm_all_to_all": (i32, [vp, vp, vp, vp, vp]),
    "mf_comm_gather_sequences": (i32, [vp, vp, vp, u64, u64, pvp]),
    "mf_cut_components_sharded": (i32, [vp, vp, vp, u64, u64, i32, i32, i32, i32, pvp]),
    "mf_cut_components_sharded_files": (i32, [vp, C.POINTER(cp), i32, i32, i32, i32, i32, cp, cp, pu64]),
    "mf_cut_components_of_shard": (i32, [vp, vp, i32, i32, i32, pvp, vp]),
    "mf_features_allgather": (i32, [vp, vp, u64, u64, vp, u64, pu64]),
    "mf_count_reads_above": (i32, [vp, C.POINTER(cp), i32, i32, i32, i32, pvp, pu64]),
    "mf_count_device": (i32, [vp, vp, vp, u64, u64, i32, i32, pvp]),
    "mf_count_device_above": (i32, [vp, vp, vp, u64, u64, i32, i32, i32, pvp, pu64]),
    "mf_table_destroy": (None, [vp]),
    "mf_table_stats": (i32, [vp, pu64, pu64]),
    "mf_table_occurrences": (i32, [vp, pu64]),
    "mf_table_records": (i32, [vp, pu64, C.POINTER(i32)]),
    "mf_table_hist": (i32, [vp, vp]),
    "mf_table_export": (i32, [vp, i32, vp, vp, u64, pu64]),
    "mf_table_device_view": (i32, [vp, pvp, pvp, pu64]),
    "mf_table_lookup": (i32, [vp, vp, u64, vp]),
    "mf_table_write_kmers": (i32, [vp, i32, cp, cp, pu64]),
    "mf_table_write_kmers_filtered": (i32, [vp, i32, vp, i32, cp, pu64]),
    "mf_table_load_kmers": (i32, [vp, C.POINTER(cp), i32, i32, i32, pvp]),
    "mf_table_filter": (i32, [vp, i32, pvp]),
    "mf_table_from_host": (i32, [vp, vp, vp, u64, i32, pvp]),
    "mf_count_device_shard": (i32, [vp, vp, vp, u64, u64, i32, i32, i32, i32, pvp]),
    "mf_dcc_create": (i32, [vp, vp, i32, i32, vp, pvp]),
    "mf_dcc_destroy": (None, [vp]),
    "mf_dcc_queries": (i32, [vp, vp]),
    "mf_dcc_queries_fill": (i32, [vp, vp]),
    "mf_dcc_answer": (i32, [vp, vp, u64, vp]),
    "mf_dcc_set_answers": (i32, [vp, vp, u64]),
    "mf_dcc_level_local": (i32, [vp, vp]),
    "mf_dcc_pairs_fill": (i32, [vp, vp]),
    "mf_dcc_pairs_complete": (i32, [vp, vp, u64]),
    "mf_dcc_merge": (i32, [vp, vp, u64, pu64]),
    "mf_dcc_stats_fill": (i32, [vp, vp]),
    "mf_dcc_classify": (i32, [vp, vp, u64, vp, u64, u64, i32, i32, i32, pu64, pu64]),
    "mf_dcc_world": (i32, [vp]),
    "mf_dcc_members_grouped": (i32, [vp, pu64, pu64]),
    "mf_dcc_members_grouped_fill": (i32, [vp, vp, vp]),
    "mf_dcc_finish_grouped": (i32, [vp, vp, u64, vp, u64, vp, vp, vp, vp, vp, u64, pvp]),
    "mf_dcc_kept_fill": (i32, [vp, vp]),
    "mf_dcc_members": (i32, [vp, pu64]),
    "mf_dcc_members_fill": (i32, [vp, vp, vp]),
    "mf_dcc_minkeys": (i32, [vp, vp, u64, vp]),
    "mf_dcc_finish": (i32, [vp, vp, vp, u64, vp, vp, vp, vp, vp, u64, pvp]),
    "mf_build_unitigs_device": (i32, [vp, vp, i32, i32, pvp]),
    "mf_seqs_destroy": (None, [vp]),
    "mf_seqs_stats": (i32, [vp, pu64, pu64]),
    "mf_seqs_device_view": (i32, [vp, pvp, pvp, pvp, pvp, pvp, pu64, pu64]),
    "mf_seqs_export": (i32, [vp, vp, vp, vp, vp, vp]),
    "mf_seqs_write_fasta": (i32, [vp, cp]),
    "mf_build_unitigs": (i32, [vp, vp, i32, i32, i32, cp, cp, pu64]),
    "mf_cut_components_device": (i32, [vp, vp, i32, i32, pvp]),
    "mf_comps_destroy": (None, [vp]),
    "mf_comps_stats": (i32, [vp, pu64, pu64]),
    "mf_comps_export": (i32, [vp, vp, vp, vp, vp, vp]),
    "mf_comps_write": (i32, [vp, cp, cp]),
    "mf_comps_load": (i32, [vp, cp, pvp]),
    "mf_cut_components": (i32, [vp, vp, i32, i32, i32, cp, cp, pu64]),
    "mf_comps_set_k": (i32, [vp, i32]),
    "mf_comps_unitigs_device": (i32, [vp, vp, i32, pvp]),
    "mf_seqs_components": (i32, [vp, vp, u64, pu64]),
    "mf_comp2seq": (i32, [vp, cp, i32, i32, cp, pu64, pu64]),
    "mf_comps_graph_device": (i32, [vp, vp, vp, i32, i32, pvp]),
    "mf_gfa_destroy": (None, [vp]),
    "mf_gfa_stats": (i32, [vp, pu64, pu64, pu64, pu64]),
    "mf_gfa_text": (i32, [vp, vp, u64, pu64]),
    "mf_comp2graph": (i32, [vp, cp, i32, C.POINTER(cp), i32, i32, cp, pu64, pu64, pu64]),
    "mf_comps_from_sequences_device": (i32, [vp, vp, vp, u64, u64, i32, pvp]),
    "mf_seq2comp": (i32, [vp, C.POINTER(cp), i32, i32, cp, cp, pu64, vp]),
    "mf_paths_create": (i32, [vp, vp, vp, u64, i32, u64, pvp]),
    "mf_paths_add": (i32, [vp, vp, vp, u64, u64]),
    "mf_paths_finish": (i32, [vp]),
    "mf_paths_destroy": (None, [vp]),
    "mf_paths_stats": (i32, [vp, pu64, pu64, pu64, pu64]),
    "mf_paths_slots": (i32, [vp, vp, vp, vp, vp]),
    "mf_paths_text": (i32, [vp, i64, vp, u64, pu64]),
    "mf_paths_write": (i32, [vp, cp, pu64]),
    "mf_component_paths": (i32, [vp, cp, i32, C.POINTER(cp), i32, vp, u64, i32, u64, cp, pu64, pu64]),
    "mf_paths_create_wide": (i32, [vp, vp, vp, u64, i32, u64, pvp]),
    "mf_component_paths_wide": (i32, [vp, cp, i32, C.POINTER(cp), i32, vp, u64, i32, u64, cp, pu64, pu64]),
    "mf_features_device": (i32, [vp, vp, vp, i32, vp, vp]),
    "mf_features_reads_device": (i32, [vp, vp, vp, vp, u64, u64, i32, i32, vp, vp]),
    "mf_features_reads": (i32, [vp, cp, C.POINTER(cp), i32, i32, i32, cp, cp]),
    "mf_features": (i32, [vp, cp, cp, i32, i32, cp, cp]),
    "mf_features_device_selected": (i32, [vp, vp, vp, vp, i32, vp, vp]),
    "mf_features_selected": (i32, [vp, cp, cp, i32, i32, vp, cp, cp]),
    "mf_features_reads_device_selected": (i32, [vp, vp, vp, vp, u64, u64, i32, vp, i32, vp, vp]),
    "mf_features_reads_selected": (i32, [vp, cp, C.POINTER(cp), i32, i32, i32, vp, cp, cp]),
    "mf_bray_curtis": (i32, [vp, i32, i32, vp]),
    "mf_reads_load": (i32, [vp, C.POINTER(cp), i32, pvp]),
    "mf_reads_destroy": (None, [vp]),
    "mf_reads_stats": (i32, [vp, pu64, pu64]),
    "mf_reads_device_view": (i32, [vp, pvp, pvp]),
    "mf_reads_export": (i32, [vp, vp, vp]),
    "mf_ctx_stat": (i64, [vp, cp]),
    "mf_device_count": (i32, []),
    "mf_device_memory": (i32, [i32, pu64]),
    "mf_ctx_device": (i32, [vp]),
    "mf_ctx_bind_thread": (i32, [vp]),
    "mf_synth_reads_device": (i32, [vp, u64, i32, u64, u64, i32, u64, vp, vp]),
    "mf_synth_reads_host": (i32, [u64, i32, u64, u64, i32, u64, vp, vp]),
    "mf_synth_reads_device_ex": (i32, [vp, u64, i32, u64, u64, i32, u64, i32, vp, vp]),
    "mf_synth_reads_host_ex": (i32, [u64, i32, u64, u64, i32, u64, i32, vp, vp]),
    "mf_stats_kmers_tables": (i32, [vp, vp, i32, vp, i32, i32, C.c_double, C.c_double, pvp, pvp, pvp, vp]),
    "mf_stats_kmers": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, C.c_double, C.c_double, cp, vp]),
    "mf_kmers_samples_count_tables": (i32, [vp, vp, i32, i32, pvp]),
    "mf_kmers_samples_count": (i32, [vp, C.POINTER(cp), i32, i32, i32, cp, cp, pu64]),
    "mf_stats_kmers3_tables": (i32, [vp, vp, i32, vp, i32, vp, i32, i32, C.c_double, C.c_double, pvp, pvp, pvp, pvp, vp]),
    "mf_stats_kmers3": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, C.c_double, C.c_double, cp, vp]),
    "mf_specific_kmers_tables": (i32, [vp, vp, i32, vp, i32, C.c_double, C.c_double, pvp, pvp, vp]),
    "mf_specific_kmers": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.c_double, C.c_double, cp, vp]),
    "mf_specific_kmers3_tables": (i32, [vp, vp, i32, vp, i32, vp, i32, C.c_double, C.c_double, pvp, pvp, pvp, vp]),
    "mf_specific_kmers3": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, C.c_double, C.c_double, cp, vp]),
    "mf_unique_kmers_tables": (i32, [vp, vp, i32, vp, i32, i32, pvp, pu64]),
    "mf_unique_kmers": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, cp, cp, pu64, pu64]),
    "mf_kmers_grouped_count_tables": (i32, [vp, vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, u64, pu64]),
    "mf_kmers_grouped_count": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, cp, pu64]),
    "mf_kmers_per_sample_tables": (i32, [vp, vp, i32, i32, i32, i32, pvp]),
    "mf_kps_destroy": (None, [vp]),
    "mf_kps_stats": (i32, [vp, pu64, C.POINTER(C.c_int)]),
    "mf_kps_device_view": (i32, [vp, pvp, pvp, pvp]),
    "mf_kps_export": (i32, [vp, vp, vp, vp]),
    "mf_kps_header_text": (i32, [vp, i32, vp, u64, pu64]),
    "mf_kps_row_text": (i32, [vp, i32, vp, u64, pu64]),
    "mf_kmers_per_sample": (i32, [vp, C.POINTER(cp), i32, i32, i32, i32, cp, pu64]),
    "mf_unique_kmers_multi_tables": (i32, [vp, vp, i32, vp, i32, i32, i32, i32, vp, C.POINTER(C.c_int), pu64, vp]),
    "mf_unique_kmers_multi": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32, i32, i32, cp, C.POINTER(C.c_int), pu64, vp]),
    "mf_kmers_multiple_filters_tables": (i32, [vp, vp, vp, vp, vp, i32, pvp, vp, vp, u64, pu64, vp]),
    "mf_kmers_multiple_filters": (i32, [vp, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, C.POINTER(cp), i32, i32, i32,
                                        C.POINTER(cp), C.POINTER(cp), vp]),
    "mf_ctable_from_host": (i32, [vp, vp, vp, u64, i32, pvp]),
    "mf_ctable_load": (i32, [vp, C.POINTER(cp), i32, i64, i32, pvp]),
    "mf_ctable_stats": (i32, [vp, pu64, C.POINTER(C.c_int)]),
    "mf_ctable_export": (i32, [vp, vp, vp, u64, pu64]),
    "mf_ctable_write": (i32, [vp, cp, cp, pu64]),
    "mf_ctable_destroy": (None, [vp]),
    "mf_kmers_color_tables": (i32, [vp, vp, vp, i32, i32, i32, pvp]),
    "mf_kmers_color": (i32, [vp, C.POINTER(cp), vp, i32, i32, i32, i32, cp, cp, pu64]),
    "mf_colored_components_device": (i32, [vp, vp, i32, i32, i32, C.c_double, vp, vp]),
    "mf_colored_components": (i32, [vp, C.POINTER(cp), i32, i32, i64, i32, i32, C.c_double, cp, cp, vp]),
    "mf_wctable_from_host": (i32, [vp, vp, vp, vp, u64, i32, pvp]),
    "mf_wctable_load": (i32, [vp, C.POINTER(cp), i32, i64, i32, pvp]),
    "mf_wctable_stats": (i32, [vp, pu64, C.POINTER(C.c_int)]),
    "mf_wctable_export": (i32, [vp, vp, vp, vp, u64, pu64]),
    "mf_wctable_write": (i32, [vp, cp, cp, pu64]),
    "mf_wctable_destroy": (None, [vp]),
    "mf_kmers_color_wide_tables": (i32, [vp, vp, vp, i32, i32, i32, pvp]),
    "mf_kmers_color_wide": (i32, [vp, C.POINTER(cp), vp, i32, i32, i32, i32, cp, cp, pu64]),
    "mf_colored_components_wide_device": (i32, [vp, vp, i32, i32, i32, C.c_double, vp, vp]),
    "mf_colored_components_wide": (i32, [vp, C.POINTER(cp), i32, i32, i64, i32, i32, C.c_double, cp, cp, vp]),
}

MAX_PATHS_COUNT = 10 ** 6       # ComponentPathsMain.java:30
STATS_COUNTERS = ("n", "scarce", "in_all", "unique", "chi2_rejected", "mw_rejected", "group_a", "group_b", "unique_left")
STATS3_COUNTERS = ("n", "scarce", "in_all", "unique", "chi2_rejected", "mw_rejected", "group_a", "group_b", "group_c", "unique_left")
SPECIFIC_COUNTERS = ("n", "unique", "scarce", "chi2_rejected", "mw_rejected", "unique_left", "group_a", "group_b")      # MF_SPECIFIC_* of the header


class MetafastError(RuntimeError):
    """Mirrors ExecutionFailedException (itmo!/utils/tool/Tool.java:450-463)."""


class DistAbort(MetafastError):
    """MF_ERR_TOGETHER: a rank could not do its part of an exchange step; EVERY rank raises this from the same call (the status rides on
    the integer gathers), so that all of them can take another route together instead of one rank raising while its peers wait inside
    a collective"""


def exported_symbols():
    """Every entry point declared in include/metafast_hip.h."""
    return sorted(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MetafastError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)          # AttributeError if the .so does not export a declared symbol
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def _check(rc):
    if rc < 0:
        raise (DistAbort if rc == -2 else MetafastError)(lib().mf_last_error().decode(errors="replace"))
    return rc


def _cfiles(files):
    return (C.c_char_p * len(files))(*[os.fsencode(f) for f in files])


def _opt(path):
    return os.fsencode(path) if path else None


class Context:
    def __init__(self, device=0, host_threads=0, stream=None):
        h = C.c_void_p()
        _check(lib().mf_ctx_create(device, host_threads or (os.cpu_count() or 1), C.byref(h)))
        self.h = h
        self.device = device
        self.stream_handle = None                     # the raw stream the library launches on when the caller gave one (else: its own)
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        c = getattr(self, "_mf_comm", None)             # (the communicator pipeline.py made for this context)
        if c is not None:
            self._mf_comm = None
            c.close()
        if getattr(self, "h", None) and _lib is not None:
            _lib.mf_ctx_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream):
        """stream: a raw hipStream_t (int), or a torch.cuda.Stream"""
        raw = getattr(stream, "cuda_stream", stream)
        _check(lib().mf_ctx_set_stream(self.h, C.c_void_p(int(raw) if raw else None)))
        self.stream_handle = int(raw) if raw else 0

    def bind_thread(self):
        """a thread other than the one that made the context calls this before its first call on it (HIP's current device is per thread)"""
        _check(lib().mf_ctx_bind_thread(self.h))

    def set_option(self, name, value):
        _check(lib().mf_ctx_set_option(self.h, name.encode(), int(value)))

    def synchronize(self):
        _check(lib().mf_ctx_synchronize(self.h))

    def trim(self, want_bytes=None):
        """give idle workspace back to the driver: all of it, or (want_bytes) the smallest idle regions until that much is free
        again -- returns the bytes given back in that case"""
        if want_bytes is None:
            _check(lib().mf_ctx_trim(self.h))
            return None
        got = C.c_uint64(0)
        _check(lib().mf_ctx_trim_bytes(self.h, int(want_bytes), C.byref(got)))
        return int(got.value)

    def reset_timers(self):
        _check(lib().mf_ctx_reset_timers(self.h))

    def stat(self, name):
        """counters and gauges of the context: slice_restarts, device_parsed_files, device_parser_stepped_back, hipmalloc_calls,
        skm_table_regrown (the dense table of a super-k-mer count grown again with entries to copy), ..."""
        v = lib().mf_ctx_stat(self.h, name.encode())
        if v < 0:
            raise MetafastError(lib().mf_last_error().decode(errors="replace"))
        return int(v)

    def kernel_time(self, name):
        ms = C.c_double()
        n = lib().mf_ctx_kernel_time(self.h, name.encode(), C.byref(ms))
        return int(n), float(ms.value)

    def kernel_report(self):
        """name -> (launches, total ms, longest launch ms)"""
        buf = C.create_string_buffer(1 << 16)
        _check(lib().mf_ctx_kernel_report(self.h, buf, len(buf)))
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms, mx = line.split("\t")
            out[name] = (int(n), float(ms), float(mx))
        return out

    # ---- A1-A4 ----
    def load_reads(self, files):
        """the readers alone (ReadersUtils.readDnaLazy): -> (bases uint8[], offsets uint64[n + 1]) on the host"""
        h = C.c_void_p()
        _check(lib().mf_reads_load(self.h, _cfiles(files), len(files), C.byref(h)))
        try:
            n, nb = C.c_uint64(), C.c_uint64()
            _check(lib().mf_reads_stats(h, C.byref(n), C.byref(nb)))
            bases = np.empty(nb.value, dtype=np.uint8)
            off = np.empty(n.value + 1, dtype=np.uint64)
            _check(lib().mf_reads_export(h, bases.ctypes.data, off.ctypes.data))
            return bases, off
        finally:
            lib().mf_reads_destroy(h)

    def count_reads(self, files, k, min_read_len=0):
        """IOUtils.loadReads (src/io/IOUtils.java:772-803)"""
        t = C.c_void_p()
        _check(lib().mf_count_reads(self.h, _cfiles(files), len(files), k, min_read_len, C.byref(t)))
        return Table(self, t)

    def count_reads_above(self, files, k, threshold, min_read_len=0):
        """KmersCounterMain.runImpl (src/tools/KmersCounterMain.java:77-99): load + the cut value > threshold of printKmers,
        made inside the counting kernels; -> (Table of the kept k-mers, distinct k-mers before the cut)"""
        t = C.c_void_p()
        n_all = C.c_uint64()
        _check(lib().mf_count_reads_above(self.h, _cfiles(files), len(files), k, min_read_len, threshold, C.byref(t), C.byref(n_all)))
        return Table(self, t), n_all.value

    def count_device(self, d_bases, d_offsets, n_reads, n_bases, k, min_read_len=0):
        """d_bases / d_offsets: raw device pointers (int) -- e.g. torch tensor.data_ptr()"""
        t = C.c_void_p()
        _check(lib().mf_count_device(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, k,
                                     min_read_len, C.byref(t)))
        return Table(self, t)

    def count_wide_device(self, d_bases, d_offsets, n_reads, n_bases, k, min_read_len=0):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63 (mf_wide.hip) -> dict(hi, lo, counts: ascending 2k-bit k-mers; n_occ)"""
        t = C.c_void_p()
        _check(lib().mf_count_wide_device(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, k, min_read_len, C.byref(t)))
        try:
            n, occ, kk = C.c_uint64(), C.c_uint64(), C.c_int()
            _check(lib().mf_wtable_stats(t, C.byref(n), C.byref(occ), C.byref(kk)))
            hi = np.empty(n.value, dtype=np.uint64); lo = np.empty(n.value, dtype=np.uint64); cnt = np.empty(n.value, dtype=np.uint16)
            m = C.c_uint64()
            _check(lib().mf_wtable_export(t, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, n.value, C.byref(m)))
            return dict(hi=hi, lo=lo, counts=cnt, n_occ=occ.value, k=kk.value)
        finally:
            lib().mf_wtable_destroy(t)

    def count_wide_table(self, d_bases, d_offsets, n_reads, n_bases, k, min_read_len=0):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63: the table left in HBM -> WideTable (pieces(): device pointers)"""
        t = C.c_void_p()
        _check(lib().mf_count_wide_device(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, k, min_read_len, C.byref(t)))
        return WideTable(self, t)

    def count_wide_above(self, d_bases, d_offsets, n_reads, n_bases, k, threshold, min_read_len=0):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63: count_wide_table with the cut count > threshold inside the pass
        -> (WideTable, distinct k-mers before the cut)"""
        t = C.c_void_p()
        n_all = C.c_uint64()
        _check(lib().mf_count_wide_device_above(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, k, min_read_len, threshold,
                                                C.byref(t), C.byref(n_all)))
        return WideTable(self, t), n_all.value

    def build_unitigs_wide(self, table, freq_threshold, min_len):
        """NO-REFERENCE EXTENSION: build_unitigs on a WideTable -> Seqs"""
        s = C.c_void_p()
        _check(lib().mf_build_unitigs_wide_device(self.h, table.h, freq_threshold, min_len, C.byref(s)))
        return Seqs(self, s)

    def cut_components_wide(self, cutter, b1, b2):
        """NO-REFERENCE EXTENSION: cut_components on a WideTable -> WideComps"""
        c = C.c_void_p()
        _check(lib().mf_cut_components_wide_device(self.h, cutter.h, b1, b2, C.byref(c)))
        return WideComps(self, c)

    def features_wide(self, comps, sample, threshold=0, selected=None):
        """NO-REFERENCE EXTENSION: features on WideComps and a WideTable; selected: WideTable of the --selected k-mers or None"""
        n = len(comps)
        vec = np.zeros(n, dtype=np.int64)
        br = np.zeros(n, dtype=np.float64)
        if selected is None:
            _check(lib().mf_features_wide_device(self.h, comps.h, sample.h, threshold, vec.ctypes.data, br.ctypes.data))
        else:
            _check(lib().mf_features_wide_device_selected(self.h, comps.h, sample.h, selected.h, threshold, vec.ctypes.data, br.ctypes.data))
        return vec, br

    def features_reads_wide(self, comps, d_bases, d_offsets, n_reads, n_bases, threshold=0, selected=None):
        """NO-REFERENCE EXTENSION: features of a sample straight from its reads in HBM on WideComps (k is theirs): 64-bit counts"""
        n = len(comps)
        vec = np.zeros(n, dtype=np.int64)
        br = np.zeros(n, dtype=np.float64)
        if selected is None:
            _check(lib().mf_features_reads_wide_device(self.h, comps.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, threshold,
                                                       vec.ctypes.data, br.ctypes.data))
        else:
            _check(lib().mf_features_reads_wide_device_selected(self.h, comps.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, selected.h,
                                                                threshold, vec.ctypes.data, br.ctypes.data))
        return vec, br

    # ---- the wide path's files (mf_wio.hip; formats: DESIGN 4.4) ----
    def count_reads_wide(self, files, k, min_read_len=0):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63: count_reads -> WideTable, uncut (its .stat.txt covers what the writer's cut drops)"""
        t = C.c_void_p()
        _check(lib().mf_count_reads_wide(self.h, _cfiles(files), len(files), k, min_read_len, C.byref(t)))
        return WideTable(self, t)

    def load_kmers_wide(self, files, k, freq_threshold=0):
        """NO-REFERENCE EXTENSION: wide .kmers.bin files (18-byte records, validated on the device) -> one-piece ascending WideTable;
        a k-mer of several files gets the saturating sum of its counts"""
        t = C.c_void_p()
        _check(lib().mf_wtable_load_kmers(self.h, _cfiles(files), len(files), freq_threshold, k, C.byref(t)))
        return WideTable(self, t)

    def load_components_wide(self, components_bin, k):
        c = C.c_void_p()
        _check(lib().mf_wcomps_load(self.h, os.fsencode(components_bin), k, C.byref(c)))
        return WideComps(self, c)

    def features_wide_files(self, components_bin, kmers_bin, k, threshold=0, vec_path=None, breadth_path=None, selected=None):
        """NO-REFERENCE EXTENSION: features (files) on wide files; .vec / .breadth as for k <= 31"""
        if selected is None:
            _check(lib().mf_features_wide(self.h, os.fsencode(components_bin), os.fsencode(kmers_bin), k, threshold, _opt(vec_path), _opt(breadth_path)))
        else:
            _check(lib().mf_features_wide_selected(self.h, os.fsencode(components_bin), os.fsencode(kmers_bin), k, threshold, selected.h, _opt(vec_path),
                                                   _opt(breadth_path)))

    def features_reads_wide_files(self, components_bin, files, k, threshold=0, vec_path=None, breadth_path=None, selected=None):
        """NO-REFERENCE EXTENSION: features (files) from the reads files of ONE library on a wide components.bin"""
        if selected is None:
            _check(lib().mf_features_reads_wide(self.h, os.fsencode(components_bin), _cfiles(files) if files else None, len(files), k, threshold,
                                                _opt(vec_path), _opt(breadth_path)))
        else:
            _check(lib().mf_features_reads_wide_selected(self.h, os.fsencode(components_bin), _cfiles(files) if files else None, len(files), k, threshold,
                                                         selected.h, _opt(vec_path), _opt(breadth_path)))

    def count_device_above(self, d_bases, d_offsets, n_reads, n_bases, k, threshold, min_read_len=0):
        """count, keeping only the k-mers with count > threshold (what the k-mer counter hands on, IOUtils.printKmers);
        -> (Table of the kept k-mers, number of distinct k-mers before the cut)"""
        t = C.c_void_p()
        n_all = C.c_uint64()
        _check(lib().mf_count_device_above(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, k,
                                           min_read_len, threshold, C.byref(t), C.byref(n_all)))
        return Table(self, t), n_all.value

    def load_kmers(self, files, freq_threshold, k):
        """IOUtils.loadKmers (src/io/IOUtils.java:369-401)"""
        t = C.c_void_p()
        _check(lib().mf_table_load_kmers(self.h, _cfiles(files), len(files), freq_threshold, k, C.byref(t)))
        return Table(self, t)

    def table_from_host(self, keys, counts, k):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        counts = np.ascontiguousarray(counts, dtype=np.uint16)
        t = C.c_void_p()
        _check(lib().mf_table_from_host(self.h, keys.ctypes.data, counts.ctypes.data, len(keys), k, C.byref(t)))
        return Table(self, t)

    def count_device_shard(self, d_bases, d_offsets, n_seqs, n_bases, k, min_len, rank, world):
        """this rank's shard (k-mers whose minimizer-partition hash starts with `rank`) of the table of all the sequences"""
        t = C.c_void_p()
        _check(lib().mf_count_device_shard(self.h, d_bases, d_offsets, n_seqs, n_bases, k, min_len, rank, world, C.byref(t)))
        return Table(self, t)

    # ---- A7 ----
    def build_unitigs(self, table, freq_threshold, min_len):
        """SequencesFinders.thresholdStrategy (src/algo/SequencesFinders.java:13-31)"""
        s = C.c_void_p()
        _check(lib().mf_build_unitigs_device(self.h, table.h, freq_threshold, min_len, C.byref(s)))
        return Seqs(self, s)

    # ---- A10 ----
    def cut_components(self, cutter_table, b1, b2):
        """ComponentsBuilder.splitStrategy (src/algo/ComponentsBuilder.java:24-32)"""
        c = C.c_void_p()
        _check(lib().mf_cut_components_device(self.h, cutter_table.h, b1, b2, C.byref(c)))
        return Comps(self, c)

    def load_components(self, path):
        c = C.c_void_p()
        _check(lib().mf_comps_load(self.h, os.fsencode(path), C.byref(c)))
        return Comps(self, c)

    # ---- comp2seq ----
    def comps_unitigs(self, comps, split=True, k=None):
        """The contigs of the components (ComponentsToSequences.java:41-76), all components in one build.  split: every component by
        itself; else the one table of all members.  k: for components that were loaded from a file (they do not know theirs).
        -> (Seqs, uint32 array: the component index of every sequence in export order -- all 0 without split)"""
        if k is not None:
            _check(lib().mf_comps_set_k(comps.h, k))
        s = C.c_void_p()
        _check(lib().mf_comps_unitigs_device(self.h, comps.h, 1 if split else 0, C.byref(s)))
        seqs = Seqs(self, s)
        return seqs, seqs.components()

    def comp2seq(self, components_bin, k, out_dir, split=False):
        """File form: kmers_fasta/, kmer-counter-many/{kmers,stats}/, seq-builder-many/sequences/ under out_dir -> (file sets, sequences)"""
        nf, ns = C.c_uint64(), C.c_uint64()
        _check(lib().mf_comp2seq(self.h, os.fsencode(components_bin), k, 1 if split else 0, os.fsencode(out_dir), C.byref(nf), C.byref(ns)))
        return nf.value, ns.value

    def wcomps_unitigs(self, wcomps, split=True):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63 (mf_wcomp2seq.hip): comps_unitigs on WideComps (they know their k) -> Seqs;
        Seqs.components() gives the component index of every sequence in export order (all 0 without split)"""
        s = C.c_void_p()
        _check(lib().mf_wcomps_unitigs_device(self.h, wcomps.h, 1 if split else 0, C.byref(s)))
        return Seqs(self, s)

    def comp2seq_wide(self, components_bin, k, out_dir, split=False):
        """NO-REFERENCE EXTENSION: comp2seq's file form on a wide components.bin (wide .kmers.bin records) -> (file sets, sequences)"""
        nf, ns = C.c_uint64(), C.c_uint64()
        _check(lib().mf_comp2seq_wide(self.h, os.fsencode(components_bin), k, 1 if split else 0, os.fsencode(out_dir), C.byref(nf), C.byref(ns)))
        return nf.value, ns.value

    # ---- comp2graph ----
    def comps_graph(self, comps, samples=None, coverage=False, k=None):
        """The compacted de Bruijn graph of every component as GFA (ComponentsToGraph.java:70-130), all components in one pass ->
        (text, dict of segments / links / cycles).  samples: Tables that colour the segments (None: every k-mer is worth 1); coverage:
        their summed counts instead of the number of samples that hold a k-mer.  k: for components loaded from a file."""
        if k is not None:
            _check(lib().mf_comps_set_k(comps.h, k))
        samples = list(samples or [])
        h = (C.c_void_p * max(len(samples), 1))(*[t.h for t in samples])
        g = C.c_void_p()
        _check(lib().mf_comps_graph_device(self.h, comps.h, h, len(samples), 1 if coverage else 0, C.byref(g)))
        return self._gfa_out(g)

    def _gfa_out(self, g):
        try:
            ns, nl, ncy, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
            _check(lib().mf_gfa_stats(g, C.byref(ns), C.byref(nl), C.byref(ncy), C.byref(nb)))
            buf = np.zeros(max(nb.value, 1), np.uint8)
            _check(lib().mf_gfa_text(g, buf.ctypes.data, nb.value, None))
        finally:
            lib().mf_gfa_destroy(g)
        return buf[:nb.value].tobytes().decode("ascii"), {"segments": ns.value, "links": nl.value, "cycles": ncy.value}

    def comp2graph(self, components_bin, k, out_gfa, kmers_files=(), coverage=False):
        """File form -> out_gfa; returns (components, segments, links)"""
        files = list(kmers_files)
        nc, ns, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().mf_comp2graph(self.h, os.fsencode(components_bin), k, _cfiles(files) if files else None, len(files), 1 if coverage else 0,
                                   os.fsencode(out_gfa), C.byref(nc), C.byref(ns), C.byref(nl)))
        return nc.value, ns.value, nl.value

    def wcomps_graph(self, wcomps, samples=None, coverage=False):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63 (mf_wcomp2graph.hip): comps_graph on WideComps (they know their k) -> (text, stats);
        samples: WideTables of the same k"""
        samples = list(samples or [])
        h = (C.c_void_p * max(len(samples), 1))(*[t.h for t in samples])
        g = C.c_void_p()
        _check(lib().mf_wcomps_graph_device(self.h, wcomps.h, h, len(samples), 1 if coverage else 0, C.byref(g)))
        return self._gfa_out(g)

    def comp2graph_wide(self, components_bin, k, out_gfa, kmers_files=(), coverage=False):
        """NO-REFERENCE EXTENSION: comp2graph's file form on a wide components.bin and wide .kmers.bin files -> out_gfa; returns
        (components, segments, links)"""
        files = list(kmers_files)
        nc, ns, nl = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().mf_comp2graph_wide(self.h, os.fsencode(components_bin), k, _cfiles(files) if files else None, len(files), 1 if coverage else 0,
                                        os.fsencode(out_gfa), C.byref(nc), C.byref(ns), C.byref(nl)))
        return nc.value, ns.value, nl.value

    # ---- seq2comp ----
    def comps_from_sequences(self, d_bases, d_offsets, n_seqs, n_bases, k):
        """One component per sequence (SequencesToComponents.java:61-103): its distinct canonical k-mers, size = their number, weight =
        the k-mer occurrences; a sequence shorter than k gives an empty component.  Input as for count_device."""
        c = C.c_void_p()
        _check(lib().mf_comps_from_sequences_device(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_seqs, n_bases, k, C.byref(c)))
        return Comps(self, c)

    def seq2comp(self, files, k, components_bin, stat_txt=None):
        """File form -> components_bin and the three-column stat_txt; returns (components, components per file)"""
        files = list(files)
        n = C.c_uint64()
        per = np.zeros(max(len(files), 1), dtype=np.uint64)
        _check(lib().mf_seq2comp(self.h, _cfiles(files) if files else None, len(files), k, os.fsencode(components_bin), _opt(stat_txt), C.byref(n),
                                 per.ctypes.data))
        return n.value, [int(x) for x in per[:len(files)]]

    def wcomps_from_sequences(self, d_bases, d_offsets, n_seqs, n_bases, k):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63: comps_from_sequences on 2k-bit k-mers -> WideComps, members ascending in (hi, lo)
        inside every component"""
        c = C.c_void_p()
        _check(lib().mf_wcomps_from_sequences_device(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_seqs, n_bases, k, C.byref(c)))
        return WideComps(self, c)

    def seq2comp_wide(self, files, k, components_bin, stat_txt=None):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63: seq2comp -> a wide components_bin and the three-column stat_txt; returns (components,
        components per file)"""
        files = list(files)
        n = C.c_uint64()
        per = np.zeros(max(len(files), 1), dtype=np.uint64)
        _check(lib().mf_seq2comp_wide(self.h, _cfiles(files) if files else None, len(files), k, os.fsencode(components_bin), _opt(stat_txt), C.byref(n),
                                      per.ctypes.data))
        return n.value, [int(x) for x in per[:len(files)]]

    # ---- component-paths ----
    def paths(self, comps, selection=None, min_len=50, max_paths=MAX_PATHS_COUNT, k=None):
        """The stretches of sequences that lie inside components (ComponentPathsMain.java:82-206) -> Paths: add() a batch of sequences
        (once per file), finish(), then counts and text.  selection: component numbers from 1 (None: all).  k: for components that
        were loaded from a file."""
        if k is not None:
            _check(lib().mf_comps_set_k(comps.h, k))
        sel = None if selection is None else np.ascontiguousarray(selection, dtype=np.uint32)
        p = C.c_void_p()
        _check(lib().mf_paths_create(self.h, comps.h, sel.ctypes.data if sel is not None else None, len(sel) if sel is not None else 0, min_len,
                                     max_paths, C.byref(p)))
        return Paths(self, p)

    def component_paths(self, components_bin, k, files, out_dir, selection=None, min_len=50, max_paths=MAX_PATHS_COUNT):
        """File form -> out_dir/component-<no>.seq.fasta; returns (components in the file, paths written)"""
        files = list(files)
        sel = None if selection is None else np.ascontiguousarray(selection, dtype=np.uint32)
        nc, npth = C.c_uint64(), C.c_uint64()
        _check(lib().mf_component_paths(self.h, os.fsencode(components_bin), k, _cfiles(files) if files else None, len(files),
                                        sel.ctypes.data if sel is not None else None, len(sel) if sel is not None else 0, min_len, max_paths,
                                        os.fsencode(out_dir), C.byref(nc), C.byref(npth)))
        return nc.value, npth.value

    def paths_wide(self, wcomps, selection=None, min_len=50, max_paths=MAX_PATHS_COUNT):
        """NO-REFERENCE EXTENSION, 32 <= k <= 63 (mf_wcomppaths.hip): paths on WideComps (they know their k) -> the same Paths object"""
        sel = None if selection is None else np.ascontiguousarray(selection, dtype=np.uint32)
        p = C.c_void_p()
        _check(lib().mf_paths_create_wide(self.h, wcomps.h, sel.ctypes.data if sel is not None else None, len(sel) if sel is not None else 0, min_len,
                                          max_paths, C.byref(p)))
        return Paths(self, p)

    def component_paths_wide(self, components_bin, k, files, out_dir, selection=None, min_len=50, max_paths=MAX_PATHS_COUNT):
        """NO-REFERENCE EXTENSION: component_paths' file form on a wide components.bin; returns (components in the file, paths written)"""
        files = list(files)
        sel = None if selection is None else np.ascontiguousarray(selection, dtype=np.uint32)
        nc, npth = C.c_uint64(), C.c_uint64()
        _check(lib().mf_component_paths_wide(self.h, os.fsencode(components_bin), k, _cfiles(files) if files else None, len(files),
                                             sel.ctypes.data if sel is not None else None, len(sel) if sel is not None else 0, min_len, max_paths,
                                             os.fsencode(out_dir), C.byref(nc), C.byref(npth)))
        return nc.value, npth.value

    # ---- A12 ----
    def features(self, comps, sample_table, threshold=0, selected=None):
        """selected: Table of the --selected k-mers (FeaturesCalculatorMain.java:113-116, 193) or None"""
        n = comps.stats()[0]
        vec = np.zeros(n, dtype=np.int64)
        br = np.zeros(n, dtype=np.float64)
        _check(lib().mf_features_device_selected(self.h, comps.h, sample_table.h, selected.h if selected is not None else None,
                                                 threshold, vec.ctypes.data, br.ctypes.data))
        return vec, br

    def features_reads(self, comps, d_bases, d_offsets, n_reads, n_bases, k, threshold=0, selected=None):
        """features of a sample straight from its reads in HBM (--use-reads-for-calculating-features): 64-bit counts"""
        n = comps.stats()[0]
        vec = np.zeros(n, dtype=np.int64)
        br = np.zeros(n, dtype=np.float64)
        _check(lib().mf_features_reads_device_selected(self.h, comps.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_reads, n_bases, k,
                                                       selected.h if selected is not None else None, threshold,
                                                       vec.ctypes.data, br.ctypes.data))
        return vec, br

    def features_reads_files(self, components_bin, files, k, threshold, vec_path, breadth_path, selected=None):
        _check(lib().mf_features_reads_selected(self.h, os.fsencode(components_bin), _cfiles(files), len(files), k, threshold,
                                                selected.h if selected is not None else None, _opt(vec_path), _opt(breadth_path)))

    def features_files(self, components_bin, kmers_bin, k, threshold, vec_path, breadth_path, selected=None):
        _check(lib().mf_features_selected(self.h, os.fsencode(components_bin), os.fsencode(kmers_bin), k, threshold,
                                          selected.h if selected is not None else None, _opt(vec_path), _opt(breadth_path)))

    # ---- group comparison (multi-sample join) ----
    def stats_kmers(self, a_tables, b_tables, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """StatsKmersFinder (src/tools/StatsKmersFinder.java:89-297) on resident tables -> (chi-squared survivors, group A, group B,
        dict of the nine counters)"""
        ha = (C.c_void_p * max(len(a_tables), 1))(*[t.h for t in a_tables])
        hb = (C.c_void_p * max(len(b_tables), 1))(*[t.h for t in b_tables])
        chi, ga, gb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctr = np.zeros(len(STATS_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers_tables(self.h, ha, len(a_tables), hb, len(b_tables), max_bad, p_chi2, p_mw, C.byref(chi), C.byref(ga),
                                           C.byref(gb), ctr.ctypes.data))
        return Table(self, chi), Table(self, ga), Table(self, gb), dict(zip(STATS_COUNTERS, map(int, ctr)))

    def stats_kmers_files(self, a_files, b_files, out_dir, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """the same from .kmers.bin files -> out_dir/filtered_{chisquared,groupA,groupB}.kmers.bin; returns the counters"""
        ctr = np.zeros(len(STATS_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers(self.h, _cfiles(a_files), len(a_files), _cfiles(b_files), len(b_files), max_bad, p_chi2, p_mw,
                                    os.fsencode(out_dir), ctr.ctypes.data))
        return dict(zip(STATS_COUNTERS, map(int, ctr)))

    def kmers_samples_count(self, tables, max_bad=1):
        """KmersSamplesCounter (src/tools/KmersSamplesCounter.java:69-140): Table of (k-mer, number of samples with count > max_bad)"""
        h = (C.c_void_p * max(len(tables), 1))(*[t.h for t in tables])
        t = C.c_void_p()
        _check(lib().mf_kmers_samples_count_tables(self.h, h, len(tables), max_bad, C.byref(t)))
        return Table(self, t)

    def kmers_samples_count_files(self, files, k, kmers_bin, stat_txt=None, max_bad=1):
        n = C.c_uint64()
        _check(lib().mf_kmers_samples_count(self.h, _cfiles(files), len(files), max_bad, k, os.fsencode(kmers_bin), _opt(stat_txt), C.byref(n)))
        return n.value

    def stats_kmers_wide(self, a_tables, b_tables, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """NO-REFERENCE EXTENSION: stats_kmers on WideTables (32 <= k <= 63) -> (chi-squared survivors, group A, group B, dict of the
        nine counters), the three as WideTables; a group table's values are Java shorts held as uint16 (0 and >= 0x8000 occur)"""
        ha = (C.c_void_p * max(len(a_tables), 1))(*[t.h if t is not None else None for t in a_tables])
        hb = (C.c_void_p * max(len(b_tables), 1))(*[t.h if t is not None else None for t in b_tables])
        chi, ga, gb = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctr = np.zeros(len(STATS_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers_wide_tables(self.h, ha, len(a_tables), hb, len(b_tables), max_bad, p_chi2, p_mw, C.byref(chi), C.byref(ga),
                                                C.byref(gb), ctr.ctypes.data))
        return WideTable(self, chi), WideTable(self, ga), WideTable(self, gb), dict(zip(STATS_COUNTERS, map(int, ctr)))

    def stats_kmers_wide_files(self, a_files, b_files, k, out_dir, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """the same from wide .kmers.bin files -> out_dir/filtered_{chisquared,groupA,groupB}.kmers.bin (wide records; a group file may
        hold values <= 0, which load_kmers_wide refuses); returns the counters"""
        ctr = np.zeros(len(STATS_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers_wide(self.h, _cfiles(a_files), len(a_files), _cfiles(b_files), len(b_files), max_bad, k, p_chi2, p_mw,
                                         os.fsencode(out_dir), ctr.ctypes.data))
        return dict(zip(STATS_COUNTERS, map(int, ctr)))

    def kmers_samples_count_wide(self, tables, max_bad=1):
        """NO-REFERENCE EXTENSION: kmers_samples_count on WideTables -> WideTable of (k-mer, number of samples with count > max_bad)"""
        h = (C.c_void_p * max(len(tables), 1))(*[t.h if t is not None else None for t in tables])
        t = C.c_void_p()
        _check(lib().mf_kmers_samples_count_wide_tables(self.h, h, len(tables), max_bad, C.byref(t)))
        return WideTable(self, t)

    def kmers_samples_count_wide_files(self, files, k, kmers_bin, stat_txt=None, max_bad=1):
        n = C.c_uint64()
        _check(lib().mf_kmers_samples_count_wide(self.h, _cfiles(files), len(files), max_bad, k, os.fsencode(kmers_bin), _opt(stat_txt), C.byref(n)))
        return n.value

    def stats_kmers3_wide(self, a_tables, b_tables, c_tables, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """NO-REFERENCE EXTENSION: stats_kmers3 on WideTables (32 <= k <= 63) -> (chi-squared survivors, group A, group B, group C, dict of
        the ten counters), the four as WideTables; a group table's values are Java shorts held as uint16 (0 and >= 0x8000 occur).  A
        library call only: the command-line tool stats-kmers-3 stays at k <= 31"""
        hs = [(C.c_void_p * max(len(g), 1))(*[t.h if t is not None else None for t in g]) for g in (a_tables, b_tables, c_tables)]
        chi, ga, gb, gc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctr = np.zeros(len(STATS3_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers3_wide_tables(self.h, hs[0], len(a_tables), hs[1], len(b_tables), hs[2], len(c_tables), max_bad, p_chi2, p_mw,
                                                 C.byref(chi), C.byref(ga), C.byref(gb), C.byref(gc), ctr.ctypes.data))
        return WideTable(self, chi), WideTable(self, ga), WideTable(self, gb), WideTable(self, gc), dict(zip(STATS3_COUNTERS, map(int, ctr)))

    def stats_kmers3_wide_files(self, a_files, b_files, c_files, k, out_dir, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """the same from wide .kmers.bin files -> out_dir/filtered_{chisquared,groupA,groupB,groupC}.kmers.bin (wide records; a group
        file may hold values <= 0, which load_kmers_wide refuses); returns the counters"""
        ctr = np.zeros(len(STATS3_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers3_wide(self.h, _cfiles(a_files), len(a_files), _cfiles(b_files), len(b_files), _cfiles(c_files), len(c_files),
                                          max_bad, k, p_chi2, p_mw, os.fsencode(out_dir), ctr.ctypes.data))
        return dict(zip(STATS3_COUNTERS, map(int, ctr)))

    def kmers_grouped_count_wide(self, kmers, cd, uc, nonibd, max_bad=1):
        """NO-REFERENCE EXTENSION: kmers_grouped_count on WideTables -> (hi uint64[n], lo uint64[n]: the k-mers of `kmers` in ascending
        order, int64[n][3] the number of cd, uc and nonibd tables that hold each with a count > max_bad)"""
        hs = [(C.c_void_p * max(len(g), 1))(*[t.h if t is not None else None for t in g]) for g in (cd, uc, nonibd)]
        cap = kmers.stats()[0] if kmers is not None else 0
        hi, lo, packed = (np.zeros(max(cap, 1), dtype=np.uint64) for _ in range(3))
        n = C.c_uint64()
        _check(lib().mf_kmers_grouped_count_wide_tables(self.h, kmers.h if kmers is not None else None, hs[0], len(cd), hs[1], len(uc), hs[2], len(nonibd),
                                                        max_bad, hi.ctypes.data, lo.ctypes.data, packed.ctypes.data, cap, C.byref(n)))
        packed = packed[:n.value]
        counts = np.stack([(packed >> np.uint64(32)) & np.uint64(0xFFFF), (packed >> np.uint64(16)) & np.uint64(0xFFFF), packed & np.uint64(0xFFFF)],
                          axis=1).astype(np.int64)
        return hi[:n.value], lo[:n.value], counts

    def kmers_grouped_count_wide_files(self, kmers_files, cd_files, uc_files, nonibd_files, k, out_txt, max_bad=1):
        """the same from wide .kmers.bin files -> out_txt (kmers.groups.txt); returns the number of k-mers written"""
        n = C.c_uint64()
        _check(lib().mf_kmers_grouped_count_wide(self.h, _cfiles(kmers_files), len(kmers_files), _cfiles(cd_files), len(cd_files), _cfiles(uc_files),
                                                 len(uc_files), _cfiles(nonibd_files), len(nonibd_files), max_bad, k, os.fsencode(out_txt), C.byref(n)))
        return n.value

    def stats_kmers3(self, a_tables, b_tables, c_tables, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """StatsKmers3GroupsFinder (src/tools/StatsKmers3GroupsFinder.java:92-377) on resident tables -> (chi-squared survivors, group A,
        group B, group C, dict of the ten counters)"""
        hs = [(C.c_void_p * max(len(g), 1))(*[t.h for t in g]) for g in (a_tables, b_tables, c_tables)]
        chi, ga, gb, gc = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctr = np.zeros(len(STATS3_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers3_tables(self.h, hs[0], len(a_tables), hs[1], len(b_tables), hs[2], len(c_tables), max_bad, p_chi2, p_mw,
                                            C.byref(chi), C.byref(ga), C.byref(gb), C.byref(gc), ctr.ctypes.data))
        return Table(self, chi), Table(self, ga), Table(self, gb), Table(self, gc), dict(zip(STATS3_COUNTERS, map(int, ctr)))

    def stats_kmers3_files(self, a_files, b_files, c_files, out_dir, p_chi2=0.05, p_mw=0.05, max_bad=0):
        """the same from .kmers.bin files -> out_dir/filtered_{chisquared,groupA,groupB,groupC}.kmers.bin; returns the counters"""
        ctr = np.zeros(len(STATS3_COUNTERS), dtype=np.uint64)
        _check(lib().mf_stats_kmers3(self.h, _cfiles(a_files), len(a_files), _cfiles(b_files), len(b_files), _cfiles(c_files), len(c_files),
                                     max_bad, p_chi2, p_mw, os.fsencode(out_dir), ctr.ctypes.data))
        return dict(zip(STATS3_COUNTERS, map(int, ctr)))

    def specific_kmers(self, a_tables, b_tables, p_chi2=0.05, p_mw=0.05):
        """SpecificKmersFinder (src/tools/SpecificKmersFinder.java:65-245) on resident tables -> (group A, group B, dict of the eight
        counters)"""
        ha = (C.c_void_p * max(len(a_tables), 1))(*[t.h for t in a_tables])
        hb = (C.c_void_p * max(len(b_tables), 1))(*[t.h for t in b_tables])
        ga, gb = C.c_void_p(), C.c_void_p()
        ctr = np.zeros(len(SPECIFIC_COUNTERS), dtype=np.uint64)
        _check(lib().mf_specific_kmers_tables(self.h, ha, len(a_tables), hb, len(b_tables), p_chi2, p_mw, C.byref(ga), C.byref(gb), ctr.ctypes.data))
        return Table(self, ga), Table(self, gb), dict(zip(SPECIFIC_COUNTERS, map(int, ctr)))

    def specific_kmers_files(self, a_files, b_files, out_dir, p_chi2=0.05, p_mw=0.05):
        """the same from .kmers.bin files -> out_dir/filtered_{groupA,groupB}.kmers.bin; returns the counters"""
        ctr = np.zeros(len(SPECIFIC_COUNTERS), dtype=np.uint64)
        _check(lib().mf_specific_kmers(self.h, _cfiles(a_files), len(a_files), _cfiles(b_files), len(b_files), p_chi2, p_mw, os.fsencode(out_dir),
                                       ctr.ctypes.data))
        return dict(zip(SPECIFIC_COUNTERS, map(int, ctr)))

    def specific_kmers3(self, a_tables, b_tables, c_tables, p_chi2=0.05, p_mw=0.05):
        """SpecificKmers3GroupsFinder (src/tools/SpecificKmers3GroupsFinder.java:70-280) on resident tables -> (group A, group B, group C,
        dict of the ten counters, named as stats_kmers3's)"""
        hs = [(C.c_void_p * max(len(g), 1))(*[t.h for t in g]) for g in (a_tables, b_tables, c_tables)]
        ga, gb, gc = C.c_void_p(), C.c_void_p(), C.c_void_p()
        ctr = np.zeros(len(STATS3_COUNTERS), dtype=np.uint64)
        _check(lib().mf_specific_kmers3_tables(self.h, hs[0], len(a_tables), hs[1], len(b_tables), hs[2], len(c_tables), p_chi2, p_mw,
                                               C.byref(ga), C.byref(gb), C.byref(gc), ctr.ctypes.data))
        return Table(self, ga), Table(self, gb), Table(self, gc), dict(zip(STATS3_COUNTERS, map(int, ctr)))

    def specific_kmers3_files(self, a_files, b_files, c_files, out_dir, p_chi2=0.05, p_mw=0.05):
        """the same from .kmers.bin files -> out_dir/filtered_{groupA,groupB,groupC}.kmers.bin; returns the counters"""
        ctr = np.zeros(len(STATS3_COUNTERS), dtype=np.uint64)
        _check(lib().mf_specific_kmers3(self.h, _cfiles(a_files), len(a_files), _cfiles(b_files), len(b_files), _cfiles(c_files), len(c_files),
                                        p_chi2, p_mw, os.fsencode(out_dir), ctr.ctypes.data))
        return dict(zip(STATS3_COUNTERS, map(int, ctr)))

    def unique_kmers(self, inputs, filters, max_bad=1):
        """UniqueKmersFinder (src/tools/UniqueKmersFinder.java:73-144) on resident tables -> (Table of the pooled k-mers that no filter
        table holds, size of the pooled map)"""
        hi = (C.c_void_p * max(len(inputs), 1))(*[t.h for t in inputs])
        hf = (C.c_void_p * max(len(filters), 1))(*[t.h for t in filters])
        out, n = C.c_void_p(), C.c_uint64()
        _check(lib().mf_unique_kmers_tables(self.h, hi, len(inputs), hf, len(filters), max_bad, C.byref(out), C.byref(n)))
        return Table(self, out), n.value

    def unique_kmers_files(self, in_files, filter_files, k, kmers_bin, stat_txt=None, max_bad=1):
        """the same from .kmers.bin files -> kmers_bin (+ stat_txt); returns (size of the pooled map, records written)"""
        n, good = C.c_uint64(), C.c_uint64()
        _check(lib().mf_unique_kmers(self.h, _cfiles(in_files), len(in_files), _cfiles(filter_files), len(filter_files), max_bad, k,
                                     os.fsencode(kmers_bin), _opt(stat_txt), C.byref(n), C.byref(good)))
        return n.value, good.value

    def kmers_grouped_count(self, kmers, cd, uc, nonibd, max_bad=1):
        """KmersGroupedSamplesCounter (src/tools/KmersGroupedSamplesCounter.java:82-190) on resident tables -> (uint64[n] the k-mers of
        `kmers` in ascending order, int64[n][3] the number of cd, uc and nonibd tables that hold each with a count > max_bad)"""
        hs = [(C.c_void_p * max(len(g), 1))(*[t.h for t in g]) for g in (cd, uc, nonibd)]
        cap = len(kmers)
        keys = np.zeros(max(cap, 1), dtype=np.uint64)
        packed = np.zeros(max(cap, 1), dtype=np.uint64)
        n = C.c_uint64()
        _check(lib().mf_kmers_grouped_count_tables(self.h, kmers.h, hs[0], len(cd), hs[1], len(uc), hs[2], len(nonibd), max_bad, keys.ctypes.data,
                                                   packed.ctypes.data, cap, C.byref(n)))
        packed = packed[:n.value]
        counts = np.stack([(packed >> np.uint64(32)) & np.uint64(0xFFFF), (packed >> np.uint64(16)) & np.uint64(0xFFFF), packed & np.uint64(0xFFFF)],
                          axis=1).astype(np.int64)
        return keys[:n.value], counts

    def kmers_grouped_count_files(self, kmers_files, cd_files, uc_files, nonibd_files, k, out_txt, max_bad=1):
        """the same from .kmers.bin files -> out_txt (kmers.groups.txt); returns the number of k-mers written"""
        n = C.c_uint64()
        _check(lib().mf_kmers_grouped_count(self.h, _cfiles(kmers_files), len(kmers_files), _cfiles(cd_files), len(cd_files), _cfiles(uc_files),
                                            len(uc_files), _cfiles(nonibd_files), len(nonibd_files), max_bad, k, os.fsencode(out_txt), C.byref(n)))
        return n.value

    def kmers_per_sample(self, tables, percent=20, max_bad=0, count_first=False):
        """KmersPerSampleCounter (src/tools/KmersPerSampleCounter.java:56-157) on resident tables -> KmersPerSample: the k-mers that at
        least len(tables) * percent / 100 (Java int arithmetic) of the samples hold with a count > max_bad, in ascending order, and every
        sample's count of each.  count_first = False is the reference: the first sample is not counted."""
        h = (C.c_void_p * max(len(tables), 1))(*[t.h for t in tables])
        r = C.c_void_p()
        _check(lib().mf_kmers_per_sample_tables(self.h, h, len(tables), max_bad, percent, 1 if count_first else 0, C.byref(r)))
        return KmersPerSample(self, r)

    def kmers_per_sample_files(self, files, k, out_txt, percent=20, count_first=False):
        """the same from .kmers.bin files, streamed -> out_txt (selected_kmers_<percent>.txt); returns the number of selected k-mers"""
        n = C.c_uint64()
        _check(lib().mf_kmers_per_sample(self.h, _cfiles(files), len(files), k, percent, 1 if count_first else 0, os.fsencode(out_txt), C.byref(n)))
        return n.value

    def kmers_per_sample_wide(self, tables, percent=20, max_bad=0, count_first=False):
        """NO-REFERENCE EXTENSION: kmers_per_sample on WideTables (32 <= k <= 63) -> KmersPerSample whose export() gives the k-mers as
        two words, (hi, lo, n, matrix)"""
        h = (C.c_void_p * max(len(tables), 1))(*[t.h if t is not None else None for t in tables])
        r = C.c_void_p()
        _check(lib().mf_kmers_per_sample_wide_tables(self.h, h, len(tables), max_bad, percent, 1 if count_first else 0, C.byref(r)))
        return KmersPerSample(self, r, wide=True)

    def kmers_per_sample_wide_files(self, files, k, out_txt, percent=20, count_first=False):
        """the same from wide .kmers.bin files, streamed -> out_txt (selected_kmers_<percent>.txt); returns the number of selected k-mers"""
        n = C.c_uint64()
        _check(lib().mf_kmers_per_sample_wide(self.h, _cfiles(files), len(files), k, percent, 1 if count_first else 0, os.fsencode(out_txt), C.byref(n)))
        return n.value

    @staticmethod
    def _ukm_slots(n_inputs, min_samples, max_samples):
        return max(1, min(max_samples, max(min_samples, n_inputs + 1)) - min_samples + 1)

    def unique_kmers_multi(self, inputs, filters, max_bad=1, min_samples=1, max_samples=1):
        """UniqueKmersMultipleSamplesFinder (src/tools/UniqueKmersMultipleSamplesFinder.java:84-185) on resident tables ->
        ([Table of filtered_<i> for i = min_samples ... up to the first empty one], n_union, [c_i])"""
        hi = (C.c_void_p * max(len(inputs), 1))(*[t.h for t in inputs])
        hf = (C.c_void_p * max(len(filters), 1))(*[t.h for t in filters])
        slots = self._ukm_slots(len(inputs), min_samples, max_samples)
        out = (C.c_void_p * slots)()
        counts = np.zeros(slots, dtype=np.uint64)
        n_out, n_union = C.c_int(), C.c_uint64()
        _check(lib().mf_unique_kmers_multi_tables(self.h, hi, len(inputs), hf, len(filters), max_bad, min_samples, max_samples, out,
                                                  C.byref(n_out), C.byref(n_union), counts.ctypes.data))
        return [Table(self, C.c_void_p(out[i])) for i in range(n_out.value)], n_union.value, [int(c) for c in counts[:n_out.value]]

    def unique_kmers_multi_files(self, in_files, filter_files, k, out_dir, max_bad=1, min_samples=1, max_samples=1):
        """the same from .kmers.bin files -> out_dir/filtered_<i>.kmers.bin; returns (n_union, [c_i])"""
        slots = self._ukm_slots(len(in_files), min_samples, max_samples)
        counts = np.zeros(slots, dtype=np.uint64)
        n_out, n_union = C.c_int(), C.c_uint64()
        _check(lib().mf_unique_kmers_multi(self.h, _cfiles(in_files), len(in_files), _cfiles(filter_files), len(filter_files), max_bad, k,
                                           min_samples, max_samples, os.fsencode(out_dir), C.byref(n_out), C.byref(n_union), counts.ctypes.data))
        return n_union.value, [int(c) for c in counts[:n_out.value]]

    def unique_kmers_multi_wide(self, inputs, filters, max_bad=1, min_samples=1, max_samples=1):
        """NO-REFERENCE EXTENSION: unique_kmers_multi on WideTables (32 <= k <= 63) ->
        ([WideTable of filtered_<i> for i = min_samples ... up to the first empty one], n_union, [c_i])"""
        hi = (C.c_void_p * max(len(inputs), 1))(*[t.h for t in inputs])
        hf = (C.c_void_p * max(len(filters), 1))(*[t.h for t in filters])
        slots = self._ukm_slots(len(inputs), min_samples, max_samples)
        out = (C.c_void_p * slots)()
        counts = np.zeros(slots, dtype=np.uint64)
        n_out, n_union = C.c_int(), C.c_uint64()
        _check(lib().mf_unique_kmers_multi_wide_tables(self.h, hi, len(inputs), hf, len(filters), max_bad, min_samples, max_samples, out,
                                                       C.byref(n_out), C.byref(n_union), counts.ctypes.data))
        return [WideTable(self, C.c_void_p(out[i])) for i in range(n_out.value)], n_union.value, [int(c) for c in counts[:n_out.value]]

    def unique_kmers_multi_wide_files(self, in_files, filter_files, k, out_dir, max_bad=1, min_samples=1, max_samples=1):
        """the same from wide .kmers.bin files -> out_dir/filtered_<i>.kmers.bin (wide records); returns (n_union, [c_i])"""
        slots = self._ukm_slots(len(in_files), min_samples, max_samples)
        counts = np.zeros(slots, dtype=np.uint64)
        n_out, n_union = C.c_int(), C.c_uint64()
        _check(lib().mf_unique_kmers_multi_wide(self.h, _cfiles(in_files), len(in_files), _cfiles(filter_files), len(filter_files), max_bad, k,
                                                min_samples, max_samples, os.fsencode(out_dir), C.byref(n_out), C.byref(n_union), counts.ctypes.data))
        return n_union.value, [int(c) for c in counts[:n_out.value]]

    def kmers_multiple_filters(self, table, cd, uc, nonibd, max_bad=1):
        """IOUtils.MultipleFiltersAndPrintKmers (src/io/IOUtils.java:125-213) on resident tables -> (Table of the kept entries,
        int64[m][3] distinct (cd, uc, nonibd) triples in ascending order, uint64[m] entries of each, found, kept)"""
        cap = max(len(table), 1)
        tri = np.zeros(cap, dtype=np.uint64)
        cnt = np.zeros(cap, dtype=np.uint64)
        fk = np.zeros(2, dtype=np.uint64)
        kept, n = C.c_void_p(), C.c_uint64()
        _check(lib().mf_kmers_multiple_filters_tables(self.h, table.h, cd.h, uc.h, nonibd.h, max_bad, C.byref(kept), tri.ctypes.data,
                                                      cnt.ctypes.data, cap, C.byref(n), fk.ctypes.data))
        tri = tri[:n.value]
        triples = np.stack([(tri >> np.uint64(32)) & np.uint64(0xFFFF), (tri >> np.uint64(16)) & np.uint64(0xFFFF), tri & np.uint64(0xFFFF)],
                           axis=1).astype(np.int64)
        return Table(self, kept), triples, cnt[:n.value], int(fk[0]), int(fk[1])

    def kmers_multiple_filters_files(self, in_files, cd_files, uc_files, nonibd_files, k, out_kmers, out_stats=None, max_bad=1):
        """KmersMultipleFilters (src/tools/KmersMultipleFilters.java:77-133): input j -> out_kmers[j] (+ out_stats[j]); returns
        [(found, kept)] per input"""
        fk = np.zeros(2 * max(len(in_files), 1), dtype=np.uint64)
        _check(lib().mf_kmers_multiple_filters(self.h, _cfiles(in_files), len(in_files), _cfiles(cd_files), len(cd_files), _cfiles(uc_files),
                                               len(uc_files), _cfiles(nonibd_files), len(nonibd_files), max_bad, k, _cfiles(out_kmers),
                                               _cfiles(out_stats) if out_stats else None, fk.ctypes.data))
        return [(int(fk[2 * j]), int(fk[2 * j + 1])) for j in range(len(in_files))]

    # ---- colored metagenomic features (pipeline 4) ----
    def kmers_color(self, tables, classes, b=1, val=False):
        """ColorKmersMain (src/tools/ColorKmersMain.java:89-136) on resident tables -> CTable of (k-mer, packed class counts)"""
        h = (C.c_void_p * max(len(tables), 1))(*[t.h for t in tables])
        cl = np.ascontiguousarray(classes, dtype=np.int32)
        if len(cl) != len(tables):
            raise MetafastError("kmers_color: %d tables, %d classes" % (len(tables), len(cl)))
        t = C.c_void_p()
        _check(lib().mf_kmers_color_tables(self.h, h, cl.ctypes.data, len(tables), b, 1 if val else 0, C.byref(t)))
        return CTable(self, t)

    def kmers_color_files(self, files, classes, k, kmers_bin, stat_txt=None, b=1, val=False):
        cl = np.ascontiguousarray(classes, dtype=np.int32)
        if len(cl) != len(files):
            raise MetafastError("kmers_color_files: %d files, %d classes" % (len(files), len(cl)))
        n = C.c_uint64()
        _check(lib().mf_kmers_color(self.h, _cfiles(files), cl.ctypes.data, len(files), b, 1 if val else 0, k, os.fsencode(kmers_bin),
                                    _opt(stat_txt), C.byref(n)))
        return n.value

    def ctable_from_host(self, keys, values, k):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        t = C.c_void_p()
        _check(lib().mf_ctable_from_host(self.h, keys.ctypes.data, values.ctypes.data, len(keys), k, C.byref(t)))
        return CTable(self, t)

    def load_ctable(self, files, min_value, k):
        """IOUtils.loadLongKmers (src/io/IOUtils.java:260-281): the records with value > min_value"""
        t = C.c_void_p()
        _check(lib().mf_ctable_load(self.h, _cfiles(files), len(files), min_value, k, C.byref(t)))
        return CTable(self, t)

    def colored_components(self, ct, n_groups=3, separate=False, perc=0.9, k=None):
        """ColoredComponentsBuilder, default and --separate modes -> [Comps of colour 0 .. n_groups - 1]"""
        out = (C.c_void_p * max(n_groups, 1))()
        _check(lib().mf_colored_components_device(self.h, ct.h, ct.k if k is None else k, n_groups, 1 if separate else 0, perc, out, None))
        return [Comps(self, C.c_void_p(out[c])) for c in range(n_groups)]

    def colored_components_files(self, files, k, out_dir, stat_txt=None, n_groups=3, separate=False, perc=0.9, min_value=None):
        """ColoredComponentMain (src/tools/ColoredComponentMain.java:83-119); min_value defaults to k, as in the reference"""
        counts = np.zeros(max(n_groups, 1), dtype=np.uint64)
        _check(lib().mf_colored_components(self.h, _cfiles(files), len(files), k, k if min_value is None else min_value, n_groups,
                                           1 if separate else 0, perc, os.fsencode(out_dir), _opt(stat_txt), counts.ctypes.data))
        return [int(c) for c in counts[:n_groups]]

    def kmers_color_wide(self, tables, classes, b=1, val=False):
        """NO-REFERENCE EXTENSION: kmers_color on WideTables (32 <= k <= 63) -> WCTable of (k-mer as two words, packed class counts)"""
        h = (C.c_void_p * max(len(tables), 1))(*[t.h if t is not None else None for t in tables])
        cl = np.ascontiguousarray(classes, dtype=np.int32)
        if len(cl) != len(tables):
            raise MetafastError("kmers_color_wide: %d tables, %d classes" % (len(tables), len(cl)))
        t = C.c_void_p()
        _check(lib().mf_kmers_color_wide_tables(self.h, h, cl.ctypes.data, len(tables), b, 1 if val else 0, C.byref(t)))
        return WCTable(self, t)

    def kmers_color_wide_files(self, files, classes, k, kmers_bin, stat_txt=None, b=1, val=False):
        """the same from wide .kmers.bin files -> kmers_bin (24-byte records) (+ stat_txt); returns the number of records written"""
        cl = np.ascontiguousarray(classes, dtype=np.int32)
        if len(cl) != len(files):
            raise MetafastError("kmers_color_wide_files: %d files, %d classes" % (len(files), len(cl)))
        n = C.c_uint64()
        _check(lib().mf_kmers_color_wide(self.h, _cfiles(files), cl.ctypes.data, len(files), b, 1 if val else 0, k, os.fsencode(kmers_bin),
                                         _opt(stat_txt), C.byref(n)))
        return n.value

    def wctable_from_host(self, hi, lo, values, k):
        hi = np.ascontiguousarray(hi, dtype=np.uint64)
        lo = np.ascontiguousarray(lo, dtype=np.uint64)
        values = np.ascontiguousarray(values, dtype=np.uint64)
        if not len(hi) == len(lo) == len(values):
            raise MetafastError("wctable_from_host: %d high words, %d low words, %d values" % (len(hi), len(lo), len(values)))
        t = C.c_void_p()
        _check(lib().mf_wctable_from_host(self.h, hi.ctypes.data, lo.ctypes.data, values.ctypes.data, len(hi), k, C.byref(t)))
        return WCTable(self, t)

    def wctable_load(self, files, min_value, k):
        """IOUtils.loadLongKmers on files of 24-byte wide records: the records with value > min_value"""
        t = C.c_void_p()
        _check(lib().mf_wctable_load(self.h, _cfiles(files), len(files), min_value, k, C.byref(t)))
        return WCTable(self, t)

    def colored_components_wide(self, ct, n_groups=3, separate=False, perc=0.9, k=None):
        """NO-REFERENCE EXTENSION: colored_components on a WCTable -> [WideComps of colour 0 .. n_groups - 1]"""
        out = (C.c_void_p * max(n_groups, 1))()
        _check(lib().mf_colored_components_wide_device(self.h, ct.h, ct.k if k is None else k, n_groups, 1 if separate else 0, perc, out, None))
        return [WideComps(self, C.c_void_p(out[c])) for c in range(n_groups)]

    def colored_components_wide_files(self, files, k, out_dir, stat_txt=None, n_groups=3, separate=False, perc=0.9, min_value=None):
        """the same from wide colored_kmers.kmers.bin files -> out_dir/components_color_<c>.bin (wide components); min_value defaults to k"""
        counts = np.zeros(max(n_groups, 1), dtype=np.uint64)
        _check(lib().mf_colored_components_wide(self.h, _cfiles(files), len(files), k, k if min_value is None else min_value, n_groups,
                                                1 if separate else 0, perc, os.fsencode(out_dir), _opt(stat_txt), counts.ctypes.data))
        return [int(c) for c in counts[:n_groups]]

    # ---- synthetic reads ----
    def synth_reads_device(self, seed, sample, first_read, n_reads, read_len, genome_scale_bp, d_bases, d_offsets, sub_per_16384=82):
        """sub_per_16384: substitutions per 16384 bases (82 = 0.5 %, the benchmark's; 164 = 1 %, BASELINE config 5)"""
        _check(lib().mf_synth_reads_device_ex(self.h, seed, sample, first_read, n_reads, read_len, genome_scale_bp, sub_per_16384,
                                              C.c_void_p(d_bases), C.c_void_p(d_offsets)))


class WideTable:
    """NO-REFERENCE EXTENSION: canonical counts of 2k-bit k-mers (32 <= k <= 63) in HBM, in ascending pieces"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        # (a handle that outlives its context -- collected late, out of a reference cycle -- has nothing left to give back: the context took its arena along)
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_wtable_destroy(self.h)
        self.h = None

    __del__ = close

    def stats(self):
        n, occ, kk = C.c_uint64(), C.c_uint64(), C.c_int()
        _check(lib().mf_wtable_stats(self.h, C.byref(n), C.byref(occ), C.byref(kk)))
        return n.value, occ.value, kk.value

    def export(self):
        """-> (hi, lo, counts) ascending"""
        n = self.stats()[0]
        hi = np.empty(n, dtype=np.uint64); lo = np.empty(n, dtype=np.uint64); cnt = np.empty(n, dtype=np.uint16)
        m = C.c_uint64()
        _check(lib().mf_wtable_export(self.h, hi.ctypes.data, lo.ctypes.data, cnt.ctypes.data, n, C.byref(m)))
        return hi, lo, cnt

    def filter(self, threshold):
        t = C.c_void_p()
        _check(lib().mf_wtable_filter(self.h, threshold, C.byref(t)))
        return WideTable(self.ctx, t)

    def drop_index(self):
        _check(lib().mf_wtable_drop_index(self.h))

    def write_kmers(self, threshold, kmers_bin, stat_txt=None):
        """wide .kmers.bin (records with count > threshold, ascending) + optionally .stat.txt; -> number of records written"""
        n = C.c_uint64()
        _check(lib().mf_wtable_write_kmers(self.h, threshold, os.fsencode(kmers_bin), _opt(stat_txt), C.byref(n)))
        return n.value

    def write_kmers_filtered(self, threshold, filter_table, filter_threshold, kmers_bin):
        """the records with count > threshold whose k-mer has a value > filter_threshold in filter_table (absent: 0) -> wide .kmers.bin;
        -> number of records written"""
        n = C.c_uint64()
        _check(lib().mf_wtable_write_kmers_filtered(self.h, threshold, filter_table.h, filter_threshold, os.fsencode(kmers_bin), C.byref(n)))
        return n.value

    def lookup(self, kmers):
        """kmers: iterable of Python ints (2k-bit k-mers) -> int32 counts, -1 = absent"""
        ks = [int(x) for x in kmers]
        hi = np.array([x >> 64 for x in ks], dtype=np.uint64); lo = np.array([x & 0xFFFFFFFFFFFFFFFF for x in ks], dtype=np.uint64)
        out = np.empty(len(ks), dtype=np.int32)
        _check(lib().mf_wtable_lookup(self.h, hi.ctypes.data, lo.ctypes.data, len(ks), out.ctypes.data))
        return out

    def pieces(self):
        """[(d_hi, d_lo, d_counts, n)]: raw device pointers of every piece (uint64, uint64, uint16)"""
        m = C.c_uint32()
        _check(lib().mf_wtable_pieces(self.h, C.byref(m)))
        out = []
        for i in range(m.value):
            a, b, c, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
            _check(lib().mf_wtable_piece_view(self.h, i, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
            out.append((a.value or 0, b.value or 0, c.value or 0, n.value))
        return out


class Reads:
    """sequences in HBM (bases + offsets) that the library owns: mf_reads (here: the gathered unitigs of all ranks)"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_reads_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        n, nb = C.c_uint64(), C.c_uint64()
        _check(lib().mf_reads_stats(self.h, C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def device_view(self):
        b, o = C.c_void_p(), C.c_void_p()
        _check(lib().mf_reads_device_view(self.h, C.byref(b), C.byref(o)))
        n, nb = self.stats()
        return dict(bases=b.value or 0, offsets=o.value or 0, n=n, n_bases=nb)

    def export(self):
        n, nb = self.stats()
        bases = np.empty(nb, dtype=np.uint8)
        off = np.empty(n + 1, dtype=np.uint64)
        _check(lib().mf_reads_export(self.h, bases.ctypes.data, off.ctypes.data))
        return bases, off


_OPS_GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.POINTER(C.c_int64))
_OPS_ALLGATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64))
_OPS_ALLTOALL = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))


class _CommOps(C.Structure):
    _fields_ = [("gather_ints", _OPS_GATHER), ("all_gather", _OPS_ALLGATHER), ("all_to_all", _OPS_ALLTOALL)]


class Comm:
    """mf_comm (include/metafast_hip.h): the exchanges of the multi-GPU path behind the C-ABI.  local(): one communicator per context for
    threads of this process; rccl(): one process per GPU; external(): the caller's own primitives (torch.distributed in pipeline.py)."""

    def __init__(self, ctx, h, keep=None):
        self.ctx, self.h, self._keep = ctx, h, keep
        self.rank, self.world = lib().mf_comm_rank(h), lib().mf_comm_world(h)
        self.kind = lib().mf_comm_kind(h).decode()

    def close(self):
        if getattr(self, "h", None) and _lib is not None:
            _lib.mf_comm_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def local(ctxs):
        n = len(ctxs)
        arr = (C.c_void_p * n)(*[c.h for c in ctxs])
        out = (C.c_void_p * n)()
        _check(lib().mf_comm_create_local(arr, n, out))
        return [Comm(ctxs[r], C.c_void_p(out[r])) for r in range(n)]

    @staticmethod
    def rccl_id():
        buf = C.create_string_buffer(128)
        _check(lib().mf_comm_rccl_id(buf))
        return buf.raw

    @staticmethod
    def rccl(ctx, id128, rank, world):
        h = C.c_void_p()
        _check(lib().mf_comm_create_rccl(ctx.h, C.c_char_p(bytes(id128)), rank, world, C.byref(h)))
        return Comm(ctx, h)

    @staticmethod
    def external(ctx, rank, world, gather_ints, all_gather, all_to_all):
        """gather_ints(list of int) -> int64 array [world, n]; all_gather(d_send, d_recv, bytes[world]); all_to_all(d_send, send_bytes[world],
        d_recv, recv_bytes[world]) -- device pointers as ints, the data has arrived when the call returns"""
        def _g(user, vals, n, out):
            try:
                m = np.asarray(gather_ints([int(vals[i]) for i in range(n)]), dtype=np.int64).reshape(-1)
                for i in range(world * n):
                    out[i] = int(m[i])
                return 0
            except Exception as e:              # (a C caller sees a status, not a Python exception)
                print("[metafast_amd] external gather_ints failed: %r" % (e,), file=__import__("sys").stderr)
                return -1

        def _ag(user, d_send, d_recv, nb):
            try:
                all_gather(d_send or 0, d_recv or 0, [int(nb[r]) for r in range(world)])
                return 0
            except Exception as e:
                print("[metafast_amd] external all_gather failed: %r" % (e,), file=__import__("sys").stderr)
                return -1

        def _aa(user, d_send, sb, d_recv, rb):
            try:
                all_to_all(d_send or 0, [int(sb[r]) for r in range(world)], d_recv or 0, [int(rb[r]) for r in range(world)])
                return 0
            except Exception as e:
                print("[metafast_amd] external all_to_all failed: %r" % (e,), file=__import__("sys").stderr)
                return -1
        ops = _CommOps(_OPS_GATHER(_g), _OPS_ALLGATHER(_ag), _OPS_ALLTOALL(_aa))
        h = C.c_void_p()
        _check(lib().mf_comm_create_external(ctx.h, rank, world, C.byref(ops), None, C.byref(h)))
        return Comm(ctx, h, keep=ops)

    def stats(self):
        return dict(collectives=int(lib().mf_comm_stat(self.h, b"collectives")), bytes_in=int(lib().mf_comm_stat(self.h, b"bytes_in")),
                    seconds=lib().mf_comm_stat(self.h, b"us") / 1e6)

    def reset_stats(self):
        _check(lib().mf_comm_reset_stats(self.h))

    def gather_ints(self, vals):
        v = np.ascontiguousarray(vals, dtype=np.int64)
        out = np.zeros((self.world, len(v)), dtype=np.int64)
        _check(lib().mf_comm_gather_ints(self.h, v.ctypes.data, len(v), out.ctypes.data))
        return out

    def all_gather(self, d_send, d_recv, bytes_per_rank):
        b = np.ascontiguousarray(bytes_per_rank, dtype=np.uint64)
        _check(lib().mf_comm_all_gather(self.h, C.c_void_p(d_send), C.c_void_p(d_recv), b.ctypes.data))

    def all_to_all(self, d_send, send_bytes, d_recv, recv_bytes):
        sb = np.ascontiguousarray(send_bytes, dtype=np.uint64); rb = np.ascontiguousarray(recv_bytes, dtype=np.uint64)
        _check(lib().mf_comm_all_to_all(self.h, C.c_void_p(d_send), sb.ctypes.data, C.c_void_p(d_recv), rb.ctypes.data))

    def gather_sequences(self, d_bases, d_offsets, n_seqs, n_bases):
        """every rank's sequences on every rank, rank after rank -> Reads"""
        h = C.c_void_p()
        _check(lib().mf_comm_gather_sequences(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_seqs, n_bases, C.byref(h)))
        return Reads(self.ctx, h)

    def cut_components_sharded(self, d_bases, d_offsets, n_seqs, n_bases, k, min_len, b1, b2):
        """ComponentCutterMain.runImpl over all ranks in one call (this rank's sequences in, the same Comps on every rank out)"""
        c = C.c_void_p()
        _check(lib().mf_cut_components_sharded(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_seqs, n_bases, k, min_len, b1, b2, C.byref(c)))
        return Comps(self.ctx, c)

    def cut_components_of_shard(self, shard, k, b1, b2):
        """... on a shard the caller has counted (None: this rank has none; all ranks raise DistAbort) -> (Comps, info)"""
        c = C.c_void_p()
        info = np.zeros(4, dtype=np.uint64)
        _check(lib().mf_cut_components_of_shard(self.h, shard.h if shard is not None else None, k, b1, b2, C.byref(c), info.ctypes.data))
        return Comps(self.ctx, c), dict(levels=int(info[0]), queries=int(info[1]), members=int(info[2]), vertices=int(info[3]))

    def features_allgather(self, rows):
        """rows int64[n_local_samples, C] -> int64[n_all_samples, C], rank-major"""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(len(rows), -1)
        n = C.c_uint64()
        _check(lib().mf_features_allgather(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], None, 0, C.byref(n)))
        out = np.zeros((n.value, rows.shape[1]), dtype=np.int64)
        _check(lib().mf_features_allgather(self.h, rows.ctypes.data, rows.shape[0], rows.shape[1], out.ctypes.data, n.value, C.byref(n)))
        return out


class WideComps:
    """NO-REFERENCE EXTENSION: connected components of 2k-bit k-mers (32 <= k <= 63)"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        # (a handle that outlives its context -- collected late, out of a reference cycle -- has nothing left to give back: the context took its arena along)
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_wcomps_destroy(self.h)
        self.h = None

    __del__ = close

    def stats(self):
        n, nk = C.c_uint64(), C.c_uint64()
        _check(lib().mf_wcomps_stats(self.h, C.byref(n), C.byref(nk)))
        return n.value, nk.value

    def __len__(self):
        return self.stats()[0]

    def export(self):
        """-> dict(sizes, weights, thr, offsets, hi, lo): k-mers grouped by component, ascending inside"""
        n, nk = self.stats()
        sizes = np.zeros(n, dtype=np.uint64); weights = np.zeros(n, dtype=np.int64); thr = np.zeros(n, dtype=np.int32)
        off = np.zeros(n + 1, dtype=np.uint64); hi = np.zeros(nk, dtype=np.uint64); lo = np.zeros(nk, dtype=np.uint64)
        _check(lib().mf_wcomps_export(self.h, sizes.ctypes.data, weights.ctypes.data, thr.ctypes.data, off.ctypes.data, hi.ctypes.data, lo.ctypes.data))
        return dict(sizes=sizes, weights=weights, thr=thr, offsets=off, hi=hi, lo=lo)

    def write(self, components_bin, stat_txt=None):
        _check(lib().mf_wcomps_write(self.h, os.fsencode(components_bin), _opt(stat_txt)))


class KmersPerSample:
    """the result of Context.kmers_per_sample (or kmers_per_sample_wide: wide = True, the k-mers as two words): M selected k-mers x N
    samples, resident in HBM"""

    def __init__(self, ctx, h, wide=False):
        self.ctx, self.h, self.wide = ctx, h, wide

    def close(self):
        if getattr(self, "h", None) and _lib is not None and self.ctx.h:
            _lib.mf_kps_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def shape(self):
        """(samples, selected k-mers)"""
        m, n = C.c_uint64(), C.c_int()
        _check(lib().mf_kps_stats(self.h, C.byref(m), C.byref(n)))
        return n.value, m.value

    def device_view(self):
        """device pointers (keys uint64[M], n(x) uint16[M], matrix uint16[N][M]); a wide result: (hi, lo, n(x), matrix)"""
        k, s, m = C.c_void_p(), C.c_void_p(), C.c_void_p()
        if self.wide:
            l = C.c_void_p()
            _check(lib().mf_kps_device_view_wide(self.h, C.byref(k), C.byref(l), C.byref(s), C.byref(m)))
            return k.value, l.value, s.value, m.value
        _check(lib().mf_kps_device_view(self.h, C.byref(k), C.byref(s), C.byref(m)))
        return k.value, s.value, m.value

    def export(self):
        """-> (keys uint64[M] ascending, n(x) uint16[M], matrix uint16[N][M]); a wide result: (hi uint64[M], lo uint64[M], n(x), matrix),
        ascending in (hi, lo)"""
        n, m = self.shape()
        if self.wide:
            hi, lo, ns, mat = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m, np.uint16), np.zeros((n, m), np.uint16)
            _check(lib().mf_kps_export_wide(self.h, hi.ctypes.data, lo.ctypes.data, ns.ctypes.data, mat.ctypes.data))
            return hi, lo, ns, mat
        keys, ns, mat = np.zeros(m, np.uint64), np.zeros(m, np.uint16), np.zeros((n, m), np.uint16)
        _check(lib().mf_kps_export(self.h, keys.ctypes.data, ns.ctypes.data, mat.ctypes.data))
        return keys, ns, mat

    def _text(self, fn, arg, cap):
        buf = np.zeros(max(cap, 1), np.uint8)
        n = C.c_uint64()
        _check(fn(self.h, arg, buf.ctypes.data, cap, C.byref(n)))
        assert n.value <= cap
        return buf[:n.value].tobytes()

    def header_text(self, k):
        """the file's first line without its newline, formatted on the device"""
        return self._text(lib().mf_kps_header_text, k, self.shape()[1] * (k + 1))

    def row_text(self, sample):
        """sample's line without the name and the newline, formatted on the device"""
        return self._text(lib().mf_kps_row_text, sample, self.shape()[1] * 6)


class Table:
    """BigLong2ShortHashMap stand-in: canonical k-mer -> saturating count, resident in HBM."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_table_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().mf_table_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def __len__(self):
        a = C.c_uint64()
        _check(lib().mf_table_stats(self.h, C.byref(a), None))
        return a.value

    def occurrences(self):
        a = C.c_uint64()
        _check(lib().mf_table_occurrences(self.h, C.byref(a)))
        return a.value

    def records(self):
        """-> (records the counting pass partitioned, bytes per record); measurement only"""
        a, b = C.c_uint64(), C.c_int32()
        _check(lib().mf_table_records(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def hist(self):
        """number of distinct k-mers per count over ALL counted k-mers (those a cut dropped included): the .stat.txt rows"""
        h = np.zeros(32768, dtype=np.uint64)
        _check(lib().mf_table_hist(self.h, h.ctypes.data))
        return h

    def export(self, threshold=-1):
        """-> (keys uint64[n] ascending, counts uint16[n]) with count > threshold"""
        n = C.c_uint64()
        _check(lib().mf_table_export(self.h, threshold, None, None, 0, C.byref(n)))
        keys = np.empty(n.value, dtype=np.uint64)
        cnts = np.empty(n.value, dtype=np.uint16)
        if n.value:
            _check(lib().mf_table_export(self.h, threshold, keys.ctypes.data, cnts.ctypes.data, n.value, C.byref(n)))
        return keys, cnts

    def device_view(self):
        k, c, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        _check(lib().mf_table_device_view(self.h, C.byref(k), C.byref(c), C.byref(n)))
        return k.value, c.value, n.value

    def lookup(self, keys):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.empty(len(keys), dtype=np.int32)
        _check(lib().mf_table_lookup(self.h, keys.ctypes.data, len(keys), out.ctypes.data))
        return out

    def drop_index(self):
        """give the lookup index back (rebuilt on the next lookup): several samples per GPU"""
        _check(lib().mf_table_drop_index(self.h))

    def write_kmers(self, threshold, kmers_bin, stat_txt=None):
        """IOUtils.printKmers (src/io/IOUtils.java:45-71)"""
        g = C.c_uint64()
        _check(lib().mf_table_write_kmers(self.h, threshold, os.fsencode(kmers_bin), _opt(stat_txt), C.byref(g)))
        return g.value

    def write_kmers_filtered(self, threshold, filter_table, filter_threshold, kmers_bin):
        """IOUtils.filterAndPrintKmers (src/io/IOUtils.java:101-123)"""
        g = C.c_uint64()
        _check(lib().mf_table_write_kmers_filtered(self.h, threshold, filter_table.h, filter_threshold, os.fsencode(kmers_bin), C.byref(g)))
        return g.value

    def filter(self, threshold):
        t = C.c_void_p()
        _check(lib().mf_table_filter(self.h, threshold, C.byref(t)))
        return Table(self.ctx, t)


class CTable:
    """BigLong2LongHashMap stand-in: k-mer -> 64-bit value, ascending keys, resident in HBM."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_ctable_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        n, k = C.c_uint64(), C.c_int()
        _check(lib().mf_ctable_stats(self.h, C.byref(n), C.byref(k)))
        return n.value, k.value

    def __len__(self):
        return self.stats()[0]

    @property
    def k(self):
        return self.stats()[1]

    def export(self):
        """-> (keys uint64[n] ascending, values uint64[n])"""
        n = len(self)
        keys = np.empty(n, dtype=np.uint64)
        vals = np.empty(n, dtype=np.uint64)
        m = C.c_uint64()
        if n:
            _check(lib().mf_ctable_export(self.h, keys.ctypes.data, vals.ctypes.data, n, C.byref(m)))
        return keys, vals

    def write(self, kmers_bin, stat_txt=None):
        w = C.c_uint64()
        _check(lib().mf_ctable_write(self.h, os.fsencode(kmers_bin), _opt(stat_txt), C.byref(w)))
        return w.value


class WCTable:
    """NO-REFERENCE EXTENSION: 2k-bit k-mer (32 <= k <= 63) -> 64-bit value, ascending, resident in HBM."""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_wctable_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        n, k = C.c_uint64(), C.c_int()
        _check(lib().mf_wctable_stats(self.h, C.byref(n), C.byref(k)))
        return n.value, k.value

    def __len__(self):
        return self.stats()[0]

    @property
    def k(self):
        return self.stats()[1]

    def export(self):
        """-> (hi uint64[n], lo uint64[n] ascending in (hi, lo), values uint64[n])"""
        n = len(self)
        hi = np.empty(n, dtype=np.uint64)
        lo = np.empty(n, dtype=np.uint64)
        vals = np.empty(n, dtype=np.uint64)
        m = C.c_uint64()
        if n:
            _check(lib().mf_wctable_export(self.h, hi.ctypes.data, lo.ctypes.data, vals.ctypes.data, n, C.byref(m)))
        return hi, lo, vals

    def write(self, kmers_bin, stat_txt=None):
        w = C.c_uint64()
        _check(lib().mf_wctable_write(self.h, os.fsencode(kmers_bin), _opt(stat_txt), C.byref(w)))
        return w.value


class Seqs:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_seqs_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().mf_seqs_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def __len__(self):
        return self.stats()[0]

    def device_view(self):
        p = [C.c_void_p() for _ in range(5)]
        n, nb = C.c_uint64(), C.c_uint64()
        _check(lib().mf_seqs_device_view(self.h, *[C.byref(x) for x in p], C.byref(n), C.byref(nb)))
        return dict(bases=p[0].value, offsets=p[1].value, avg=p[2].value, min=p[3].value, max=p[4].value,
                    n=n.value, n_bases=nb.value)

    def export(self):
        """-> list of (sequence str, avg, min, max)"""
        n, nb = self.stats()
        bases = np.empty(max(nb, 1), dtype=np.uint8)
        off = np.empty(n + 1, dtype=np.uint64)
        a = np.empty(max(n, 1), dtype=np.int32)
        mn = np.empty(max(n, 1), dtype=np.int32)
        mx = np.empty(max(n, 1), dtype=np.int32)
        _check(lib().mf_seqs_export(self.h, bases.ctypes.data, off.ctypes.data, a.ctypes.data, mn.ctypes.data,
                                    mx.ctypes.data))
        raw = bases.tobytes()
        return [(raw[int(off[i]):int(off[i + 1])].decode(), int(a[i]), int(mn[i]), int(mx[i])) for i in range(n)]

    def write_fasta(self, path):
        _check(lib().mf_seqs_write_fasta(self.h, os.fsencode(path)))

    def components(self):
        """the component index of every sequence in export order (sequences of Context.comps_unitigs only)"""
        n = self.stats()[0]
        comp = np.zeros(n, dtype=np.uint32)
        m = C.c_uint64()
        _check(lib().mf_seqs_components(self.h, comp.ctypes.data if n else None, n, C.byref(m)))
        return comp


class Comps:
    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_comps_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self):
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().mf_comps_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def __len__(self):
        return self.stats()[0]

    def export(self):
        """-> list of (size, weight, thr, kmers uint64[] ascending)"""
        n, nk = self.stats()
        sizes = np.empty(max(n, 1), dtype=np.uint64)
        w = np.empty(max(n, 1), dtype=np.int64)
        thr = np.empty(max(n, 1), dtype=np.int32)
        off = np.empty(n + 1, dtype=np.uint64)
        km = np.empty(max(nk, 1), dtype=np.uint64)
        _check(lib().mf_comps_export(self.h, sizes.ctypes.data, w.ctypes.data, thr.ctypes.data, off.ctypes.data,
                                     km.ctypes.data))
        return [(int(sizes[i]), int(w[i]), int(thr[i]), km[int(off[i]):int(off[i + 1])].copy()) for i in range(n)]

    def write(self, components_bin, stat_txt=None):
        _check(lib().mf_comps_write(self.h, os.fsencode(components_bin), _opt(stat_txt)))


class Paths:
    """The paths of the selected components (mf_paths_* in include/metafast_hip.h)"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_paths_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, d_bases, d_offsets, n_seqs, n_bases):
        _check(lib().mf_paths_add(self.h, C.c_void_p(d_bases), C.c_void_p(d_offsets), n_seqs, n_bases))

    def finish(self):
        _check(lib().mf_paths_finish(self.h))

    def max_listings(self):
        """the most selected components that list one k-mer (1: they share none)"""
        m = C.c_uint64()
        _check(lib().mf_paths_stats(self.h, None, None, None, C.byref(m)))
        return m.value

    def slots(self):
        """after finish() -> (component numbers, paths, bytes of text, count reached max_paths), one entry per slot"""
        n = C.c_uint64()
        _check(lib().mf_paths_stats(self.h, C.byref(n), None, None, None))
        n = n.value
        no, cnt, nb, cap = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint8)
        _check(lib().mf_paths_slots(self.h, no.ctypes.data, cnt.ctypes.data, nb.ctypes.data, cap.ctypes.data))
        return no[:n], cnt[:n], nb[:n], cap[:n].astype(bool)

    def text(self, slot=-1):
        """after finish(): the text of one slot, or of all of them one after the other (slot = -1), as bytes"""
        n = C.c_uint64()
        _check(lib().mf_paths_text(self.h, slot, None, 0, C.byref(n)))
        buf = np.zeros(max(n.value, 1), np.uint8)
        _check(lib().mf_paths_text(self.h, slot, buf.ctypes.data, n.value, None))
        return buf[:n.value].tobytes()

    def files(self):
        """after finish() -> {file name: bytes}, as mf_paths_write names them"""
        no, _, nb, _ = self.slots()
        whole, at, out = self.text(), 0, {}
        for i in range(len(no)):
            out[f"component-{int(no[i])}.seq.fasta"] = whole[at:at + int(nb[i])]
            at += int(nb[i])
        return out

    def write(self, out_dir):
        n = C.c_uint64()
        _check(lib().mf_paths_write(self.h, os.fsencode(out_dir), C.byref(n)))
        return n.value


class DistCutter:
    """One rank's part of the distributed component cutter (mf_dcc_* in include/metafast_hip.h): it owns a shard of the
    cutter table; the exchange steps in between are the caller's (metafast_amd/pipeline.py: distributed_components)."""

    def __init__(self, ctx, shard, rank, world, base):
        self.ctx, self.shard = ctx, shard
        base = np.ascontiguousarray(base, dtype=np.uint32)
        h = C.c_void_p()
        _check(lib().mf_dcc_create(ctx.h, shard.h, rank, world, base.ctypes.data, C.byref(h)))
        self.h, self.world, self.rank = h, world, rank

    def close(self):
        if getattr(self, "h", None) and _lib is not None and getattr(self.ctx, "h", None):
            _lib.mf_dcc_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _counts(self, fn):
        c = np.zeros(self.world, dtype=np.uint64)
        _check(fn(self.h, c.ctypes.data))
        return c

    def queries(self):
        return self._counts(lib().mf_dcc_queries)

    def queries_fill(self, d_q):
        _check(lib().mf_dcc_queries_fill(self.h, d_q))

    def answer(self, d_q, n, d_a):
        _check(lib().mf_dcc_answer(self.h, d_q, n, d_a))

    def set_answers(self, d_a, n):
        _check(lib().mf_dcc_set_answers(self.h, d_a, n))

    def level_local(self):
        return self._counts(lib().mf_dcc_level_local)

    def pairs_fill(self, d_out):
        _check(lib().mf_dcc_pairs_fill(self.h, d_out))

    def pairs_complete(self, d_pairs, n):
        _check(lib().mf_dcc_pairs_complete(self.h, d_pairs, n))

    def merge(self, d_pairs, n):
        m = C.c_uint64()
        _check(lib().mf_dcc_merge(self.h, d_pairs, n, C.byref(m)))
        return m.value

    def stats_fill(self, d_out):
        _check(lib().mf_dcc_stats_fill(self.h, d_out))

    def classify(self, d_stats, n, seg_first, own_n, b1, b2, thr, rank):
        """seg_first: first record of every rank (world + 1 entries) -> (kept, oversize) components of the level over ALL ranks"""
        seg = np.ascontiguousarray(seg_first, dtype=np.uint64)
        a, b = C.c_uint64(), C.c_uint64()
        _check(lib().mf_dcc_classify(self.h, d_stats, n, seg.ctypes.data, int(seg[rank]), own_n, b1, b2, thr, C.byref(a), C.byref(b)))
        return a.value, b.value

    def kept_fill(self, d_out):
        _check(lib().mf_dcc_kept_fill(self.h, d_out))

    def members(self):
        n = C.c_uint64()
        _check(lib().mf_dcc_members(self.h, C.byref(n)))
        return n.value

    def members_fill(self, d_keys, d_roots):
        _check(lib().mf_dcc_members_fill(self.h, d_keys, d_roots))

    def members_grouped(self):
        """-> (members, runs): this rank's members sorted by component, 8 B each + one (root, count) record per component"""
        n, r = C.c_uint64(), C.c_uint64()
        _check(lib().mf_dcc_members_grouped(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def members_grouped_fill(self, d_keys, d_runs):
        _check(lib().mf_dcc_members_grouped_fill(self.h, d_keys, d_runs))

    def finish_grouped(self, d_keys, nm, d_runs, n_runs, roots, sizes, weights, thrs, minkeys):
        roots = np.ascontiguousarray(roots, dtype=np.uint32); sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        weights = np.ascontiguousarray(weights, dtype=np.int64); thrs = np.ascontiguousarray(thrs, dtype=np.int32)
        minkeys = np.ascontiguousarray(minkeys, dtype=np.uint64)
        c = C.c_void_p()
        _check(lib().mf_dcc_finish_grouped(self.h, d_keys, nm, d_runs, n_runs, roots.ctypes.data, sizes.ctypes.data, weights.ctypes.data,
                                           thrs.ctypes.data, minkeys.ctypes.data, len(roots), C.byref(c)))
        return Comps(self.ctx, c)

    def minkeys(self, roots, d_out):
        roots = np.ascontiguousarray(roots, dtype=np.uint32)
        _check(lib().mf_dcc_minkeys(self.h, roots.ctypes.data, len(roots), d_out))

    def finish(self, d_keys, d_roots, nm, roots, sizes, weights, thrs, minkeys):
        roots = np.ascontiguousarray(roots, dtype=np.uint32); sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
        weights = np.ascontiguousarray(weights, dtype=np.int64); thrs = np.ascontiguousarray(thrs, dtype=np.int32)
        minkeys = np.ascontiguousarray(minkeys, dtype=np.uint64)
        c = C.c_void_p()
        _check(lib().mf_dcc_finish(self.h, d_keys, d_roots, nm, roots.ctypes.data, sizes.ctypes.data, weights.ctypes.data,
                                   thrs.ctypes.data, minkeys.ctypes.data, len(roots), C.byref(c)))
        return Comps(self.ctx, c)


def bray_curtis(vecs):
    """DistanceMatrixCalculatorMain.brayCurtisDistance (:140-152) for all sample pairs."""
    vecs = np.ascontiguousarray(vecs, dtype=np.int64)
    s, c = vecs.shape
    out = np.zeros((s, s), dtype=np.float64)
    _check(lib().mf_bray_curtis(vecs.ctypes.data, s, c, out.ctypes.data))
    return out


def synth_reads_host(seed, sample, first_read, n_reads, read_len, genome_scale_bp, sub_per_16384=82):
    bases = np.empty(n_reads * read_len, dtype=np.uint8)
    off = np.empty(n_reads + 1, dtype=np.uint64)
    _check(lib().mf_synth_reads_host_ex(seed, sample, first_read, n_reads, read_len, genome_scale_bp, sub_per_16384,
                                        bases.ctypes.data, off.ctypes.data))
    return bases, off

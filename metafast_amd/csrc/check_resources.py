#!/usr/bin/env python3
"""Reads hipcc's stderr of one compile with -Rpass-analysis=kernel-resource-usage: passes the compiler's own messages through, writes
the per-kernel table to <out>, and FAILS the build when one of the neighbour-lookup kernels (mf_nbr.h: waves that hand data to each
other through LDS between wave-level barriers, at a forced occupancy) needs scratch -- a build of k_ut_flags_part that spilled hung
on the GPU (round 4)."""
import os
import re
import sys

NO_SCRATCH = re.compile(r"k_ut_flags_part|k_cc_adjacency_part|k_dcc_adjacency_part|k_c2s_flags|k_kps_|k_c2g_|k_s2c_|k_ws2c_|k_cp_|k_specific|k_uk_|k_wf_|k_w_features|k_wj_|k_wkps_|k_wstats_|k_wcolor_")
# ... and the ones that are to run without LDS as well (one thread per row, nothing shared: mf_comp2seq.hip; one thread per key, entry,
# column or value: mf_kps.hip; one thread per node, segment, segment end, link or row: mf_comp2graph.hip, mf_wcomp2graph.hip; one thread per run of positions, per
# run, per record, or one wave per record: mf_comppaths.hip; one thread per entry or per run of equal k-mers: mf_wjoin.hip; one thread per entry or
# column: mf_wkps.hip; one thread per k-mer of a slice's union, per entry of a sample or per row: mf_wstats.hip; one thread per entry of a sample:
# mf_wcolor.hip)
NO_LDS = re.compile(r"k_c2s_flags|k_kps_|k_c2g_|k_cp_|k_wj_|k_wkps_|k_wstats_|k_wcolor_")
# the translation units that hold those kernels: the guard must SEE them there (a renamed kernel, or a remark format that changed,
# is a failed check, not a passed one)
EXPECT = {"mf_unitig": ["k_ut_flags_part"], "mf_cc": ["k_cc_adjacency_part", "k_dcc_adjacency_part"], "mf_comp2seq": ["k_c2s_flags"],
          "mf_kps": ["k_kps_index", "k_kps_gather", "k_kps_header", "k_kps_widths", "k_kps_format"],
          "mf_comp2graph": ["k_c2g_links", "k_c2g_double", "k_c2g_ends", "k_c2g_assign", "k_c2g_segments", "k_c2g_links_of", "k_c2g_write_s",
                            "k_c2g_write_bases", "k_c2g_write_l", "k_c2g_values"],
          # (the same steps on 2k-bit k-mers: mf_c2g.h's kernels, the three k-mer reading ones instantiated over 128-bit keys)
          "mf_wcomp2graph": ["k_c2g_links", "k_c2g_double", "k_c2g_ends", "k_c2g_assign", "k_c2g_segments", "k_c2g_links_of", "k_c2g_write_s",
                             "k_c2g_write_bases", "k_c2g_write_l", "k_c2g_wvalues"],
          # (k_s2c_lds: waves that share a workgroup's LDS table between wave-level barriers, two workgroups per CU)
          "mf_seq2comp": ["k_s2c_sizes", "k_s2c_lds", "k_s2c_pairs", "k_s2c_heads", "k_s2c_seg_heads", "k_s2c_seg_sizes", "k_s2c_compact", "k_s2c_place",
                          "k_s2c_shift"],
          # (k_ws2c_lds: the same teams on 2k-bit k-mers -- a sequence's k-mers sorted in two LDS word arrays between team barriers; a spill
          # would cost it the four workgroups per CU its 32 KiB of LDS leave room for)
          "mf_wseq2comp": ["k_ws2c_sizes", "k_ws2c_lds", "k_ws2c_pairs", "k_ws2c_gather64", "k_ws2c_gather32", "k_ws2c_heads", "k_ws2c_seg_sizes",
                           "k_ws2c_compact", "k_ws2c_place", "k_ws2c_shift"],
          "mf_comppaths": ["k_cp_select", "k_cp_members", "k_cp_heads", "k_cp_distinct", "k_cp_maxlist", "k_cp_split", "k_cp_join", "k_cp_sizes", "k_cp_mark",
                           "k_cp_pair", "k_cp_keep", "k_cp_bump", "k_cp_records", "k_cp_copy", "k_cp_keys", "k_cp_widths", "k_cp_slot_bytes",
                           "k_cp_write_head", "k_cp_write_bases"],
          # (the member side and the marking kernel on 2k-bit k-mers: k_cp_mark of mf_cp.h instantiated over 128-bit keys)
          # (the wide features, mf_wfeatures.hip: a thread per listing or per run of read positions, two 128-bit registers rolled per thread)
          "mf_wfeatures": ["k_wf_index", "k_wf_sizes", "k_wf_split", "k_wf_join", "k_wf_presence", "k_wf_select", "k_wf_occ", "k_w_features"],
          "mf_wcomppaths": ["k_cp_wmembers", "k_cp_gather64", "k_cp_gather32", "k_cp_wheads", "k_cp_wdistinct", "k_cp_mark"],
          # (the row kernels of specific-kmers and specific-kmers-3 keep a row in LDS: a spill would cost them their occupancy)
          "mf_specific": ["k_specific_select", "k_specific_gather", "k_specific_rows_thread", "k_specific_rows_wave"],
          "mf_stats": ["k_specific3_rows_thread", "k_specific3_rows_wave"], "mf_kmersets": ["k_uk_knock"],
          # (the wide join, mf_wjoin.hip: a thread per entry, per run of equal k-mers or per filter entry, nothing shared)
          "mf_wjoin": ["k_wj_gather", "k_wj_reduce", "k_wj_reduce_groups", "k_wj_knock", "k_wj_mark", "k_wj_flag", "k_wj_pick", "k_wj_keep"],
          # (the wide kmers-per-sample, mf_wkps.hip: a thread per entry of a sample (15 VGPRs) or per column (36), nothing shared)
          "mf_wkps": ["k_wkps_gather", "k_wkps_header"],
          # (the wide stats-kmers and stats-kmers-3, mf_wstats.hip: a thread per k-mer of the union, per entry of a sample or per row number, nothing
          # shared; the row kernels it launches are mf_stats.hip's.  The wide kmers-grouped-counter's probe: a thread per k-mer of the -kf table)
          "mf_wstats": ["k_wstats_select", "k_wstats_select3", "k_wstats_probe", "k_wstats_gather", "k_wstats_iota", "k_wstats_keys"],
          # (the wide kmers-color, mf_wcolor.hip: a thread per entry of a sample -- a binary search and a 64-bit compare-and-swap, nothing shared)
          "mf_wcolor": ["k_wcolor_add"]}


def main():
    src, out = sys.argv[1], sys.argv[2]
    lines = open(src, errors="replace").read().splitlines()
    kernels, cur, skip, bad = {}, None, 0, []
    for ln in lines:
        if "[-Rpass-analysis=kernel-resource-usage]" in ln:
            skip = 2
            m = re.search(r"remark:\s+Function Name: (\S+)", ln)
            if m:
                cur = m.group(1)
                kernels[cur] = {}
            else:
                m = re.search(r"remark:\s+([^:]+): (\S+)", ln)
                if m and cur:
                    kernels[cur][m.group(1).strip()] = m.group(2)
            continue
        if skip and (re.match(r"^\s*\d+ \| ", ln) or re.match(r"^\s*\| ", ln)):
            skip -= 1
            continue
        skip = 0
        if re.match(r"^\d+ warnings? generated", ln) or "remarks generated" in ln:
            continue
        print(ln, file=sys.stderr)
    unit = os.path.splitext(os.path.basename(src))[0]
    missing = []
    with open(out, "w") as f:
        for name, r in kernels.items():
            f.write(f"{name} vgprs={r.get('VGPRs')} scratch={r.get('ScratchSize [bytes/lane]')} occupancy={r.get('Occupancy [waves/SIMD]')} lds={r.get('LDS Size [bytes/block]')}\n")
            if NO_SCRATCH.search(name):
                sc = r.get("ScratchSize [bytes/lane]")
                if sc is None:
                    missing.append(f"{name}: no 'ScratchSize [bytes/lane]' remark was parsed")
                elif sc != "0":
                    bad.append((name, sc))
            if NO_LDS.search(name) and r.get("LDS Size [bytes/block]") != "0":
                missing.append(f"{name}: {r.get('LDS Size [bytes/block]')} bytes of LDS per block, it is to use none")
    for want in EXPECT.get(unit, []):
        if not any(want in name for name in kernels):
            missing.append(f"{unit}: no resource record of a kernel named *{want}* (renamed? remark format changed?)")
    for name, sc in bad:
        print(f"error: {name} uses {sc} bytes of scratch per lane (see check_resources.py)", file=sys.stderr)
    for m in missing:
        print(f"error: resource check cannot vouch for the no-scratch kernels -- {m}", file=sys.stderr)
    return 1 if bad or missing else 0


if __name__ == "__main__":
    sys.exit(main())

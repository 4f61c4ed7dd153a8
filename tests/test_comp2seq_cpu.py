"""comp2seq: the Python restatement (tests/comp2seq_ref.py) pinned on hand-worked cases, and the new entry points' declarations."""
import os
import struct
import subprocess

import numpy as np
import pytest

import comp2seq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_points_are_declared():
    from metafast_amd import lib as L
    header = open(L.HEADER_PATH).read()
    for name in ("mf_comps_unitigs_device", "mf_seqs_components", "mf_comp2seq", "mf_comps_set_k"):
        assert f" {name}(" in header, name
        assert name in L.exported_symbols(), name
    assert callable(L.Context.comps_unitigs) and callable(L.Context.comp2seq) and callable(L.Seqs.components)


def test_the_driver_lists_and_knows_the_tool(tmp_path):
    # the stub build of the driver (no GPU): the tool's line is in the -ts listing, and -t comp2seq is a known tool
    import test_driver_tools_cpu as D
    cli = D.stub_driver()
    r = subprocess.run([cli, "-ts"], capture_output=True, text=True, env=D.ENV, cwd=str(tmp_path))
    assert r.returncode == 0 and "\ncomp2seq\t\tTransforms components in binary format to FASTA sequences (contigs)\n" in r.stdout, r.stdout
    r = subprocess.run([cli, "-t", "comp2seq", "-w", str(tmp_path / "w")], capture_output=True, text=True, env=D.ENV, cwd=str(tmp_path))
    assert r.returncode == 1 and "not found" not in r.stderr and r.stderr == "ERROR: Mandatory argument --components-file (-cf) not set\n", r.stderr


def test_encoding_and_canonical_form():
    assert R.encode("AGCT") == 0b00011011 and R.decode(0b00011011, 4) == "AGCT"
    assert R.canon(R.encode("TTTT"), 4) == R.encode("AAAA") == 0
    assert R.kmers_of("ACGTT", 4) == [R.canon(R.encode("ACGT"), 4), R.canon(R.encode("CGTT"), 4)]
    assert R.kmers_of("ACGTT", 4, canonical=False) == [R.encode("ACGT"), R.encode("CGTT")]
    assert R.order_key("TTTTG", 4) == (0, 1) and R.order_key("AAAAG", 4) == (0, 0)


def test_two_adjacent_components_give_two_sequences_and_the_union_one(oracle):
    k = 5
    s = "AACCGATTGC"                                       # six 5-mers, a simple path
    km = R.kmers_of(s, k)
    assert len(set(km)) == 6
    comps = [km[:3], km[3:]]
    per = R.expected_split(oracle, comps, k)
    assert [len(p) for p in per] == [1, 1]
    (a, a_av, a_mn, a_mx), (b, *_) = per[0][0], per[1][0]
    assert {a, R.rc_str(a)} & {s[:7]} and {b, R.rc_str(b)} & {s[3:]}
    assert (a_av, a_mn, a_mx) == (1, 1, 1)
    union = R.expected_union(oracle, comps, k)
    assert len(union) == 1 and union[0][0] in (s, R.rc_str(s))
    seqs, ids = R.flatten(per)
    assert len(seqs) == 2 and ids.tolist() == [0, 1]


def test_a_member_listed_twice_weighs_two(oracle):
    k = 5
    km = R.kmers_of("AACCGAT", k)                          # three 5-mers
    (tab,) = R.component_tables([[km[0], km[1], km[1], km[2]]], k)
    assert tab == {km[0]: 1, km[1]: 2, km[2]: 1}
    ((seq, av, mn, mx),) = R.expected_split(oracle, [[km[0], km[1], km[1], km[2]]], k)[0]
    assert len(seq) == 7 and (av, mn, mx) == (4 // 3, 1, 2)
    assert R.component_tables([[km[0]] * 40000], k)[0][km[0]] == R.MAX_COUNT


def test_the_files_numbering_and_record_order(oracle):
    k = 5
    km = R.kmers_of("AACCGATTGC", k)
    comps = [[km[2], km[0], km[1]], [km[5], km[3], km[4]]]  # members in file order, not ascending
    files = R.expected_files(oracle, comps, k, split=True)
    assert sorted(files) == sorted(f"{d}/component_{i}{e}" for i in (1, 2) for d, e in (("kmers_fasta", ".fasta"), ("kmer-counter-many/kmers", ".kmers.bin"),
                                                                                   ("kmer-counter-many/stats", ".stat.txt"), ("seq-builder-many/sequences", ".seq.fasta")))
    fa = files["kmers_fasta/component_1.fasta"].decode().split("\n")
    assert fa[0::2][:3] == [">1", ">2", ">3"] and fa[1] == R.decode(km[2], k)       # file order, numbered from 1
    for i in (1, 2):
        rec = files[f"kmer-counter-many/kmers/component_{i}.kmers.bin"]
        keys = [struct.unpack(">QH", rec[j:j + 10]) for j in range(0, len(rec), 10)]
        assert [x for x, _ in keys] == sorted(comps[i - 1]) and all(c == 1 for _, c in keys)
        assert files[f"kmer-counter-many/stats/component_{i}.stat.txt"] == b"# k-mer frequency\tnumber of such k-mers\n1\t3\n\n"
        assert files[f"seq-builder-many/sequences/component_{i}.seq.fasta"].startswith(b">1 length=7 av_weight=1 min_weight=1 max_weight=1\n")   # numbered from 1 in EVERY file
    one = R.expected_files(oracle, comps, k, split=False)
    assert sorted(one) == ["kmer-counter-many/kmers/component.kmers.bin", "kmer-counter-many/stats/component.stat.txt", "kmers_fasta/component.fasta",
                           "seq-builder-many/sequences/component.seq.fasta"]
    assert one["kmers_fasta/component.fasta"].decode().split("\n")[0::2][:6] == [">1_1", ">1_2", ">1_3", ">2_1", ">2_2", ">2_3"]
    assert one["seq-builder-many/sequences/component.seq.fasta"].startswith(b">1 length=10 ")


def test_the_case_builders():
    k, comps = R.case_adjacent(21)
    assert [len(c) for c in comps] == [5, 4, 3]
    k, comps = R.case_shared()
    assert len(set(comps[0]) & set(comps[1])) == 1
    k, comps = R.case_dense()
    assert len(comps) == 7 and sum(len(c) for c in comps) == 542 and len({x for c in comps for x in c}) == 512
    k, comps = R.case_palindromes()
    assert k == 20 and len(comps[1]) == 1 and R.canon(comps[1][0], k) == comps[1][0]
    k, comps = R.case_shapes()
    assert len(comps[1]) == 1 and len(comps[2]) == 15 and len(comps[3]) == 10 and len(set(comps[3])) == 9
    k, comps = R.case_long()
    assert len(comps) == 51 and len(comps[0]) == 5000
    k, comps = R.case_many()
    assert len(comps) == 3000 and all(1 <= len(c) <= 40 for c in comps)
    k, comps = R.case_singles()
    assert len(comps) == 70000 > 2 ** 16 and all(len(c) == 1 for c in comps)


def test_write_components_is_the_loaders_format(tmp_path):
    p = tmp_path / "c.bin"
    R.write_components(p, [[5, 6], [7]])
    raw = p.read_bytes()
    assert raw == struct.pack(">I", 2) + struct.pack(">Iq", 2, 2) + struct.pack(">QQ", 5, 6) + struct.pack(">Iq", 1, 1) + struct.pack(">Q", 7)
    assert np.frombuffer(raw[16:32], dtype=">u8").tolist() == [5, 6]

"""The sharded component cutter (metafast_amd/csrc/mf_cc.hip: the k_dcc_* kernels and mf_dcc_*, mf_cut_components_of_shard,
mf_cut_components_sharded; metafast_amd/pipeline.py: distributed_components) on the crafted k-mer graphs of tests/dcc_cases.py, over
2, 4 and 8 virtual ranks (threads of this process, a context each on the one GPU, the library's local communicator).

tests/test_dcc_cases_cpu.py has shown on the oracle alone that every case reaches what it was made for: ties in (size, weight) that
only the smallest k-mer orders; components of exactly b1 - 1, b1, b1 + 1, b2 - 1, b2, b2 + 1 k-mers with b1 < b2, b1 == b2, b2 < b1;
components of one k-mer with b1 = 1, on fewer k-mers than ranks too; one path of 29 970 k-mers that changes rank at every change of
the minimizer, kept whole or emptied by the thresholds; a ladder of six threshold levels that leaves something at each; runs, periods
and a cycle (a k-mer that is its own neighbour, k-mers that are their own reverse complement).  ties, ladder and low_complexity run at
k = 20 (the smallest k with minimizer partitions), 21, 22, 25 (13-mer minimizers up to here), 26, 30 and 31; the others at 31 and 21.

Every run is held against three things, bit for bit -- no tolerance anywhere:
  * the oracle's components of the same sequences: (size, weight, threshold) in the oracle's order, every component's k-mers;
  * the other ranks: the same export on every rank, order included;
  * mf_cut_components_device on the whole table of the same sequences.
The shards must partition the oracle's table (lengths sum to the protocol's vertex count, keys disjoint, union = the oracle's keys), and
the case must really be distributed: which rank owns which k-mer of a kept component is read off the shards' keys."""
import numpy as np
import pytest

import dcc_cases as D
from dcc_util import _oracle_of_sequences, _virtual_ranks

pytestmark = pytest.mark.gpu

WORLDS = (2, 4, 8)
SPREAD = ("ties", "ladder", "long_path_whole")              # a kept component of these must lie on several ranks
WITH_OPTIONS = ("ties", "ladder") + tuple(f"bounds_{b1}_{b2}" for b1, b2 in D.BOUNDS)

RUNS = [(name, k, w) for k in D.BOTH_K for name in list(D.SWEEP) + list(D.OTHER) for w in WORLDS]
RUNS += [(name, k, 4) for k in D.SWEEP_K if k not in D.BOTH_K for name in D.SWEEP]
RUNS += [(name, k, 8) for k in D.BOTH_K for name in D.FEW]

_REF = {}


def _reference(oracle, gpu_ctx, name, k):
    """once per (case, k): the case, the oracle's keys and components, mf_cut_components_device's components"""
    if (name, k) not in _REF:
        from util import to_device
        case = D.by_name(name, k)
        table, want = _oracle_of_sequences(oracle, case.seqs, k, case.l, case.b1, case.b2)
        keys = table.export()[0]
        bases, offsets = D.pack(case.seqs)
        db, do = to_device(bases, offsets)
        whole = gpu_ctx.count_device(db.data_ptr(), do.data_ptr(), len(offsets) - 1, len(bases), k, case.l)
        assert np.array_equal(whole.export()[0], keys)
        comps = gpu_ctx.cut_components(whole, case.b1, case.b2)
        single = comps.export()
        comps.close(); whole.close()
        for a in [keys] + [c[3] for c in want] + [c[3] for c in single]:
            a.setflags(write=False)
        _REF[name, k] = (case, keys, want, single)
    return _REF[name, k]


def _same(got, want, what, sort=False):
    """(size, weight, threshold) in order and the k-mers of every component"""
    assert [c[:3] for c in got] == [c[:3] for c in want], what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g[3].dtype == w[3].dtype == np.uint64, what
        assert np.array_equal(np.sort(g[3]) if sort else g[3], w[3]), (what, "component", i)


def _check_results(res, want, single, what):
    for rank, r in enumerate(res):
        assert r[0] != "abort", (what, rank, r)
    for rank, (comps, _) in enumerate(res):
        _same(comps, want, (what, "rank", rank, "against the oracle"), sort=True)
        _same(comps, res[0][0], (what, "rank", rank, "against rank 0"))
        _same(comps, single, (what, "rank", rank, "against mf_cut_components_device"))


def _owners(res, keys, what):
    """the shards partition the table -> the rank that owns every k-mer of keys"""
    shards = [info["shard_keys"] for _, info in res]
    assert all(info["shard_len"] == len(s) for s, (_, info) in zip(shards, res)), what
    assert sum(len(s) for s in shards) == len(keys), what
    assert all(info["vertices"] == len(keys) for _, info in res), what
    allk = np.concatenate(shards)
    assert len(np.unique(allk)) == len(allk), what                      # disjoint
    assert np.array_equal(np.sort(allk), keys), what                    # their union: the oracle's table
    owner = np.full(len(keys), -1, dtype=np.int64)
    for rank, s in enumerate(shards):
        owner[np.searchsorted(keys, s)] = rank
    assert owner.min() >= 0
    return owner


@pytest.mark.parametrize("name,k,world", RUNS)
def test_crafted_case(oracle, gpu_ctx, name, k, world):
    case, keys, want, single = _reference(oracle, gpu_ctx, name, k)
    what = (name, k, world)
    res = _virtual_ranks(world, None, case.b1, case.b2, k=k, l=case.l, seqs=case.seqs)
    _check_results(res, want, single, what)
    owner = _owners(res, keys, what)
    on = [len(np.unique(owner[np.searchsorted(keys, c[3])])) for c in want]          # ranks a kept component lies on
    print(what, "levels", [info["levels"] for _, info in res], "shards", [info["shard_len"] for _, info in res], "most ranks of a kept component", max(on, default=0))
    if name in SPREAD:
        assert max(on) == world if world == 2 else max(on) >= 2, (what, on)
    if name in D.FEW:
        assert min(info["shard_len"] for _, info in res) == 0, what     # ranks that own nothing from the first level on
    if name == "ladder":
        assert all(info["levels"] == case.want["levels"] for _, info in res), what


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", WITH_OPTIONS)
def test_crafted_case_sparse_setup(oracle, gpu_ctx, name, world):
    """option dcc_sparse: after the first level the arrays over all vertex ids are reset only where the level's pairs and the rank's own
    fragment roots touch them, at every level"""
    case, keys, want, single = _reference(oracle, gpu_ctx, name, 31)
    res = _virtual_ranks(world, None, case.b1, case.b2, k=31, l=case.l, seqs=case.seqs, options={"dcc_sparse": 1})
    _check_results(res, want, single, (name, world, "dcc_sparse"))
    _owners(res, keys, (name, world, "dcc_sparse"))
    if name == "ladder":
        assert all(info["levels"] == case.want["levels"] for _, info in res)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", WITH_OPTIONS)
def test_crafted_case_in_one_call(oracle, gpu_ctx, name, world):
    """mf_cut_components_sharded: the sequences dealt round-robin to the ranks (a stretch and the sequence it repeats come from
    different ranks; with more ranks than sequences some bring none), gathered, counted and cut in one call"""
    case, keys, want, single = _reference(oracle, gpu_ctx, name, 31)
    res = _virtual_ranks(world, None, case.b1, case.b2, k=31, l=case.l, seqs=case.seqs, one_call=True)
    _check_results(res, want, single, (name, world, "one call"))
    assert all(info["kind"] == "local" for _, info in res)

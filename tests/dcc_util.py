"""Helpers of the sharded cutter's tests (tests/test_distributed_gpu.py, tests/test_dcc_crafted_gpu.py): W ranks as THREADS of one
process, a context each on the one GPU, on the library's local communicator (mf_comm_create_local) -- what metafast.sh --devices a,b,...
runs; on a multi-GPU box the same copies cross xGMI -- and the oracle's components of the same input."""
import numpy as np


def _virtual_ranks(world, inputs, b1, b2, k=31, b=1, l=100, fail_rank=None, fail_at=None, options=None, one_call=False, seqs=None):
    """inputs: (bases, offsets) host arrays of the samples; their unitigs (count -> filter b -> unitigs of at least l bases) are what the
    cutter gets.  seqs (a list of str, inputs = None): these sequences are the "unitigs" as they are, every one a sample of its own.
    one_call=False: every rank counts its shard of ALL sequences itself (min_len = l) and runs mf_cut_components_of_shard (failures
    can be injected: fail_at = "shard" / "merge" / "merge:3" / "level_local:3"); one_call=True: rank r holds the sequences of samples
    r, r + W, ... and calls mf_cut_components_sharded (gather + shard count + protocol in one call).
    -> per rank (components export, info) or ("abort", message); with one_call=False info has shard_len, and with seqs shard_keys (the rank's k-mers)"""
    import threading
    import torch
    from util import to_device
    from metafast_amd import lib as L, pipeline as P
    ctx0 = L.Context(0)
    per_sample = []
    if seqs is not None:
        assert inputs is None
        for s in seqs:
            sb = torch.from_numpy(np.frombuffer(s.encode(), dtype=np.uint8).copy()).to("cuda")
            per_sample.append((sb, torch.tensor([0, len(s)], dtype=torch.int64, device="cuda"), len(s)))
    else:
        for bases, offsets in inputs:
            db, do = to_device(bases, offsets)
            t = ctx0.count_device(db.data_ptr(), do.data_ptr(), len(offsets) - 1, len(bases), k, 0)
            g = t.filter(b)
            sq = ctx0.build_unitigs(g, b, l)
            v = sq.device_view()
            per_sample.append((P.device_tensor(v["bases"], v["n_bases"], "cuda").clone(), P.device_tensor(v["offsets"], (v["n"] + 1) * 8, "cuda").view(torch.int64).clone(), v["n_bases"]))
            sq.close(); g.close(); t.close()

    def cat(samples):
        bs, os_, nb = [], [], 0
        for sb, so, n in samples:
            bs.append(sb); os_.append(so[:-1] + nb); nb += n
        allb = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        if bs:
            allb[:nb] = torch.cat(bs)
        allo = torch.cat(os_ + [torch.tensor([nb], dtype=torch.int64, device="cuda")])
        return allb, allo, nb
    allb, allo, nb = cat(per_sample)
    mine = [cat(per_sample[r::world]) for r in range(world)]
    torch.cuda.synchronize()
    ctxs = [L.Context(0) for _ in range(world)]
    comms = L.Comm.local(ctxs)
    out, errs = [None] * world, []

    def work(rank):
        try:
            torch.cuda.set_device(0)
            ctx, comm = ctxs[rank], comms[rank]
            ctx.bind_thread()
            for name, val in (options or {}).items():
                ctx.set_option(name, val)
            if one_call:
                mb, mo, mnb = mine[rank]
                try:
                    comps = comm.cut_components_sharded(mb.data_ptr(), mo.data_ptr(), int(mo.numel()) - 1, mnb, k, l, b1, b2)
                except L.DistAbort as e:
                    out[rank] = ("abort", str(e))
                    return
                out[rank] = (comps.export(), dict(comm.stats(), kind=comm.kind))
                return
            shard = ctx.count_device_shard(allb.data_ptr(), allo.data_ptr(), int(allo.numel()) - 1, nb, k, l, rank, world)
            shard_keys = shard.export()[0] if seqs is not None else None
            info = {}
            if rank == fail_rank and fail_at == "shard":
                shard = None                                     # (the count failed on this rank)
            elif rank == fail_rank and fail_at:                  # (the n-th call of a library function inside the protocol fails on this rank only)
                which, _, nth = fail_at.partition(":")
                ctx.set_option("dcc_test_fail", {"merge": 1000, "level_local": 2000}[which] + int(nth or 1))
            try:
                comps = P.distributed_components(ctx, comm, shard, k, b1, b2, info=info)
            except L.DistAbort as e:
                out[rank] = ("abort", str(e))
                return
            info["shard_len"] = len(shard)
            if shard_keys is not None:
                info["shard_keys"] = shard_keys
            out[rank] = (comps.export(), info)
        except BaseException as e:          # (a rank that dies must not leave the others waiting: the barrier gives up after a while)
            errs.append(e)

    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for c in comms:
        c.close()
    if errs:
        raise errs[0]
    return out


def _oracle_components(oracle, inputs, b1, b2, k=31, b=1, l=100):
    o_cutter = oracle.Table()
    for bases, offsets in inputs:
        t = oracle.Table().count_buffer(bases, offsets, k)
        keys, vals = t.export(b)
        g = oracle.Table()
        for kk, vv in zip(keys.tolist(), vals.tolist()):
            g.add(kk, vv)
        o_cutter.count_seqs(oracle.build_unitigs(g, k, b, l), k, l)
    return oracle.cut_components(o_cutter, k, b1, b2).all()


def _oracle_of_sequences(oracle, seqs, k, l, b1, b2):
    """the cutter's table of the given sequences and its components: Table.count_seqs counts the oracle's own unitigs sequence by sequence
    with count_buffer(.., k, min_len = l); the same call on sequences that come as strings -> (Table, Comps.all())"""
    from dcc_cases import pack
    bases, offsets = pack(seqs)
    table = oracle.Table().count_buffer(bases, offsets, k, l)
    return table, oracle.cut_components(table, k, b1, b2).all()

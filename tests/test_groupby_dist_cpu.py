"""CPU-side checks of the two-stage GROUP BY (partial agg -> hash Motion of
the partial groups by group key -> combine agg, cdbgroupingpaths.c:251):
the library exports the new entry points, the ctypes mirror of gx_gb_stats
matches the C struct, and a gloo replay pins the orchestration
gx_groupby_dist performs with RCCL on GPUs."""
import ctypes
import os
import sys

import numpy as np
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(ROOT, "cloudberry_amd", "libgpuexec.so")


def _build_if_needed():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()


def test_groupby_dist_symbols_exported():
    _build_if_needed()
    lib = ctypes.CDLL(SO)
    for n in ("gx_groupby_dist", "gx_test_gb_partial", "gx_test_gb_combine"):
        assert hasattr(lib, n), f"symbol {n} not exported"


def test_gb_stats_ctypes_size_matches_c():
    _build_if_needed()
    import cloudberry_amd as gx_pkg
    lib = gx_pkg.lib()
    lib.gx_abi_sizeof.restype = ctypes.c_int64
    lib.gx_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.gx_abi_sizeof(6) == ctypes.sizeof(gx_pkg._GbStats) == 72
    # the numpy wire-row dtype mirrors gx_kv_group (kind 2)
    assert lib.gx_abi_sizeof(2) == gx_pkg.KV_GROUP_DTYPE.itemsize == 32


# ---------------- gloo replay of partial -> Motion -> combine ----------------

N_ROWS = 20000


def _global_input():
    """Same seeded table on every rank: group key (15% NULL), integer-valued
    f64 measure (10% NULL; every summation order is exact) and a separate
    distribution column that is NOT the group key."""
    rng = np.random.default_rng(73)
    keys = rng.integers(-50, 2000, N_ROWS).astype(np.int64)
    knull = rng.random(N_ROWS) < 0.15
    vals = rng.integers(-1000, 1001, N_ROWS).astype(np.float64)
    vnull = rng.random(N_ROWS) < 0.10
    dist_col = rng.integers(1, 10**6, N_ROWS).astype(np.int64)
    return keys, knull, vals, vnull, dist_col


def _np_groupby(keys, knull, vals, vnull):
    """numpy GROUP BY key, COUNT(*), SUM(val): NULL keys form one group
    (last), SUM skips NULL inputs.  Returns wire-row arrays."""
    k, inv = np.unique(keys[~knull], return_inverse=True)
    cnt = np.bincount(inv, minlength=len(k)).astype(np.int64)
    w = np.where(vnull[~knull], 0.0, vals[~knull])
    sm = np.bincount(inv, weights=w, minlength=len(k)).astype(np.float64)
    isnull = np.zeros(len(k), np.uint8)
    if knull.any():
        k = np.append(k, 0)
        cnt = np.append(cnt, int(knull.sum()))
        sm = np.append(sm, vals[knull & ~vnull].sum())
        isnull = np.append(isnull, np.uint8(1))
    return {"key": k, "key_is_null": isnull, "sum": sm, "count": cnt}


def _np_combine(rows):
    """combine agg: sum += partial.sum, count += partial.count per key."""
    isnull = rows["key_is_null"].astype(bool)
    k, inv = np.unique(rows["key"][~isnull], return_inverse=True)
    cnt = np.bincount(inv, weights=rows["count"][~isnull],
                      minlength=len(k)).astype(np.int64)
    sm = np.bincount(inv, weights=rows["sum"][~isnull], minlength=len(k))
    out_null = np.zeros(len(k), np.uint8)
    if isnull.any():
        k = np.append(k, 0)
        cnt = np.append(cnt, int(rows["count"][isnull].sum()))
        sm = np.append(sm, rows["sum"][isnull].sum())
        out_null = np.append(out_null, np.uint8(1))
    return {"key": k, "key_is_null": out_null, "sum": sm, "count": cnt}


def _exchange(dist, arrays, dest, nsegs, rank):
    """counts all-gather, then pairwise payload send/recv with the self
    share bypassing the transport — the shape of the RCCL path."""
    counts = torch.tensor([int((dest == d).sum()) for d in range(nsegs)],
                          dtype=torch.int64)
    all_counts = [torch.zeros(nsegs, dtype=torch.int64) for _ in range(nsegs)]
    dist.all_gather(all_counts, counts)
    out = {}
    for k, v in arrays.items():
        chunks = [torch.from_numpy(np.ascontiguousarray(v[dest == d]))
                  for d in range(nsegs)]
        recv = []
        for src in range(nsegs):
            if src == rank:
                recv.append(chunks[rank])
                continue
            buf = torch.zeros(int(all_counts[src][rank]), dtype=chunks[0].dtype)
            if rank < src:
                dist.send(chunks[src], dst=src)
                dist.recv(buf, src=src)
            else:
                dist.recv(buf, src=src)
                dist.send(chunks[src], dst=src)
            recv.append(buf)
        out[k] = np.concatenate([b.numpy() for b in recv])
    return out


def _worker(rank, world, result_q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(29900 + 13 * world)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from oracle import pyapi as orc

    keys, knull, vals, vnull, dist_col = _global_input()
    mine = orc.route(dist_col, world) == rank       # shard by a non-group col
    part = _np_groupby(keys[mine], knull[mine], vals[mine], vnull[mine])

    # Motion: partial groups by route(group key); the NULL group routes as
    # cdbhash routes a NULL attribute (rotation only)
    dest = orc.route(part["key"], world)
    null_dest = orc.route_multi([[0]], [0], world, isnull=[[1]])[0]
    dest[part["key_is_null"] == 1] = null_dest
    got = _exchange(dist, part, dest, world, rank)

    res = _np_combine(got)
    result_q.put((rank, res, int(len(part["key"]))))
    dist.destroy_process_group()


def _run_two_stage(nsegs):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, nsegs, q)) for r in range(nsegs)]
    for p in procs:
        p.start()
    results, nparts = {}, 0
    for _ in range(nsegs):
        rank, res, npart = q.get(timeout=300)
        results[rank] = res
        nparts += npart
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    from oracle import pyapi as orc
    want = _np_groupby(*_global_input()[:4])
    # the shards overlap in keys, so the partials really collide
    assert nparts > len(want["key"])
    null_owner = orc.route_multi([[0]], [0], nsegs, isnull=[[1]])[0]
    body_keys = []
    for r in range(nsegs):
        res = results[r]
        isnull = res["key_is_null"].astype(bool)
        assert (orc.route(res["key"][~isnull], nsegs) == r).all()
        assert int(isnull.sum()) == (1 if r == null_owner else 0)
        if isnull.any():
            assert isnull[-1]                      # NULL group last
        assert (np.diff(res["key"][~isnull]) > 0).all()
        body_keys.append(res["key"][~isnull])
    allk = np.concatenate(body_keys)
    assert len(np.unique(allk)) == len(allk)       # ranks' key sets disjoint

    def body(res):
        m = ~res["key_is_null"].astype(bool)
        return res["key"][m], res["sum"][m], res["count"][m]
    k = np.concatenate([body(results[r])[0] for r in range(nsegs)])
    s = np.concatenate([body(results[r])[1] for r in range(nsegs)])
    c = np.concatenate([body(results[r])[2] for r in range(nsegs)])
    order = np.argsort(k)
    wk, ws, wc = body(want)
    np.testing.assert_array_equal(k[order], wk)
    np.testing.assert_array_equal(c[order], wc)
    np.testing.assert_array_equal(s[order], ws)    # integer-valued: exact
    own = results[null_owner]
    assert own["count"][-1] == want["count"][-1]
    assert own["sum"][-1] == want["sum"][-1]


def test_two_rank_gloo_two_stage_groupby_equals_global():
    _run_two_stage(2)


def test_four_rank_gloo_two_stage_groupby_equals_global():
    _run_two_stage(4)

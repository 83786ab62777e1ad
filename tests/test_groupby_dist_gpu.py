"""GPU tests of the two-stage GROUP BY (pytest -m gpu, real MI355X): partial
agg -> partition of the partial groups by route(group key) -> exchange ->
combine agg, against numpy and the oracle's bit-exact routing.

Except for the float test every measure is integer-valued f64, so every
summation order is exact and sums are asserted bit-equal."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

INT64_MIN = -2**63


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


def _ref(keys, knull, vals, vnull, hidden=None):
    """numpy GROUP BY key, COUNT(*), SUM(val) over the visible rows: NULL
    keys form one group, SUM skips NULL inputs, COUNT(*) counts them."""
    if hidden is not None:
        keys, knull, vals, vnull = (a[~hidden] for a in (keys, knull, vals, vnull))
    k, inv = np.unique(keys[~knull], return_inverse=True)
    cnt = np.bincount(inv, minlength=len(k)).astype(np.int64)
    w = np.where(vnull[~knull], 0.0, vals[~knull])
    sm = np.bincount(inv, weights=w, minlength=len(k)).astype(np.float64)
    return {"key": k, "sum": sm, "count": cnt,
            "null_count": int(knull.sum()),
            "null_sum": float(vals[knull & ~vnull].sum())}


def _make_input(val_rng=None):
    rng = np.random.default_rng(71)
    n = 40000
    keys = rng.integers(-50, 2000, n).astype(np.int64)
    knull = rng.random(n) < 0.15
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    vnull = rng.random(n) < 0.10
    if val_rng is not None:
        vals = val_rng.uniform(-5, 5, n)
    return keys, knull, vals, vnull


@pytest.fixture(scope="module")
def inp():
    """input (1) and its numpy reference, computed once and never modified"""
    cols = _make_input()
    for a in cols:
        a.setflags(write=False)
    return cols, _ref(*cols)


def _bind(c, orc, keys, knull, vals, vnull, hidden=None):
    n = len(keys)
    if n == 0:
        t = c.bind([(b"", 8, 0, 1), (b"", 8, 0, 1)])
    else:
        t = c.bind([(orc.aocs_encode_orig_nulls(keys, knull), 8, n, 1),
                    (orc.aocs_encode_orig_nulls(vals, vnull), 8, n, 1)])
    if hidden is not None and n:
        t.set_visimap(hidden)
    return t


def _null_dest(orc, nsegs):
    return int(orc.route_multi([[0]], [0], nsegs, isnull=[[1]])[0])


def _blocks(counts, rows):
    off = np.concatenate([[0], np.cumsum(counts)])
    return [rows[off[d]:off[d + 1]] for d in range(len(counts))]


def _two_stage(ctx, orc, cols, nsegs, hidden=None):
    """Simulated N-segment plan on one GPU: round-robin shards, partial agg
    + partition per shard, regroup the blocks by destination on the host
    (the exchange), combine per destination."""
    inbox = [[] for _ in range(nsegs)]
    nparts = 0
    for s in range(nsegs):
        shard = [a[s::nsegs] for a in cols]
        t = _bind(ctx, orc, *shard,
                  hidden=None if hidden is None else hidden[s::nsegs])
        counts, rows = ctx.test_gb_partial(t, 0, 1, nsegs)
        t.free()
        assert counts.sum() == len(rows)
        nparts += len(rows)
        for d, b in enumerate(_blocks(counts, rows)):
            inbox[d].append(b)
    return [ctx.test_gb_combine(np.concatenate(inbox[d]))
            for d in range(nsegs)], nparts


def _check_union(orc, per_dest, ref, nsegs, exact=True):
    owner = _null_dest(orc, nsegs)
    ks, ss, cs = [], [], []
    for d, res in enumerate(per_dest):
        isnull = res["key_is_null"]
        body = res["key"][~isnull]
        # each destination holds exactly the keys the Motion routes there
        assert (orc.route(body, nsegs) == d).all()
        np.testing.assert_array_equal(
            body, ref["key"][orc.route(ref["key"], nsegs) == d])
        want_null = 1 if (d == owner and ref["null_count"] > 0) else 0
        assert int(isnull.sum()) == want_null
        if want_null:
            assert isnull[-1]                       # NULL group last
            assert res["count"][-1] == ref["null_count"]
            if exact:
                assert res["sum"][-1] == ref["null_sum"]
            else:
                np.testing.assert_allclose(res["sum"][-1], ref["null_sum"],
                                           rtol=1e-9, atol=1e-9)
        ks.append(body); ss.append(res["sum"][~isnull]); cs.append(res["count"][~isnull])
    k, s, c = np.concatenate(ks), np.concatenate(ss), np.concatenate(cs)
    order = np.argsort(k, kind="stable")
    np.testing.assert_array_equal(k[order], ref["key"])
    np.testing.assert_array_equal(c[order], ref["count"])
    if exact:
        np.testing.assert_array_equal(s[order], ref["sum"])
    else:
        np.testing.assert_allclose(s[order], ref["sum"], rtol=1e-9, atol=1e-9)


def _check_single(res, ref):
    """one segment's complete result (nsegs == 1) against numpy, exact"""
    nn = 1 if ref["null_count"] > 0 else 0
    assert len(res["key"]) == len(ref["key"]) + nn
    m = len(ref["key"])
    np.testing.assert_array_equal(res["key"][:m], ref["key"])
    assert not res["key_is_null"][:m].any()
    np.testing.assert_array_equal(res["count"][:m], ref["count"])
    np.testing.assert_array_equal(res["sum"][:m], ref["sum"])
    if nn:
        assert res["key_is_null"][-1]
        assert res["count"][-1] == ref["null_count"]
        assert res["sum"][-1] == ref["null_sum"]


def _forced_motion(ctx, table):
    """groupby_dist through the FULL exchange branch by self-exchange"""
    ctx.comm_init(ctx.comm_unique_id())
    os.environ["GX_FORCE_MOTION"] = "1"
    try:
        return ctx.groupby_dist(table, 0, 1, stats=True)
    finally:
        del os.environ["GX_FORCE_MOTION"]


# ---------------- 1. partition routing and conservation ----------------

@pytest.mark.parametrize("nsegs", [1, 2, 3, 8])
def test_partition_routing_and_conservation(ctx, orc, inp, nsegs):
    cols, ref = inp
    t = _bind(ctx, orc, *cols)
    counts, rows = ctx.test_gb_partial(t, 0, 1, nsegs)
    t.free()
    assert len(counts) == nsegs
    assert counts.sum() == len(ref["key"]) + 1 == len(rows)
    assert not rows["_pad"].any()                    # deterministic wire bytes
    owner = _null_dest(orc, nsegs)
    nulls_seen = 0
    for d, b in enumerate(_blocks(counts, rows)):
        body = b[b["key_is_null"] == 0]
        assert (orc.route(body["key"], nsegs) == d).all()
        nn = int((b["key_is_null"] != 0).sum())
        assert nn == (1 if d == owner else 0)
        nulls_seen += nn
    assert nulls_seen == 1
    body = rows[rows["key_is_null"] == 0]
    order = np.argsort(body["key"], kind="stable")
    np.testing.assert_array_equal(body["key"][order], ref["key"])  # unique too
    np.testing.assert_array_equal(body["count"][order], ref["count"])
    np.testing.assert_array_equal(body["sum"][order], ref["sum"])
    nrow = rows[rows["key_is_null"] != 0][0]
    assert nrow["count"] == ref["null_count"]
    assert nrow["sum"] == ref["null_sum"]


# ---------------- 2. simulated N-segment two-stage plan ----------------

@pytest.mark.parametrize("nsegs", [2, 3])
def test_two_stage_plan_simulated(ctx, orc, inp, nsegs):
    cols, ref = inp
    per_dest, nparts = _two_stage(ctx, orc, cols, nsegs)
    # every shard holds most keys, so the partials really collide
    assert nparts > 1.5 * len(ref["key"])
    _check_union(orc, per_dest, ref, nsegs)


# ---------------- 3. combine merges duplicates ----------------

def test_combine_merges_duplicates(ctx):
    rows = np.zeros(8, gx.KV_GROUP_DTYPE)
    spec = [(7, 0, 1.5, 1), (-3, 0, 8.0, 2), (0, 1, 10.0, 4), (7, 0, 2.25, 2),
            (2**62, 0, -1.0, 1), (0, 0, 3.0, 5), (7, 0, -4.0, 3),
            (0, 1, -2.5, 1)]
    for i, (k, isnull, s, c) in enumerate(spec):
        rows[i]["key"], rows[i]["key_is_null"] = k, isnull
        rows[i]["sum"], rows[i]["count"] = s, c
    got = ctx.test_gb_combine(rows)
    np.testing.assert_array_equal(got["key"][:4], [-3, 0, 7, 2**62])
    np.testing.assert_array_equal(got["key_is_null"],
                                  [False, False, False, False, True])
    np.testing.assert_array_equal(got["sum"], [8.0, 3.0, -0.25, -1.0, 7.5])
    np.testing.assert_array_equal(got["count"], [2, 5, 6, 1, 5])
    empty = ctx.test_gb_combine(np.zeros(0, gx.KV_GROUP_DTYPE))
    assert len(empty["key"]) == 0 and len(empty["count"]) == 0


# ---------------- 4. full branch by self-exchange ----------------

def test_full_branch_self_exchange(ctx, orc, inp):
    cols, ref = inp
    t = _bind(ctx, orc, *cols)
    want = ctx.groupby(t, 0, 1)
    got, st = _forced_motion(ctx, t)
    for f in ("key", "key_is_null", "sum", "count"):
        np.testing.assert_array_equal(got[f], want[f])
    _check_single(got, ref)
    assert st["rows_in"] == len(cols[0])
    assert st["partial_groups"] == len(ref["key"]) + 1
    assert st["sent_rows"] == st["recv_rows"] == st["partial_groups"]
    assert st["final_groups"] == len(got["key"])

    # one-stage plan without the env var: same result, motion stats zero
    got1, st1 = ctx.groupby_dist(t, 0, 1, stats=True)
    for f in ("key", "key_is_null", "sum", "count"):
        np.testing.assert_array_equal(got1[f], want[f])
    for f in ("ms_partition", "ms_exchange", "ms_combine", "sent_rows",
              "recv_rows"):
        assert st1[f] == 0
    assert st1["final_groups"] == len(got1["key"])
    # without stats the call returns just the groups
    assert set(ctx.groupby_dist(t, 0, 1)) == set(want)
    t.free()


# ---------------- 5. edge shapes ----------------

def _edge_case(name):
    rng = np.random.default_rng(75)
    hidden = None
    if name in ("n0", "n1", "n63", "n65"):
        n = int(name[1:])
        keys = (rng.permutation(1000)[:n] - 500).astype(np.int64)
        knull = np.zeros(n, bool)
    elif name == "one_key":
        n = 5000
        keys = np.full(n, 123456789, np.int64)
        knull = np.zeros(n, bool)
    elif name == "all_null":
        n = 300
        keys = rng.integers(0, 50, n).astype(np.int64)
        knull = np.ones(n, bool)
    else:
        assert name == "visimap"
        n = 5000
        keys = rng.integers(0, 400, n).astype(np.int64)
        knull = rng.random(n) < 0.1
        hidden = rng.random(n) < 0.3
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    vnull = rng.random(n) < 0.10
    return (keys, knull, vals, vnull), hidden


@pytest.mark.parametrize("name", ["n0", "n1", "n63", "n65", "one_key",
                                  "all_null", "visimap"])
def test_edge_shapes(ctx, orc, name):
    cols, hidden = _edge_case(name)
    ref = _ref(*cols, hidden=hidden)
    per_dest, _ = _two_stage(ctx, orc, cols, 3, hidden=hidden)
    _check_union(orc, per_dest, ref, 3)

    t = _bind(ctx, orc, *cols, hidden=hidden)
    got, st = _forced_motion(ctx, t)
    t.free()
    _check_single(got, ref)
    assert st["sent_rows"] == st["recv_rows"] == st["final_groups"]


def test_table_larger_than_one_grid_pass(ctx, orc):
    """300k rows size the partial table at 2^20 slots, twice what the
    2048x256-thread grid covers in one pass: every workgroup of the
    partition kernels loops and claims for slots of both passes."""
    rng = np.random.default_rng(76)
    n = 300000
    keys = rng.integers(-3000, 3000, n).astype(np.int64)
    knull = rng.random(n) < 0.05
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    vnull = rng.random(n) < 0.10
    ref = _ref(keys, knull, vals, vnull)
    t = _bind(ctx, orc, keys, knull, vals, vnull)
    counts, rows = ctx.test_gb_partial(t, 0, 1, 3)
    per_dest = [ctx.test_gb_combine(b) for b in _blocks(counts, rows)]
    _check_union(orc, per_dest, ref, 3)
    got, st = _forced_motion(ctx, t)
    t.free()
    _check_single(got, ref)
    assert st["sent_rows"] == st["recv_rows"] == len(ref["key"]) + 1


# ---------------- 6. state and guard errors ----------------

def test_needs_comm_init(orc, inp):
    cols, _ = inp
    c2 = gx.Context(device=0, seg=0, nsegs=2)
    try:
        t = _bind(c2, orc, *(a[:1000] for a in cols))
        with pytest.raises(gx.GxError) as ei:
            c2.groupby_dist(t, 0, 1)
        assert ei.value.status == 7                  # GX_ERR_STATE
        assert "gx_comm_init" in str(ei.value)
        t.free()
    finally:
        c2.close()


def test_int64_min_key_rejected(ctx, orc):
    keys = np.array([5, INT64_MIN, 9], np.int64)
    vals = np.array([1.0, 2.0, 3.0])
    no = np.zeros(3, bool)
    t = _bind(ctx, orc, keys, no, vals, no)
    with pytest.raises(gx.GxError) as ei:
        ctx.groupby_dist(t, 0, 1)
    assert ei.value.status == 3 and "INT64_MIN" in str(ei.value)
    with pytest.raises(gx.GxError) as ei:
        ctx.test_gb_partial(t, 0, 1, 3)
    assert ei.value.status == 3 and "INT64_MIN" in str(ei.value)
    with pytest.raises(gx.GxError) as ei:
        _forced_motion(ctx, t)
    assert ei.value.status == 3 and "INT64_MIN" in str(ei.value)
    t.free()


def test_hbm_budget_guards(ctx, orc, inp, monkeypatch):
    cols, ref = inp
    t = _bind(ctx, orc, *cols)
    rows = np.zeros(40000, gx.KV_GROUP_DTYPE)
    rows["key"] = np.arange(40000)
    rows["count"] = 1
    monkeypatch.setenv("GX_HBM_BUDGET_MB", "1")
    with pytest.raises(gx.GxError) as ei:
        ctx.groupby_dist(t, 0, 1)
    assert ei.value.status == 5                      # GX_ERR_OOM
    assert "HBM budget" in str(ei.value) and "GB" in str(ei.value)
    with pytest.raises(gx.GxError) as ei:
        _forced_motion(ctx, t)
    assert ei.value.status == 5
    assert "HBM budget" in str(ei.value) and "GB" in str(ei.value)
    with pytest.raises(gx.GxError) as ei:
        ctx.test_gb_combine(rows)
    assert ei.value.status == 5
    assert "combine table needs" in str(ei.value) and "GB" in str(ei.value)
    monkeypatch.delenv("GX_HBM_BUDGET_MB")
    # the same calls run fine without the cap
    _check_single(ctx.groupby_dist(t, 0, 1), ref)
    assert len(ctx.test_gb_combine(rows)["key"]) == 40000
    t.free()


# ---------------- 7. float sums ----------------

def test_float_sums(ctx, orc):
    cols = _make_input(val_rng=np.random.default_rng(72))
    ref = _ref(*cols)
    per_dest, _ = _two_stage(ctx, orc, cols, 3)
    _check_union(orc, per_dest, ref, 3, exact=False)

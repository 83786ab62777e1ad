"""GPU tests of the two-stage descriptor GROUP BY (pytest -m gpu, real MI355X):
partial agg -> partition of the partial states by the owner of the group key
-> exchange -> combine agg, against the numpy group-by of gb_ref (NOT
DISTINCT grouping, strict aggregates, PG's float order for MIN / MAX), the
oracle's bit-exact routing, and gx_groupby_desc, which stays as it is.

Apart from the float-sum test every summed measure is integer-valued, so every
summation order is exact and results are asserted bit-equal."""
import numpy as np
import pytest

import gb_ref as G
from gb_ref import (bind as _bind, ref as _ref, same as _same, take as _take,
                    sorted_nulls_last as _sorted_nulls_last)

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


# ---------------- the simulated plan (binding and the numpy reference: gb_ref) ----------------

def _forced(ctx, t, keys, aggs, **kw):
    """groupby_desc_dist through the FULL exchange branch by self-exchange"""
    return G.forced(ctx, lambda: ctx.groupby_desc_dist(t, keys, aggs, stats=True, **kw))


def _widths(cols, keys):
    return [cols[c][0].itemsize for c in keys]


def _route(orc, keys, key_null, widths, nsegs):
    """owner of every (n, nkeys) key row by the oracle: hashint8 for a
    width-8 column, hashint4 for the narrower ones; a plain aggregate is
    gathered on segment 0"""
    if len(widths) == 0 or len(keys) == 0:
        return np.zeros(len(keys), np.int32)
    return orc.route_multi(np.where(key_null, 0, keys),
                           [0 if w == 8 else 1 for w in widths], nsegs,
                           isnull=np.asarray(key_null, np.uint8))


def _blocks(counts, rows):
    off = np.concatenate([[0], np.cumsum(counts)])
    return [rows[off[d]:off[d + 1]] for d in range(len(counts))]


def _shard(cols, s, nsegs):
    return [(v[s::nsegs], None if nl is None else nl[s::nsegs]) for v, nl in cols]


def _two_stage(ctx, orc, cols, keys, aggs, nsegs, quals=(), hidden=None, rle=()):
    """Simulated N-segment plan on one GPU: round-robin shards, partial agg
    + partition per shard, regroup the blocks by destination on the host
    (the exchange), combine per destination."""
    inbox = [[] for _ in range(nsegs)]
    nparts = 0
    for s in range(nsegs):
        t = _bind(ctx, orc, _shard(cols, s, nsegs),
                  hidden=None if hidden is None else hidden[s::nsegs], rle=rle)
        counts, rows = ctx.test_gbd_partial(t, keys, aggs, nsegs, quals=quals)
        t.free()
        assert len(counts) == nsegs and counts.sum() == len(rows)
        nparts += len(rows)
        for d, b in enumerate(_blocks(counts, rows)):
            inbox[d].append(b)
    return [ctx.test_gbd_combine(np.concatenate(inbox[d]), keys, aggs)
            for d in range(nsegs)], nparts


def _check_dests(orc, per_dest, ref, widths, nsegs, float_tol=None):
    """each destination holds exactly the reference's groups routed to it, in
    the reference's order (sorted, NULLS LAST per column); the destinations
    partition the reference, so their union is the reference"""
    owner = _route(orc, ref["keys"], ref["key_null"], widths, nsegs)
    total = 0
    for d, res in enumerate(per_dest):
        _same(res, _take(ref, owner == d), float_tol)
        assert _sorted_nulls_last(res)
        total += res["ngroups"]
    assert total == ref["ngroups"]


# ---------------- 1. partition routing and conservation ----------------

AGGS1 = [("count*", None), ("count", 4), ("sum", 4, True), ("sum", 5),
         ("min", 5), ("max", 4, True)]
KEYSETS = {1: [2], 2: [0, 2], 4: [3, 0, 1, 2]}


def _input1():
    rng = np.random.default_rng(211)
    n = 40000
    k8 = rng.integers(-3, 4, n).astype(np.int8)
    k32 = (rng.integers(-4, 5, n) * 100003).astype(np.int32)
    k64 = rng.choice(np.array([INT64_MIN, -2**40, -7, -1, 0, 1, 2**40 + 3],
                              np.int64), n)
    k16 = (rng.integers(-2, 3, n) * 300).astype(np.int16)
    f = rng.integers(-1000, 1001, n).astype(np.float64)
    m32 = rng.integers(-10**6, 10**6, n).astype(np.int32)
    cols = [(k8, rng.random(n) < 0.15), (k32, rng.random(n) < 0.15),
            (k64, rng.random(n) < 0.15), (k16, rng.random(n) < 0.15),
            (f, rng.random(n) < 0.10), (m32, rng.random(n) < 0.10)]
    for v, nl in cols:
        v.setflags(write=False)
        nl.setflags(write=False)
    return cols


@pytest.fixture(scope="module")
def inp1(ctx, orc):
    """input (1), bound once, with its references per key set"""
    cols = _input1()
    t = _bind(ctx, orc, cols)
    refs = {nk: _ref(cols, ks, AGGS1) for nk, ks in KEYSETS.items()}
    yield cols, t, refs
    t.free()


@pytest.mark.parametrize("nsegs", [1, 2, 3, 8])
@pytest.mark.parametrize("nk", [1, 2, 4])
def test_partition_routing_and_conservation(ctx, orc, inp1, nk, nsegs):
    cols, t, refs = inp1
    keys, ref = KEYSETS[nk], refs[nk]
    widths = _widths(cols, keys)
    counts, rows = ctx.test_gbd_partial(t, keys, AGGS1, nsegs)
    assert rows.dtype == gx.gbd_wire_dtype(keys, AGGS1)
    assert len(counts) == nsegs
    assert counts.sum() == len(rows) == ref["ngroups"]
    # deterministic wire bytes: flags 0 / 1, padding zero, NULL key words 0
    assert not rows["_pad"].any()
    assert rows["key_null"].max() <= 1 and rows["key_null"].any()
    assert (rows["keys"][rows["key_null"] != 0] == 0).all()
    # every row of block d routes to d
    block_of = np.repeat(np.arange(nsegs), counts)
    np.testing.assert_array_equal(
        _route(orc, rows["keys"], rows["key_null"], widths, nsegs), block_of)
    if nsegs > 1:
        assert (counts > 0).sum() > 1
    # key tuples are unique across the blocks, and they are the reference's
    tup = np.concatenate([rows["keys"], rows["key_null"].astype(np.int64)], axis=1)
    assert len(np.unique(tup, axis=0)) == len(rows)
    # the states themselves: combined as one destination they are the result
    _same(ctx.test_gbd_combine(rows, keys, AGGS1), ref)


# ---------------- 2. simulated N-segment two-stage plan ----------------

def _input3():
    rng = np.random.default_rng(233)
    n = 30000
    key = rng.integers(-3, 4, n).astype(np.int32)
    m8 = rng.integers(-128, 128, n).astype(np.int8)
    m32 = rng.integers(-2**31, 2**31, n).astype(np.int32)
    m64 = rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True)
    f = rng.integers(-5000, 5001, n).astype(np.float64)
    cols = [(key, None)]
    for v in (m8, m32, m64, f):
        nl = rng.random(n) < 0.10
        nl[key == 2] = True            # group 2: every input NULL
        cols.append((v, nl))
    return cols


AGGS3 = {
    "a": [("count*", None), ("count", 2), ("sum", 2), ("sum", 4, True),
          ("min", 4, True), ("max", 4, True), ("min", 1), ("max", 1)],
    "b": [("min", 2), ("max", 2), ("min", 3), ("max", 3), ("count", 4),
          ("sum", 1), ("count", 3), ("count*", None)],
}


@pytest.fixture(scope="module")
def inp3(ctx, orc):
    cols = _input3()
    t = _bind(ctx, orc, cols)
    refs = {k: _ref(cols, [0], a) for k, a in AGGS3.items()}
    whole = {k: ctx.groupby_desc(t, [0], a) for k, a in AGGS3.items()}
    t.free()
    return cols, refs, whole


@pytest.mark.parametrize("nsegs", [2, 3])
@pytest.mark.parametrize("which", ["a", "b"])
def test_two_stage_plan_simulated(ctx, orc, inp3, which, nsegs):
    cols, refs, whole = inp3
    aggs, ref = AGGS3[which], refs[which]
    _same(whole[which], ref)
    per_dest, nparts = _two_stage(ctx, orc, cols, [0], aggs, nsegs)
    # every shard holds every group, so the partials really collide
    assert nparts > 1.5 * ref["ngroups"]
    _check_dests(orc, per_dest, ref, [4], nsegs)
    _check_dests(orc, per_dest, whole[which], [4], nsegs)
    # the all-NULL group stays NULL through the combine, COUNT(*) still counts
    for res in per_dest:
        for g in np.nonzero(res["keys"][:, 0] == 2)[0]:
            for j, spec in enumerate(aggs):
                assert res["agg_null"][g, j] == (spec[0] in ("sum", "min", "max"))


# ---------------- 3. combine state edges ----------------

AGGS_EDGE = [("count*", None), ("count", 4), ("sum", 4), ("min", 2), ("max", 2),
             ("min", 3, True), ("max", 3, True), ("sum", 5, True)]
# state words of AGGS_EDGE: 1 + 1 + 2 + 2 + 2 + 2 + 2 + 2; SUM(int4) at word 2
EDGE_SUM_WORD = 2


def _edge_shards():
    """three hand-made shards over (k0 int64 NULLable, k1 int32, m64, f, m32,
    fs); one tuple per row: (k0 or None, k1, m64, f, m32, fs), None = NULL"""
    nan, inf = np.nan, np.inf
    N = None
    return [
        [   # shard 0
            (5, 1, N, N, N, N),                      # A: NULL here ...
            (6, 1, N, N, N, N),                      # B: NULL everywhere
            (7, 1, -5, 1.0, 10, 1.0),                # C: integer extremes
            (7, 1, INT64_MAX, 2.0, -3, 2.0),
            (8, 1, 0, nan, 1, 3.0),                  # D: float order
            (8, 1, 0, 1.5, N, N),
            (9, 1, 1, -0.0, 1, 1.0),                 # E: -0.0 is the max
            (10, 1, 1, nan, 1, 1.0),                 # F: only NaNs
            (0, 2, 1, 1.0, 1, 1.0),                  # keys 0, INT64_MIN,
            (N, 1, 2, 2.0, 2, 2.0),                  # (NULL, 1), (0, 1)
        ],
        [   # shard 1
            (5, 1, 40, 4.5, 7, 8.0),                 # A: ... non-NULL here
            (5, 1, -40, -4.5, 8, -3.0),
            (6, 1, N, N, N, N),
            (7, 1, INT64_MIN, 3.0, 2**31 - 1, 4.0),
            (8, 1, 0, -inf, 5, 6.0),
            (9, 1, 1, -2.0, N, 2.0),
            (10, 1, 1, nan, 1, 1.0),
            (INT64_MIN, 2, 3, 3.0, 3, 3.0),
            (0, 1, 4, 4.0, 4, 4.0),
            (N, 1, 5, 5.0, 5, 5.0),
        ],
        [   # shard 2
            (6, 1, N, N, N, N),
            (7, 1, -6, 0.5, -2**31, 16.0),
            (8, 1, 0, inf, 6, 7.0),
            (0, 1, 6, 6.0, 6, 6.0),
            (0, 2, 7, 7.0, 7, 7.0),
            (INT64_MIN, 2, 8, 8.0, 8, 8.0),
        ],
    ]


def _edge_cols(rows):
    dts = (np.int64, np.int32, np.int64, np.float64, np.int32, np.float64)
    cols = []
    for c, dt in enumerate(dts):
        nl = np.array([r[c] is None for r in rows], np.bool_)
        v = np.array([0 if r[c] is None else r[c] for r in rows], dt)
        cols.append((v, nl))
    return cols


def test_combine_state_edges(ctx, orc):
    shards = _edge_shards()
    parts = []
    for rows in shards:
        t = _bind(ctx, orc, _edge_cols(rows))
        counts, wire = ctx.test_gbd_partial(t, [0, 1], AGGS_EDGE, 1)
        t.free()
        assert counts.tolist() == [len(wire)]
        parts.append(wire)
    wire = np.concatenate(parts)
    ref = _ref(_edge_cols([r for s in shards for r in s]), [0, 1], AGGS_EDGE)
    assert len(wire) > ref["ngroups"] == 10
    got = ctx.test_gbd_combine(wire, [0, 1], AGGS_EDGE)
    _same(got, ref)
    # the same rows through the 8-byte slot word, and in another order
    _same(ctx.test_gbd_combine(wire, [0, 1], AGGS_EDGE, wide_rowid=True), got)
    _same(ctx.test_gbd_combine(wire[::-1], [0, 1], AGGS_EDGE), got)

    def group(k0, k0_null, k1):
        m = ((got["keys"][:, 0] == k0) & (got["key_null"][:, 0] == k0_null) &
             (got["keys"][:, 1] == k1))
        assert m.sum() == 1
        return int(np.nonzero(m)[0][0])
    val = lambda g: [a[g] for a in got["aggs"]]
    # A: all-NULL on one shard, values on another -> non-NULL
    a = group(5, False, 1)
    assert not got["agg_null"][a].any()
    assert val(a)[:5] == [3, 2, 15, -40, 40] and val(a)[5:] == [-4.5, 4.5, 5.0]
    # B: NULL on every shard; COUNT(*) still counts, COUNT(col) is 0
    b = group(6, False, 1)
    assert got["agg_null"][b].tolist() == [False, False] + [True] * 6
    assert val(b)[:2] == [3, 0]
    # C: integer MIN / MAX over negatives and both extremes; COUNT(col) adds
    c = group(7, False, 1)
    assert val(c)[:5] == [4, 4, 10 - 3 + 2**31 - 1 - 2**31, INT64_MIN, INT64_MAX]
    # D: NaN above +inf for MAX, -inf the MIN
    d = group(8, False, 1)
    assert val(d)[5] == -np.inf and np.isnan(val(d)[6])
    # E: -0.0 above -2.0;  F: only NaNs -> MIN is NaN as well
    e = group(9, False, 1)
    assert val(e)[5] == -2.0 and val(e)[6] == 0.0 and np.signbit(val(e)[6])
    f = group(10, False, 1)
    assert np.isnan(val(f)[5]) and np.isnan(val(f)[6])
    # 0, INT64_MIN, (NULL, 1) and (0, 1) stay four groups
    assert val(group(0, False, 2))[0] == 2
    assert val(group(INT64_MIN, False, 2))[0] == 2
    assert val(group(0, True, 1))[0] == 2
    assert val(group(0, False, 1))[0] == 2

    # SUM(int4) is int64 with two's-complement adds, in the combine as well:
    # one shard's state at INT64_MAX - 1 plus 15 from the other shards wraps
    bent = wire.copy()
    hit = np.nonzero((bent["keys"][:, 0] == 5) & (bent["key_null"][:, 0] == 0))[0]
    assert len(hit) == 2
    src = [i for i in hit if bent["acc"][i, EDGE_SUM_WORD + 1] != 0]
    assert len(src) == 1 and bent["acc"][src[0], EDGE_SUM_WORD] == 15
    other = [i for i in hit if i != src[0]][0]
    bent["acc"][other, EDGE_SUM_WORD] = INT64_MAX - 1
    bent["acc"][other, EDGE_SUM_WORD + 1] = 1
    res = ctx.test_gbd_combine(bent, [0, 1], AGGS_EDGE)
    g = int(np.nonzero((res["keys"][:, 0] == 5) & (res["keys"][:, 1] == 1))[0][0])
    assert res["aggs"][2][g] == INT64_MIN + 13 and not res["agg_null"][g, 2]

    # no rows: zero groups, for every key count
    for keys in ([], [0], [0, 1]):
        empty = np.zeros(0, gx.gbd_wire_dtype(keys, AGGS_EDGE))
        res = ctx.test_gbd_combine(empty, keys, AGGS_EDGE)
        assert res["ngroups"] == 0 and res["keys"].shape == (0, len(keys))
        assert all(len(x) == 0 for x in res["aggs"])


# ---------------- 4. plain aggregate over 3 segments ----------------

AGGS7 = [("count*", None), ("count", 1), ("sum", 1, True), ("min", 0),
         ("max", 0), ("sum", 2)]


def _plain_cols(n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64), None),
            (rng.integers(-50, 51, n).astype(np.float64), rng.random(n) < 0.1),
            (rng.integers(-2**31, 2**31, n).astype(np.int32), rng.random(n) < 0.1)]


def test_plain_aggregate_three_segments(ctx, orc):
    full, filtered, empty = _plain_cols(4321, 41), _plain_cols(999, 42), _plain_cols(0, 43)
    none = [(2, "<", -2**31)]                  # no int32 is below INT32_MIN
    parts = []
    for cols, quals in ((full, ()), (empty, ()), (filtered, none)):
        t = _bind(ctx, orc, cols)
        counts, rows = ctx.test_gbd_partial(t, [], AGGS7, 3, quals=quals)
        t.free()
        # exactly one state row per shard, gathered on segment 0
        assert counts.tolist() == [1, 0, 0] and len(rows) == 1
        assert rows.dtype.names == ("acc",)
        parts.append(rows)
    assert not parts[1]["acc"].any() and not parts[2]["acc"].any()
    got = ctx.test_gbd_combine(np.concatenate(parts), [], AGGS7)
    _same(got, _ref(full, [], AGGS7))
    assert got["ngroups"] == 1 and got["aggs"][0][0] == 4321
    # all shards empty: COUNTs 0, the others NULL
    res = ctx.test_gbd_combine(np.concatenate([parts[1], parts[2], parts[1]]),
                               [], AGGS7)
    assert res["ngroups"] == 1 and res["keys"].shape == (1, 0)
    assert res["agg_null"][0].tolist() == [False, False, True, True, True, True]
    assert [int(a[0]) for a in res["aggs"]] == [0] * 6
    # through the full branch: the one group, also over the empty table
    t = _bind(ctx, orc, full)
    f, st = _forced(ctx, t, [], AGGS7)
    _same(f, _ref(full, [], AGGS7))
    assert st["sent_rows"] == st["recv_rows"] == st["final_groups"] == 1
    t.free()
    t = _bind(ctx, orc, empty)
    f, st = _forced(ctx, t, [], AGGS7)
    _same(f, res)
    assert st["sent_rows"] == 1 and st["rows_in"] == 0
    t.free()


# ---------------- 5. full branch by self-exchange ----------------

def test_full_branch_self_exchange(ctx, inp1):
    cols, t, refs = inp1
    keys = KEYSETS[4]
    want = ctx.groupby_desc(t, keys, AGGS1)
    _same(want, refs[4])
    got, st = _forced(ctx, t, keys, AGGS1)
    _same(got, want)
    assert st["rows_in"] == len(cols[0][0])
    assert (st["sent_rows"] == st["recv_rows"] == st["partial_groups"]
            == st["final_groups"] == want["ngroups"])

    # one-stage plan without the variable: same result, motion stats zero
    got1, st1 = ctx.groupby_desc_dist(t, keys, AGGS1, stats=True)
    _same(got1, want)
    for f in ("ms_partition", "ms_exchange", "ms_combine", "sent_rows",
              "recv_rows"):
        assert st1[f] == 0
    assert st1["rows_in"] == len(cols[0][0])
    assert st1["partial_groups"] == st1["final_groups"] == want["ngroups"]
    # without stats the call returns just the groups
    _same(ctx.groupby_desc_dist(t, keys, AGGS1), want)


# ---------------- 6. edge shapes ----------------

AGGS6 = [("count*", None), ("sum", 1, True), ("min", 2), ("count", 1)]


def _edge_case(name):
    rng = np.random.default_rng(275)
    hidden, quals, rle, mask = None, (), (), None
    if name in ("n0", "n1", "n63", "n65"):
        n = int(name[1:])
        keys = (rng.permutation(1000)[:n] - 500).astype(np.int64)
        knull = None
    elif name == "one_key":
        n = 5000
        keys, knull = np.full(n, 123456789, np.int64), None
    elif name == "all_null":
        n = 300
        keys, knull = rng.integers(0, 50, n).astype(np.int64), np.ones(n, bool)
    elif name == "visimap_quals":
        n = 5000
        keys, knull = rng.integers(0, 400, n).astype(np.int64), rng.random(n) < 0.1
        hidden = rng.random(n) < 0.3
        quals = [(2, ">", -50), (3, "<=", 60)]
    else:
        assert name in ("fmt0", "rle")
        n = 6000
        keys = np.repeat(rng.integers(-300, 300, n // 20).astype(np.int64), 20)
        knull = None
        rle = (0,) if name == "rle" else ()
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    q32 = rng.integers(-100, 101, n).astype(np.int32)
    q8 = rng.integers(-128, 128, n).astype(np.int8)
    q32_null = rng.random(n) < 0.1 if name == "visimap_quals" else None
    cols = [(keys, knull), (vals, rng.random(n) < 0.10), (q32, q32_null), (q8, None)]
    if name == "visimap_quals":
        mask = ~hidden & ~q32_null & (q32 > -50) & (q8 <= 60)
        assert (~hidden & q32_null).any() and 0 < mask.sum() < (~hidden).sum()
    return cols, hidden, quals, rle, mask


@pytest.mark.parametrize("name", ["n0", "n1", "n63", "n65", "one_key", "all_null",
                                  "visimap_quals", "fmt0", "rle"])
def test_edge_shapes(ctx, orc, name):
    cols, hidden, quals, rle, mask = _edge_case(name)
    ref = _ref(cols, [0], AGGS6, mask)
    per_dest, _ = _two_stage(ctx, orc, cols, [0], AGGS6, 3, quals=quals,
                             hidden=hidden, rle=rle)
    _check_dests(orc, per_dest, ref, [8], 3)
    if name == "one_key":
        assert ref["ngroups"] == 1 and ref["aggs"][0][0] == 5000
    if name == "all_null":
        assert ref["ngroups"] == 1 and ref["key_null"].all()

    t = _bind(ctx, orc, cols, hidden=hidden, rle=rle)
    if name in ("fmt0", "rle"):
        assert t.nrows == 6000
    got, st = _forced(ctx, t, [0], AGGS6, quals=quals)
    t.free()
    _same(got, ref)
    assert st["sent_rows"] == st["recv_rows"] == st["final_groups"] == ref["ngroups"]
    assert st["rows_in"] == len(cols[0][0])


# ---------------- 7. more groups than one grid pass ----------------

def test_more_groups_than_one_grid_pass(ctx, orc):
    """about 550 000 groups: more than the 2048 x 256 threads of one pass, so
    the partition and the combine kernels loop"""
    rng = np.random.default_rng(276)
    n, nd = 600000, 550000
    k64 = rng.integers(-2**40, 2**40, nd).astype(np.int64)
    k32 = rng.integers(-2**31, 2**31, nd).astype(np.int32)
    pick = np.concatenate([np.arange(nd), rng.integers(0, nd, n - nd)])
    rng.shuffle(pick)
    cols = [(k64[pick], None), (k32[pick], None),
            (rng.integers(-2**31, 2**31, n).astype(np.int32), rng.random(n) < 0.1)]
    aggs = [("count*", None), ("sum", 2)]
    ref = _ref(cols, [0, 1], aggs)
    assert 2048 * 256 < ref["ngroups"] <= nd
    t = _bind(ctx, orc, cols)
    counts, rows = ctx.test_gbd_partial(t, [0, 1], aggs, 3)
    assert counts.sum() == len(rows) == ref["ngroups"] and (counts > 100000).all()
    per_dest = [ctx.test_gbd_combine(b, [0, 1], aggs) for b in _blocks(counts, rows)]
    _check_dests(orc, per_dest, ref, [8, 4], 3)
    want = ctx.groupby_desc(t, [0, 1], aggs)
    got, st = _forced(ctx, t, [0, 1], aggs)
    t.free()
    _same(want, ref)
    _same(got, want)
    assert st["sent_rows"] == st["recv_rows"] == st["final_groups"] == ref["ngroups"]


# ---------------- 8. many destinations ----------------

def test_many_destinations(ctx, orc):
    rng = np.random.default_rng(278)
    n = 12000
    cols = [(rng.integers(-1500, 1500, n).astype(np.int64), rng.random(n) < 0.05),
            (rng.integers(-9, 10, n).astype(np.float64), None)]
    aggs = [("count*", None), ("sum", 1, True)]
    ref = _ref(cols, [0], aggs)
    assert 2500 < ref["ngroups"] < 3500
    t = _bind(ctx, orc, cols)
    counts, rows = ctx.test_gbd_partial(t, [0], aggs, 2048)   # LDS arrays at the cap
    assert len(counts) == 2048 and counts.sum() == len(rows) == ref["ngroups"]
    np.testing.assert_array_equal(
        _route(orc, rows["keys"], rows["key_null"], [8], 2048),
        np.repeat(np.arange(2048), counts))
    assert (counts > 0).sum() > 1000
    _same(ctx.test_gbd_combine(rows, [0], aggs), ref)
    with pytest.raises(gx.GxError) as e:
        ctx.test_gbd_partial(t, [0], aggs, 2049)
    assert e.value.status == 3                        # GX_ERR_INVALID
    _same(ctx.groupby_desc_dist(t, [0], aggs), ref)   # still usable
    t.free()


# ---------------- 9. errors ----------------

GOOD = [("count*", None), ("sum", 1, True)]


@pytest.fixture(scope="module")
def inp9(ctx, orc):
    rng = np.random.default_rng(279)
    n = 40000
    cols = [((np.arange(n) % 10).astype(np.int64), None),          # 10 groups
            (rng.integers(-9, 10, n).astype(np.float64), None),
            (rng.integers(-9, 10, n).astype(np.int32), None)]
    t = _bind(ctx, orc, cols)
    yield cols, t, _ref(cols, [0], GOOD)
    t.free()


def test_needs_comm_init(orc, inp9):
    cols, _, _ = inp9
    c2 = gx.Context(device=0, seg=0, nsegs=2)
    try:
        t = _bind(c2, orc, [(v[:1000], nl) for v, nl in cols])
        with pytest.raises(gx.GxError) as e:
            c2.groupby_desc_dist(t, [0], GOOD)
        assert e.value.status == 7                    # GX_ERR_STATE
        assert "gx_comm_init" in str(e.value)
        # the one-stage operator on the same context still works
        assert c2.groupby_desc(t, [0], GOOD)["ngroups"] == 10
        t.free()
    finally:
        c2.close()


def test_max_groups_bounds_both_stages(ctx, inp9):
    cols, t, ref = inp9

    def bad(call):
        with pytest.raises(gx.GxError) as e:
            call()
        assert e.value.status == 3, e.value           # GX_ERR_INVALID
        assert "max_groups" in str(e.value), e.value
        _same(ctx.groupby_desc_dist(t, [0], GOOD), ref)           # still usable

    counts, rows = ctx.test_gbd_partial(t, [0], GOOD, 3, max_groups=10)
    assert counts.sum() == 10
    bad(lambda: ctx.test_gbd_partial(t, [0], GOOD, 3, max_groups=4))
    bad(lambda: ctx.test_gbd_combine(rows, [0], GOOD, max_groups=4))
    bad(lambda: ctx.test_gbd_combine(rows, [0], GOOD, max_groups=9))
    bad(lambda: _forced(ctx, t, [0], GOOD, max_groups=4))
    bad(lambda: ctx.groupby_desc_dist(t, [0], GOOD, max_groups=4))
    for mg in (10, 11, 0):
        _same(ctx.test_gbd_combine(rows, [0], GOOD, max_groups=mg), ref)
        _same(_forced(ctx, t, [0], GOOD, max_groups=mg)[0], ref)


def test_hbm_budget_guards(ctx, inp9, monkeypatch):
    cols, t, ref = inp9
    rows = np.zeros(40000, gx.gbd_wire_dtype([0], GOOD))
    rows["keys"][:, 0] = np.arange(40000)
    rows["acc"][:, 0] = 1
    monkeypatch.setenv("GX_HBM_BUDGET_MB", "1")
    for call in (lambda: ctx.groupby_desc_dist(t, [0], GOOD),
                 lambda: _forced(ctx, t, [0], GOOD),
                 lambda: ctx.test_gbd_combine(rows, [0], GOOD)):
        with pytest.raises(gx.GxError) as e:
            call()
        assert e.value.status == 5, e.value           # GX_ERR_OOM
        assert "HBM budget" in str(e.value) and "GB" in str(e.value)
    monkeypatch.delenv("GX_HBM_BUDGET_MB")
    # the same calls run fine without the cap
    _same(ctx.groupby_desc_dist(t, [0], GOOD), ref)
    _same(_forced(ctx, t, [0], GOOD)[0], ref)
    res = ctx.test_gbd_combine(rows, [0], GOOD)
    assert res["ngroups"] == 40000 and (res["aggs"][0] == 1).all()
    assert res["agg_null"][:, 1].all()


def test_descriptor_errors_keep_their_messages(ctx, inp9):
    cols, t, ref = inp9
    cases = [("column 3 out of range", dict(keys=[3])),
             ("SUM over a width-8 integer", dict(aggs=[("sum", 0)])),
             ("op 9", dict(quals=[(0, 9, 1)]))]
    for needle, kw in cases:
        args = dict(keys=[0], aggs=GOOD, quals=())
        args.update(kw)
        calls = [lambda: ctx.groupby_desc(t, args["keys"], args["aggs"],
                                          quals=args["quals"]),
                 lambda: ctx.groupby_desc_dist(t, args["keys"], args["aggs"],
                                               quals=args["quals"]),
                 lambda: _forced(ctx, t, args["keys"], args["aggs"],
                                 quals=args["quals"]),
                 lambda: ctx.test_gbd_partial(t, args["keys"], args["aggs"], 3,
                                              quals=args["quals"])]
        msgs = []
        for call in calls:
            with pytest.raises(gx.GxError) as e:
                call()
            assert e.value.status == 3, e.value       # GX_ERR_INVALID
            assert needle in str(e.value), e.value
            msgs.append(str(e.value))
        assert len(set(msgs)) == 1                    # gx_groupby_desc's text
        _same(ctx.groupby_desc_dist(t, [0], GOOD), ref)           # still usable


# ---------------- 10. float sums ----------------

def test_float_sums(ctx, orc):
    rng = np.random.default_rng(71)
    n = 40000
    keys = rng.integers(-50, 2000, n).astype(np.int64)
    knull = rng.random(n) < 0.15
    rng.integers(-1000, 1001, n)                      # the integer measure's draw
    vnull = rng.random(n) < 0.10
    vals = np.random.default_rng(72).uniform(-5, 5, n)
    cols = [(keys, knull), (vals, vnull)]
    aggs = [("sum", 1, True), ("count*", None)]
    ref = _ref(cols, [0], aggs)
    per_dest, nparts = _two_stage(ctx, orc, cols, [0], aggs, 3)
    assert nparts > 1.5 * ref["ngroups"]
    _check_dests(orc, per_dest, ref, [8], 3, float_tol=1e-9)

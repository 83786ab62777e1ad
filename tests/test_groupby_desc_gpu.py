"""GPU tests of the descriptor-form GROUP BY (pytest -m gpu, real MI355X):
gx_groupby_desc and its test seam against the numpy group-by of gb_ref
(np.unique over a structured (null, value) view plus masked reductions), and
against gx_groupby / gx_q1, which stay as they are.

Apart from the float-order test and the Q1 cross-check every float8 measure is
integer-valued and small, so every summation order is exact and sums are
asserted bit-equal."""
import numpy as np
import pytest

import gb_ref as G
from gb_ref import (ref as _ref, same as _same, stream as _stream,
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


# ---------------- binding (the numpy reference: gb_ref) ----------------

def _bind(ctx, orc, cols, hidden=None):
    """cols: list of (values, nulls or None); an empty visimap is set too"""
    return G.bind(ctx, orc, cols, hidden, empty_hidden=True)


# ---------------- (1) key shapes, (6) the 8-byte slot word ----------------

AGGS1 = [("count*", None), ("count", 4), ("sum", 4, True), ("sum", 5),
         ("min", 5), ("max", 4, True)]
KEYSETS = {1: [2], 2: [0, 2], 3: [1, 0, 2], 4: [3, 0, 1, 2]}


def _input1():
    rng = np.random.default_rng(11)
    n = 20000
    k8 = rng.integers(-3, 4, n).astype(np.int8)
    k32 = (rng.integers(-4, 5, n) * 100003).astype(np.int32)
    k64 = rng.choice(np.array([-2**40, -7, -1, 0, 1, 2**40 + 3], np.int64), n)
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


@pytest.mark.parametrize("nk", [1, 2, 3, 4])
def test_key_shapes(ctx, inp1, nk):
    cols, t, refs = inp1
    # the value 0 stands beside NULL in every key column
    for c in KEYSETS[4]:
        assert ((cols[c][0] == 0) & ~cols[c][1]).any() and cols[c][1].any()
        assert (cols[c][0] < 0).any()
    res = ctx.groupby_desc(t, KEYSETS[nk], AGGS1)
    _same(res, refs[nk])
    assert _sorted_nulls_last(res)
    assert res["key_null"].any() and res["ngroups"] > 6


@pytest.mark.parametrize("grid", [0, 1])
def test_wide_rowid_same_result(ctx, inp1, grid):
    cols, t, refs = inp1
    narrow = ctx.test_groupby_desc(t, KEYSETS[4], AGGS1, grid=grid)
    wide = ctx.test_groupby_desc(t, KEYSETS[4], AGGS1, grid=grid, wide_rowid=True)
    _same(narrow, refs[4])
    _same(wide, narrow)


# ---------------- (2) no reserved key value ----------------

def test_reserved_values_are_plain_keys(ctx, orc):
    keys = np.tile(np.array([INT64_MIN, INT64_MAX, 0, -1], np.int64), 250)
    vals = np.arange(len(keys), dtype=np.float64)
    cols = [(keys, None), (vals, None)]
    t = _bind(ctx, orc, cols)
    aggs = [("count*", None), ("sum", 1, True)]
    for grid in (0, 1):
        res = ctx.test_groupby_desc(t, [0], aggs, grid=grid)
        _same(res, _ref(cols, [0], aggs))
        assert res["keys"][:, 0].tolist() == [INT64_MIN, -1, 0, INT64_MAX]
        assert (res["aggs"][0] == 250).all()
    t.free()


# ---------------- (3) every aggregate ----------------

def _input3():
    rng = np.random.default_rng(33)
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
    yield cols, t, refs
    t.free()


@pytest.mark.parametrize("grid", [0, 1, 3])
@pytest.mark.parametrize("which", ["a", "b"])
def test_every_aggregate(ctx, inp3, which, grid):
    cols, t, refs = inp3
    res = ctx.test_groupby_desc(t, [0], AGGS3[which], grid=grid)
    _same(res, refs[which])
    g2 = res["keys"][:, 0].tolist().index(2)
    for j, spec in enumerate(AGGS3[which]):
        strict = spec[0] in ("sum", "min", "max")
        assert res["agg_null"][g2, j] == strict
        assert res["aggs"][j][g2] == (0 if spec[0] != "count*" else
                                      (cols[0][0] == 2).sum())
    assert not np.delete(res["agg_null"], g2, axis=0).any()
    assert all((v < 0).any() for v, _ in cols)        # negative inputs


# ---------------- (4) float8 MIN / MAX order ----------------

def test_float_min_max_total_order(ctx, orc):
    nan, inf = np.nan, np.inf
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    groups = {
        0: [1.5, nan, -2.0, 7.25],            # NaN with finite values
        1: [nan, neg_nan, nan],               # only NaNs
        2: [inf, -inf, 3.0, -3.0],            # both infinities
        3: [-1.0, -1e300, -5e-324, -2.5],     # negative values only
        4: [-inf, neg_nan, -4.0],             # NaN above everything else
        5: [inf, 1e308],                      # +inf without NaN
        6: [0.0, 2.0, 5e-324],                # +0 (no group mixes -0 and +0)
        7: [-0.0, -2.0],
    }
    key = np.concatenate([[g] * len(v) for g, v in groups.items()]).astype(np.int64)
    val = np.concatenate(list(groups.values())).astype(np.float64)
    reps = 40                                   # enough rows for several waves
    key, val = np.tile(key, reps), np.tile(val, reps)
    nl = np.zeros(len(key), np.bool_)
    nl[::7] = True
    nl[:len(key) // reps] = False               # every value present once
    cols = [(key, None), (val, nl)]
    t = _bind(ctx, orc, cols)
    aggs = [("min", 1, True), ("max", 1, True)]
    ref = _ref(cols, [0], aggs)
    want_min = [-2.0, nan, -inf, -1e300, -inf, 1e308, 0.0, -2.0]
    want_max = [nan, nan, inf, -5e-324, nan, inf, 2.0, -0.0]
    for grid in (0, 1):
        res = ctx.test_groupby_desc(t, [0], aggs, grid=grid)
        assert not res["agg_null"].any()
        for j, want in ((0, want_min), (1, want_max)):
            got = res["aggs"][j]
            for g in range(8):
                if np.isnan(want[g]):
                    assert np.isnan(got[g]) and np.isnan(ref["aggs"][j][g])
                else:
                    assert got[g] == want[g] == ref["aggs"][j][g]
    t.free()


# ---------------- (5) LDS capacity edges ----------------

AGGS5 = [("count*", None), ("sum", 1, True)]


def _edge_groups():
    """the group counts of the edge cases, by parameter name"""
    cap = gx.gb_lds_groups(len(AGGS5))
    return cap, {"one": 1, "cap-1": cap - 1, "cap": cap, "cap+1": cap + 1,
                 "4cap": 4 * cap}


@pytest.fixture(scope="module")
def inp5(ctx, orc):
    """one table per group count, bound once: 1, cap - 1, cap, cap + 1, 4 cap"""
    made = {}
    rng = np.random.default_rng(55)
    for ng in _edge_groups()[1].values():
        n = max(6 * ng, 5000)
        key = rng.integers(0, ng, n).astype(np.int64)
        key[:ng] = np.arange(ng)                # every group present
        key = (key - ng // 2) * 1000003         # spread, negative ones too
        val = rng.integers(-100, 101, n).astype(np.float64)
        cols = [(key, None), (val, rng.random(n) < 0.10)]
        made[ng] = (cols, _bind(ctx, orc, cols), _ref(cols, [0], AGGS5))
    yield made
    for _, t, _ in made.values():
        t.free()


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("which", ["one", "cap-1", "cap", "cap+1", "4cap"])
def test_lds_capacity_edges(ctx, inp5, monkeypatch, which, grid):
    cap, by_name = _edge_groups()
    ng = by_name[which]
    cols, t, ref = inp5[ng]
    assert ref["ngroups"] == ng
    monkeypatch.delenv("GX_GB_LDS", raising=False)
    res, st = ctx.test_groupby_desc(t, [0], AGGS5, grid=grid, stats=True)
    monkeypatch.setenv("GX_GB_LDS", "0")
    off, st_off = ctx.test_groupby_desc(t, [0], AGGS5, grid=grid, stats=True)
    _same(res, ref)
    _same(off, res)
    n = len(cols[0][0])
    for s in (st, st_off):
        assert s["rows_in"] == s["rows_pass"] == n
        assert s["rows_lds"] + s["rows_global"] == s["rows_pass"]
        assert s["groups"] == ng
    assert st_off["rows_lds"] == 0
    assert st["rows_lds"] > 0
    if ng == 1:
        assert st["rows_global"] == 0
    if which == "4cap" and grid == 1:
        # one workgroup's LDS table holds at most cap groups: every other
        # group sends at least one row to the global table
        assert st["rows_global"] >= ng - cap


# ---------------- (7) plain aggregates and empty inputs ----------------

AGGS7 = [("count*", None), ("count", 1), ("sum", 1, True), ("min", 0),
         ("max", 0), ("sum", 2)]


def _check_empty_plain(res):
    assert res["ngroups"] == 1 and res["keys"].shape == (1, 0)
    assert res["agg_null"][0].tolist() == [False, False, True, True, True, True]
    assert [int(a[0]) for a in res["aggs"]] == [0] * 6


def test_plain_aggregate_populated(ctx, orc):
    rng = np.random.default_rng(77)
    n = 12345
    cols = [(rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64), None),
            (rng.integers(-50, 51, n).astype(np.float64), rng.random(n) < 0.1),
            (rng.integers(-2**31, 2**31, n).astype(np.int32), rng.random(n) < 0.1)]
    t = _bind(ctx, orc, cols)
    for grid in (0, 1):
        res = ctx.test_groupby_desc(t, [], AGGS7, grid=grid)
        _same(res, _ref(cols, [], AGGS7))
    v, nl = cols[1]
    assert res["aggs"][0][0] == n and res["aggs"][1][0] == (~nl).sum()
    assert res["aggs"][2][0] == v[~nl].sum()
    assert res["aggs"][3][0] == cols[0][0].min()
    assert res["aggs"][4][0] == cols[0][0].max()
    assert res["aggs"][5][0] == cols[2][0][~cols[2][1]].astype(np.int64).sum()
    # every row filtered: still one group, counts 0, the others NULL
    _check_empty_plain(ctx.groupby_desc(t, [], AGGS7,
                                        quals=[(2, "<", -2**31)]))
    assert ctx.groupby_desc(t, [0], AGGS7, quals=[(2, "<", -2**31)])["ngroups"] == 0
    t.free()


def test_plain_aggregate_and_keys_over_empty_table(ctx):
    t = ctx.bind([(b"", 8, 0, 1), (b"", 8, 0, 1), (b"", 4, 0, 1)])
    _check_empty_plain(ctx.groupby_desc(t, [], AGGS7))
    res, st = ctx.groupby_desc(t, [0], AGGS7, stats=True)
    assert res["ngroups"] == 0 and res["keys"].shape == (0, 1)
    assert all(len(a) == 0 for a in res["aggs"])
    assert st["rows_in"] == st["rows_pass"] == st["groups"] == 0
    t.free()


# ---------------- (8) quals and visibility ----------------

def test_quals_and_visimap(ctx, orc):
    rng = np.random.default_rng(88)
    n = 40000
    key = rng.integers(-20, 21, n).astype(np.int32)
    q32 = rng.integers(-100, 101, n).astype(np.int32)
    q32_null = rng.random(n) < 0.15
    q8 = rng.integers(-128, 128, n).astype(np.int8)
    val = rng.integers(-9, 10, n).astype(np.float64)
    cols = [(key, rng.random(n) < 0.15), (q32, q32_null), (q8, None),
            (val, rng.random(n) < 0.10)]
    hidden = rng.random(n) < 0.20
    aggs = [("count*", None), ("sum", 3, True), ("count", 1), ("max", 2)]
    t = _bind(ctx, orc, cols, hidden=hidden)
    vis = ~hidden

    # two AND-ed quals; a NULL q32 fails the row
    mask = vis & ~q32_null & (q32 > 10) & (q8 <= 50)
    assert (vis & q32_null & (q8 <= 50)).any()
    for grid in (0, 1):
        res, st = ctx.test_groupby_desc(
            t, [0], aggs, quals=[(1, ">", 10), (2, "<=", 50)], grid=grid,
            stats=True)
        _same(res, _ref(cols, [0], aggs, mask))
        assert st["rows_in"] == n and st["rows_pass"] == mask.sum()

    # literals outside int8: folded to always-true ...
    for op, lit in (("<", 300), ("!=", 300), (">", -300), (">=", -129)):
        res = ctx.groupby_desc(t, [0], aggs, quals=[(2, op, lit)])
        _same(res, _ref(cols, [0], aggs, vis))
    # ... and to always-false
    for op, lit in (("==", 300), (">", 127 + 1), ("<", -300), ("<=", -129)):
        res = ctx.groupby_desc(t, [0], aggs, quals=[(2, op, lit)])
        assert res["ngroups"] == 0
    # the boundary literals themselves are in range and compare normally
    res = ctx.groupby_desc(t, [0], aggs, quals=[(2, "<", 127)])
    _same(res, _ref(cols, [0], aggs, vis & (q8 < 127)))

    # visimap cleared: every row again
    t.set_visimap(None)
    _same(ctx.groupby_desc(t, [0], aggs), _ref(cols, [0], aggs))
    t.free()


# ---------------- (9) formats ----------------

def test_same_input_in_three_formats(ctx, orc):
    rng = np.random.default_rng(99)
    n = 50000
    key = np.repeat(rng.integers(-500, 500, n // 25).astype(np.int64), 25)  # runs
    k8 = rng.integers(-5, 6, n).astype(np.int8)
    val = rng.integers(-1000, 1001, n).astype(np.float64)
    cols = [(key, None), (k8, None), (val, None)]
    aggs = [("count*", None), ("sum", 2, True), ("min", 2, True), ("max", 1)]
    ref = _ref(cols, [0, 1], aggs)
    no = np.zeros(n, np.bool_)
    binds = {
        "orig": [_stream(orc, v) for v, _ in cols],
        "orig_nulls": [_stream(orc, v, no) for v, _ in cols],
        "rle_key": [_stream(orc, key, rle=True), _stream(orc, k8),
                    _stream(orc, val)],
    }
    assert [s[3] for s in binds["orig"]] == [0, 0, 0]
    assert [s[3] for s in binds["orig_nulls"]] == [1, 1, 1]
    assert len(binds["rle_key"][0][0]) < len(binds["orig"][0][0]) // 4
    for name, streams in binds.items():
        t = ctx.bind(streams)
        for grid in (0, 3):
            _same(ctx.test_groupby_desc(t, [0, 1], aggs, grid=grid), ref)
        t.free()


# ---------------- (10) cross-checks against the code that stays ----------------

def test_matches_gx_groupby(ctx, orc):
    rng = np.random.default_rng(71)
    n = 40000
    keys = rng.integers(-50, 2000, n).astype(np.int64)
    knull = rng.random(n) < 0.15
    vals = rng.integers(-1000, 1001, n).astype(np.float64)
    vnull = rng.random(n) < 0.10
    t = _bind(ctx, orc, [(keys, knull), (vals, vnull)])
    old = ctx.groupby(t, 0, 1)
    new = ctx.groupby_desc(t, [0], [("sum", 1, True), ("count*", None)])
    t.free()
    assert new["ngroups"] == len(old["key"])
    np.testing.assert_array_equal(new["keys"][:, 0], old["key"])
    np.testing.assert_array_equal(new["key_null"][:, 0], old["key_is_null"])
    assert old["key_is_null"][-1] and not old["key_is_null"][:-1].any()
    np.testing.assert_array_equal(new["aggs"][1], old["count"])
    # gx_groupby reports SUM over no input as 0.0, not NULL
    got = np.where(new["agg_null"][:, 0], 0.0, new["aggs"][0])
    assert got.tobytes() == old["sum"].tobytes()      # bit for bit
    np.testing.assert_array_equal(new["agg_null"][:, 0],
                                  _ref([(keys, knull), (vals, vnull)], [0],
                                       [("sum", 1, True)])["agg_null"][:, 0])


def test_matches_gx_q1(ctx):
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, 0.01)
    cutoff = gx.CUTOFF_19950315
    q1 = ctx.q1(t, cutoff)
    res, st = ctx.groupby_desc(t, [0, 1], [("count*", None), ("sum", 2, True)],
                               quals=[(4, "<=", cutoff)], stats=True)
    t.free()
    assert 0 < st["rows_pass"] < st["rows_in"]
    assert not res["key_null"].any() and not res["agg_null"].any()
    slot = res["keys"][:, 0] * 2 + res["keys"][:, 1]
    assert (np.diff(slot) > 0).all()                  # (flag, status) ascending
    want = np.nonzero(q1["count"])[0]
    np.testing.assert_array_equal(slot, want)
    np.testing.assert_array_equal(res["aggs"][0], q1["count"][want])
    assert res["aggs"][0].sum() == st["rows_pass"]
    # f64 SUM tolerance of the project (BASELINE): 1e-6 relative
    np.testing.assert_allclose(res["aggs"][1], q1["sum_price"][want],
                               rtol=1e-6, atol=0)


# ---------------- (11) errors ----------------

def test_errors_name_the_item_and_leave_the_context_usable(ctx, orc):
    rng = np.random.default_rng(111)
    n = 3000
    k64 = (np.arange(n) % 10).astype(np.int64)        # 10 groups
    cols = [(k64, None), (rng.integers(-9, 10, n).astype(np.float64), None),
            (rng.integers(-9, 10, n).astype(np.int32), None)]
    t = _bind(ctx, orc, cols)
    good = [("count*", None), ("sum", 1, True)]
    ref = _ref(cols, [0], good)

    def bad(needle, keys=(0,), aggs=good, quals=(), max_groups=0):
        with pytest.raises(gx.GxError) as e:
            ctx.groupby_desc(t, list(keys), aggs, quals=quals,
                             max_groups=max_groups)
        assert e.value.status == 3, e.value            # GX_ERR_INVALID
        assert needle in str(e.value), e.value
        _same(ctx.groupby_desc(t, [0], good), ref)     # still usable

    bad("column 3 out of range", keys=(3,))
    bad("column -1 out of range", keys=(-1,))
    bad("column 7 out of range", aggs=[("sum", 7, True)])
    bad("column 9 out of range", quals=[(9, "<", 1)])
    bad("nkeys 5", keys=(0, 0, 0, 0, 0))
    bad("naggs 0", aggs=[])
    bad("naggs 9", aggs=[("count*", None)] * 9)
    bad("nquals 5", quals=[(0, "<", 1)] * 5)
    bad("SUM over a width-8 integer", aggs=[("sum", 0)])
    bad("is_f64 on a column of width 4", aggs=[("max", 2, True)])
    bad("unknown fn 5", aggs=[(5, 0)])
    bad("op 6", quals=[(0, 6, 1)])
    bad("more groups than max_groups", max_groups=4)
    for mg in (10, 0, 11):
        _same(ctx.groupby_desc(t, [0], good, max_groups=mg), ref)
    t.free()

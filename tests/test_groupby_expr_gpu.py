"""GPU tests of the descriptor GROUP BY's float8 expression aggregates and
float8 quals (pytest -m gpu, real MI355X): gx_groupby_expr, its test seam and
gx_groupby_expr_dist against the numpy group-by of gb_ref (with expression
columns and float8 quals),
against gx_groupby_desc and against gx_q1.

Summed inputs are quarter- and eighth-valued (price = k / 4, disc in {0, .25,
.5, .75}, tax in {0, .125, .25, .5}), so every product is exact, every partial
sum a multiple of 1/128 far below 2^53, every summation order gives the same
double and sums are asserted bit-equal.  MIN and MAX do not depend on order at
all, so the per-row test runs them over full-mantissa doubles."""
import os

import numpy as np
import pytest

import gb_ref as G
from gb_ref import (bind as _bind, expr_col as _expr_col, fq_mask as _fq_mask,
                    ref as _ref, same as _same, stream as _stream)

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


# ---------------- the Q1 / Q6 input ----------------
# columns: 0 flag i8, 1 status i8, 2 qty f8, 3 price f8, 4 disc f8, 5 tax f8,
# 6 ship i32

def _lineitem(n, seed):
    rng = np.random.default_rng(seed)
    flag = rng.integers(0, 3, n).astype(np.int8)
    status = rng.integers(0, 2, n).astype(np.int8)
    qty = rng.integers(1, 51, n).astype(np.float64)
    price = rng.integers(1, 4001, n).astype(np.float64) * 0.25
    disc = rng.choice(np.array([0.0, 0.25, 0.5, 0.75]), n)
    tax = rng.choice(np.array([0.0, 0.125, 0.25, 0.5]), n)
    ship = rng.integers(-3000, 0, n).astype(np.int32)
    cols = [(flag, None), (status, None), (qty, None), (price, None),
            (disc, None), (tax, None), (ship, None)]
    for v, _ in cols:
        v.setflags(write=False)
    return cols


Q1_KEYS = [0, 1]
Q1_AGGS = [("count*", None), ("sum", 2, True), ("sum", 3, True),
           ("sum", [3, ("1-", 4)]), ("sum", [3, ("1-", 4), ("1+", 5)]),
           ("sum", 4, True)]
Q1_CUT = -600
Q1_QUALS = [(6, "<=", Q1_CUT)]


@pytest.fixture(scope="module")
def li(ctx, orc):
    """the 6000-row lineitem-like input, bound once, with the Q1 reference"""
    cols = _lineitem(6000, 1)
    t = _bind(ctx, orc, cols)
    ref = _ref(cols, Q1_KEYS, Q1_AGGS, cols[6][0] <= Q1_CUT)
    yield cols, t, ref
    t.free()


def test_sums_of_this_input_do_not_depend_on_order():
    """the premise of every bit-equal SUM below, checked on the host"""
    cols = _lineitem(6000, 1)
    for factors in ([3, ("1-", 4)], [3, ("1-", 4), ("1+", 5)], [3, 4]):
        v, _ = _expr_col(cols, factors)
        assert (v * 128 == np.round(v * 128)).all() and v.sum() * 128 < 2**53
        rng = np.random.default_rng(2)
        sums = {float(np.sum(v[rng.permutation(len(v))])) for _ in range(5)}
        for _ in range(3):
            acc = 0.0
            for x in v[rng.permutation(len(v))]:
                acc += x
            sums.add(acc)
        assert sums == {float(np.sum(np.round(v * 128).astype(np.int64))) / 128}


# ---------------- (1) Q1 whole ----------------

@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("grid", [0, 1, 3])
def test_q1_whole(ctx, li, grid, wide):
    cols, t, ref = li
    assert ref["ngroups"] == 6
    res, st = ctx.test_groupby_expr(t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS,
                                    grid=grid, wide_rowid=wide, stats=True)
    _same(res, ref)
    want_pass = int((cols[6][0] <= Q1_CUT).sum())
    assert 0 < want_pass < len(cols[0][0])
    assert st["rows_in"] == len(cols[0][0]) and st["rows_pass"] == want_pass
    assert st["rows_lds"] + st["rows_global"] == st["rows_pass"]
    assert all(a.dtype == np.float64 for a in res["aggs"][1:])
    if grid == 1:
        assert st["rows_global"] == 0           # all of it through the LDS stage
    if grid == 0 and not wide:
        _same(ctx.groupby_expr(t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS), ref)


# ---------------- (2) Q6 whole ----------------

Q6_AGGS = [("sum", [3, 4]), ("count*", None)]
Q6_QUALS = [(6, ">=", -2000), (6, "<", -1000)]
Q6_FQUALS = [(4, ">=", 0.25), (4, "<=", 0.5), (2, "<", 24.0)]


def _q6_mask(cols):
    ship = cols[6][0]
    return (ship >= -2000) & (ship < -1000) & _fq_mask(cols, Q6_FQUALS)


def test_q6_whole(ctx, orc, li):
    cols, t, _ = li
    mask = _q6_mask(cols)
    assert 0 < mask.sum() < len(mask) // 4
    ref = _ref(cols, [], Q6_AGGS, mask)
    for grid in (0, 1):
        res, st = ctx.test_groupby_expr(t, [], Q6_AGGS, quals=Q6_QUALS,
                                        fquals=Q6_FQUALS, grid=grid, stats=True)
        _same(res, ref)
        assert res["ngroups"] == 1 and st["rows_pass"] == mask.sum()
    assert res["aggs"][1][0] == mask.sum() and not res["agg_null"].any()

    # an input the fquals filter completely: COUNT 0, SUM NULL, still one row
    gone = [c for c in cols]
    gone[4] = (np.full(len(cols[0][0]), 0.75), None)
    assert _q6_mask(gone).sum() == 0 and (gone[6][0] >= -2000).any()
    t2 = _bind(ctx, orc, gone)
    res, st = ctx.groupby_expr(t2, [], Q6_AGGS, quals=Q6_QUALS, fquals=Q6_FQUALS,
                               stats=True)
    t2.free()
    assert res["ngroups"] == 1 and st["rows_pass"] == 0
    assert res["aggs"][1][0] == 0 and res["aggs"][0][0] == 0
    assert res["agg_null"][0].tolist() == [True, False]

    # an empty table: the same one row; with keys, no group
    t3 = ctx.bind([(b"", v.itemsize, 0, 1) for v, _ in cols])
    res = ctx.groupby_expr(t3, [], Q6_AGGS, quals=Q6_QUALS, fquals=Q6_FQUALS)
    assert res["ngroups"] == 1 and res["aggs"][1][0] == 0
    assert res["agg_null"][0].tolist() == [True, False]
    assert ctx.groupby_expr(t3, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS)["ngroups"] == 0
    t3.free()


# ---------------- (3) per-row bit exactness ----------------

def test_per_row_values_are_bit_exact(ctx, orc):
    rng = np.random.default_rng(3)
    n, ng = 4000, 7
    key = rng.integers(0, ng, n).astype(np.int32)
    key[:ng] = np.arange(ng)

    def full_mantissa():
        return rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)
    a, b, c = full_mantissa(), full_mantissa(), full_mantissa()
    # group 1: a NaN among finite values; group 2: both infinities;
    # group 3: NaN and -inf; group 4: nothing but NaN
    a[np.nonzero(key == 1)[0][:3]] = np.nan
    g2 = np.nonzero(key == 2)[0]
    a[g2[0]], a[g2[1]] = np.inf, -np.inf
    b[g2[0]], b[g2[1]] = -1.0, -1.0            # keep inf * (1 - b) an infinity
    c[g2[0]], c[g2[1]] = 1.0, 1.0
    g3 = np.nonzero(key == 3)[0]
    b[g3[0]], a[g3[1]] = np.nan, -np.inf
    b[g3[1]], c[g3[1]] = -1.0, 1.0
    a[key == 4] = np.nan
    cols = [(key, None), (a, None), (b, None), (c, None)]
    e2, e3 = [1, ("1-", 2)], [1, ("1-", 2), ("1+", 3)]
    aggs = [("min", e2), ("max", e2), ("min", e3), ("max", e3)]
    ref = _ref(cols, [0], aggs)
    # the reference's MIN / MAX are values of its own per-row products
    v2, _ = _expr_col(cols, e2)
    fused = a - a * b                                  # what an fma would give
    assert (v2 != fused)[~np.isnan(v2)].any()
    assert np.isnan(ref["aggs"][1][[1, 3, 4]]).all()   # NaN is the MAX
    assert np.isnan(ref["aggs"][0][4]) and not np.isnan(ref["aggs"][0][[1, 3]]).any()
    assert ref["aggs"][0][2] == -np.inf and ref["aggs"][1][2] == np.inf
    t = _bind(ctx, orc, cols)
    for grid in (0, 1, 3):
        res = ctx.test_groupby_expr(t, [0], aggs, grid=grid)
        _same(res, ref)                                # bit for bit
        assert not res["agg_null"].any()
    t.free()


# ---------------- (4) NULL strictness ----------------

def _input4():
    rng = np.random.default_rng(4)
    n = 5000
    key = rng.integers(0, 5, n).astype(np.int32)
    a = rng.integers(1, 2001, n).astype(np.float64) * 0.25
    b = np.repeat(rng.choice(np.array([0.0, 0.25, 0.5, 0.75]), n // 20), 20)  # runs
    c = rng.choice(np.array([0.0, 0.125, 0.25, 0.5]), n)
    an, cn = rng.random(n) < 0.2, rng.random(n) < 0.2
    cn[key == 3] = True                      # group 3: c is NULL in every row
    return [(key, None), (a, an), (b, None), (c, cn)]


AGGS4 = [("count*", None), ("count", [1, ("1-", 2)]), ("sum", [1, ("1-", 2)]),
         ("count", [1, ("1-", 2), ("1+", 3)]), ("sum", [1, ("1-", 2), ("1+", 3)]),
         ("min", [1, ("1+", 3)]), ("max", [("1+", 3)]), ("count", 1)]


def test_null_strictness_and_rle_operand(ctx, orc):
    cols = _input4()
    key, (a, an), (c, cn) = cols[0][0], cols[1], cols[3]
    ref = _ref(cols, [0], AGGS4)
    g3 = ref["keys"][:, 0].tolist().index(3)
    # COUNT(expr) = rows where every factor is non-NULL
    for g in range(5):
        assert ref["aggs"][1][g] == ((key == g) & ~an).sum()
        assert ref["aggs"][3][g] == ((key == g) & ~an & ~cn).sum()
    assert ref["agg_null"][g3].tolist() == [False, False, False, False, True,
                                            True, True, False]
    assert not np.delete(ref["agg_null"], g3, axis=0).any()
    fq = [(3, ">=", 0.125)]                   # NULL c fails the row
    mask = _fq_mask(cols, fq)
    assert (mask == (~cn & (c >= 0.125))).all() and (cn & (c >= 0.125)).any()
    ref_fq = _ref(cols, [0], AGGS4, mask)
    assert 3 not in ref_fq["keys"][:, 0]
    results = []
    for rle in ((), (2,)):
        streams = [_stream(orc, v, nl, rle=i in rle) for i, (v, nl) in enumerate(cols)]
        assert [s[3] for s in streams] == [0, 1, 1 if rle else 0, 1]
        t = ctx.bind(streams)
        for grid in (0, 1):
            res = ctx.test_groupby_expr(t, [0], AGGS4, grid=grid)
            _same(res, ref)
            _same(ctx.test_groupby_expr(t, [0], AGGS4, fquals=fq, grid=grid), ref_fq)
        results.append(res)
        t.free()
    _same(results[0], results[1])
    assert results[0]["aggs"][0][g3] == (key == 3).sum()
    assert results[0]["aggs"][4][g3] == 0


# ---------------- (5) both accumulation paths ----------------

AGGS5 = [("count*", None), ("sum", [1, ("1-", 2)]), ("max", [1, 2])]


@pytest.fixture(scope="module")
def inp5(ctx, orc):
    made = {}
    for ng in (gx.gb_lds_groups(len(AGGS5)) + 1, 5000):
        rng = np.random.default_rng(50 + ng % 7)
        n = max(4 * ng, 6000)
        key = rng.integers(0, ng, n).astype(np.int64)
        key[:ng] = np.arange(ng)
        key = (key - ng // 2) * 1000003
        a = rng.integers(1, 4001, n).astype(np.float64) * 0.25
        b = rng.choice(np.array([0.0, 0.25, 0.5, 0.75]), n)
        cols = [(key, None), (a, rng.random(n) < 0.1), (b, None)]
        made[ng] = (cols, _bind(ctx, orc, cols), _ref(cols, [0], AGGS5))
    yield made
    for _, t, _ in made.values():
        t.free()


@pytest.mark.parametrize("which", ["cap+1", "5000"])
def test_lds_and_global_paths(ctx, inp5, monkeypatch, which):
    ng = gx.gb_lds_groups(len(AGGS5)) + 1 if which == "cap+1" else 5000
    cols, t, ref = inp5[ng]
    assert ref["ngroups"] == ng
    monkeypatch.delenv("GX_GB_LDS", raising=False)
    res, st = ctx.test_groupby_expr(t, [0], AGGS5, grid=1, stats=True)
    monkeypatch.setenv("GX_GB_LDS", "0")
    off, st_off = ctx.test_groupby_expr(t, [0], AGGS5, grid=1, stats=True)
    _same(res, ref)
    _same(off, ref)
    for s in (st, st_off):
        assert s["rows_in"] == s["rows_pass"] == len(cols[0][0])
        assert s["rows_lds"] + s["rows_global"] == s["rows_pass"]
        assert s["groups"] == ng
    assert st["rows_lds"] > 0 and st["rows_global"] > 0
    assert st_off["rows_lds"] == 0


# ---------------- (6) operand sharing ----------------

def test_operand_sharing_and_the_operand_limit(ctx, orc):
    rng = np.random.default_rng(6)
    n = 3000
    key = rng.integers(0, 4, n).astype(np.int8)
    fcols = [(rng.integers(0, 9, n).astype(np.float64) * 0.25, None)
             for _ in range(9)]                    # columns 1..9
    cols = [(key, None)] + fcols
    t = _bind(ctx, orc, cols)
    # column 1 in three expressions and one fqual; 8 distinct operands (1..8)
    aggs = [("sum", [1, ("1-", 2)]), ("sum", [1, 3, ("1+", 4)]), ("max", [("1+", 1)]),
            ("sum", [5, 6]), ("min", [7, ("1-", 8)]), ("count*", None)]
    fq = [(1, ">", 0.0), (8, "<=", 1.75)]
    ref = _ref(cols, [0], aggs, _fq_mask(cols, fq))
    for grid in (0, 1):
        _same(ctx.test_groupby_expr(t, [0], aggs, fquals=fq, grid=grid), ref)
    # a ninth distinct column, in an expression or in an fqual
    for aggs9, fq9 in ((aggs + [("sum", [9])], fq), (aggs, fq + [(9, "<", 5.0)])):
        with pytest.raises(gx.GxError) as e:
            ctx.groupby_expr(t, [0], aggs9, fquals=fq9)
        assert e.value.status == 3 and "more than 8 distinct" in str(e.value)
    # columns the plain aggregates and keys read do not count as operands
    aggs8 = aggs + [("sum", 9, True)]
    _same(ctx.groupby_expr(t, [0], aggs8, fquals=fq),
          _ref(cols, [0], aggs8, _fq_mask(cols, fq)))
    t.free()


# ---------------- (7) fqual edge values on the device ----------------

def test_fqual_edge_values(ctx, orc):
    nan, inf = np.nan, np.inf
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    vals = np.array([-0.0, 0.0, nan, neg_nan, inf, -inf, 1.5, -1.5, 5e-324,
                     -5e-324])
    x = np.tile(vals, 70)                          # several waves
    nl = np.zeros(len(x), np.bool_)
    nl[3::11] = True
    key = (np.arange(len(x)) % 3).astype(np.int32)
    cols = [(key, None), (x, nl)]
    t = _bind(ctx, orc, cols)
    aggs = [("count*", None)]
    for lit in (0.0, nan, inf, -0.0):
        for op in ("<", ">", "==", "!=", "<=", ">="):
            fq = [(1, op, lit)]
            mask = _fq_mask(cols, fq)
            res, st = ctx.groupby_expr(t, [], aggs, fquals=fq, stats=True)
            assert st["rows_pass"] == mask.sum(), (op, lit)
            assert res["aggs"][0][0] == mask.sum(), (op, lit)
            _same(ctx.groupby_expr(t, [0], aggs, fquals=fq),
                  _ref(cols, [0], aggs, mask))
    # what the reference's order means, in numbers of this input
    per = lambda m: int((m & ~nl).sum())
    res, st = ctx.groupby_expr(t, [], aggs, fquals=[(1, "==", 0.0)], stats=True)
    assert st["rows_pass"] == per((x == 0))               # -0 and +0 both
    res, st = ctx.groupby_expr(t, [], aggs, fquals=[(1, "==", nan)], stats=True)
    assert st["rows_pass"] == per(np.isnan(x))            # every NaN
    res, st = ctx.groupby_expr(t, [], aggs, fquals=[(1, ">", inf)], stats=True)
    assert st["rows_pass"] == per(np.isnan(x))            # NaN above +inf
    res, st = ctx.groupby_expr(t, [], aggs, fquals=[(1, "<", nan)], stats=True)
    assert st["rows_pass"] == per(~np.isnan(x))
    t.free()


# ---------------- (8) ext=None and an empty ext ----------------

AGGS8 = [("count*", None), ("count", 2), ("sum", 2), ("sum", 4, True),
         ("min", 4, True), ("max", 4, True), ("min", 1), ("max", 1)]


def test_no_ext_and_empty_ext_are_groupby_desc(ctx, orc):
    rng = np.random.default_rng(33)
    n = 8000
    key = rng.integers(-3, 4, n).astype(np.int32)
    cols = [(key, None)]
    for v in (rng.integers(-128, 128, n).astype(np.int8),
              rng.integers(-2**31, 2**31, n).astype(np.int32),
              rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64, endpoint=True),
              rng.integers(-5000, 5001, n).astype(np.float64)):
        nl = rng.random(n) < 0.10
        nl[key == 2] = True
        cols.append((v, nl))
    t = _bind(ctx, orc, cols)
    quals = [(2, ">", -2**30)]
    for grid in (0, 1, 3):
        old, st_old = ctx.test_groupby_desc(t, [0], AGGS8, quals=quals, grid=grid,
                                            stats=True)
        for ext in (None, True):
            new, st = ctx.test_groupby_expr(t, [0], AGGS8, quals=quals, grid=grid,
                                            stats=True, ext=ext)
            assert new["keys"].tobytes() == old["keys"].tobytes()
            assert new["key_null"].tobytes() == old["key_null"].tobytes()
            assert new["agg_null"].tobytes() == old["agg_null"].tobytes()
            for x, y in zip(new["aggs"], old["aggs"]):
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
            for f in ("rows_in", "rows_pass", "rows_lds", "rows_global", "groups"):
                assert st[f] == st_old[f]
    _same(old, _ref(cols, [0], AGGS8, ~cols[2][1] & (cols[2][0] > -2**30)))
    # the old error texts come back unchanged through the new entry point
    with pytest.raises(gx.GxError) as e_old:
        ctx.groupby_desc(t, [0], [("max", 2, True)])
    with pytest.raises(gx.GxError) as e_new:
        ctx.groupby_expr(t, [0], [("max", 2, True)])
    assert str(e_new.value) == str(e_old.value)
    assert "is_f64 on a column of width 4" in str(e_new.value)
    t.free()


# ---------------- (9) against gx_q1 ----------------

def test_matches_gx_q1_revenue(ctx):
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, 0.01)
    cutoff = gx.CUTOFF_19950315
    q1 = ctx.q1(t, cutoff)
    res, st = ctx.groupby_expr(
        t, [0, 1], [("count*", None), ("sum", 2, True), ("sum", [2, ("1-", 3)])],
        quals=[(4, "<=", cutoff)], stats=True)
    t.free()
    assert 0 < st["rows_pass"] < st["rows_in"]
    assert not res["key_null"].any() and not res["agg_null"].any()
    slot = res["keys"][:, 0] * 2 + res["keys"][:, 1]
    want = np.nonzero(q1["count"])[0]
    np.testing.assert_array_equal(slot, want)
    np.testing.assert_array_equal(res["aggs"][0], q1["count"][want])
    assert res["aggs"][0].sum() == st["rows_pass"]
    # f64 SUM tolerance of the project (BASELINE): 1e-6 relative
    np.testing.assert_allclose(res["aggs"][1], q1["sum_price"][want],
                               rtol=1e-6, atol=0)
    np.testing.assert_allclose(res["aggs"][2], q1["sum_revenue"][want],
                               rtol=1e-6, atol=0)


# ---------------- (10) the two-stage form ----------------

def _forced(ctx, t, keys, aggs, **kw):
    """groupby_expr_dist through the FULL exchange branch by self-exchange"""
    return G.forced(ctx, lambda: ctx.groupby_expr_dist(t, keys, aggs, stats=True, **kw))


def test_two_stage_form(ctx, li):
    cols, t, ref = li
    one = ctx.groupby_expr(t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS)
    got, st = _forced(ctx, t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS)
    _same(got, one)
    _same(got, ref)
    assert st["rows_in"] == len(cols[0][0])
    assert st["sent_rows"] == st["recv_rows"] == st["partial_groups"] == 6
    assert st["final_groups"] == 6
    # a plain aggregate is a Gather: one state row
    one = ctx.groupby_expr(t, [], Q6_AGGS, quals=Q6_QUALS, fquals=Q6_FQUALS)
    got, st = _forced(ctx, t, [], Q6_AGGS, quals=Q6_QUALS, fquals=Q6_FQUALS)
    _same(got, one)
    _same(got, _ref(cols, [], Q6_AGGS, _q6_mask(cols)))
    assert st["sent_rows"] == st["recv_rows"] == st["partial_groups"] == 1
    # the one-stage plan without the variable: same result, motion stats zero
    got, st = ctx.groupby_expr_dist(t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS, stats=True)
    _same(got, ref)
    assert st["sent_rows"] == st["recv_rows"] == 0 and st["final_groups"] == 6


def test_two_stage_form_needs_comm_init(orc, li):
    cols, _, ref = li
    c2 = gx.Context(device=0, seg=0, nsegs=1)
    os.environ["GX_FORCE_MOTION"] = "1"
    try:
        t = _bind(c2, orc, cols)
        with pytest.raises(gx.GxError) as e:
            c2.groupby_expr_dist(t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS)
        assert e.value.status == 7, e.value            # GX_ERR_STATE
        assert "gx_comm_init" in str(e.value)
        _same(c2.groupby_expr(t, Q1_KEYS, Q1_AGGS, quals=Q1_QUALS), ref)
        t.free()
    finally:
        del os.environ["GX_FORCE_MOTION"]
        c2.close()


# ---------------- (11) errors ----------------

def test_errors_name_the_item_and_leave_the_context_usable(ctx, orc):
    rng = np.random.default_rng(111)
    n = 3000
    cols = [((np.arange(n) % 10).astype(np.int64), None),
            (rng.integers(0, 9, n).astype(np.float64) * 0.25, None),
            (rng.integers(-9, 10, n).astype(np.int32), None),
            (rng.integers(0, 4, n).astype(np.float64) * 0.25, None)]
    t = _bind(ctx, orc, cols)
    good = [("count*", None), ("sum", [1, ("1-", 3)])]
    good_fq = [(3, "<=", 0.5)]
    ref = _ref(cols, [0], good, _fq_mask(cols, good_fq))

    def bad(needle, aggs=good, fquals=good_fq, ext=True):
        with pytest.raises(gx.GxError) as e:
            ctx.test_groupby_expr(t, [0], aggs, fquals=fquals, ext=ext)
        assert e.value.status == 3, e.value            # GX_ERR_INVALID
        assert needle in str(e.value), e.value
        _same(ctx.groupby_expr(t, [0], good, fquals=good_fq), ref)   # usable

    def put(**kw):
        def tweak(ext):
            for k, v in kw.items():
                setattr(ext, k, v)
        return tweak

    def put_agg_expr(j, v):
        def tweak(ext):
            ext.agg_expr[j] = v
        return tweak

    bad("nexprs 9 outside 0..8", ext=put(nexprs=9))
    bad("nexprs -1 outside 0..8", ext=put(nexprs=-1))
    bad("nfquals 5 outside 0..4", fquals=good_fq * 5)
    bad("nfquals -1 outside 0..4", ext=put(nfquals=-1))
    bad("expr 0: nfactors 0 outside 1..3", aggs=[("sum", [])])
    bad("expr 0: nfactors 4 outside 1..3", aggs=[("sum", [1, 1, 3, 3])])
    bad("expr 0 factor 1: column 4 out of range", aggs=[("sum", [1, ("1-", 4)])])
    bad("expr 0 factor 0: column -1 out of range", aggs=[("sum", [-1])])
    bad("expr 0 factor 1: column width 4 is not 8", aggs=[("sum", [1, 2])])
    bad("expr 1 factor 0: form 3 outside 0..2",
        aggs=[("sum", [1]), ("max", [(3, 1)])])
    bad("expr 0 factor 0: form -1 outside 0..2", aggs=[("sum", [(-1, 1)])])
    bad("aggregate 1: agg_expr 1 outside -1..0", ext=put_agg_expr(1, 1))
    bad("aggregate 1: agg_expr -2 outside -1..0", ext=put_agg_expr(1, -2))
    bad("aggregate 0: agg_expr 0 on COUNT(*)", ext=put_agg_expr(0, 0))
    bad("fqual 0: column 4 out of range", fquals=[(4, "<", 1.0)])
    bad("fqual 1: column width 4 is not 8", fquals=good_fq + [(2, "<", 1.0)])
    bad("fqual 0: op 6 outside 0..5", fquals=[(3, 6, 1.0)])
    bad("fqual 0: op -1 outside 0..5", fquals=[(3, -1, 1.0)])
    # the descriptor's own errors are still the descriptor's
    bad("column 7 out of range", aggs=good + [("sum", 7, True)])
    bad("naggs 9", aggs=[("sum", [1])] * 9)
    t.free()

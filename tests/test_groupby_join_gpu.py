"""GPU tests of the descriptor GROUP BY over a join (pytest -m gpu, real
MI355X): gx_groupby_join, its test seam and its two-stage form against a numpy
reference that joins with a dict over the participating dimension rows,
materialises the joined columns and runs the numpy group-by of gb_ref.

Every float8 measure is a small integer (or a multiple of 0.25 in the
expression test), so every summation order is exact and results are asserted
bit-equal."""
import numpy as np
import pytest

import gb_ref as G

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1
INVALID, OOM = 3, 5


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


def _frozen(cols):
    for v, nl in cols:
        v.setflags(write=False)
        if nl is not None:
            nl.setflags(write=False)
    return cols


def _dim0():
    """5000 rows: key int64 (unique, some NULL), attr int32 in -2..2 (some
    NULL), dm float8 (NULL wherever attr == 2), q int32, hi int64 distinct"""
    rng = np.random.default_rng(1701)
    n = 5000
    key = (rng.permutation(40000)[:n].astype(np.int64) - 20000) * 1000003
    key[:6] = [0, -1, INT64_MIN, INT64_MAX, 2**32, 5 + 2**32]
    assert len(np.unique(key)) == n
    attr = rng.integers(-2, 3, n).astype(np.int32)
    attr_null = rng.random(n) < 0.10
    dm = rng.integers(-20, 21, n).astype(np.float64)
    dm_null = (rng.random(n) < 0.10) | (attr == 2)
    q = rng.integers(0, 100, n).astype(np.int32)
    hi = (np.arange(n, dtype=np.int64) - 1300) * (2**33 + 7)
    key_null = rng.random(n) < 0.03
    key_null[:6] = False
    return _frozen([(key, key_null), (attr, attr_null), (dm, dm_null),
                    (q, rng.random(n) < 0.02), (hi, None)])


def _dim1():
    """300 rows: key int32 (unique, negatives), attr int16 in -1..1 (some
    NULL), v int8"""
    rng = np.random.default_rng(1702)
    n = 300
    key = (rng.permutation(2000)[:n] - 1000).astype(np.int32)
    attr = rng.integers(-1, 2, n).astype(np.int16)
    return _frozen([(key, None), (attr, rng.random(n) < 0.10),
                    (rng.integers(-100, 101, n).astype(np.int8), None)])


def _fact(d0, d1):
    """20000 rows: fk0 int64 -> dim0 (NULLs, misses), fk1 int64 -> dim1's
    int32 key (NULLs, misses), c2 float8, c3 float8 in {0, .25, .5}, k8 int8,
    m32 int32"""
    rng = np.random.default_rng(1703)
    n = 20000
    pool0 = np.concatenate([d0[0][0], np.array([7, -7, 2**40, 5 + 2**33], np.int64)])
    pool1 = np.concatenate([d1[0][0].astype(np.int64),
                            np.array([5000, -5000, 2**32 + int(d1[0][0][0])], np.int64)])
    fk0 = rng.choice(pool0, n)
    fk0[:6] = d0[0][0][:6]              # 0, -1, both extremes, 2^32, 5 + 2^32
    fk0_null = rng.random(n) < 0.05
    fk0_null[:6] = False
    fk1 = rng.choice(pool1, n)
    fk1[:6] = d1[0][0][:6]
    c2 = rng.integers(-50, 51, n).astype(np.float64)
    c3 = rng.choice(np.array([0.0, 0.25, 0.5]), n)
    k8 = rng.integers(-3, 4, n).astype(np.int8)
    m32 = rng.integers(-10**6, 10**6, n).astype(np.int32)
    return _frozen([(fk0, fk0_null), (fk1, rng.random(n) < 0.03),
                    (c2, rng.random(n) < 0.10), (c3, rng.random(n) < 0.05),
                    (k8, rng.random(n) < 0.10), (m32, rng.random(n) < 0.10)])


@pytest.fixture(scope="module")
def data(ctx, orc):
    d0, d1 = _dim0(), _dim1()
    fact = _fact(d0, d1)
    t = {"fact": G.bind(ctx, orc, fact), "d0": G.bind(ctx, orc, d0),
         "d1": G.bind(ctx, orc, d1)}
    yield fact, d0, d1, t
    for x in t.values():
        x.free()


def _tr(c, offs):
    return offs[c.j] + c.col if isinstance(c, gx.DimCol) else c


def _want(fact, dims, on, keys, aggs, fmask=None, extra_cols=()):
    """the reference: dims = [(cols, live mask or None)], on = [(fact_col,
    dim_key_col)]; DimCol(j, c) becomes the joined column of dims[j]"""
    ms = [G.match(fact[fc], dc[dk], np.ones(len(dc[0][0]), bool) if live is None else live)
          for (dc, live), (fc, dk) in zip(dims, on)]
    cols, ok = G.joined(list(fact) + list(extra_cols), [dc for dc, _ in dims], ms)
    offs = np.cumsum([len(fact) + len(extra_cols)] + [len(dc) for dc, _ in dims])
    if fmask is not None:
        ok = ok & fmask
    raggs = [(a[0], None if a[1] is None else _tr(a[1], offs)) + tuple(a[2:])
             for a in aggs]
    return G.ref(cols, [_tr(k, offs) for k in keys], raggs, ok), ms, ok


D = gx.DimCol


# ---------------- 1. one join, key from the dimension ----------------

AGGS1 = [("count*", None), ("sum", 2, True), ("sum", D(0, 2), True),
         ("min", D(0, 3)), ("max", 5), ("count", D(0, 2))]


@pytest.fixture(scope="module")
def want1(data):
    fact, d0, d1, t = data
    return _want(fact, [(d0, None)], [(0, 0)], [D(0, 1)], AGGS1)


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("grid", [0, 1, 3])
def test_one_join_dim_key(ctx, data, want1, grid, wide):
    fact, d0, d1, t = data
    ref, (m0,), ok = want1
    # the input holds a NULL fact key, a miss, a NULL dimension key whose value
    # fact rows carry, and collision-prone keys (2^32 apart)
    assert fact[0][1].any() and (m0[~fact[0][1]] < 0).any() and ok.any()
    dead = set(d0[0][0][d0[0][1]].tolist())
    assert any(int(k) in dead for k in fact[0][0][~fact[0][1]])
    assert {2**32, 5 + 2**32} <= set(fact[0][0][ok].tolist())
    # fact rows with different join values share one attribute value: one group
    a1 = ok & (d0[1][0][m0] == 1) & ~d0[1][1][m0]
    assert len(np.unique(fact[0][0][a1])) > 100
    res, st = ctx.test_groupby_join(t["fact"], [D(0, 1)], AGGS1,
                                    [(t["d0"], 0, 0)], stats=True, grid=grid,
                                    wide_rowid=wide)
    G.same(res, ref)
    assert res["ngroups"] == 6 and res["key_null"][-1, 0]       # -2..2 and NULL
    assert st["rows_in"] == len(ok) == st["rows_probed"]
    assert st["rows_pass"] == ok.sum() == res["aggs"][0].sum()
    assert st["dim_rows"] == [int((~d0[0][1]).sum()), 0]
    assert st["rows_lds"] + st["rows_global"] == st["rows_pass"]
    if grid:
        assert st["rows_lds"] > 0


def test_same_attribute_one_group_different_two(ctx, orc):
    fact = [(np.array([10, 20, 30, 20, 40], np.int64), None)]
    dim = [(np.array([30, 10, 20], np.int64), None),
           (np.array([2, 1, 1], np.int32), None)]
    tf, td = G.bind(ctx, orc, fact), G.bind(ctx, orc, dim)
    res = ctx.groupby_join(tf, [D(0, 1)], [("count*", None), ("min", 0)],
                           [(td, 0, 0)])
    # 10 and 20 carry attribute 1: one group of three rows; 30 carries 2
    assert res["keys"][:, 0].tolist() == [1, 2]
    assert res["aggs"][0].tolist() == [3, 1] and res["aggs"][1].tolist() == [10, 30]
    tf.free()
    td.free()


# ---------------- 2. mixed keys, two joins ----------------

def test_mixed_keys_two_joins(ctx, data):
    fact, d0, d1, t = data
    keys = [4, D(0, 1), D(1, 1)]
    aggs = [("count*", None), ("sum", D(1, 2)), ("sum", D(0, 2), True),
            ("max", 2, True)]
    ref, (m0, m1), ok = _want(fact, [(d0, None), (d1, None)], [(0, 0), (1, 0)],
                              keys, aggs)
    # rows missing exactly one of the joins exist and are dropped
    assert ((m0 >= 0) & (m1 < 0)).any() and ((m0 < 0) & (m1 >= 0)).any()
    assert 0 < ok.sum() < (m0 >= 0).sum()
    for grid in (0, 1):
        res, st = ctx.test_groupby_join(t["fact"], keys, aggs,
                                        [(t["d0"], 0, 0), (t["d1"], 1, 0)],
                                        stats=True, grid=grid)
        G.same(res, ref)
        assert st["rows_pass"] == ok.sum() and st["dim_rows"][1] == 300
    assert res["key_null"].any(axis=0).all()        # a NULL in every key column
    assert res["ngroups"] > 100


# ---------------- 3. cross-width join columns ----------------

@pytest.mark.parametrize("fdt,ddt", [(np.int32, np.int64), (np.int8, np.int32)])
def test_cross_width(ctx, orc, fdt, ddt):
    rng = np.random.default_rng(1730)
    lo, hi = np.iinfo(fdt).min, np.iinfo(fdt).max
    n = 6000
    if fdt == np.int8:
        fk = rng.integers(lo, hi + 1, n).astype(fdt)
        inside = np.arange(lo, hi + 1, 2, dtype=np.int64)          # every other value
    else:
        inside = np.unique(np.concatenate([rng.integers(lo, hi + 1, 400),
                                           [lo, hi, -1, 0]])).astype(np.int64)
        fk = rng.choice(np.concatenate([inside, inside[:-1] + 1]), n).astype(fdt)
    # dimension keys outside the narrower type, congruent to keys inside it
    span = int(hi) - int(lo) + 1
    outside = np.array([int(inside[2]) + span, int(inside[3]) - span, int(hi) + 1,
                        int(lo) - 1], np.int64)
    dkey = np.concatenate([inside, outside]).astype(ddt)
    assert len(np.unique(dkey)) == len(dkey)
    assert (dkey[-4:].astype(fdt) != dkey[-4:]).all()              # would wrap
    dattr = (np.arange(len(dkey)) % 5).astype(np.int32)
    fact = [(fk, None), (rng.integers(-9, 10, n).astype(np.float64), None)]
    dim = [(dkey, None), (dattr, None)]
    aggs = [("count*", None), ("sum", 1, True), ("min", D(0, 0)), ("max", D(0, 0))]
    ref, (m,), ok = _want(fact, [(dim, None)], [(0, 0)], [D(0, 1)], aggs)
    assert (fk[ok] < 0).any() and (m < 0).any()
    assert not np.isin(m, np.arange(len(dkey) - 4, len(dkey))).any()
    tf, td = G.bind(ctx, orc, fact), G.bind(ctx, orc, dim)
    res = ctx.groupby_join(tf, [D(0, 1)], aggs, [(td, 0, 0)])
    G.same(res, ref)
    # no out-of-range dimension key was matched: MIN / MAX stay inside
    assert res["aggs"][2].min() >= lo and res["aggs"][3].max() <= hi
    tf.free()
    td.free()


# ---------------- 4. NULLs ----------------

def test_nulls(ctx, data, want1):
    fact, d0, d1, t = data
    ref, (m0,), ok = want1
    res = ctx.groupby_join(t["fact"], [D(0, 1)], AGGS1, [(t["d0"], 0, 0)])
    G.same(res, ref)
    # NULL fact join values are dropped, NULL dimension keys never matched
    assert (m0[fact[0][1]] == -1).all() and not d0[0][1][m0[ok]].any()
    # the NULL attribute is a group of its own beside the 0 group
    k, kn = res["keys"][:, 0], res["key_null"][:, 0]
    g0 = int(np.nonzero((k == 0) & ~kn)[0][0])
    gn = int(np.nonzero(kn)[0][0])
    assert g0 != gn and res["aggs"][0][g0] > 0 and res["aggs"][0][gn] > 0
    # NULL dimension aggregate inputs are skipped: COUNT(dm) < COUNT(*)
    assert 0 < res["aggs"][5][g0] < res["aggs"][0][g0]
    # attribute 2: every dm is NULL -> SUM(dm) is NULL, COUNT(dm) 0
    g2 = int(np.nonzero((k == 2) & ~kn)[0][0])
    assert res["agg_null"][g2].tolist() == [False, False, True, False, False, False]
    assert res["aggs"][5][g2] == 0 and res["aggs"][0][g2] > 0
    assert not res["agg_null"][g0].any()


# ---------------- 5. dimension quals, visimap, duplicates ----------------

def test_dim_quals_visimap_duplicates(ctx, orc, data):
    fact, d0, d1, t = data
    rng = np.random.default_rng(1750)
    n0 = len(d0[0][0])
    hidden = rng.random(n0) < 0.2
    quals = [(3, ">=", 30), (3, "<", 90)]
    live = ~hidden & ~d0[3][1] & (d0[3][0] >= 30) & (d0[3][0] < 90)
    assert (~hidden & d0[3][1]).any() and 0 < live.sum() < (~hidden).sum()
    aggs = [("count*", None), ("sum", D(0, 2), True)]
    th = G.bind(ctx, orc, d0, hidden=hidden)
    ref, (m0,), ok = _want(fact, [(d0, live)], [(0, 0)], [D(0, 1)], aggs)
    res, st = ctx.groupby_join(t["fact"], [D(0, 1)], aggs, [(th, 0, 0, quals)],
                               stats=True)
    G.same(res, ref)
    assert st["dim_rows"][0] == (live & ~d0[0][1]).sum() and st["rows_pass"] == ok.sum()
    th.free()

    # a duplicated key: rows a and b carry the same key
    dup = [(v.copy(), None if nl is None else nl.copy()) for v, nl in d0]
    a, b = [int(r) for r in np.nonzero(~d0[0][1] & ~d0[3][1])[0][10:12]]
    dup[0][0][b] = dup[0][0][a]
    dup[3][0][a], dup[3][0][b] = 50, 10
    key = int(dup[0][0][a])
    td = G.bind(ctx, orc, dup)
    with pytest.raises(gx.GxError) as e:
        ctx.groupby_join(t["fact"], [D(0, 1)], aggs, [(td, 0, 0)])
    assert e.value.status == INVALID, e.value
    assert "join 0" in str(e.value) and str(key) in str(e.value), e.value
    # second join position is named as such
    with pytest.raises(gx.GxError) as e:
        ctx.groupby_join(t["fact"], [D(1, 1)], aggs[:1],
                         [(t["d1"], 1, 0), (td, 0, 0)])
    assert e.value.status == INVALID and "join 1" in str(e.value), e.value
    # hidden by a qual: row b fails q >= 30
    live_q = ~dup[3][1] & (dup[3][0] >= 30)
    ref, _, _ = _want(fact, [(dup, live_q)], [(0, 0)], [D(0, 1)], aggs)
    G.same(ctx.groupby_join(t["fact"], [D(0, 1)], aggs,
                            [(td, 0, 0, [(3, ">=", 30)])]), ref)
    td.free()
    # hidden by the visimap: row a is deleted
    hid = np.zeros(n0, bool)
    hid[a] = True
    td = G.bind(ctx, orc, dup, hidden=hid)
    ref, (m,), _ = _want(fact, [(dup, ~hid)], [(0, 0)], [D(0, 1)], aggs)
    assert (m == b).any() and not (m == a).any()
    G.same(ctx.groupby_join(t["fact"], [D(0, 1)], aggs, [(td, 0, 0)]), ref)
    td.free()


# ---------------- 6. high cardinality ----------------

@pytest.mark.parametrize("lds", [True, False])
def test_high_cardinality_from_dimension(ctx, data, monkeypatch, lds):
    fact, d0, d1, t = data
    aggs = [("count*", None), ("sum", 2, True)]
    ref, _, ok = _want(fact, [(d0, None)], [(0, 0)], [D(0, 4)], aggs)
    assert ref["ngroups"] > 3 * gx.gb_lds_groups(len(aggs))
    if not lds:
        monkeypatch.setenv("GX_GB_LDS", "0")
    for grid in (0, 1):
        res, st = ctx.test_groupby_join(t["fact"], [D(0, 4)], aggs,
                                        [(t["d0"], 0, 0)], stats=True, grid=grid)
        G.same(res, ref)
        assert st["rows_pass"] == ok.sum()
        if not lds:
            assert st["rows_lds"] == 0
        elif grid == 1:
            # one workgroup: its LDS table fills, then it gives up
            assert st["rows_lds"] > 0 and st["rows_global"] > st["rows_lds"]


# ---------------- 7. plain aggregate and empty inputs ----------------

AGGS7 = [("count*", None), ("count", D(0, 1)), ("sum", 1, True), ("min", D(0, 1))]


def test_plain_aggregate_and_empty_inputs(ctx, orc):
    rng = np.random.default_rng(1770)
    n = 3000
    fact = [(rng.integers(0, 50, n).astype(np.int64), None),
            (rng.integers(-9, 10, n).astype(np.float64), None)]
    dim = [(np.arange(100, 150, dtype=np.int64), None),
           (np.arange(50, dtype=np.int32), None)]
    empty_f = [(np.zeros(0, np.int64), None), (np.zeros(0, np.float64), None)]
    empty_d = [(np.zeros(0, np.int64), None), (np.zeros(0, np.int32), None)]
    hit = [(np.arange(0, 50, dtype=np.int64), None), dim[1]]
    tf, td, tef, ted, thit = (G.bind(ctx, orc, c) for c in
                              (fact, dim, empty_f, empty_d, hit))
    assert not np.isin(fact[0][0], dim[0][0]).any()             # nothing joins
    none = [(1, "<", -2**31)]                       # no int32 is below INT32_MIN
    cases = [(tf, td, ()), (tef, thit, ()), (tf, ted, ()), (tf, thit, none)]
    for f, d, q in cases:
        res, st = ctx.groupby_join(f, [], AGGS7, [(d, 0, 0, q)], stats=True)
        assert res["ngroups"] == 1 and res["keys"].shape == (1, 0)
        assert [int(a[0]) for a in res["aggs"]] == [0, 0, 0, 0]
        assert res["agg_null"][0].tolist() == [False, False, True, True]
        assert st["rows_pass"] == 0 and st["rows_probed"] == f.nrows
        for keys in ([D(0, 1)], [0], [0, D(0, 1)]):
            res = ctx.groupby_join(f, keys, AGGS7, [(d, 0, 0, q)])
            assert res["ngroups"] == 0 and res["keys"].shape == (0, len(keys))
            assert all(len(a) == 0 for a in res["aggs"])
    # the same shapes do join when the dimension holds the keys
    ref, _, ok = _want(fact, [(hit, None)], [(0, 0)], [], AGGS7)
    assert ok.all()
    G.same(ctx.groupby_join(tf, [], AGGS7, [(thit, 0, 0)]), ref)
    for x in (tf, td, tef, ted, thit):
        x.free()


# ---------------- 8. expressions with a join ----------------

def test_expression_with_join(ctx, data):
    fact, d0, d1, t = data
    c2, c3 = fact[2], fact[3]
    e = (c2[0] * (1.0 - c3[0]), c2[1] | c3[1])
    aggs = [("sum", [2, ("1-", 3)]), ("count*", None), ("max", [2, ("1-", 3)]),
            ("sum", D(0, 2), True)]
    raggs = [("sum", len(fact), True), ("count*", None), ("max", len(fact), True),
             ("sum", D(0, 2), True)]
    fmask = ~c2[1] & (c2[0] > 0)
    assert (c2[1] & ~fact[0][1]).any() and (e[1] & fmask).any()
    ref, _, ok = _want(fact, [(d0, None)], [(0, 0)], [D(0, 1)], raggs, fmask=fmask,
                       extra_cols=[e])
    for grid in (0, 3):
        res, st = ctx.test_groupby_join(t["fact"], [D(0, 1)], aggs,
                                        [(t["d0"], 0, 0)], fquals=[(2, ">", 0.0)],
                                        stats=True, grid=grid)
        G.same(res, ref)
        assert st["rows_probed"] == fmask.sum() and st["rows_pass"] == ok.sum()
    assert (res["aggs"][0] % 1 != 0).any()          # the quarters really occur


# ---------------- 9. njoins == 0 is groupby_expr ----------------

def test_no_join_equals_groupby_expr(ctx, data):
    fact, d0, d1, t = data
    keys = [4]
    aggs = [("count*", None), ("sum", [2, ("1-", 3)]), ("min", 5), ("sum", 2, True)]
    quals, fquals = [(5, ">", -500000)], [(3, "<", 0.5)]
    for grid in (0, 1):
        a, sa = ctx.test_groupby_expr(t["fact"], keys, aggs, quals=quals,
                                      fquals=fquals, stats=True, grid=grid)
        b, sb = ctx.test_groupby_join(t["fact"], keys, aggs, [], quals=quals,
                                      fquals=fquals, stats=True, grid=grid)
        G.same(a, b)
        for x, y in zip(a["aggs"], b["aggs"]):
            assert x.tobytes() == y.tobytes()
        for f in ("rows_in", "rows_pass", "rows_lds", "rows_global", "groups"):
            assert sa[f] == sb[f], f
        assert sb["rows_probed"] == sb["rows_pass"] and sb["dim_rows"] == [0, 0]
    # the same error text for the same bad descriptor
    msgs = []
    for call in (lambda: ctx.groupby_expr(t["fact"], [9], aggs),
                 lambda: ctx.groupby_join(t["fact"], [9], aggs, [])):
        with pytest.raises(gx.GxError) as e:
            call()
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "column 9 out of range" in msgs[0]


# ---------------- 10. errors ----------------

def test_errors_name_their_item(ctx, orc, data):
    fact, d0, d1, t = data
    good_aggs = [("count*", None), ("sum", D(0, 2), True)]
    odd = ctx.bind([(b"", 16, 0, 1), (b"", 8, 0, 1)])   # a 16-byte column, no rows
    J = [(t["d0"], 0, 0)]

    def setter(**kw):
        def f(e):
            for k, v in kw.items():
                if k == "njoins":
                    e.njoins = v
                else:
                    name, i = k.rsplit("_", 1)
                    getattr(e, name)[int(i)] = v
        return f

    cases = [
        ("njoins 3", dict(joins=J, jext=setter(njoins=3))),
        ("njoins -1", dict(joins=J, jext=setter(njoins=-1))),
        ("join 0: no dimension table", dict(joins=[(None, 0, 0)])),
        ("join 1: no dimension table", dict(joins=J + [(None, 1, 0)],
                                            keys=[D(0, 1)])),
        ("key 0: side 2", dict(joins=J, jext=setter(key_side_0=2))),
        ("key 0: side -1", dict(joins=J, jext=setter(key_side_0=-1))),
        ("key 0: side 1", dict(joins=[], keys=[D(0, 1)], aggs=[("count*", None)])),
        ("aggregate 1: side 2", dict(joins=J, jext=setter(agg_side_1=2))),
        # column 5 exists in the fact table (6 columns), not in dim0 (5)
        ("key 0: column 5 out of range", dict(joins=J, keys=[D(0, 5)])),
        ("aggregate 1: column 5 out of range",
         dict(joins=J, aggs=[("count*", None), ("sum", D(0, 5), True)])),
        # column 4 is 8 bytes wide in dim0, 1 byte in the fact table
        ("aggregate 1: is_f64 on a column of width 1",
         dict(joins=J, aggs=[("count*", None), ("max", 4, True)])),
        ("join 0: fact column 17 out of range", dict(joins=[(t["d0"], 17, 0)])),
        ("join 0: dimension key column 17 out of range",
         dict(joins=[(t["d0"], 0, 17)])),
        ("join 0: dimension key column width 16", dict(joins=[(odd, 0, 0)])),
        ("join 0 qual 1: column width 16",
         dict(joins=[(odd, 0, 1, [(1, "<", 3), (0, "<", 3)])])),
        ("join 0 qual 1: op 6",
         dict(joins=[(t["d0"], 0, 0, [(3, "<", 3), (3, 6, 3)])])),
        ("join 0 qual 0: column 5 out of range",
         dict(joins=[(t["d0"], 0, 0, [(5, "<", 3)])])),
        ("join 0: nquals 5", dict(joins=[(t["d0"], 0, 0, [(3, "<", 3)] * 5)])),
    ]
    want = ctx.groupby_join(t["fact"], [D(0, 1)], good_aggs, J)
    for needle, kw in cases:
        args = dict(keys=[D(0, 1)], aggs=good_aggs, jext=None)
        args.update(kw)
        with pytest.raises(gx.GxError) as e:
            ctx.test_groupby_join(t["fact"], args["keys"], args["aggs"],
                                  args["joins"], jext=args["jext"])
        assert e.value.status == INVALID, (needle, e.value)
        assert needle in str(e.value), (needle, e.value)
        # the context still answers a good call
        G.same(ctx.groupby_join(t["fact"], [D(0, 1)], good_aggs, J), want)
    # the fact side of a join column: a 16-byte column of an empty fact table
    with pytest.raises(gx.GxError) as e:
        ctx.groupby_join(odd, [D(0, 1)], [("count*", None)], [(t["d0"], 0, 0)])
    assert e.value.status == INVALID
    assert "join 0: fact column width 16" in str(e.value), e.value
    # the two-stage form and its test seam give the same text
    for call in (lambda: ctx.groupby_join_dist(t["fact"], [D(0, 5)], good_aggs, J),
                 lambda: ctx.test_gbj_partial(t["fact"], [D(0, 5)], good_aggs, J, 3)):
        with pytest.raises(gx.GxError) as e:
            call()
        assert e.value.status == INVALID
        assert "key 0: column 5 out of range" in str(e.value), e.value
    G.same(ctx.groupby_join(t["fact"], [D(0, 1)], good_aggs, J), want)
    odd.free()


# ---------------- 11. HBM budget ----------------

def test_hbm_budget_counts_the_join_table(ctx, orc, data, monkeypatch):
    """a dimension of 300000 rows: 2^20 slots of 4 bytes = 4 MiB of join
    table; the group table for max_groups = 8 is 1024 slots (under 100 KiB
    with its compacted groups).  A budget of 2 MiB lies between the two."""
    fact, d0, d1, t = data
    nd = 300000
    big = [(np.arange(nd, dtype=np.int64) * 3 - 1000, None),
           ((np.arange(nd) % 5).astype(np.int32), None)]
    fk = [(np.random.default_rng(1790).integers(-500, 3 * nd, 20000).astype(np.int64),
           None)]
    tf, td = G.bind(ctx, orc, fk), G.bind(ctx, orc, big)
    aggs = [("count*", None), ("max", 0)]
    ref, _, ok = _want(fk, [(big, None)], [(0, 0)], [D(0, 1)], aggs)
    assert ok.any() and not ok.all()
    monkeypatch.setenv("GX_HBM_BUDGET_MB", "2")
    # the group table alone fits ...
    alone = ctx.groupby_expr(tf, [], aggs, max_groups=8)
    assert alone["aggs"][0][0] == 20000
    # ... the group table and the join table do not
    with pytest.raises(gx.GxError) as e:
        ctx.groupby_join(tf, [D(0, 1)], aggs, [(td, 0, 0)], max_groups=8)
    assert e.value.status == OOM, e.value
    assert "HBM budget" in str(e.value) and "join" in str(e.value), e.value
    monkeypatch.delenv("GX_HBM_BUDGET_MB")
    G.same(ctx.groupby_join(tf, [D(0, 1)], aggs, [(td, 0, 0)], max_groups=8), ref)
    tf.free()
    td.free()


# ---------------- 12. two-stage form ----------------

def test_two_stage_form(ctx, data):
    fact, d0, d1, t = data
    # key 0: fact column 1 (int64); key 1: dim0 column 1 (int32) -- the FACT
    # table's column 1 is 8 bytes wide, so widths taken from the wrong table
    # would route key 1 with hashint8
    keys = [1, D(0, 1)]
    aggs = [("count*", None), ("sum", D(0, 2), True), ("min", 5)]
    J = [(t["d0"], 0, 0)]
    assert fact[1][0].itemsize == 8 and d0[1][0].itemsize == 4
    ref, (m0,), ok = _want(fact, [(d0, None)], [(0, 0)], keys, aggs)
    want = ctx.groupby_join(t["fact"], keys, aggs, J)
    G.same(want, ref)
    counts, rows = ctx.test_gbj_partial(t["fact"], keys, aggs, J, 3)
    plain = [("count*", None), ("sum", 0, True), ("min", 0)]    # the same state words
    assert rows.dtype == gx.gbd_wire_dtype([0, 0], plain)
    assert len(counts) == 3 and (counts > 0).all()
    assert counts.sum() == len(rows) == ref["ngroups"]          # conserved
    assert rows["acc"][:, 0].sum() == ok.sum()                  # COUNT(*) words
    dest = gx.gbd_route(rows["keys"], rows["key_null"], [8, 4], 3)
    np.testing.assert_array_equal(dest, np.repeat(np.arange(3), counts))
    assert rows["key_null"].any()
    # hashint8 of a value that fits int32 IS hashint4 of it, so the narrow
    # dim-side key above routes alike under either reading.  The wide one does
    # not: dim0 column 4 is int64 with values past int32, the fact table's
    # column 4 is one byte wide.
    assert fact[4][0].itemsize == 1 and d0[4][0].itemsize == 8
    c2, r2 = ctx.test_gbj_partial(t["fact"], [D(0, 4)], aggs[:1], J, 3)
    assert c2.sum() == len(r2) == len(np.unique(d0[4][0][m0[ok]]))
    d8 = gx.gbd_route(r2["keys"], r2["key_null"], [8], 3)
    np.testing.assert_array_equal(d8, np.repeat(np.arange(3), c2))
    assert (gx.gbd_route(r2["keys"], r2["key_null"], [4], 3) != d8).any()
    G.same(ctx.test_gbd_combine(rows, [0, 0], plain), ref)
    got, st = G.forced(ctx, lambda: ctx.groupby_join_dist(t["fact"], keys, aggs, J,
                                                          stats=True))
    G.same(got, want)
    assert st["rows_in"] == len(ok)
    assert (st["sent_rows"] == st["recv_rows"] == st["partial_groups"]
            == st["final_groups"] == ref["ngroups"])
    # one segment without the variable: the one-stage plan
    got1, st1 = ctx.groupby_join_dist(t["fact"], keys, aggs, J, stats=True)
    G.same(got1, want)
    assert st1["sent_rows"] == 0 and st1["final_groups"] == ref["ngroups"]

"""Join/agg table with packed 16-byte {sum, count} slots that are zeroed at
claim time instead of by a per-run clear, the single-read block-ordered
extract, and the probe's adds into the packed slot across hit densities.

Every result is checked against the oracle or a numpy brute force of the
plan: keys, attrs and counts bit-equal, revenue within rtol=1e-6 (the f64
summation order differs)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

RTOL = 1e-6


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


@pytest.fixture(scope="module")
def rows001(orc):
    """oracle-generated SF 0.01 tables (shared, read-only)"""
    return orc.gen_customer(0.01), orc.gen_orders(0.01), orc.gen_lineitem(0.01)


@pytest.fixture(scope="module")
def want005(orc):
    """oracle Q3 at SF 0.05 (shared, read-only)"""
    sf = 0.05
    return orc.q3(orc.gen_customer(sf), orc.gen_orders(sf), orc.gen_lineitem(sf))


def _gen(ctx, sf, li_kind=None):
    return (ctx.tpch_gen(gx.TPCH_CUSTOMER, sf),
            ctx.tpch_gen(gx.TPCH_ORDERS, sf),
            ctx.tpch_gen(gx.TPCH_LINEITEM if li_kind is None else li_kind, sf))


def _assert_q3(got, want):
    np.testing.assert_array_equal(got["l_orderkey"], want["l_orderkey"])
    np.testing.assert_array_equal(got["o_orderdate"], want["o_orderdate"])
    np.testing.assert_array_equal(got["o_shippriority"], want["o_shippriority"])
    np.testing.assert_array_equal(got["nitems"], want["nitems"])
    np.testing.assert_allclose(got["revenue"], want["revenue"], rtol=RTOL)


# ---------------- 1. stale state across runs of one q ----------------

def test_stale_state_three_runs_local_and_motion(ctx, want005, monkeypatch):
    """Run 2 finds run 1's sums in the very slots it claims: without the
    claim-time zero they would double.  Local path, then the forced-Motion
    build (k_build_from_rows), three runs of one q each."""
    cust, ordr, li = _gen(ctx, 0.05)
    q = ctx.q3(cust, ordr, li)
    for _ in range(3):
        _assert_q3(q.run().result(), want005)
    q.free()

    ctx.comm_init(ctx.comm_unique_id())
    monkeypatch.setenv("GX_FORCE_MOTION", "1")
    qm = ctx.q3(cust, ordr, li)
    for _ in range(3):
        _assert_q3(qm.run().result(), want005)
    qm.free(); li.free(); ordr.free(); cust.free()


# ---------------- 2. hit-density ladder for the probe's adds ----------------

CUT = gx.CUTOFF_19950315
# (dim filter, mid filter, fact filter); hits per aligned 64-row window of
# the 60,133 lineitem rows at SF 0.01:
LADDER = {
    # mean 3.15, 24 % of windows empty
    "a_default": ((1, "==", 0), (2, "<", CUT), (3, ">", CUT)),
    # mean 34.45, min 22, max 47: both sides of half a wave (a paired-lane
    # flush of the two adds drains 32 hits per instruction)
    # (83 windows at exactly 32, 95 at exactly 33)
    "b_straddle32": ((1, ">=", 0), (2, ">=", -2922), (3, ">", CUT)),
    # every row hits: 64 per window, and the partial last window of 37
    "c_all": ((1, ">=", 0), (2, ">=", -2922), (3, ">=", -2921)),
    # no row hits: zero groups
    "d_none": ((1, ">=", 0), (2, ">=", -2922), (3, ">", -396)),
}
_OPS = {"==": np.equal, "<": np.less, ">": np.greater, ">=": np.greater_equal}


def _brute(rows, plan):
    c, o, w = rows
    (_, dop, dlit), (_, mop, mlit), (_, fop, flit) = plan
    ckeys = c["c_custkey"][_OPS[dop](c["c_mktsegment"], dlit)]
    om = _OPS[mop](o["o_orderdate"], mlit) & np.isin(o["o_custkey"], ckeys)
    okeys = o["o_orderkey"][om]
    lm = _OPS[fop](w["l_shipdate"], flit) & np.isin(w["l_orderkey"], okeys)
    keys, inv, counts = np.unique(w["l_orderkey"][lm], return_inverse=True,
                                  return_counts=True)
    val = w["l_extendedprice"][lm] * (1.0 - w["l_discount"][lm])
    rev = np.bincount(inv, weights=val, minlength=len(keys))
    at = np.searchsorted(o["o_orderkey"][om], keys)   # o_orderkey ascending
    return {"fact_mask": lm,
            "l_orderkey": keys, "nitems": counts, "revenue": rev,
            "o_orderdate": o["o_orderdate"][om][at],
            "o_shippriority": o["o_shippriority"][om][at]}


def _window_hits(mask):
    """hits per aligned 64-row window (what one wave sees per iteration)"""
    pad = np.zeros((len(mask) + 63) // 64 * 64, dtype=bool)
    pad[:len(mask)] = mask
    return pad.reshape(-1, 64).sum(axis=1)


@pytest.mark.parametrize("name", list(LADDER))
def test_hit_density_ladder(ctx, rows001, name):
    plan = LADDER[name]
    assert len(rows001[2]["l_orderkey"]) == 60133
    assert np.all(np.diff(rows001[1]["o_orderkey"]) > 0)
    want = _brute(rows001, plan)
    # the plans must really have the densities they are named for
    h = _window_hits(want["fact_mask"])
    if name == "a_default":
        assert 3.0 < h.mean() < 3.3 and 0.2 < (h == 0).mean() < 0.3
    if name == "b_straddle32":
        assert (h.min(), h.max()) == (22, 47)
        assert ((h == 32).sum(), (h == 33).sum()) == (83, 95)
        assert 0.3 < (h <= 32).mean() < 0.35
    if name == "c_all":
        assert (h[:-1] == 64).all() and h[-1] == 60133 % 64 == 37
        assert int(want["nitems"].sum()) == 60133
    if name == "d_none":
        assert h.max() == 0 and len(want["l_orderkey"]) == 0
    cust, ordr, li = _gen(ctx, 0.01)
    desc = {"dim": cust, "dim_key_col": 0, "dim_filter": plan[0],
            "mid": ordr, "mid_key_col": 0, "mid_fk_col": 1,
            "mid_attr1_col": 2, "mid_attr2_col": 3, "mid_filter": plan[1],
            "fact": li, "fact_key_col": 0, "fact_a_col": 1, "fact_b_col": 2,
            "fact_filter": plan[2]}
    q = ctx.q3_desc(desc).run()
    got = q.result()
    assert q.stats()["probe_hits"] == int(want["nitems"].sum())
    assert len(got["l_orderkey"]) == len(want["l_orderkey"])
    if len(want["l_orderkey"]):
        _assert_q3(got, want)
    q.free(); li.free(); ordr.free(); cust.free()


# ---------------- 3. extract geometry ----------------

def test_extract_table_smaller_than_one_tile(ctx, orc):
    sf = 0.001
    cust, ordr, li = _gen(ctx, sf)
    q = ctx.q3(cust, ordr, li).run()
    c, o, w = orc.gen_customer(sf), orc.gen_orders(sf), orc.gen_lineitem(sf)
    want = orc.q3(c, o, w)
    # slots = pow2 >= 3 x qualifying orders: well under the 2,048-slot tile
    qual = int(((o["o_orderdate"] < CUT) &
                np.isin(o["o_custkey"], c["c_custkey"][c["c_mktsegment"] == 0])).sum())
    assert 0 < qual and 2 * (3 * qual + 1) < 2048
    assert len(want["l_orderkey"]) > 0
    _assert_q3(q.result(), want)
    q.free(); li.free(); ordr.free(); cust.free()


@pytest.mark.parametrize("tf", [100, 1600])
def test_extract_table_factor(ctx, want005, monkeypatch, tf):
    """dense (load factor 0.5-1) and sparse (0.03-0.06) tables"""
    monkeypatch.setenv("GX_TABLE_FACTOR_PCT", str(tf))
    cust, ordr, li = _gen(ctx, 0.05)
    q = ctx.q3(cust, ordr, li).run()
    _assert_q3(q.result(), want005)
    q.free(); li.free(); ordr.free(); cust.free()


# ---------------- 4. count type ----------------

def test_numeric_mode_keeps_u64_slot(ctx, orc, rows001):
    """numeric mode views the same 16 bytes as {u64, u64}: sums and counts
    stay bit-exact beside the f64-count default path"""
    cust, ordr, li = _gen(ctx, 0.01, gx.TPCH_LINEITEM_NUMERIC)
    q = ctx.q3(cust, ordr, li, numeric=True).run()
    got = q.result()
    want = orc.q3_numeric(*rows001)
    np.testing.assert_array_equal(got["l_orderkey"], want["l_orderkey"])
    np.testing.assert_array_equal(got["o_orderdate"], want["o_orderdate"])
    np.testing.assert_array_equal(got["o_shippriority"], want["o_shippriority"])
    np.testing.assert_array_equal(got["revenue_num"], want["revenue_num"])
    np.testing.assert_array_equal(got["nitems"], want["nitems"])
    # a second run claims the slots that hold the first run's u64 sums
    again = q.run().result()
    for f in ("l_orderkey", "o_orderdate", "o_shippriority", "revenue_num",
              "nitems"):
        np.testing.assert_array_equal(again[f], want[f])
    q.free(); li.free(); ordr.free(); cust.free()

"""CPU checks of the two pure host pieces at the tail of the Q3 pipeline, run
through their no-GPU symbols: the bound that sizes the LEFT-OUTER unmatched
table (gx_selftest_unmatched_bound) and the host merge of the top-N stage's
per-block candidates (gx_selftest_topn_merge).  gx_q3_run and gx_q3_topn call
the same two functions."""
import numpy as np
import pytest

import cloudberry_amd as gx

U64 = 2**64
I64_MIN, I64_MAX = -2**63, 2**63 - 1
I32_MAX = np.iinfo(np.int32).max


# ---------------- unmatched-table bound ----------------

def _true_floor(nrows, lmin, lmax):
    """min(nrows, true span) + 1 in exact integers: the distinct keys of a
    column cannot exceed either, and one more slot holds the NULL-key group."""
    span = lmax - lmin + 1 if (nrows > 0 and lmax >= lmin) else 0
    return min(nrows, span) + 1


@pytest.mark.parametrize("lmin,lmax,nrows", [
    (0, U64 - 1, 1000),        # a 0 (or a NULL decoded as 0) next to a -1:
    (0, U64 - 1, 2),           # the span is 2^64 and wraps to 0 in a uint64
    (0, U64 - 1, 1 << 40),
    (0, 0, 1000),              # one distinct key
    (5, 4, 0),                 # empty column: stats stay at their seeds
    (U64 - 1, 0, 0),           # ... as the min/max kernel seeds them
    (1, 2**63, 1000),          # INT64_MIN as an unsigned word
    (1, 2**63, 3),
    (10, 19, 1000),            # small dense range below nrows
    (10, 19, 4),               # ... and above it
    (2**63 - 5, 2**63 + 5, 100),   # negative and positive keys mixed
    (1, U64 - 1, 7),           # span 2^64 - 1: the largest that does not wrap
    (7, 7, 1),
])
def test_unmatched_bound_never_below_distinct_keys(lmin, lmax, nrows):
    got = gx.unmatched_bound(nrows, lmin, lmax)
    assert got >= _true_floor(nrows, lmin, lmax)
    # never wraps, never sizes past one slot per row plus the NULL group
    assert 1 <= got <= nrows + 1


def test_unmatched_bound_covers_brute_force_columns():
    """Random small columns from a domain that straddles both ends of the
    unsigned range: the bound from their unsigned min/max is never below the
    number of distinct keys plus the NULL group."""
    rng = np.random.default_rng(7)
    domain = np.array([0, 1, 2, 3, -1, -2, -5, I64_MIN, I64_MIN + 1, I64_MAX,
                       1 << 40, (1 << 40) + 1], np.int64)
    for _ in range(200):
        n = int(rng.integers(1, 30))
        col = rng.choice(domain, n)
        u = col.astype(np.uint64)
        got = gx.unmatched_bound(n, int(u.min()), int(u.max()))
        assert got >= len(np.unique(col)) + 1
        assert got <= n + 1


# ---------------- top-N candidate merge ----------------

def _cands(n, rng):
    """n valid candidates with distinct fields everywhere but (rev, date)."""
    return dict(cidx=np.arange(n, dtype=np.int64) * 3 + 1,
                okey=rng.permutation(n).astype(np.int64) + 100,
                odate=rng.integers(-3000, 3000, n).astype(np.int32),
                oprio=rng.integers(0, 5, n).astype(np.int32),
                rev=rng.uniform(-50, 50, n),
                cnt=rng.integers(1, 8, n).astype(np.int64),
                flags=np.zeros(n, np.uint8))


def _merge(c, topn=10, numeric=False):
    return gx.topn_merge(c["cidx"], c["okey"], c["odate"], c["oprio"],
                         c["rev"], c["cnt"], c["flags"], topn, numeric)


def _want_order(c, numeric=False):
    valid = np.flatnonzero(c["cidx"] >= 0)
    eff = np.where(c["flags"][valid] & 2, I32_MAX, c["odate"][valid])
    rev = c["rev"][valid]
    # numerators stay far below 2^63: negation is exact
    order = np.lexsort((eff, -rev))
    return valid[order], eff[order]


def _assert_rows(got, c, want_idx, numeric=False):
    np.testing.assert_array_equal(got["l_orderkey"], c["okey"][want_idx])
    np.testing.assert_array_equal(got["o_orderdate"], c["odate"][want_idx])
    np.testing.assert_array_equal(got["o_shippriority"], c["oprio"][want_idx])
    np.testing.assert_array_equal(got["nitems"], c["cnt"][want_idx])
    np.testing.assert_array_equal(got["key_is_null"], c["flags"][want_idx] & 1)
    np.testing.assert_array_equal(got["attrs_null"],
                                  (c["flags"][want_idx] >> 1) & 1)
    if numeric:
        np.testing.assert_array_equal(got["revenue_num"], c["rev"][want_idx])
        np.testing.assert_array_equal(got["revenue"],
                                      c["rev"][want_idx] / 1e4)
    else:
        np.testing.assert_array_equal(got["revenue"], c["rev"][want_idx])
        assert (got["revenue_num"] == 0).all()
    assert (got["_pad"] == 0).all()


@pytest.mark.parametrize("topn", [1, 3, 10])
def test_merge_every_key_is_data(topn):
    """Keys -1, INT64_MIN, 0, 1 and 2^40 carry the largest revenues and sit
    between empty candidates whose key fields hold the same values: all five
    come back, and no empty candidate does."""
    rng = np.random.default_rng(11)
    c = _cands(40, rng)
    special = np.array([-1, I64_MIN, 0, 1, 1 << 40], np.int64)
    at = np.array([3, 9, 17, 25, 39])
    c["okey"][at] = special
    c["rev"][at] = np.array([900.0, 800.0, 700.0, 600.0, 500.0])
    empty = np.array([0, 4, 10, 18, 26, 38])
    c["cidx"][empty] = -1
    c["okey"][empty] = np.array([-1, I64_MIN, 0, 1, 1 << 40, -1], np.int64)
    c["rev"][empty] = 1e9               # would win if it were considered
    got = _merge(c, topn)
    want_idx, _ = _want_order(c)
    assert len(got) == topn
    _assert_rows(got, c, want_idx[:topn])
    np.testing.assert_array_equal(got["l_orderkey"][:min(topn, 5)],
                                  special[:min(topn, 5)])


def test_merge_fewer_valid_than_topn_and_none():
    rng = np.random.default_rng(12)
    c = _cands(30, rng)
    c["cidx"][:] = -1
    assert len(_merge(c, 10)) == 0
    keep = np.array([2, 11, 29])
    c["cidx"][keep] = keep
    got = _merge(c, 10)
    want_idx, _ = _want_order(c)
    assert len(got) == 3 and sorted(want_idx) == keep.tolist()
    _assert_rows(got, c, want_idx)
    c0 = {k: v[:0] for k, v in c.items()}
    assert len(_merge(c0, 10)) == 0


def test_merge_order_revenue_desc_date_asc_null_dates_last():
    """Clusters of equal revenue: inside one the order is effective date
    ascending, where flag bit 1 (NULL date) ranks after every real date,
    whatever date value is stored with it."""
    rng = np.random.default_rng(13)
    n = 60
    c = _cands(n, rng)
    c["rev"] = np.repeat([5.0, -2.5, 0.0, 7.25, 5.0, -2.5], 10)
    c["odate"] = rng.permutation(n).astype(np.int32) - 30   # all distinct
    nulls = np.array([1, 12, 13, 27, 33, 48, 59])
    c["flags"][nulls] = 2
    c["odate"][nulls] = np.array([0, -5000, 7, I32_MAX - 1, 0, -1, 3],
                                 np.int32)
    c["flags"][[5, 12]] |= 1            # bit 0 does not enter the order
    c["cidx"][[0, 20, 41]] = -1
    want_idx, want_eff = _want_order(c)
    got = _merge(c, 10)
    # (rev, effective date) pairs are unique except among the NULL dates of
    # one revenue; compare the pair sequence, then the rows where unique
    got_eff = np.where(got["attrs_null"] == 1, I32_MAX, got["o_orderdate"])
    np.testing.assert_array_equal(got["revenue"], c["rev"][want_idx[:10]])
    np.testing.assert_array_equal(got_eff, want_eff[:10])
    # the ten rows of revenue 7.25 fill the whole top 10: the one NULL date
    # among them must be the last row
    assert (got["revenue"] == 7.25).all()
    assert got["attrs_null"][-1] == 1 and not got["attrs_null"][:-1].any()
    _assert_rows(got[:-1], c, want_idx[:9])
    # every cluster in turn, through a window that drops the rows above it
    for r in (5.0, 0.0, -2.5):
        c2 = {k: v.copy() for k, v in c.items()}
        c2["cidx"][c2["rev"] > r] = -1
        w_idx, w_eff = _want_order(c2)
        g = _merge(c2, 10)
        g_eff = np.where(g["attrs_null"] == 1, I32_MAX, g["o_orderdate"])
        np.testing.assert_array_equal(g["revenue"], c2["rev"][w_idx[:10]])
        np.testing.assert_array_equal(g_eff, w_eff[:10])


def test_merge_numeric_orders_by_int64_numerators():
    """Numeric mode hands the merge int64 numerators.  0, 1, 2, ... are
    denormal bit patterns as doubles and values near 2^62 differ only in
    low bits: the order is the integer order, and the numerators come back
    exact."""
    rng = np.random.default_rng(14)
    small = np.arange(0, 12, dtype=np.int64)
    big = (1 << 62) - np.arange(0, 12, dtype=np.int64)
    num = rng.permutation(np.concatenate([small, big]))
    n = len(num)
    c = _cands(n, rng)
    c["rev"] = num
    c["cidx"][int(np.flatnonzero(num == (1 << 62) - 3)[0])] = -1
    want_idx, _ = _want_order(c, numeric=True)
    got = _merge(c, 10, numeric=True)
    _assert_rows(got, c, want_idx[:10], numeric=True)
    # only the small ones: flushed to zero they would all tie
    c["cidx"][num > 100] = -1
    want_idx, _ = _want_order(c, numeric=True)
    got = _merge(c, 10, numeric=True)
    _assert_rows(got, c, want_idx[:10], numeric=True)
    np.testing.assert_array_equal(got["revenue_num"], np.arange(11, 1, -1))


@pytest.mark.parametrize("topn", [0, -1, 11])
def test_merge_rejects_bad_topn(topn):
    c = _cands(5, np.random.default_rng(15))
    with pytest.raises(ValueError):
        _merge(c, topn)

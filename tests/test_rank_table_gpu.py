"""Rank-addressed join/agg table of the Q3 local path: one bit per mid key of
[kmin, kmax] plus per-word prefix popcounts, a key's rank indexing dense
payload arrays; and the open-addressing hash table every other run keeps.

Every result is checked against the oracle or a numpy brute force of the
plan: keys, attrs and counts bit-equal, revenue within rtol=1e-6 (the f64
summation order differs).  Each case also pins which form the run used
(Q3.table_mode(): 0 hash, 1 rank)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

RTOL = 1e-6
I64_MAX = 2**63 - 1
TILE = 2048                     # slots of one extract tile (8 rows x 256)


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
def want001(orc):
    """oracle Q3 at SF 0.01 (shared, read-only)"""
    sf = 0.01
    return orc.q3(orc.gen_customer(sf), orc.gen_orders(sf), orc.gen_lineitem(sf))


@pytest.fixture(autouse=True)
def _default_env(monkeypatch):
    for v in ("GX_RANK_TABLE", "GX_DIM_BITMAP", "GX_FORCE_MOTION",
              "GX_TABLE_FACTOR_PCT"):
        monkeypatch.delenv(v, raising=False)


def _comm(ctx):
    try:
        ctx.comm_init(ctx.comm_unique_id())
    except gx.GxError:
        pass                    # communicator may already exist


def _assert_q3(got, want):
    np.testing.assert_array_equal(got["l_orderkey"], want["l_orderkey"])
    np.testing.assert_array_equal(got["o_orderdate"], want["o_orderdate"])
    np.testing.assert_array_equal(got["o_shippriority"], want["o_shippriority"])
    np.testing.assert_array_equal(got["nitems"], want["nitems"])
    np.testing.assert_allclose(got["revenue"], want["revenue"], rtol=RTOL)
    for f in ("key_is_null", "attrs_null"):
        if f in want:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f)


class Plan:
    """dim(1..100, keys 1..50 qualify) -> mid(o_keys in the given row order;
    row i passes the date filter and the dim semi join iff o_qual[i]) ->
    fact(li_keys), all bound through aocs_encode.  Rows with o_qual False
    fail the date filter or carry a non-qualifying fk, alternately.  Mid rows
    qualify on o_date < 0, fact rows on ship > 0.  Prices are whole cents and
    discounts whole hundredths, so the same rows serve numeric mode."""

    def __init__(self, ctx, orc, o_keys, o_qual, li_keys, seed=7,
                 o_hidden=None, li_hidden=None, li_null=None, rle=False,
                 numeric=False, ship_all=False):
        rng = np.random.default_rng(seed)
        enc = orc.aocs_encode
        self.ctx, self.numeric = ctx, numeric
        self.o_keys = np.asarray(o_keys, np.int64)
        o_qual = np.asarray(o_qual, bool)
        no = len(self.o_keys)
        bad_date = ~o_qual & (np.arange(no) % 2 == 0)
        bad_fk = ~o_qual & ~bad_date
        self.o_date = np.where(bad_date, rng.integers(0, 100, no),
                               rng.integers(-100, 0, no)).astype(np.int32)
        self.o_cust = np.where(bad_fk, rng.integers(51, 121, no),
                               rng.integers(1, 51, no)).astype(np.int64)
        self.o_prio = rng.integers(0, 5, no).astype(np.int32)
        self.o_hidden = None if o_hidden is None else np.asarray(o_hidden, bool)
        self.li_keys = np.asarray(li_keys, np.int64)
        nl = len(self.li_keys)
        self.li_hidden = None if li_hidden is None else np.asarray(li_hidden, bool)
        self.li_null = (np.zeros(nl, bool) if li_null is None
                        else np.asarray(li_null, bool))
        self.cents = rng.integers(100, 200000, nl).astype(np.int64)
        self.disc = rng.integers(0, 11, nl).astype(np.int64)
        self.ship = (np.ones(nl, np.int32) if ship_all
                     else rng.integers(-5, 45, nl).astype(np.int32))
        c_keys = np.arange(1, 101, dtype=np.int64)
        c_seg = (c_keys > 50).astype(np.int8)
        self.cust = ctx.bind([(enc(c_keys), 8, 100), (enc(c_seg), 1, 100)])
        self.ordr = ctx.bind([(enc(self.o_keys), 8, no), (enc(self.o_cust), 8, no),
                              (enc(self.o_date), 4, no), (enc(self.o_prio), 4, no)])
        if self.o_hidden is not None:
            self.ordr.set_visimap(self.o_hidden)
        if rle:
            key_stream = (orc.aocs_encode_rle(self.li_keys), 8, nl, 1)
        elif li_null is not None:
            key_stream = (orc.aocs_encode_orig_nulls(self.li_keys, self.li_null),
                          8, nl, 1)
        else:
            key_stream = (enc(self.li_keys), 8, nl)
        if numeric:
            a, b = self.cents, self.disc
        else:
            a, b = self.cents / 100.0, self.disc / 100.0
        self.li = ctx.bind([key_stream, (enc(a), 8, nl), (enc(b), 8, nl),
                            (enc(self.ship), 4, nl)])
        if self.li_hidden is not None:
            self.li.set_visimap(self.li_hidden)

    def free(self):
        self.li.free(); self.ordr.free(); self.cust.free()

    def qual_rows(self, dim_join="semi"):
        member = (self.o_cust >= 1) & (self.o_cust <= 50)
        if dim_join != "semi":
            member = ~member
        om = (self.o_date < 0) & member
        if self.o_hidden is not None:
            om &= ~self.o_hidden
        return om

    def brute(self, dim_join="semi", outer=False):
        om = self.qual_rows(dim_join)
        # a key on several qualifying rows: the rows are identical by design
        uk, first = np.unique(self.o_keys[om], return_index=True)
        u_date, u_prio = self.o_date[om][first], self.o_prio[om][first]
        lm = self.ship > 0
        if self.li_hidden is not None:
            lm &= ~self.li_hidden
        real = lm & ~self.li_null
        matched = real & np.isin(self.li_keys, uk)
        sel = real if outer else matched
        keys, inv, counts = np.unique(self.li_keys[sel], return_inverse=True,
                                      return_counts=True)
        num = np.zeros(len(keys), np.int64)
        np.add.at(num, inv, self.cents[sel] * (100 - self.disc[sel]))
        rev = np.zeros(len(keys))
        np.add.at(rev, inv, (self.cents[sel] / 100.0)
                  * (1.0 - self.disc[sel] / 100.0))
        hit = np.isin(keys, uk)
        at = np.searchsorted(uk, keys[hit])
        date = np.zeros(len(keys), np.int32)
        prio = np.zeros(len(keys), np.int32)
        date[hit], prio[hit] = u_date[at], u_prio[at]
        want = {"l_orderkey": keys, "o_orderdate": date, "o_shippriority": prio,
                "nitems": counts, "revenue": rev, "revenue_num": num,
                "key_is_null": np.zeros(len(keys), bool), "attrs_null": ~hit}
        nullsel = lm & self.li_null
        if outer and nullsel.any():     # the NULL-key group comes last
            tail = {"l_orderkey": 0, "o_orderdate": 0, "o_shippriority": 0,
                    "nitems": int(nullsel.sum()),
                    "revenue": float(((self.cents[nullsel] / 100.0)
                                      * (1.0 - self.disc[nullsel] / 100.0)).sum()),
                    "revenue_num": int((self.cents[nullsel]
                                        * (100 - self.disc[nullsel])).sum()),
                    "key_is_null": True, "attrs_null": True}
            want = {f: np.append(v, np.asarray(tail[f], v.dtype))
                    for f, v in want.items()}
        return want

    def q(self, dim_join="semi", outer=False):
        q = self.ctx.q3_desc({
            "dim": self.cust, "dim_key_col": 0, "dim_filter": (1, "==", 0),
            "mid": self.ordr, "mid_key_col": 0, "mid_fk_col": 1,
            "mid_attr1_col": 2, "mid_attr2_col": 3, "mid_filter": (2, "<", 0),
            "fact": self.li, "fact_key_col": 0, "fact_a_col": 1,
            "fact_b_col": 2, "fact_filter": (3, ">", 0),
            "dim_join": dim_join,
            "fact_join": "left_outer" if outer else "inner"})
        if self.numeric:
            q.set_numeric(True)
        return q

    def run(self, dim_join="semi", outer=False):
        q = self.q(dim_join, outer).run()
        got, mode = q.result(), q.table_mode()
        q.free()
        return got, mode

    def check(self, mode_want, dim_join="semi", outer=False):
        got, mode = self.run(dim_join, outer)
        assert mode == mode_want
        want = self.brute(dim_join, outer)
        _assert_q3(got, want)
        if self.numeric:
            np.testing.assert_array_equal(got["revenue_num"], want["revenue_num"])
        return want


def facts_for(rng, o_keys, planted=(), extra=3000, copies=3):
    """one fact row per mid key (a wrongly kept or dropped order is a wrong
    group), `extra` random repeats, each planted key `copies` times; sorted"""
    o_keys = np.asarray(o_keys, np.int64)
    return np.sort(np.concatenate([
        o_keys, rng.choice(o_keys, extra),
        np.repeat(np.asarray(planted, np.int64), copies)])).astype(np.int64)


# ---------------- 1. the default Q3 ----------------

def _default_q3(ctx):
    sf = 0.01
    t = (ctx.tpch_gen(gx.TPCH_CUSTOMER, sf), ctx.tpch_gen(gx.TPCH_ORDERS, sf),
         ctx.tpch_gen(gx.TPCH_LINEITEM, sf))
    return t, ctx.q3(*t)


def _free(t, q):
    q.free()
    for x in reversed(t):
        x.free()


def test_default_q3_rank_three_runs(ctx, want001):
    """TPC-H orderkeys are dense: the default plan takes the rank form.
    Three runs of one q: the per-run clears leave nothing behind."""
    t, q = _default_q3(ctx)
    for _ in range(3):
        _assert_q3(q.run().result(), want001)
        assert q.table_mode() == 1
    _free(t, q)


def test_default_q3_hash_when_switched_off(ctx, want001, monkeypatch):
    monkeypatch.setenv("GX_RANK_TABLE", "0")
    t, q = _default_q3(ctx)
    _assert_q3(q.run().result(), want001)
    assert q.table_mode() == 0
    _free(t, q)


def test_default_q3_forced_motion_keeps_hash(ctx, want001, monkeypatch):
    _comm(ctx)
    monkeypatch.setenv("GX_FORCE_MOTION", "1")
    t, q = _default_q3(ctx)
    _assert_q3(q.run().result(), want001)
    assert q.table_mode() == 0
    _free(t, q)


def test_one_q_local_motion_local(ctx, want001, monkeypatch):
    """each form allocates its own table at its first run; the shared result
    arrays stay valid for the other"""
    _comm(ctx)
    t, q = _default_q3(ctx)
    for force, mode in ((None, 1), ("1", 0), (None, 1)):
        if force is None:
            monkeypatch.delenv("GX_FORCE_MOTION", raising=False)
        else:
            monkeypatch.setenv("GX_FORCE_MOTION", force)
        _assert_q3(q.run().result(), want001)
        assert q.table_mode() == mode
    _free(t, q)


# ---------------- 2. range edges ----------------

@pytest.mark.parametrize("outer", [False, True], ids=["inner", "left_outer"])
@pytest.mark.parametrize("kmin", [1, 2**40 + 5], ids=["kmin1", "kmin2p40"])
def test_range_edges(ctx, orc, kmin, outer):
    """range 6437 = 100 words + 37 bits.  Qualifying: the first and the last
    key, bit 0 and bit 63 of word 3 with their neighbours not qualifying, all
    of word 7, none of word 9.  Fact keys just outside the range, past the
    last word, aliasing modulo 2^32, INT64_MAX and negative must not match;
    under LEFT OUTER they, and the NULL (decoded 0) key, are unmatched
    groups."""
    rng = np.random.default_rng(11)
    n = 64 * 100 + 37
    nwords = (n + 63) // 64
    keys = kmin + np.arange(n, dtype=np.int64)
    qual = rng.random(n) < 0.3
    qual[[0, n - 1, 192, 255]] = True
    qual[[191, 256]] = False
    qual[448:512] = True
    qual[576:640] = False
    kmax = kmin + n - 1
    outside = [kmin - 1, kmax + 1, kmin + 64 * nwords, kmin + 64 * nwords + 63,
               2**32 + kmin, I64_MAX, -5]
    li_null = None
    if outer:
        # a real fact key 0 is refused under LEFT OUTER; 0 arrives as NULL
        outside = [k for k in outside if k != 0]
    li_keys = facts_for(rng, keys, outside)
    if outer:
        li_keys = np.concatenate([li_keys, np.zeros(5, np.int64)])
        li_null = np.arange(len(li_keys)) >= len(li_keys) - 5
    p = Plan(ctx, orc, keys, qual, li_keys, li_null=li_null, ship_all=True)
    try:
        want = p.check(1, outer=outer)
        got_keys = want["l_orderkey"][~want["attrs_null"]]
        assert not np.isin(got_keys, outside).any()
        assert {kmin, kmax, kmin + 192, kmin + 255} <= set(got_keys.tolist())
        assert set((kmin + np.arange(448, 512)).tolist()) <= set(got_keys.tolist())
        assert not np.isin(got_keys, [kmin + 191, kmin + 256]).any()
        assert not np.isin(got_keys, kmin + np.arange(576, 640)).any()
        if outer:
            un = want["l_orderkey"][want["attrs_null"] & ~want["key_is_null"]]
            assert set(outside) <= set(un.tolist())
            assert want["key_is_null"][-1] and want["nitems"][-1] == 5
    finally:
        p.free()


# ---------------- 3. ranks across scan blocks ----------------

def test_ranks_across_scan_blocks(ctx, orc):
    """the key range spans four blocks of the prefix-popcount scan: block 1
    has no qualifying key, block 2 only qualifying keys, the rest random"""
    rng = np.random.default_rng(13)
    B = gx.rank_scan_block_keys()
    assert B % 64 == 0
    n = 3 * B + 1000
    keys = 17 + np.arange(n, dtype=np.int64)
    qual = rng.random(n) < 0.5
    qual[0] = qual[-1] = True
    qual[B:2 * B] = False
    qual[2 * B:3 * B] = True
    edges = 17 + np.array([0, B - 1, B, 2 * B - 1, 2 * B, 3 * B - 1, 3 * B, n - 1])
    li_keys = np.sort(np.concatenate([rng.choice(keys, 150000), edges]))
    p = Plan(ctx, orc, keys, qual, li_keys, ship_all=True)
    try:
        want = p.check(1)
        assert len(want["l_orderkey"]) > 50000
        kept = set(want["l_orderkey"].tolist())
        assert {17, 17 + 2 * B, 17 + 3 * B - 1, 17 + n - 1} <= kept
        assert not {17 + B, 17 + 2 * B - 1} & kept
    finally:
        p.free()


# ---------------- 4. eligibility ----------------

@pytest.mark.parametrize("span,mode_want", [(640, 1), (641, 0), (10**9, 0)],
                         ids=["range64n", "range64n+1", "sparse"])
def test_eligibility_boundary(ctx, orc, span, mode_want):
    """n qualifying keys over a range of `span`: the rank form needs
    range <= 64 n.  n = 10 for the first two, keys {1, 10^9} for the third."""
    rng = np.random.default_rng(19)
    kmin = 100
    if span == 10**9:
        qk = np.array([1, 10**9], np.int64)
        other = np.array([2, 3, 500, 10**9 - 1], np.int64)
    else:
        qk = np.concatenate([[kmin, kmin + span - 1],
                             kmin + 1 + rng.choice(span - 2, 8, replace=False)])
        other = np.setdiff1d(np.arange(kmin - 20, kmin + span + 20), qk)
    keys = np.concatenate([qk, other]).astype(np.int64)
    qual = np.arange(len(keys)) < len(qk)
    order = np.argsort(keys)
    keys, qual = keys[order], qual[order]
    p = Plan(ctx, orc, keys, qual,
             facts_for(rng, keys, [int(qk.min()) - 1, int(qk.max()) + 1], extra=500),
             ship_all=True)
    try:
        want = p.check(mode_want)
        np.testing.assert_array_equal(want["l_orderkey"], np.sort(qk))
    finally:
        p.free()


def test_no_qualifying_order(ctx, orc):
    rng = np.random.default_rng(23)
    keys = np.arange(1, 3001, dtype=np.int64)
    p = Plan(ctx, orc, keys, np.zeros(3000, bool), facts_for(rng, keys))
    try:
        got, mode = p.run()
        assert mode == 0
        assert len(got["l_orderkey"]) == 0
    finally:
        p.free()


# ---------------- 5. row order and duplicates ----------------

def test_mid_row_order_and_duplicates(ctx, orc):
    rng = np.random.default_rng(29)
    n = 64 * 300 + 5
    keys = 1000 + np.arange(n, dtype=np.int64)
    qual = rng.random(n) < 0.3
    qual[0] = qual[-1] = True
    li_keys = rng.permutation(facts_for(rng, keys, [999, 1000 + n]))
    orders = {"asc": np.arange(n), "desc": np.arange(n)[::-1],
              "shuffled": np.random.default_rng(31).permutation(n)}
    want = None
    for name, idx in orders.items():
        p = Plan(ctx, orc, keys[idx], qual[idx], li_keys, ship_all=True)
        try:
            got, mode = p.run()
            assert mode == 1, name
            w = p.brute()
            if want is None:
                want = w
                assert len(want["l_orderkey"]) > 1000
            # the attrs are drawn per row position: compare to this plan's own
            np.testing.assert_array_equal(w["l_orderkey"], want["l_orderkey"])
            _assert_q3(got, w)
        finally:
            p.free()


@pytest.mark.parametrize("order", ["adjacent", "shuffled"])
def test_mid_key_on_two_identical_rows(ctx, orc, order):
    rng = np.random.default_rng(37)
    n = 5000
    keys = 1 + np.arange(n, dtype=np.int64)
    qual = rng.random(n) < 0.4
    qual[0] = qual[-1] = True
    li_keys = rng.permutation(facts_for(rng, keys))
    p = Plan(ctx, orc, keys, qual, li_keys, ship_all=True)
    idx = np.repeat(np.arange(n), 1 + qual)          # qualifying rows twice
    if order == "shuffled":
        idx = np.random.default_rng(41).permutation(idx)
    # a second mid table holding the duplicated rows of the first, verbatim
    enc = orc.aocs_encode
    m = len(idx)
    ordr2 = ctx.bind([(enc(p.o_keys[idx]), 8, m), (enc(p.o_cust[idx]), 8, m),
                      (enc(p.o_date[idx]), 4, m), (enc(p.o_prio[idx]), 4, m)])
    try:
        want = p.brute()
        p.ordr.free()
        p.ordr = ordr2
        got, mode = p.run()
        assert mode == 1
        _assert_q3(got, want)
    finally:
        p.free()


def test_mid_key_on_a_qualifying_and_a_failing_row(ctx, orc):
    """every key twice: one row fails the filter and carries other attrs;
    the qualifying row's attrs come back whichever row is first"""
    rng = np.random.default_rng(43)
    n = 4000
    keys = 1 + np.arange(n, dtype=np.int64)
    both = np.concatenate([keys, keys])
    qual = np.concatenate([np.ones(n, bool), np.zeros(n, bool)])
    perm = rng.permutation(2 * n)
    both, qual = both[perm], qual[perm]
    drop = rng.random(n) < 0.5                       # keys with no good row
    qual &= ~drop[both - 1]
    p = Plan(ctx, orc, both, qual, facts_for(rng, keys), ship_all=True)
    try:
        want = p.check(1)
        np.testing.assert_array_equal(want["l_orderkey"], keys[~drop])
    finally:
        p.free()


# ---------------- 6. the other kernel forms ----------------

def _dense_plan_args(seed, n=64 * 150 + 9, kmin=1, frac=0.4):
    rng = np.random.default_rng(seed)
    keys = kmin + np.arange(n, dtype=np.int64)
    qual = rng.random(n) < frac
    qual[0] = qual[-1] = True
    return rng, keys, qual


def test_visimap_on_mid_hides_qualifying_rows(ctx, orc):
    rng, keys, qual = _dense_plan_args(47)
    hidden = rng.random(len(keys)) < 0.3
    hidden[0] = True                 # the first key goes: the range shrinks
    assert (qual & hidden).sum() > 100
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys), o_hidden=hidden,
             ship_all=True)
    try:
        want = p.check(1)
        assert not np.isin(want["l_orderkey"], keys[hidden]).any()
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual & ~hidden])
    finally:
        p.free()


@pytest.mark.parametrize("outer", [False, True], ids=["inner", "left_outer"])
def test_visimap_on_fact(ctx, orc, outer):
    rng, keys, qual = _dense_plan_args(53)
    li_keys = facts_for(rng, keys, [len(keys) + 1, -3])
    hidden = rng.random(len(li_keys)) < 0.4
    p = Plan(ctx, orc, keys, qual, li_keys, li_hidden=hidden)
    try:
        p.check(1, outer=outer)
    finally:
        p.free()


@pytest.mark.parametrize("dim_join", ["anti", "anti_notin"])
def test_anti_joins(ctx, orc, dim_join):
    rng, keys, qual = _dense_plan_args(59)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys))
    try:
        want = p.check(1, dim_join=dim_join)
        assert len(want["l_orderkey"]) > 1000
    finally:
        p.free()


def test_hash_dim_set_with_rank_table(ctx, orc, monkeypatch):
    monkeypatch.setenv("GX_DIM_BITMAP", "0")
    rng, keys, qual = _dense_plan_args(61)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys))
    try:
        q = p.q().run()
        assert (q.dim_mode(), q.table_mode()) == (0, 1)
        _assert_q3(q.result(), p.brute())
        q.free()
    finally:
        p.free()


# ---------------- 7. form fallbacks ----------------

def test_numeric_mode_runs_hash_form(ctx, orc):
    rng, keys, qual = _dense_plan_args(67)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys), numeric=True)
    try:
        p.check(0)
    finally:
        p.free()


def test_fused_rle_fact_key_runs_hash_form(ctx, orc):
    rng, keys, qual = _dense_plan_args(71)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys), rle=True)
    try:
        p.check(0)
    finally:
        p.free()


def test_rank_then_numeric_on_one_q(ctx, orc):
    """a q that ran in rank form allocates the hash table when numeric mode
    first needs it.  The f64 run reads the scaled-integer measures as
    doubles: only its form is of interest."""
    rng, keys, qual = _dense_plan_args(73)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys), numeric=True)
    try:
        q = p.q()
        q.set_numeric(False)
        q.run()
        assert q.table_mode() == 1
        want = p.brute()
        np.testing.assert_array_equal(q.result()["l_orderkey"], want["l_orderkey"])
        q.set_numeric(True)
        got = q.run().result()
        assert q.table_mode() == 0
        _assert_q3(got, want)
        np.testing.assert_array_equal(got["revenue_num"], want["revenue_num"])
        q.free()
    finally:
        p.free()


# ---------------- 8. sizes ----------------

@pytest.mark.parametrize("nqual", [TILE - 1, TILE, TILE + 1])
def test_qual_around_one_extract_tile(ctx, orc, nqual):
    rng = np.random.default_rng(79)
    n = 3 * TILE
    keys = 5 + np.arange(n, dtype=np.int64)
    qual = np.zeros(n, bool)
    qual[rng.choice(n, nqual, replace=False)] = True
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys), ship_all=True)
    try:
        assert p.qual_rows().sum() == nqual
        want = p.check(1)
        assert len(want["l_orderkey"]) == nqual     # every qualifying order hit
    finally:
        p.free()


def test_no_fact_row_hits(ctx, orc):
    rng, keys, qual = _dense_plan_args(83)
    li_keys = np.sort(np.concatenate([keys[~qual], [0, -1, len(keys) + 1]]))
    p = Plan(ctx, orc, keys, qual, li_keys, ship_all=True)
    try:
        got, mode = p.run()
        assert mode == 1
        assert len(got["l_orderkey"]) == 0
    finally:
        p.free()


# ---------------- 9. the hash form keeps its cover ----------------

def test_hash_form_table_smaller_than_one_tile(ctx, orc, monkeypatch):
    monkeypatch.setenv("GX_RANK_TABLE", "0")
    sf = 0.001
    t = (ctx.tpch_gen(gx.TPCH_CUSTOMER, sf), ctx.tpch_gen(gx.TPCH_ORDERS, sf),
         ctx.tpch_gen(gx.TPCH_LINEITEM, sf))
    q = ctx.q3(*t).run()
    assert q.table_mode() == 0
    c, o, w = orc.gen_customer(sf), orc.gen_orders(sf), orc.gen_lineitem(sf)
    want = orc.q3(c, o, w)
    nq = int(((o["o_orderdate"] < gx.CUTOFF_19950315) &
              np.isin(o["o_custkey"], c["c_custkey"][c["c_mktsegment"] == 0])).sum())
    assert 0 < nq and 2 * (3 * nq + 1) < TILE
    assert len(want["l_orderkey"]) > 0
    _assert_q3(q.result(), want)
    _free(t, q)


@pytest.mark.parametrize("tf", [100, 1600])
def test_hash_form_table_factor(ctx, want001, monkeypatch, tf):
    """dense (load factor 0.5-1) and sparse (0.03-0.06) hash tables"""
    monkeypatch.setenv("GX_RANK_TABLE", "0")
    monkeypatch.setenv("GX_TABLE_FACTOR_PCT", str(tf))
    t, q = _default_q3(ctx)
    _assert_q3(q.run().result(), want001)
    assert q.table_mode() == 0
    _free(t, q)

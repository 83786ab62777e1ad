"""Dimension membership of the Q3 mid-table filter: the exact bitmap that
dense (sequence) dim keys get on the local path, and the bloom + hash set
every other case keeps.

Every result is checked against the oracle or a numpy brute force of the
plan: keys, attrs and counts bit-equal, revenue within rtol=1e-6 (the f64
summation order differs).  Each case also pins which form the run read
(Q3.dim_mode(): 0 hash, 1 bitmap)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

RTOL = 1e-6
NO, NL = 20000, 30000           # order rows, extra fact rows (plus one per order)


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
    monkeypatch.delenv("GX_DIM_BITMAP", raising=False)
    monkeypatch.delenv("GX_FORCE_MOTION", raising=False)


def _assert_q3(got, want):
    np.testing.assert_array_equal(got["l_orderkey"], want["l_orderkey"])
    np.testing.assert_array_equal(got["o_orderdate"], want["o_orderdate"])
    np.testing.assert_array_equal(got["o_shippriority"], want["o_shippriority"])
    np.testing.assert_array_equal(got["nitems"], want["nitems"])
    np.testing.assert_allclose(got["revenue"], want["revenue"], rtol=RTOL)


class Plan:
    """dim(c_keys, c_seg) -> orders(o_cust fks) -> fact, all bound through
    aocs_encode.  The dim qualifies on c_seg == 0 (or text == BUILDING), the
    orders on o_date < 0, the fact rows on ship > 0."""

    def __init__(self, ctx, orc, c_keys, c_seg, o_cust, seed=7, text=False,
                 hidden=None):
        rng = np.random.default_rng(seed)
        enc = orc.aocs_encode
        self.ctx = ctx
        self.c_keys = np.asarray(c_keys, np.int64)
        self.c_seg = np.asarray(c_seg, np.int8)
        self.hidden = hidden
        self.text = text
        no = len(o_cust)
        self.o_keys = np.arange(1, no + 1, dtype=np.int64)
        self.o_cust = np.asarray(o_cust, np.int64)
        self.o_date = rng.integers(-100, 100, no).astype(np.int32)
        self.o_prio = rng.integers(0, 5, no).astype(np.int32)
        # every order has a fact row, so a wrongly kept order is a wrong group
        self.li_keys = np.sort(np.concatenate(
            [self.o_keys, rng.integers(1, no + 1, NL)])).astype(np.int64)
        nl = len(self.li_keys)
        self.price = rng.uniform(1, 50, nl)
        self.disc = rng.integers(0, 11, nl) / 100.0
        self.ship = rng.integers(-5, 95, nl).astype(np.int32)
        nc = len(self.c_keys)
        if text:
            segs = [b"BUILDING", b"AUTOMOBILE", b"MACHINERY", b"HOUSEHOLD"]
            strings = [segs[min(int(s), 3)] for s in self.c_seg]
            seg_col = (orc.aocs_encode_varlena(strings), -1, nc, 1)
        else:
            seg_col = (enc(self.c_seg), 1, nc)
        self.cust = ctx.bind([(enc(self.c_keys), 8, nc), seg_col])
        if hidden is not None:
            self.cust.set_visimap(hidden)
        self.ordr = ctx.bind([(enc(self.o_keys), 8, no), (enc(self.o_cust), 8, no),
                              (enc(self.o_date), 4, no), (enc(self.o_prio), 4, no)])
        self.li = ctx.bind([(enc(self.li_keys), 8, nl), (enc(self.price), 8, nl),
                            (enc(self.disc), 8, nl), (enc(self.ship), 4, nl)])

    def free(self):
        self.li.free(); self.ordr.free(); self.cust.free()

    def qual_keys(self):
        m = self.c_seg == 0
        if self.hidden is not None:
            m &= ~np.asarray(self.hidden, bool)
        return self.c_keys[m]

    def brute(self, dim_join="semi"):
        member = np.isin(self.o_cust, self.qual_keys())
        if dim_join != "semi":
            member = ~member
        om = (self.o_date < 0) & member
        lm = (self.ship > 0) & np.isin(self.li_keys, self.o_keys[om])
        keys, inv, counts = np.unique(self.li_keys[lm], return_inverse=True,
                                      return_counts=True)
        rev = np.zeros(len(keys))
        np.add.at(rev, inv, self.price[lm] * (1.0 - self.disc[lm]))
        return {"l_orderkey": keys, "o_orderdate": self.o_date[keys - 1],
                "o_shippriority": self.o_prio[keys - 1], "nitems": counts,
                "revenue": rev}

    def run(self, dim_join="semi"):
        q = self.ctx.q3_desc({
            "dim": self.cust, "dim_key_col": 0,
            "dim_filter": (1, "==", "BUILDING" if self.text else 0),
            "mid": self.ordr, "mid_key_col": 0, "mid_fk_col": 1,
            "mid_attr1_col": 2, "mid_attr2_col": 3, "mid_filter": (2, "<", 0),
            "fact": self.li, "fact_key_col": 0, "fact_a_col": 1,
            "fact_b_col": 2, "fact_filter": (3, ">", 0),
            "dim_join": dim_join}).run()
        got, mode = q.result(), q.dim_mode()
        q.free()
        return got, mode


def dense_dim(rng, kmin, n, frac=0.2):
    """keys kmin..kmin+n-1 in ascending rows; seg 0 (qualifying) on ~frac of
    them and always on the first and the last key"""
    keys = kmin + np.arange(n, dtype=np.int64)
    seg = np.where(rng.random(n) < frac, 0, rng.integers(1, 4, n)).astype(np.int8)
    seg[0] = seg[-1] = 0
    return keys, seg


def fks_with(rng, base_lo, base_hi, planted, no=NO, copies=8):
    """random in-range fks with each planted value on `copies` rows that
    sit between ordinary neighbours"""
    fk = rng.integers(base_lo, base_hi + 1, no).astype(np.int64)
    pos = rng.choice(np.arange(1, no - 1), len(planted) * copies, replace=False)
    fk[pos] = np.repeat(np.asarray(planted, np.int64), copies)
    return fk


# ---------------- 1. the default Q3 in both forms ----------------

def _default_q3(ctx):
    sf = 0.01
    t = (ctx.tpch_gen(gx.TPCH_CUSTOMER, sf), ctx.tpch_gen(gx.TPCH_ORDERS, sf),
         ctx.tpch_gen(gx.TPCH_LINEITEM, sf))
    return t, ctx.q3(*t)


def test_default_q3_bitmap_three_runs(ctx, want001):
    """TPC-H custkeys are a sequence: the default plan takes the bitmap.
    Three runs of one q: the per-run clear leaves nothing behind."""
    t, q = _default_q3(ctx)
    for _ in range(3):
        _assert_q3(q.run().result(), want001)
        assert q.dim_mode() == 1
    q.free()
    for x in reversed(t):
        x.free()


def test_default_q3_hash_when_switched_off(ctx, want001, monkeypatch):
    monkeypatch.setenv("GX_DIM_BITMAP", "0")
    t, q = _default_q3(ctx)
    _assert_q3(q.run().result(), want001)
    assert q.dim_mode() == 0
    q.free()
    for x in reversed(t):
        x.free()


def test_default_q3_forced_motion_keeps_set_and_bloom(ctx, want001, monkeypatch):
    """the Motion path reads set + bloom whatever sizing chose"""
    try:
        ctx.comm_init(ctx.comm_unique_id())
    except gx.GxError:
        pass    # communicator may already exist
    monkeypatch.setenv("GX_FORCE_MOTION", "1")
    t, q = _default_q3(ctx)
    _assert_q3(q.run().result(), want001)
    assert q.dim_mode() == 0
    q.free()
    for x in reversed(t):
        x.free()


# ---------------- 2. range edges ----------------

@pytest.mark.parametrize("kmin", [1, 2**40 + 5], ids=["kmin1", "kmin2p40"])
def test_range_edges(ctx, orc, kmin):
    """range 6437 = 100 words + 37 bits.  Qualifying: first and last key,
    bit 0 and bit 63 of a word, and one whole word whose 64 keys sit in the
    64 rows of one wave.  fks just outside the range, past the last word,
    aliasing modulo 2^32, 0, INT64_MAX and negative must not match."""
    rng = np.random.default_rng(11)
    n = 64 * 100 + 37
    keys, seg = dense_dim(rng, kmin, n)
    seg[192] = 0                     # bit 0 of word 3
    seg[255] = 0                     # bit 63 of word 3
    seg[256] = seg[319] = 1          # their neighbours in word 4 do not qualify
    seg[448:512] = 0                 # word 7 entirely, rows 448..511 = wave 7
    kmax = kmin + n - 1
    nwords = (n + 63) // 64
    outside = [kmin - 1, kmax + 1, 0, kmin + 64 * nwords, 2**32 + kmin,
               2**63 - 1, -5, kmin - 64, kmin + 64 * nwords + 63]
    inside = [kmin, kmax, kmin + 192, kmin + 255, kmin + 256, kmin + 319,
              kmin + 448, kmin + 511, kmin + 447, kmin + 512]
    p = Plan(ctx, orc, keys, seg,
             fks_with(rng, kmin, kmax, outside + inside, copies=16))
    try:
        got, mode = p.run()
        assert mode == 1
        want = p.brute()
        _assert_q3(got, want)
        kept_fk = p.o_cust[want["l_orderkey"] - 1]
        assert not np.isin(kept_fk, outside).any()
        assert {kmin, kmax, kmin + 192, kmin + 255} <= set(kept_fk.tolist())
        assert not np.isin(kept_fk, [kmin + 256, kmin + 319]).any()
    finally:
        p.free()


# ---------------- 3. degenerate sets ----------------

def test_one_qualifying_key(ctx, orc):
    rng = np.random.default_rng(13)
    keys = np.arange(1, 3001, dtype=np.int64)
    seg = np.ones(3000, np.int8)
    seg[1234] = 0                                   # key 1235, range 1
    p = Plan(ctx, orc, keys, seg,
             fks_with(rng, 1200, 1270, [1235, 1234, 1236, 1235 + 64, 0], copies=40))
    try:
        got, mode = p.run()
        assert mode == 1
        want = p.brute()
        assert len(want["l_orderkey"]) > 0
        _assert_q3(got, want)
        assert (p.o_cust[want["l_orderkey"] - 1] == 1235).all()
    finally:
        p.free()


@pytest.mark.parametrize("dim_join", ["semi", "anti"])
def test_no_qualifying_key(ctx, orc, dim_join):
    rng = np.random.default_rng(17)
    keys = np.arange(1, 3001, dtype=np.int64)
    p = Plan(ctx, orc, keys, np.ones(3000, np.int8), fks_with(rng, 1, 3000, [0]))
    try:
        got, mode = p.run(dim_join)
        assert mode == 0             # nothing to span: the empty hash set
        want = p.brute(dim_join)
        _assert_q3(got, want)
        if dim_join == "semi":
            assert len(got["l_orderkey"]) == 0
        else:                        # every date-passing order with a fact row
            lm = (p.ship > 0) & np.isin(p.li_keys, p.o_keys[p.o_date < 0])
            np.testing.assert_array_equal(got["l_orderkey"],
                                          np.unique(p.li_keys[lm]))
    finally:
        p.free()


# ---------------- 4. eligibility boundary ----------------

@pytest.mark.parametrize("span,mode_want", [(640, 1), (641, 0), (10**9, 0)],
                         ids=["range64n", "range64n+1", "sparse"])
def test_eligibility_boundary(ctx, orc, span, mode_want):
    """n qualifying keys over a range of `span`: the bitmap needs
    range <= 64 n.  n = 10 for the first two, keys {1, 10^9} for the third."""
    rng = np.random.default_rng(19)
    kmin = 100
    if span == 10**9:
        qual = np.array([1, 10**9], np.int64)
        other = np.array([2, 3, 500, 10**9 - 1], np.int64)
    else:
        qual = np.concatenate([[kmin, kmin + span - 1],
                               kmin + 1 + rng.choice(span - 2, 8, replace=False)])
        other = np.setdiff1d(np.arange(kmin - 20, kmin + span + 20), qual)
    keys = np.concatenate([qual, other]).astype(np.int64)
    seg = np.concatenate([np.zeros(len(qual), np.int8), np.ones(len(other), np.int8)])
    order = np.argsort(keys)
    planted = list(qual) + [int(qual.min()) - 1, int(qual.max()) + 1, 0]
    p = Plan(ctx, orc, keys[order], seg[order],
             fks_with(rng, int(qual.min()) - 20, int(qual.min()) + 700, planted,
                      copies=30))
    try:
        got, mode = p.run()
        assert mode == mode_want
        want = p.brute()
        assert len(want["l_orderkey"]) > 0
        _assert_q3(got, want)
    finally:
        p.free()


# ---------------- 5. anti joins on the bitmap ----------------

@pytest.mark.parametrize("dim_join", ["anti", "anti_notin"])
def test_anti_joins_bitmap(ctx, orc, dim_join):
    rng = np.random.default_rng(23)
    kmin, n = 1000, 5000
    keys, seg = dense_dim(rng, kmin, n, frac=0.5)
    outside = [kmin - 1, kmin + n, 1, 2**32 + kmin, 2**63 - 1, -7,
               kmin + 64 * ((n + 63) // 64)]
    p = Plan(ctx, orc, keys, seg, fks_with(rng, kmin - 50, kmin + n + 50, outside))
    try:
        got, mode = p.run(dim_join)
        assert mode == 1
        want = p.brute(dim_join)
        _assert_q3(got, want)
        # an anti join keeps the fks outside the range
        kept_fk = set(p.o_cust[want["l_orderkey"] - 1].tolist())
        assert set(outside) <= kept_fk
    finally:
        p.free()


# ---------------- 6. dimension row order and duplicates ----------------

def test_dim_row_order_and_duplicates(ctx, orc):
    rng = np.random.default_rng(29)
    keys, seg = dense_dim(rng, 17, 64 * 300 + 5, frac=0.3)
    fk = fks_with(rng, 1, 17 + len(keys) + 30, [16, 17, 17 + len(keys)])
    perm = np.random.default_rng(31).permutation(len(keys))
    dup = np.repeat(np.arange(len(keys)), 1 + (seg == 0))   # qualifying twice
    orders = {"asc": np.arange(len(keys)), "desc": np.arange(len(keys))[::-1],
              "shuffled": perm, "dup_adjacent": dup,
              "dup_shuffled": np.random.default_rng(37).permutation(dup)}
    want = None
    for name, idx in orders.items():
        p = Plan(ctx, orc, keys[idx], seg[idx], fk)
        try:
            got, mode = p.run()
            assert mode == 1, name
            if want is None:
                want = p.brute()
                assert len(want["l_orderkey"]) > 1000
            _assert_q3(got, want)
        finally:
            p.free()


# ---------------- 7. the other build kernels ----------------

def test_visimap_hides_qualifying_keys(ctx, orc):
    rng = np.random.default_rng(41)
    keys, seg = dense_dim(rng, 1, 64 * 150 + 9, frac=0.4)
    hidden = rng.random(len(keys)) < 0.3
    hidden[0] = True                 # the first key goes: the range shrinks
    assert ((seg == 0) & hidden).sum() > 100
    p = Plan(ctx, orc, keys, seg, fks_with(rng, 1, len(keys) + 5, [1, 0]),
             hidden=hidden)
    try:
        got, mode = p.run()
        assert mode == 1
        want = p.brute()
        _assert_q3(got, want)
        hidden_keys = keys[(seg == 0) & hidden]
        assert not np.isin(p.o_cust[want["l_orderkey"] - 1], hidden_keys).any()
    finally:
        p.free()


def test_text_dim_filter_bitmap(ctx, orc):
    """texteq dim filter: the flat-mask build kernel (k_cust_build_mask)"""
    rng = np.random.default_rng(43)
    keys, seg = dense_dim(rng, 5, 64 * 40 + 21, frac=0.3)
    p = Plan(ctx, orc, keys, seg, fks_with(rng, 1, len(keys) + 40, [4, 0]),
             text=True)
    try:
        got, mode = p.run()
        assert mode == 1
        want = p.brute()
        assert len(want["l_orderkey"]) > 1000
        _assert_q3(got, want)
    finally:
        p.free()

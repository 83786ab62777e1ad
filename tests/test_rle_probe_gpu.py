"""The fused RLE fact-key probe (k_li_probe_agg_rle) on every block shape a
conforming writer emits, and the prepare-time routing around it.

One small synthetic Q3 per case: a few thousand customers and orders bound
plain, a fact table whose KEY column is the thing under test, plain measures
and ship date.  Every case is checked three ways:

- brute force: the plan evaluated in numpy with math.fsum per group; keys,
  nitems and stats()["probe_hits"] bit-equal, revenue within
  (n_max + 2) * 2^-52 relative, n_max the case's largest group (positive terms
  in any summation order, plus the two roundings of p * (1 - d));
- plain stream: the same plan over the same keys bound as a format-0 stream,
  keys and counts bit-equal;
- decode: decode_column of the key stream equals the source keys, so a
  failure separates codec from probe.

Each case asserts the block headers it relies on (rle_shapes.walk_blocks) and
how bind classified them (gx.rle_block_classes)."""
import math

import numpy as np
import pytest

import rle_shapes as S

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

NOB, VAR, FIX, UNF = (gx.RLEBLK_NOBITMAP, gx.RLEBLK_VARINT, gx.RLEBLK_FIXED2,
                      gx.RLEBLK_UNFUSED)
DIM_F, MID_F, FACT_F = ("==", 1), ("<", 200), ("<", 70)


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


# ---------------------------------------------------------------------------
# key streams: (source keys, bind spec of the key column)
# ---------------------------------------------------------------------------

def rle(orc, keys, bs=32768):
    return (orc.aocs_encode_rle(keys, bs), 8, len(keys), 1, 0, bs)


def rle_delta(orc, keys):
    return (orc.aocs_encode_rle_delta(keys), 8, len(keys), 1)


def orig_segments(orc, keys, cuts):
    """Orig segment files concatenated: a format-1 stream of version-0 blocks"""
    parts = np.split(keys, cuts)
    return (b"".join(orc.aocs_encode(p) for p in parts), 8, len(keys), 1)


def orig_then_rle(orc, a, b):
    return (orc.aocs_encode(a) + orc.aocs_encode_rle(b), 8, len(a) + len(b), 1)


def h_rle_keys():
    return np.concatenate([S.shape_a()[:3000], S.shape_b() + 20000])


# name -> (keys, encoder, expected bind classes or None, header assertions)
def _hdr_a(bl):
    assert [(b["flags"], b["phys"]) for b in bl] == [(0, 4090), (0, 4090), (0, 820)]


def _hdr_b(bl):
    (b,) = bl
    assert b["flags"] == 2 and b["kind"] == 1
    assert set(b["cnt_lens"]) == {1, 2} and b["cnt_lens"].count(2) == 6


def _hdr_c(bl):
    (b,) = bl
    assert b["flags"] == 2 and b["kind"] == 3 and set(b["cnt_lens"]) == {2}
    assert b["phys"] == b["ncnt"] == 301 and b["csize"] == 602
    assert b["phys"] % 8 and b["phys"] % 256


def _hdr_d(bl):
    (b,) = bl
    assert b["kind"] == 3 and b["flags"] == 2 and b["cnt_lens"] == [2, 3, 1]


def _hdr_e(bl):
    (b,) = bl
    assert b["flags"] == 2 and b["ncnt"] == 2 and b["csize"] == 4
    assert sorted(b["cnt_lens"]) == [1, 3]


def _hdr_e_tail(bl):
    _hdr_e(bl)
    assert bl[0]["phys"] == 32


def _hdr_f_split(bl):
    assert [(b["rows"], b["flags"], b["phys"]) for b in bl] == \
        [(4090, 0, 4090), (14, 2, 3)]
    k = S.shape_f("split")
    assert k[4089] == k[4090]              # the run crosses the boundary


def _hdr_rows(*rows):
    def chk(bl):
        assert [b["rows"] for b in bl] == list(rows)
    return chk


def _hdr_f_one_run(bl):
    (b,) = bl
    assert (b["rows"], b["phys"], b["cnt_lens"]) == (300, 1, [2])


def _hdr_g(bl):
    assert all(b["version"] == 2 for b in bl) and any(b["flags"] & 4 for b in bl)
    assert not any(b["flags"] & 1 for b in bl)


def _hdr_h3(bl):
    assert all(b["version"] == 0 for b in bl) and len(bl) == 4
    assert [b["rows"] for b in bl] == [3000, 5, 4090, 1905]   # partial in the middle


def _hdr_h_rle(bl):
    assert [(b["version"], b["flags"]) for b in bl] == [(0, 0), (2, 2)]


def _hdr_i(bl):
    (b,) = bl
    assert b["flags"] == 2 and b["phys"] == 6500 > 4096 and b["kind"] == 1


CASES = {
    "a": (S.shape_a, rle, [NOB] * 3, _hdr_a),
    "b": (S.shape_b, rle, [VAR], _hdr_b),
    "c": (S.shape_c, rle, [FIX], _hdr_c),
    "d": (S.shape_d, rle, [VAR], _hdr_d),
    "e_fwd": (lambda: S.shape_e("fwd"), rle, [VAR], _hdr_e),
    "e_rev": (lambda: S.shape_e("rev"), rle, [VAR], _hdr_e),
    "e_tail": (lambda: S.shape_e("tail"), rle, [VAR], _hdr_e_tail),
    "f_split": (lambda: S.shape_f("split"), rle, [NOB, VAR], _hdr_f_split),
    "f_one_row": (lambda: S.shape_f("one_row"), rle, [NOB], _hdr_rows(1)),
    "f_one_run": (lambda: S.shape_f("one_run"), rle, [FIX], _hdr_f_one_run),
    "f_last1": (lambda: S.shape_f("last_block_one_row"), rle, [NOB, NOB],
                _hdr_rows(4090, 1)),
    "g": (S.shape_g, rle_delta, [UNF], _hdr_g),
    "h_orig3": (S.shape_a,
                lambda orc, k: orig_segments(orc, k, [3000, 3005]),
                [UNF] * 4, _hdr_h3),
    "h_orig_rle": (h_rle_keys,
                   lambda orc, k: orig_then_rle(orc, k[:3000], k[3000:]),
                   [UNF, VAR], _hdr_h_rle),
    "i": (S.shape_i, lambda orc, k: rle(orc, k, 65536), [UNF], _hdr_i),
}
CROSS = ["a", "c", "e_tail", "g"]          # shapes the plan variations cross


# ---------------------------------------------------------------------------
# the synthetic Q3 around a key column
# ---------------------------------------------------------------------------

def run_keys(keys):
    """(key, start, length) of every run, in stream order"""
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    lens = np.diff(np.r_[starts, len(keys)])
    return keys[starts], starts, lens


class Plan:
    """Data of one case.  The run keys are split into hit (their order
    qualifies), decoy (the order exists and fails the dim or the mid filter)
    and absent (no such order); `remap(u, hit, decoy, absent)` may rewrite the
    run keys before the tables are built.  One hit key has every row rejected
    by the fact filter; ship dates are otherwise random inside each run."""

    def __init__(self, keys, remap=None, no_hits=False, hide=False):
        u, starts, lens = run_keys(keys)
        assert len(np.unique(u)) == len(u), "equal keys must be contiguous"
        rng = np.random.default_rng(1000 + len(keys))
        r = rng.random(len(u))
        hit, decoy = r < 0.6, (r >= 0.6) & (r < 0.8)
        edge = [0, -1, int(np.argmax(lens))]    # first, last and longest run
        hit[edge] = True
        decoy[edge] = False
        if len(u) >= 3 and hit.all():
            hit[1] = False
        if no_hits:
            hit[:] = False
            decoy = r < 0.5
        absent = ~hit & ~decoy
        # orders that qualify and have no fact rows
        extra = u.max() + 10 + 3 * np.arange(40, dtype=np.int64)
        if remap is not None:
            u, extra = remap(u, extra, hit, decoy, absent)
            assert len(np.unique(u)) == len(u)
        self.li_keys = np.repeat(u, lens)
        self.hit_keys, self.run_lens = u[hit], lens[hit]
        n = len(keys)
        self.price = rng.uniform(1, 50, n)
        self.disc = rng.integers(0, 11, n) / 100.0
        self.ship = rng.integers(0, 100, n).astype(np.int32)
        if hit.any():
            self.ship[starts[hit][0]] = 0   # a one-row table still has a group
        self.rejected = None
        if hit.sum() >= 3:
            self.rejected = self.hit_keys[hit.sum() // 2]
            self.ship[self.li_keys == self.rejected] = 99
        self.hidden = None
        if hide:
            self.hidden = rng.random(n) < 0.05
            order = np.argsort(-lens[hit], kind="stable")
            hs, hl = starts[hit][order], lens[hit][order]
            self.hidden[hs[0]:hs[0] + hl[0]] = False
            self.hidden[[hs[0], hs[0] + hl[0] // 2, hs[0] + hl[0] - 1]] = True
            if len(hs) > 1:
                self.hidden[hs[1]:hs[1] + hl[1]] = True      # a whole run
                self.whole_hidden = self.li_keys[hs[1]]
        nc = 2000
        self.c_keys = np.arange(1, nc + 1, dtype=np.int64)
        self.c_seg = (np.arange(nc) % 5).astype(np.int8)
        good_c, bad_c = self.c_keys[self.c_seg == 1], self.c_keys[self.c_seg != 1]
        qual = np.concatenate([u[hit], extra])
        dec = u[decoy]
        o_keys = np.concatenate([qual, dec])
        o_cust = np.concatenate([rng.choice(good_c, len(qual)),
                                 rng.choice(good_c, len(dec))])
        o_date = rng.integers(0, 100, len(o_keys)).astype(np.int32)
        half = len(qual) + np.arange(len(dec))[::2]
        o_cust[half] = rng.choice(bad_c, len(half))           # fails the dim
        rest = len(qual) + np.arange(len(dec))[1::2]
        o_date[rest] = 500                                     # fails the mid
        perm = rng.permutation(len(o_keys))
        self.o_keys, self.o_cust, self.o_date = o_keys[perm], o_cust[perm], o_date[perm]
        self.o_prio = rng.integers(0, 5, len(o_keys)).astype(np.int32)
        self.build_keys = np.sort(qual)     # what the join table holds

    def expect(self):
        """brute force over the three tables, nothing taken from hit/decoy"""
        segok = self.c_keys[self.c_seg == DIM_F[1]]
        om = (self.o_date < MID_F[1]) & np.isin(self.o_cust, segok)
        np.testing.assert_array_equal(np.sort(self.o_keys[om]), self.build_keys)
        lm = (self.ship < FACT_F[1]) & np.isin(self.li_keys, self.o_keys[om])
        if self.hidden is not None:
            lm &= ~self.hidden
        k, term = self.li_keys[lm], (self.price * (1.0 - self.disc))[lm]
        order = np.argsort(k, kind="stable")
        k, term = k[order], term[order]
        keys, first, counts = np.unique(k, return_index=True, return_counts=True)
        rev = np.array([math.fsum(term[f:f + c]) for f, c in zip(first, counts)])
        odate = dict(zip(self.o_keys.tolist(), self.o_date.tolist()))
        dates = np.array([odate[x] for x in keys.tolist()], np.int32)
        return keys, counts, rev, dates


class Bound:
    """A Plan on the GPU: the key column under test, and the same keys plain"""

    def __init__(self, ctx, orc, plan, key_spec):
        p, enc = plan, orc.aocs_encode
        nc, no, nl = len(p.c_keys), len(p.o_keys), len(p.li_keys)
        self.plan, self.ctx = plan, ctx
        self.cust = ctx.bind([(enc(p.c_keys), 8, nc), (enc(p.c_seg), 1, nc)])
        self.ordr = ctx.bind([(enc(p.o_keys), 8, no), (enc(p.o_cust), 8, no),
                              (enc(p.o_date), 4, no), (enc(p.o_prio), 4, no)])
        rest = [(enc(p.price), 8, nl), (enc(p.disc), 8, nl), (enc(p.ship), 4, nl)]
        self.li = ctx.bind([key_spec] + rest)
        self.li_plain = ctx.bind([(enc(p.li_keys), 8, nl)] + rest)
        if p.hidden is not None:
            self.li.set_visimap(p.hidden)
            self.li_plain.set_visimap(p.hidden)

    def free(self):
        for t in (self.li, self.li_plain, self.ordr, self.cust):
            t.free()

    def desc(self, li):
        return {"dim": self.cust, "dim_key_col": 0, "dim_filter": (1,) + DIM_F,
                "mid": self.ordr, "mid_key_col": 0, "mid_fk_col": 1,
                "mid_attr1_col": 2, "mid_attr2_col": 3,
                "mid_filter": (2,) + MID_F,
                "fact": li, "fact_key_col": 0, "fact_a_col": 1,
                "fact_b_col": 2, "fact_filter": (3,) + FACT_F}

    def check_result(self, q, want, tag):
        keys, counts, rev, dates = want
        got, hits = q.result(), q.stats()["probe_hits"]
        np.testing.assert_array_equal(got["l_orderkey"], keys, err_msg=tag)
        np.testing.assert_array_equal(got["nitems"], counts, err_msg=tag)
        np.testing.assert_array_equal(got["o_orderdate"], dates, err_msg=tag)
        assert hits == counts.sum(), tag
        if len(keys):
            rtol = (int(counts.max()) + 2) * 2.0 ** -52
            np.testing.assert_allclose(got["revenue"], rev, rtol=rtol, atol=0,
                                       err_msg=f"{tag} rtol={rtol:.3g}")
        return got, hits

    def check(self, runs=1):
        """the three checks; returns the expected (keys, counts, ...)"""
        p, ctx = self.plan, self.ctx
        np.testing.assert_array_equal(
            self.li.decode_column(0, np.int64, verify=True), p.li_keys)
        want = p.expect()
        q = ctx.q3_desc(self.desc(self.li))
        for i in range(runs):       # a re-run re-zeroes the claimed agg slots
            got, hits = self.check_result(q.run(), want, f"run {i}")
        q.free()
        qp = ctx.q3_desc(self.desc(self.li_plain))
        gotp, hitsp = self.check_result(qp.run(), want, "plain stream")
        qp.free()
        np.testing.assert_array_equal(got["l_orderkey"], gotp["l_orderkey"])
        np.testing.assert_array_equal(got["nitems"], gotp["nitems"])
        assert hits == hitsp
        return want


def run_case(ctx, orc, name, runs=1, **plan_kw):
    keys_fn, encode, classes, _ = CASES[name]
    plan = Plan(keys_fn(), **plan_kw)
    spec = encode(orc, plan.li_keys)
    got_cls = list(gx.rle_block_classes(spec[0]))
    if name != "g":                 # remapped keys change what DELTA can take
        assert got_cls == classes
    assert (UNF in got_cls) == (UNF in classes)
    b = Bound(ctx, orc, plan, spec)
    try:
        return plan, b.check(runs)
    finally:
        b.free()


# ---------------------------------------------------------------------------
# cases a-j
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_key_shape(ctx, orc, name):
    keys_fn, encode, classes, hdr = CASES[name]
    keys = keys_fn()
    stream = encode(orc, keys)[0]
    hdr(S.walk_blocks(stream))
    assert list(gx.rle_block_classes(stream)) == classes
    plan, (gkeys, counts, _, _) = run_case(ctx, orc, name)
    assert len(gkeys) > 0
    if plan.rejected is not None:   # the fact filter emptied a matching run
        assert plan.rejected in plan.build_keys and plan.rejected not in gkeys
    if name in ("c", "d", "e_fwd", "e_rev", "e_tail"):
        assert counts.max() > 10000         # the bound is stated from the data


def test_host_writer_stream_case_j(ctx, orc):
    """TPCH_LINEITEM_RLEKEY at SF 0.01: this project's own writer, every count
    in the fixed 2-byte form whatever the run length"""
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_RLEKEY, 0.01)
    stream = t.dump_stream(0)
    t.free()
    keys = np.ascontiguousarray(orc.gen_lineitem(0.01)["l_orderkey"], np.int64)
    bl = S.walk_blocks(stream)
    assert sum(b["rows"] for b in bl) == len(keys) and len(bl) > 1
    assert all(b["version"] == 2 and b["flags"] in (0, 2) for b in bl)
    lens = [n for b in bl if b["flags"] for n in b["cnt_lens"]]
    assert lens and set(lens) == {2}        # 2 bytes even for runs of 2..7 rows
    _, _, run_lens = run_keys(keys)
    assert run_lens.max() <= 7
    cls = list(gx.rle_block_classes(stream))
    assert set(cls) <= {FIX, NOB} and FIX in cls
    plan = Plan(keys)
    b = Bound(ctx, orc, plan, (stream, 8, len(keys), 1))
    try:
        gkeys = b.check()[0]
        assert len(gkeys) > 1000
    finally:
        b.free()


# ---------------------------------------------------------------------------
# plan variations
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", CROSS)
def test_visimap(ctx, orc, name):
    """VM=true instantiation: first, middle and last row of the longest
    matching run hidden, the second longest hidden whole, 5 % elsewhere"""
    plan, (gkeys, _, _, _) = run_case(ctx, orc, name, hide=True)
    assert plan.hidden.any() and len(gkeys) > 0
    assert plan.whole_hidden in plan.build_keys
    assert plan.whole_hidden not in gkeys


def _miss32(u, extra, hit, decoy, absent):
    """absent runs become 2^32 + k, k a build key: a table of 4-byte keys must
    compare zero-extended, not truncated"""
    u = u.copy()
    ks = u[hit][:absent.sum()]
    idx = np.flatnonzero(absent)[:len(ks)]
    u[idx] = 2**32 + ks
    return u, extra


def _high(u, extra, hit, decoy, absent):
    return u + 2**33, extra + 2**33


def _sparse(u, extra, hit, decoy, absent):
    return u * 977, extra * 977


@pytest.mark.parametrize("name", CROSS)
def test_u32_table_misses_keys_past_2_32(ctx, orc, name):
    plan, (gkeys, _, _, _) = run_case(ctx, orc, name, remap=_miss32)
    assert plan.build_keys.max() < 2**32            # 4-byte key table
    high = plan.li_keys[plan.li_keys >= 2**32]
    assert len(high) and np.isin(high - 2**32, plan.build_keys).all()
    assert gkeys.max() < 2**32


@pytest.mark.parametrize("name", CROSS)
def test_u64_table(ctx, orc, name):
    plan, (gkeys, _, _, _) = run_case(ctx, orc, name, remap=_high)
    assert plan.build_keys.min() > 2**32 and len(gkeys) > 0


def slot0(keys, lay):
    """gx_slotmap::slot0 mirrored in numpy for the layout `lay`"""
    k = keys.astype(np.uint64)
    mask = np.uint64(lay["slots"] - 1)
    if not lay["interpolated"]:
        with np.errstate(over="ignore"):
            x = k ^ (k >> np.uint64(33))
            x = x * np.uint64(0xFF51AFD7ED558CCD)
            x ^= x >> np.uint64(33)
            x = x * np.uint64(0xC4CEB9FE1A85EC53)
            x ^= x >> np.uint64(33)
        return x & mask
    s = ((keys - lay["kmin"]).astype(np.float64) * lay["scale"]).astype(np.uint64)
    return np.minimum(s, mask)


@pytest.mark.parametrize("remap,interpolated", [(None, 1), (_sparse, 0)],
                         ids=["dense", "sparse"])
@pytest.mark.parametrize("name", CROSS)
def test_slot_map_with_collision_walks(ctx, orc, monkeypatch, name, remap,
                                       interpolated):
    """GX_TABLE_FACTOR_PCT=100: the smallest table, so probes walk.  The layout
    rule comes from the library (motion_table_layout states the same rule the
    local sizing applies at nsegs = 1); slot0 is mirrored here."""
    monkeypatch.setenv("GX_TABLE_FACTOR_PCT", "100")
    plan, (gkeys, _, _, _) = run_case(ctx, orc, name, remap=remap)
    bk = plan.build_keys
    lay = gx.motion_table_layout(len(bk), int(bk.min()), int(bk.max()), 1, 100)
    assert lay["interpolated"] == interpolated and lay["key_width"] == 4
    # two probed build keys with one home slot: whichever was inserted second
    # is found only by walking past the other.  A table never has fewer than
    # 1024 slots, so the few hundred keys of c (interpolated: scale > 1) and
    # the 52 of e_tail cannot be made to collide; no walk is asserted there.
    home = slot0(bk[np.isin(bk, gkeys)], lay)
    if name in ("a", "g") or (name == "c" and not interpolated):
        assert len(np.unique(home)) < len(home)
    else:
        assert lay["slots"] == 1024


@pytest.mark.parametrize("name", CROSS)
def test_no_matching_run(ctx, orc, name):
    """every fact key is absent from the join table or fails upstream: 0 groups,
    0 hits, on a table that is not empty"""
    plan, (gkeys, _, _, _) = run_case(ctx, orc, name, no_hits=True)
    assert len(gkeys) == 0 and len(plan.build_keys) == 40


@pytest.mark.parametrize("name", CROSS)
def test_rerun_equals_first_run(ctx, orc, name):
    run_case(ctx, orc, name, runs=2)


def test_numeric_with_fused_rle_key_is_refused_at_prepare(ctx, orc):
    plan = Plan(S.shape_c())
    b = Bound(ctx, orc, plan, rle(orc, plan.li_keys))
    try:
        with pytest.raises(gx.GxError) as ei:
            ctx.q3(b.cust, b.ordr, b.li, numeric=True)      # never reaches run
        assert ei.value.status == 3 and "GX_ERR_INVALID" in str(ei.value)
        assert "numeric" in str(ei.value) and "RLE" in str(ei.value)
    finally:
        b.free()

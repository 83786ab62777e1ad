"""The stages of the multi-segment (nsegs > 1) Q3 path, one rank at a time on
one GPU, through the same launch / dispatch / layout helpers gx_q3_run calls
(gx_test_m1, gx_test_dim, gx_test_m2, gx_test_m3).  Tables are hand-made
numpy arrays bound as AOCS streams, so every shape is exact; the reference
is numpy plus the oracle's brute-force routing.  The exchange between stages
is done here on the host with the counts the entry points return."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

GRID, TPB = 2048, 256            # the library's grid-stride launch geometry
BWORDS = 4096                    # production's bloom floor
DIM_FILTER = ("==", 0)           # c_attr == 0 selects ~20 % of the customers
LI_FILTER = (">", 0)             # l_shipdate > 0
NP_OPS = {"<": np.less, ">": np.greater, "==": np.equal,
          "!=": np.not_equal, "<=": np.less_equal, ">=": np.greater_equal}
U64 = np.uint64


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


@pytest.fixture(scope="module")
def ctxs():
    """gx.Context(device=0, seg=r, nsegs=N), made on demand and kept."""
    made = {}

    def get(seg, nsegs):
        if (seg, nsegs) not in made:
            made[(seg, nsegs)] = gx.Context(device=0, seg=seg, nsegs=nsegs)
        return made[(seg, nsegs)]
    yield get
    for c in made.values():
        c.close()


# ---------------- numpy restatement of the dim bloom ----------------

def np_hmix64(x):
    x = np.array(x, U64, copy=True)
    x ^= x >> U64(33)
    x *= U64(0xFF51AFD7ED558CCD)
    x ^= x >> U64(33)
    x *= U64(0xC4CEB9FE1A85EC53)
    x ^= x >> U64(33)
    return x


def np_bloom_mask(h):
    one = U64(1)
    return (one << ((h >> U64(32)) & U64(63))) | (one << ((h >> U64(38)) & U64(63)))


def np_bloom_build(keys, bwords):
    """Two-bit blocked bloom: one 64-bit word per key, two bits in it."""
    words = np.zeros(bwords, U64)
    h = np_hmix64(np.asarray(keys, np.int64).astype(U64))
    np.bitwise_or.at(words, (h & U64(bwords - 1)).astype(np.int64),
                     np_bloom_mask(h))
    return words


def np_bloom_test(words, keys):
    h = np_hmix64(np.asarray(keys, np.int64).astype(U64))
    m = np_bloom_mask(h)
    return (words[(h & U64(len(words) - 1)).astype(np.int64)] & m) == m


# ---------------- table makers and references ----------------

def make_orders(n, seed, ncust=1000, key0=1):
    """n orders with unique keys >= 1 in random order."""
    rng = np.random.default_rng(seed)
    o = np.zeros(n, gx.ORD_ROW_DTYPE)
    o["okey"] = rng.permutation(n).astype(np.int64) + key0
    o["ocust"] = rng.integers(1, ncust + 1, n)
    o["odate"] = rng.integers(-3000, 3000, n)
    o["oprio"] = rng.integers(-2**31, 2**31, n)
    return o


def bind_orders(ctx, orc, o):
    n = len(o)
    return ctx.bind([(orc.aocs_encode(np.ascontiguousarray(o["okey"])), 8, n),
                     (orc.aocs_encode(np.ascontiguousarray(o["ocust"])), 8, n),
                     (orc.aocs_encode(np.ascontiguousarray(o["odate"])), 4, n),
                     (orc.aocs_encode(np.ascontiguousarray(o["oprio"])), 4, n)])


def bind_customer(ctx, orc, ckey, cattr):
    n = len(ckey)
    return ctx.bind([(orc.aocs_encode(np.ascontiguousarray(ckey, np.int64)), 8, n),
                     (orc.aocs_encode(np.ascontiguousarray(cattr, np.int8)), 1, n)])


def bind_lineitem(ctx, orc, li):
    n = len(li["lkey"])
    return ctx.bind([(orc.aocs_encode(np.ascontiguousarray(li["lkey"], np.int64)), 8, n),
                     (orc.aocs_encode(np.ascontiguousarray(li["price"], np.float64)), 8, n),
                     (orc.aocs_encode(np.ascontiguousarray(li["disc"], np.float64)), 8, n),
                     (orc.aocs_encode(np.ascontiguousarray(li["ship"], np.int32)), 4, n)])


def passes(vals, op, lit):
    """The mathematically correct cross-type comparison (int64 literal)."""
    return NP_OPS[op](np.asarray(vals).astype(np.int64), np.int64(lit))


def split_by_counts(rows, counts):
    out, off = [], 0
    for c in counts:
        out.append(rows[off:off + int(c)])
        off += int(c)
    assert off == len(rows)
    return out


def check_partition(orc, counts, rows, want, key, nsegs):
    """counts / regions / full rows of one Motion output against the rows
    expected to ship, routed by `key`."""
    assert len(counts) == nsegs and counts.sum() == len(rows)
    np.testing.assert_array_equal(
        counts, np.bincount(orc.route(want[key], nsegs), minlength=nsegs))
    for d, region in enumerate(split_by_counts(rows, counts)):
        assert (orc.route(region[key], nsegs) == d).all(), f"region {d}"
    np.testing.assert_array_equal(rows[np.argsort(rows["okey"], kind="stable")],
                                  want[np.argsort(want["okey"], kind="stable")])


def run_m1_case(ctxs, orc, o, nsegs, filt=(2, "<", 0), hidden=None):
    ctx = ctxs(0, nsegs)
    t = bind_orders(ctx, orc, o)
    keep = passes(o["odate"], filt[1], filt[2])
    if hidden is not None:
        t.set_visimap(hidden)
        keep = keep & ~hidden
    counts, rows = ctx.test_m1(t, filt, nsegs)
    t.free()
    check_partition(orc, counts, rows, o[keep], "ocust", nsegs)
    return counts


# ---------------- Motion 1, prefilter off ----------------

@pytest.mark.parametrize("nsegs", [1, 2, 3, 7, 8, 16])
@pytest.mark.parametrize("nrows", [0, 1, 63, 64, 65, 255, 256, 257, 4097])
def test_m1_matrix(ctxs, orc, nrows, nsegs):
    """Wave (64), block (256) and multi-block edges at every destination
    count: counts, per-destination regions and the full shipped rows."""
    run_m1_case(ctxs, orc, make_orders(nrows, 1000 + nrows), nsegs)


def test_m1_second_grid_stride_pass(ctxs, orc):
    """GRID*TPB + 65 rows: 65 rows are reached only in the second pass of
    the grid-stride loop."""
    run_m1_case(ctxs, orc, make_orders(GRID * TPB + 65, 5, ncust=100000), 3)


@pytest.fixture(scope="module")
def o4097():
    return make_orders(4097, 77)


@pytest.mark.parametrize("op", ["<", ">", "==", "!=", "<=", ">="])
def test_m1_ops_against_median(ctxs, orc, o4097, op):
    med = int(np.sort(o4097["odate"])[len(o4097) // 2])
    assert (o4097["odate"] == med).any()
    run_m1_case(ctxs, orc, o4097, 3, filt=(2, op, med))


@pytest.mark.parametrize("lit", [2**31, -2**31 - 1])
@pytest.mark.parametrize("op", ["<", ">", "==", "!=", "<=", ">="])
def test_m1_out_of_range_literals_fold(ctxs, orc, o4097, op, lit):
    """A literal outside int32 makes the qual constant; the folded pair must
    ship everything or nothing, never the narrowed literal's result."""
    o = o4097.copy()
    o["odate"][:4] = [-2**31, 2**31 - 1, 0, -1]     # the type's own extremes
    keep = passes(o["odate"], op, lit)
    assert keep.all() or not keep.any()
    counts = run_m1_case(ctxs, orc, o, 3, filt=(2, op, lit))
    assert counts.sum() == (len(o) if keep.all() else 0)


def test_m1_visimap(ctxs, orc, o4097):
    rng = np.random.default_rng(3)
    hidden = rng.random(len(o4097)) < 0.3
    hidden[0] = hidden[-1] = True
    run_m1_case(ctxs, orc, o4097, 3, hidden=hidden)


@pytest.mark.parametrize("nsegs", [3, 8])
def test_m1_skew_one_destination_takes_all(ctxs, orc, nsegs):
    o = make_orders(4097, 11)
    o["ocust"] = 4242
    counts = run_m1_case(ctxs, orc, o, nsegs)
    assert (counts > 0).sum() == 1


def test_m1_skew_empty_destinations(ctxs, orc):
    o = make_orders(4097, 12)
    o["ocust"] = np.array([7, 4242, 99991], np.int64)[np.arange(len(o)) % 3]
    counts = run_m1_case(ctxs, orc, o, 8)
    assert (counts == 0).sum() >= 5


# ---------------- the simulated multi-rank world ----------------

NCUST, NORD, NLI = 3000, 20000, 60000
MID_FILTER = (2, "<", 0)         # about half the orders qualify


def make_world(orc, nsegs, variant="plain"):
    """Global tables plus their shards as production distributes them:
    customer by route(c_custkey), orders by route(o_orderkey), lineitem by
    route(l_orderkey)."""
    rng = np.random.default_rng(20260 + nsegs)
    ckey = rng.permutation(NCUST).astype(np.int64) + 1
    cattr = rng.integers(0, 5, NCUST).astype(np.int8)
    o = make_orders(NORD, 900 + nsegs, ncust=NCUST)
    li = {"lkey": rng.integers(1, NORD + NORD // 10, NLI).astype(np.int64),
          "price": np.round(rng.uniform(900.0, 105000.0, NLI), 2),
          "disc": rng.integers(0, 11, NLI) / 100.0,
          "ship": rng.integers(-1000, 1000, NLI).astype(np.int32)}
    odest = orc.route(o["okey"], nsegs)
    victim = nsegs - 1
    if variant == "empty_shard":         # one rank holds no orders at all
        o = o[odest != victim]
    elif variant == "none_qualify":      # one rank's orders all fail the filter
        o["odate"][odest == victim] = 5
    odest = orc.route(o["okey"], nsegs)
    cdest = orc.route(ckey, nsegs)
    ldest = orc.route(li["lkey"], nsegs)
    w = {"nsegs": nsegs, "ckey": ckey, "cattr": cattr, "o": o, "li": li,
         "cshard": [(ckey[cdest == r], cattr[cdest == r]) for r in range(nsegs)],
         "oshard": [o[odest == r] for r in range(nsegs)],
         "lshard": [{k: v[ldest == r] for k, v in li.items()}
                    for r in range(nsegs)]}
    w["sel"] = [ck[passes(ca, *DIM_FILTER)] for ck, ca in w["cshard"]]
    return w


def world_blooms(ctxs, orc, w):
    """Every rank's bloom from the dim entry point, concatenated as the
    all-gather would; each is checked against the numpy restatement."""
    n = w["nsegs"]
    blooms = np.zeros((n, BWORDS), U64)
    for r in range(n):
        ctx = ctxs(r, n)
        t = bind_customer(ctx, orc, *w["cshard"][r])
        blooms[r], nsel, width = ctx.test_dim(t, DIM_FILTER, BWORDS)
        t.free()
        assert nsel == len(w["sel"][r]) and width == 4
        np.testing.assert_array_equal(blooms[r],
                                      np_bloom_build(w["sel"][r], BWORDS))
    return blooms


_m1_cache = {}


def world_after_m1(ctxs, orc, nsegs):
    """Motion 1 with the prefilter on for every rank of the plain world;
    shared by the prefilter and Motion-2 tests (read-only)."""
    if nsegs not in _m1_cache:
        w = make_world(orc, nsegs)
        blooms = world_blooms(ctxs, orc, w)
        sent = []
        for r in range(nsegs):
            ctx = ctxs(r, nsegs)
            t = bind_orders(ctx, orc, w["oshard"][r])
            on = ctx.test_m1(t, MID_FILTER, nsegs, "semi", blooms)
            off = ctx.test_m1(t, MID_FILTER, nsegs, "semi", None)
            anti = ctx.test_m1(t, MID_FILTER, nsegs, "anti", blooms)
            t.free()
            sent.append({"on": on, "off": off, "anti": anti})
        recv = {k: [np.concatenate([split_by_counts(sent[r][k][1],
                                                    sent[r][k][0])[d]
                                    for r in range(nsegs)])
                    for d in range(nsegs)] for k in ("on", "off")}
        for a in recv["on"] + recv["off"]:
            a.setflags(write=False)
        _m1_cache[nsegs] = (w, blooms, sent, recv)
    return _m1_cache[nsegs]


def member_of_dest(orc, w, ocust):
    """custkey selected on the rank it routes to (the shards hold exactly
    the customers routing there, so that is global membership)."""
    return np.isin(ocust, np.concatenate(w["sel"]))


# ---------------- Motion 1, destination-bloom prefilter ----------------

# false positives the numpy bloom alone ships for make_world's seeds, out of
# the qualifying non-members (measured on the CPU before any GPU run)
NUMPY_FALSE_POSITIVES = {2: 0, 3: 0, 8: 0}


@pytest.mark.parametrize("nsegs", [2, 3, 8])
def test_m1_prefilter(ctxs, orc, nsegs):
    """Destination-aware bloom prefilter, bloom_all indexed at every d.

    No false negatives, nothing outside the qualifying set, subset of the
    prefilter-off rows, and the shipped set equals the numpy bloom exactly.
    The filter must be seen to filter: shipped non-members <= 1 % of the
    qualifying non-members.  The numpy restatement alone, on the CPU with
    these seeds (about 600 selected keys spread over nsegs blooms of 4096
    words, about 2400 distinct non-member custkeys), ships 0 of 7778
    qualifying non-member rows at nsegs 2, 0 of 7979 at 3 and 0 of 7990 at
    8 (NUMPY_FALSE_POSITIVES); the GPU must ship exactly the same rows."""
    w, blooms, sent, _ = world_after_m1(ctxs, orc, nsegs)
    fp = nonmembers = 0
    for r in range(nsegs):
        o = w["oshard"][r]
        qual = passes(o["odate"], MID_FILTER[1], MID_FILTER[2])
        member = member_of_dest(orc, w, o["ocust"])
        dest = orc.route(o["ocust"], nsegs)
        ref_pass = np.zeros(len(o), bool)
        for d in range(nsegs):
            m = dest == d
            ref_pass[m] = np_bloom_test(blooms[d], o["ocust"][m])
        assert ref_pass[member].all()       # the reference has no negatives
        counts_on, rows_on = sent[r]["on"]
        counts_off, rows_off = sent[r]["off"]
        check_partition(orc, counts_off, rows_off, o[qual], "ocust", nsegs)
        # exact: what ships is the qualifying rows passing the bloom of the
        # rank they route to
        check_partition(orc, counts_on, rows_on, o[qual & ref_pass], "ocust",
                        nsegs)
        shipped = np.isin(o["okey"], rows_on["okey"])
        assert shipped[qual & member].all(), "false negative"
        assert not shipped[~qual].any()
        assert np.isin(rows_on["okey"], rows_off["okey"]).all()
        fp += int((shipped & ~member).sum())
        nonmembers += int((qual & ~member).sum())
        # anti join: a bloom is supplied but the prefilter is off
        check_partition(orc, *sent[r]["anti"], o[qual], "ocust", nsegs)
    assert nonmembers == {2: 7778, 3: 7979, 8: 7990}[nsegs]
    assert fp == NUMPY_FALSE_POSITIVES[nsegs]
    assert fp <= 0.01 * nonmembers, (fp, nonmembers)


# ---------------- Motion 2 ----------------

def key_routing_to(orc, lo, rank, nsegs):
    cand = np.arange(lo, lo + 4096, dtype=np.int64)
    return int(cand[orc.route(cand, nsegs) == rank][0])


def wide_key_passing_bloom(sel, words):
    """A key >= 2^32 whose low 32 bits are a selected key and which passes
    the bloom, so that the probe walks the 4-byte set with it."""
    for j in range(1, 4000, 100):
        hi = (np.arange(j, j + 100, dtype=np.int64) << 32)[:, None]
        cand = (np.asarray(sel, np.int64)[None, :] + hi).ravel()
        hit = np_bloom_test(words, cand)
        if hit.any():
            return int(cand[hit][0])
    raise AssertionError("no wide key passes the bloom")


@pytest.mark.parametrize("src", ["on", "off"])
@pytest.mark.parametrize("width", [4, 8])
@pytest.mark.parametrize("join", ["semi", "anti"])
@pytest.mark.parametrize("nsegs", [2, 3, 8])
def test_m2_semi_anti_both_widths(ctxs, orc, nsegs, join, width, src):
    """The rows each rank received from Motion 1 with the prefilter on (the
    numpy bloom ships no false positive for these seeds, so nearly all are
    members) and, for a set probe that has to reject most rows, with it off,
    against each rank's set.  Width 8: one selected key >= 2^32 routing to the rank is in its
    shard and among the received custkeys.  Width 4: a received custkey
    equal to a selected key + k * 2^32 (one of them passing the bloom) must
    not match the 4-byte slot."""
    w, blooms, _, recv = world_after_m1(ctxs, orc, nsegs)
    for r in range(nsegs):
        ctx = ctxs(r, nsegs)
        ck, ca = w["cshard"][r]
        sel = w["sel"][r]
        extra = np.zeros(2, gx.ORD_ROW_DTYPE)
        extra["okey"] = [NORD + 1 + 2 * r, NORD + 2 + 2 * r]
        extra["odate"] = [-5, -6]
        extra["oprio"] = [17, -17]
        big = key_routing_to(orc, 2**32 + 12345, r, nsegs)
        if width == 8:
            ck = np.append(ck, big)
            ca = np.append(ca, np.int8(0))
            sel = np.append(sel, big)
            extra["ocust"] = [big, big + 1]
        else:
            extra["ocust"] = [int(sel[0]) + 2**32,
                              wide_key_passing_bloom(sel, blooms[r])]
        rows = np.concatenate([recv[src][r], extra])
        t = bind_customer(ctx, orc, ck, ca)
        counts, out, got_width = ctx.test_m2(t, DIM_FILTER, rows, nsegs, join,
                                             BWORDS)
        t.free()
        assert got_width == width
        in_set = np.isin(rows["ocust"], sel)
        assert in_set.any() and not in_set.all()
        want_rows = rows[in_set if join == "semi" else ~in_set]
        want = np.zeros(len(want_rows), gx.QUAL_ROW_DTYPE)
        for f in ("okey", "odate", "oprio"):
            want[f] = want_rows[f]
        check_partition(orc, counts, out, want, "okey", nsegs)


@pytest.mark.parametrize("join", ["semi", "anti"])
def test_m2_rank_receives_nothing(ctxs, orc, join):
    w, _, _, _ = world_after_m1(ctxs, orc, 3)
    ctx = ctxs(1, 3)
    t = bind_customer(ctx, orc, *w["cshard"][1])
    counts, out, _ = ctx.test_m2(t, DIM_FILTER, np.zeros(0, gx.ORD_ROW_DTYPE),
                                 3, join, BWORDS)
    t.free()
    assert len(out) == 0 and (counts == 0).all()


@pytest.mark.parametrize("join", ["semi", "anti"])
def test_m2_customer_visimap_hides_selected_keys(ctxs, orc, join):
    nsegs, r = 3, 2
    w, _, _, recv = world_after_m1(ctxs, orc, nsegs)
    ctx = ctxs(r, nsegs)
    ck, ca = w["cshard"][r]
    selected = passes(ca, *DIM_FILTER)
    hidden = np.zeros(len(ck), bool)
    hidden[np.nonzero(selected)[0][::2]] = True     # every other selected key
    hidden[np.nonzero(~selected)[0][:5]] = True
    sel = ck[selected & ~hidden]
    rows = recv["off"][r]
    assert np.isin(rows["ocust"], ck[selected & hidden]).any()
    t = bind_customer(ctx, orc, ck, ca)
    t.set_visimap(hidden)
    counts, out, _ = ctx.test_m2(t, DIM_FILTER, rows, nsegs, join, BWORDS)
    t.free()
    in_set = np.isin(rows["ocust"], sel)
    want_rows = rows[in_set if join == "semi" else ~in_set]
    want = np.zeros(len(want_rows), gx.QUAL_ROW_DTYPE)
    for f in ("okey", "odate", "oprio"):
        want[f] = want_rows[f]
    check_partition(orc, counts, out, want, "okey", nsegs)


# ---------------- Motion 3 ----------------

def brute_groups(qual, li, filt=LI_FILTER, hidden=None):
    """Inner join of lineitem with the qualifying rows, grouped by key:
    revenue is math.fsum of the per-row price * (1 - disc)."""
    ok = passes(li["ship"], *filt) & np.isin(li["lkey"], qual["okey"])
    if hidden is not None:
        ok &= ~hidden
    k = li["lkey"][ok]
    terms = (li["price"] * (1.0 - li["disc"]))[ok]
    order = np.argsort(k, kind="stable")
    k, terms = k[order], terms[order]
    keys, start, cnt = np.unique(k, return_index=True, return_counts=True)
    q = np.sort(qual, order="okey")
    at = np.searchsorted(q["okey"], keys)
    return {"l_orderkey": keys.astype(np.int64),
            "o_orderdate": q["odate"][at], "o_shippriority": q["oprio"][at],
            "nitems": cnt.astype(np.int64),
            "revenue": np.array([math.fsum(terms[s:s + c])
                                 for s, c in zip(start, cnt)], np.float64)}


def check_groups(got, want):
    for f in ("l_orderkey", "o_orderdate", "o_shippriority", "nitems"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f)
    assert not got["key_is_null"].any() and not got["attrs_null"].any()
    assert not got["_pad"].any() and not got["revenue_num"].any()
    # reordered f64 addition of nitems positive terms, room for a contracted
    # multiply: the bound this project uses for Q1
    tol = (want["nitems"] + 2) * 2.0**-52 * np.abs(want["revenue"])
    err = np.abs(got["revenue"] - want["revenue"])
    assert (err <= tol).all(), (err / np.maximum(tol, 1e-300)).max()


def make_qual(keys, seed):
    rng = np.random.default_rng(seed)
    q = np.zeros(len(keys), gx.QUAL_ROW_DTYPE)
    q["okey"] = rng.permutation(np.asarray(keys, np.int64))
    q["odate"] = rng.integers(-2**31, 2**31, len(keys))
    q["oprio"] = rng.integers(-2**31, 2**31, len(keys))
    return q


def make_lineitem(hit_keys, miss_keys, seed):
    """1..7 items per hit key (cycled), one row per miss key, shuffled."""
    rng = np.random.default_rng(seed)
    hit_keys = np.asarray(hit_keys, np.int64)
    reps = 1 + np.arange(len(hit_keys)) % 7
    lkey = np.concatenate([np.repeat(hit_keys, reps),
                           np.asarray(miss_keys, np.int64)])
    lkey = rng.permutation(lkey)
    n = len(lkey)
    return {"lkey": lkey,
            "price": np.round(rng.uniform(900.0, 105000.0, n), 2),
            "disc": rng.integers(0, 11, n) / 100.0,
            "ship": rng.integers(-50, 200, n).astype(np.int32)}


def run_m3_case(ctxs, orc, nsegs, qual, li, hidden=None):
    ctx = ctxs(0, nsegs)
    t = bind_lineitem(ctx, orc, li)
    if hidden is not None:
        t.set_visimap(hidden)
    got, lay = ctx.test_m3(qual, t, LI_FILTER)
    t.free()
    check_groups(got, brute_groups(qual, li, hidden=hidden))
    n = len(qual)
    kmin = int(qual["okey"].min()) if n else 2**64 - 1
    kmax = int(qual["okey"].max()) if n else 0
    assert lay == gx.motion_table_layout(n, kmin, kmax, nsegs)
    assert lay["slots"] > n
    return got, lay


@pytest.mark.parametrize("vm", [False, True])
@pytest.mark.parametrize("kind", ["below", "straddle"])
def test_m3_key_width(ctxs, orc, kind, vm):
    """4-byte table when every received key is < 2^32, 8-byte when they
    straddle it; lineitem keys >= 2^32 aliasing a 4-byte slot must miss."""
    rng = np.random.default_rng(31)
    lo = {"below": 2**32 - 5000, "straddle": 2**32 - 1500}[kind]
    ends = [lo, 2**32 - 1] if kind == "below" else [lo, lo + 3999]
    keys = np.concatenate([ends, lo + 1 + rng.choice(3998, 2998, replace=False)])
    assert len(np.unique(keys)) == 3000
    assert (keys.max() >= 2**32) == (kind == "straddle")
    qual = make_qual(keys, 32)
    absent = np.setdiff1d(lo + np.arange(4000), keys)[:300]
    miss = np.concatenate([absent, keys[:500] + 2**32, keys[:50] + 2**33])
    li = make_lineitem(keys[:2500], miss, 33)
    hidden = None
    if vm:
        hidden = rng.random(len(li["lkey"])) < 0.3
        hidden[0] = hidden[-1] = True
    got, lay = run_m3_case(ctxs, orc, 3, qual, li, hidden)
    assert lay["key_width"] == (4 if kind == "below" else 8)
    assert len(got["l_orderkey"]) > 2000
    assert (got["nitems"] <= 7).all() and got["nitems"].max() >= 6


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("nsegs", [1, 8])
def test_m3_density_rule(ctxs, orc, nsegs, dense):
    """Keys on both sides of qual >= range / (64 * nsegs): the interpolated
    and the hashed layout, as the host helper says which."""
    rng = np.random.default_rng(41 + nsegs)
    n = 1000
    span = n * 64 * nsegs + (0 if dense else 1)
    kmin = 17
    inner = kmin + 1 + rng.choice(span - 2, n - 2, replace=False)
    keys = np.concatenate([[kmin, kmin + span - 1], inner])
    qual = make_qual(keys, 42)
    li = make_lineitem(keys[:900], [kmin - 1, kmin + span, 1, kmin + span + 7], 43)
    _, lay = run_m3_case(ctxs, orc, nsegs, qual, li)
    assert lay["interpolated"] == (1 if dense else 0)
    # the same keys at the other nsegs sit on the other side of the rule
    other = gx.motion_table_layout(n, kmin, kmin + span - 1, 9 - nsegs)
    assert other["interpolated"] == (1 if nsegs == 1 else 0)


@pytest.mark.parametrize("vm", [False, True])
@pytest.mark.parametrize("n", [0, 1])
def test_m3_zero_and_one_received_rows(ctxs, orc, n, vm):
    qual = make_qual([777][:n], 51)
    li = make_lineitem([778, 777, 779], [5, 6], 52)     # 777 has two items
    li["ship"][:] = 5                      # every row passes the filter
    hidden = None
    if vm:
        hidden = np.zeros(len(li["lkey"]), bool)
        hidden[np.nonzero(li["lkey"] == 777)[0][0]] = True
    got, _ = run_m3_case(ctxs, orc, 3, qual, li, hidden)
    assert len(got["l_orderkey"]) == n


# ---------------- all stages chained ----------------

def brute_q3(w, join):
    o, li = w["o"], w["li"]
    sel = w["ckey"][passes(w["cattr"], *DIM_FILTER)]
    in_set = np.isin(o["ocust"], sel)
    keep = passes(o["odate"], MID_FILTER[1], MID_FILTER[2]) & \
        (in_set if join == "semi" else ~in_set)
    qual = np.zeros(int(keep.sum()), gx.QUAL_ROW_DTYPE)
    for f in ("okey", "odate", "oprio"):
        qual[f] = o[f][keep]
    return brute_groups(qual, li)


def run_pipeline(ctxs, orc, nsegs, join, variant):
    w = make_world(orc, nsegs, variant)
    blooms = world_blooms(ctxs, orc, w)
    sent1 = []
    for r in range(nsegs):
        ctx = ctxs(r, nsegs)
        t = bind_orders(ctx, orc, w["oshard"][r])
        counts, rows = ctx.test_m1(t, MID_FILTER, nsegs, join, blooms)
        t.free()
        sent1.append(split_by_counts(rows, counts))
    sent2 = []
    for r in range(nsegs):
        ctx = ctxs(r, nsegs)
        recv = np.concatenate([sent1[src][r] for src in range(nsegs)])
        t = bind_customer(ctx, orc, *w["cshard"][r])
        counts, rows, _ = ctx.test_m2(t, DIM_FILTER, recv, nsegs, join, BWORDS)
        t.free()
        sent2.append(split_by_counts(rows, counts))
    parts = []
    for r in range(nsegs):
        ctx = ctxs(r, nsegs)
        recv = np.concatenate([sent2[src][r] for src in range(nsegs)])
        t = bind_lineitem(ctx, orc, w["lshard"][r])
        got, _ = ctx.test_m3(recv, t, LI_FILTER)
        t.free()
        assert (orc.route(got["l_orderkey"], nsegs) == r).all()
        parts.append(got)
    union = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    order = np.argsort(union["l_orderkey"], kind="stable")
    union = {f: v[order] for f, v in union.items()}
    want = brute_q3(w, join)
    assert len(want["l_orderkey"]) > 500
    check_groups(union, want)
    return w, sent1


@pytest.mark.parametrize("join", ["semi", "anti"])
@pytest.mark.parametrize("nsegs", [2, 3, 8])
def test_pipeline_equals_global_q3(ctxs, orc, nsegs, join):
    """Motion 1 (prefilter on for the semi join) -> Motion 2 -> table build
    and probe on every rank, rows moved with the returned counts: the union
    of the per-rank groups is the brute-force Q3 over the global tables."""
    run_pipeline(ctxs, orc, nsegs, join, "plain")


@pytest.mark.parametrize("join", ["semi", "anti"])
def test_pipeline_one_orders_shard_empty(ctxs, orc, join):
    w, sent1 = run_pipeline(ctxs, orc, 3, join, "empty_shard")
    assert len(w["oshard"][2]) == 0
    assert sum(len(x) for x in sent1[2]) == 0


@pytest.mark.parametrize("join", ["semi", "anti"])
def test_pipeline_no_order_of_one_rank_qualifies(ctxs, orc, join):
    w, sent1 = run_pipeline(ctxs, orc, 3, join, "none_qualify")
    assert len(w["oshard"][2]) > 1000
    assert sum(len(x) for x in sent1[2]) == 0

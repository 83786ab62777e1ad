"""Codec matrix on the GPU: every decode kernel instantiation (widths 1/4/8,
Orig / Orig+NULL / Dense RLE / RLE+DELTA, block sizes, block-boundary row
counts, type-range values) against the source array AND the oracle's decode
of the same bytes; the device encoder byte-compared for every generated
table; Q1 against an exactly-summed reference; and the loud rejections
gx_table_bind / gx_q1 owe malformed input.

Rejection tests end at the pytest.raises: the object is never scanned."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

I64 = np.iinfo(np.int64)


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
# the one checker every matrix case goes through
# ---------------------------------------------------------------------------

def check_stream(ctx, orc, stream, vals, nulls=None, formats=(1,),
                 blocksize=32768, tag=""):
    """Bind `stream` (the encoding of `vals`, NULL where nulls[i]) under each
    format and require, with checksums verified: GPU values == source, GPU
    values/validity == the oracle's decode of the same bytes, and all-ones
    validity for a NOT NULL stream."""
    vals = np.ascontiguousarray(vals)
    dtype, width, n = vals.dtype, vals.itemsize, len(vals)
    valid = np.ones(n, bool) if nulls is None else ~np.asarray(nulls, bool)
    for fmt in formats:
        t = ctx.bind([(stream, width, n, fmt, 0, blocksize)])
        try:
            assert t.nrows == n
            if fmt == 0:
                assert nulls is None
                got = t.decode_column(0, dtype, verify=True)
                np.testing.assert_array_equal(got, vals, err_msg=f"{tag} fmt0 vs source")
                want = orc.aocs_decode(stream, width, n, dtype, verify=True)
                np.testing.assert_array_equal(got, want, err_msg=f"{tag} fmt0 vs oracle")
                continue
            gv, gval = t.decode_column_nullable(0, dtype, verify=True)
            wv, wval = orc.aocs_decode_nullable(stream, width, n, dtype)
            np.testing.assert_array_equal(gval, valid.astype(np.uint8),
                                          err_msg=f"{tag} validity vs source")
            np.testing.assert_array_equal(gv[valid], vals[valid],
                                          err_msg=f"{tag} values vs source")
            np.testing.assert_array_equal(gval, wval, err_msg=f"{tag} validity vs oracle")
            np.testing.assert_array_equal(gv, wv, err_msg=f"{tag} values vs oracle")
            if nulls is None:
                assert gval.all(), f"{tag}: NOT NULL stream with zero validity"
                np.testing.assert_array_equal(
                    t.decode_column(0, dtype, verify=True), vals,
                    err_msg=f"{tag} plain decode vs source")
        finally:
            t.free()


def full_range(rng, dtype, n):
    """n values over the whole type range with min, max, 0, -1 planted."""
    if dtype == np.float64:
        v = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
        special = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf,
                            np.finfo(np.float64).max, np.finfo(np.float64).tiny,
                            5e-324], np.float64).view(np.int64)
    else:
        ii = np.iinfo(dtype)
        v = rng.integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
        special = np.array([ii.min, ii.max, 0, -1, ii.min + 1, ii.max - 1], dtype)
    v = v.astype(np.int64 if dtype == np.float64 else dtype)
    k = min(n, len(special))
    pos = rng.choice(n, k, replace=False)
    pos[0] = n - 1                         # an extreme in the last slot
    if k > 1:
        pos[1] = 0                         # and in the first
    v[pos] = special[:k]
    return v


def clustered(rng, dtype, nruns, maxrun=40, lo=None, hi=None):
    ii = np.iinfo(dtype)
    lo = ii.min if lo is None else lo
    hi = ii.max if hi is None else hi
    heads = rng.integers(lo, hi, nruns, dtype=dtype, endpoint=True)
    return np.repeat(heads, rng.integers(1, maxrun + 1, nruns))


# ---------------------------------------------------------------------------
# Orig, format 0 (k_decode / k_verify_crc) and format 1 (version-0 branch of
# k_decode_dense): dtype x blocksize x rows at every block boundary
# ---------------------------------------------------------------------------

ORIG_DTYPES = {"i8": np.int8, "i32": np.int32, "i64": np.int64, "f64": np.float64}
ROWS = ["1", "rpb-1", "rpb", "rpb+1", "2rpb+1"]


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("blocksize", [8192, 32768, 65536])
@pytest.mark.parametrize("dt", list(ORIG_DTYPES))
def test_orig_block_boundaries(ctx, orc, dt, blocksize, rows):
    dtype = ORIG_DTYPES[dt]
    width = np.dtype(dtype).itemsize
    rpb = orc.lib.orc_aocs_rows_per_block(width, blocksize)
    if blocksize == 32768:
        assert rpb == {1: 16382, 4: 8181, 8: 4090}[width]
    n = {"1": 1, "rpb-1": rpb - 1, "rpb": rpb, "rpb+1": rpb + 1,
         "2rpb+1": 2 * rpb + 1}[rows]
    rng = np.random.default_rng([width, blocksize, n])
    vals = full_range(rng, dtype, n)
    stream = orc.aocs_encode(vals, blocksize)
    formats = (0, 1) if blocksize == 32768 else (0,)
    check_stream(ctx, orc, stream, vals, None, formats, blocksize,
                 tag=f"orig {dt} bs={blocksize} n={n}")


# ---------------------------------------------------------------------------
# Orig + NULL bitmap, format 1
# ---------------------------------------------------------------------------

def null_pattern(rng, name, n):
    m = np.zeros(n, bool)
    if name == "first":
        m[0] = True
    elif name == "last":
        m[-1] = True
    elif name == "alternating":
        m[::2] = True
    elif name == "random20":
        m = rng.random(n) < 0.2
    elif name == "all":
        m[:] = True
    else:
        raise KeyError(name)
    return m


NULL_PATTERNS = ["first", "last", "alternating", "random20", "all"]


@pytest.mark.parametrize("pattern", NULL_PATTERNS)
@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64],
                         ids=["i8", "i32", "i64"])
def test_orig_null_bitmap(ctx, orc, dtype, pattern):
    width = np.dtype(dtype).itemsize
    rpb = orc.lib.orc_aocs_rows_per_block(width, 32768)
    n = 3 * rpb + 7          # >= 3 blocks even if every row is physical
    rng = np.random.default_rng([width, NULL_PATTERNS.index(pattern)])
    vals = full_range(rng, dtype, n)
    nulls = null_pattern(rng, pattern, n)
    stream = orc.aocs_encode_orig_nulls(vals, nulls)
    check_stream(ctx, orc, stream, vals, nulls, tag=f"orig-null w{width} {pattern}")


# ---------------------------------------------------------------------------
# Dense RLE
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64],
                         ids=["i8", "i32", "i64"])
def test_rle_clustered_runs(ctx, orc, dtype):
    rng = np.random.default_rng([11, np.dtype(dtype).itemsize])
    vals = clustered(rng, dtype, 6000)          # runs of 1..40, full range
    vals[0], vals[-1] = np.iinfo(dtype).min, np.iinfo(dtype).max
    check_stream(ctx, orc, orc.aocs_encode_rle(vals), vals, tag="rle")
    # the same through the nulls encoder with an all-false bitmap
    s = orc.aocs_encode_rle_delta_nulls(vals, np.zeros(len(vals), bool), delta=0)
    check_stream(ctx, orc, s, vals, tag="rle/nulls-encoder")


# one value, a run of L, one value: L-1 extra repeats span the 1/2/3/4-byte
# count encodings (6/14/22/30 payload bits) and, above 16383 rows, the
# kind-3 (large-content) envelope
RUN_LADDER = [2, 64, 65, 16384, 16385, 100000, 4194304, 4194310]


@pytest.mark.parametrize("L", RUN_LADDER)
def test_rle_int8_run_ladder(ctx, orc, L):
    vals = np.empty(L + 2, np.int8)
    vals[0], vals[1:-1], vals[-1] = -128, 127, -1
    stream = orc.aocs_encode_rle(vals)
    if L >= 100000:
        assert len(stream) < 128, "the whole run must sit in one small block"
    check_stream(ctx, orc, stream, vals, tag=f"ladder L={L}")


@pytest.mark.parametrize("dtype", [np.int8, np.int32, np.int64],
                         ids=["i8", "i32", "i64"])
def test_rle_nulls_inside_and_between_runs(ctx, orc, dtype):
    rng = np.random.default_rng([13, np.dtype(dtype).itemsize])
    vals = clustered(rng, dtype, 5000)
    n = len(vals)
    nulls = rng.random(n) < 0.2                  # lands inside runs
    edges = np.flatnonzero(np.diff(vals.astype(np.int64)) != 0)
    nulls[edges[::3]] = True                     # and exactly between runs
    nulls[0] = nulls[-1] = True
    s = orc.aocs_encode_rle_delta_nulls(vals, nulls, delta=0)
    check_stream(ctx, orc, s, vals, nulls, tag="rle+nulls")


@pytest.mark.parametrize("dtype,delta", [(np.int8, 0), (np.int32, 0),
                                         (np.int32, 1), (np.int64, 0),
                                         (np.int64, 1)])
def test_dense_all_null_column(ctx, orc, dtype, delta):
    n = 40000
    vals = np.zeros(n, dtype)
    nulls = np.ones(n, bool)
    s = orc.aocs_encode_rle_delta_nulls(vals, nulls, delta=delta)
    check_stream(ctx, orc, s, vals, nulls, tag=f"all-null delta={delta}")


# ---------------------------------------------------------------------------
# Dense RLE+DELTA, widths 4/8 (the reference refuses DELTA on width 1, so
# that combination is not a case)
# ---------------------------------------------------------------------------

def delta_shapes(dtype):
    ii = np.iinfo(dtype)
    rng = np.random.default_rng([17, np.dtype(dtype).itemsize])
    n = 30000
    out = {
        "monotone": (ii.min + np.cumsum(rng.integers(0, 4, n))).astype(dtype),
        "negative": (ii.max - np.cumsum(rng.integers(0, 1000, n))).astype(dtype),
        "extremes": np.tile(np.array(
            [ii.max, ii.min, ii.max, 0, -1, 1, ii.min, ii.min + 1, ii.max - 1,
             ii.max], dtype), 500),
    }
    if dtype == np.int64:
        steps = np.array([0x1FFFFFFF, -0x1FFFFFFF, 0x20000000, -0x20000000,
                          0x1FFFFFFE, 1, -1], np.int64)
        walk = np.cumsum(steps[rng.integers(0, len(steps), n)])
        out["limit-walk"] = walk.astype(np.int64)
    return out


DELTA_CASES = [(dt, name) for dt in (np.int32, np.int64)
               for name in delta_shapes(dt)]


@pytest.mark.parametrize("with_nulls", [False, True], ids=["notnull", "nulls20"])
@pytest.mark.parametrize("dtype,name", DELTA_CASES,
                         ids=[f"{np.dtype(d).name}-{n}" for d, n in DELTA_CASES])
def test_rle_delta_shapes(ctx, orc, dtype, name, with_nulls):
    vals = delta_shapes(dtype)[name]
    if with_nulls:
        rng = np.random.default_rng(19)
        nulls = rng.random(len(vals)) < 0.2
        s = orc.aocs_encode_rle_delta_nulls(vals, nulls, delta=1)
        check_stream(ctx, orc, s, vals, nulls, tag=f"delta {name} nulls")
    else:
        s = orc.aocs_encode_rle_delta(vals)
        check_stream(ctx, orc, s, vals, tag=f"delta {name}")


# ---------------------------------------------------------------------------
# seeded fuzz
# ---------------------------------------------------------------------------

def fuzz_case(orc, seed):
    """-> (stream, vals, nulls|None, formats, description)"""
    rng = np.random.default_rng([20261020, seed])
    dtype = [np.int8, np.int32, np.int64][int(rng.integers(0, 3))]
    width = np.dtype(dtype).itemsize
    encoders = ["orig", "rle"] + (["rle_delta"] if width > 1 else [])
    enc = encoders[int(rng.integers(0, len(encoders)))]
    null_rate = [0.0, 0.05, 0.5, 1.0][int(rng.integers(0, 4))]
    run_scale = [1, 3, 40, 3000][int(rng.integers(0, 4))]
    ii = np.iinfo(dtype)
    span = [(ii.min, ii.max), (-3, 3), (ii.max - 50, ii.max),
            (ii.min, ii.min + 50)][int(rng.integers(0, 4))]
    rpb = orc.lib.orc_aocs_rows_per_block(width, 32768)
    n = int(rng.integers(1, 3 * rpb + 1))
    nruns = max(1, n // max(1, run_scale // 2))
    vals = clustered(rng, dtype, nruns, run_scale, span[0], span[1])
    if len(vals) < n:
        vals = np.resize(vals, n)
    vals = np.ascontiguousarray(vals[:n])
    nulls = (rng.random(n) < null_rate) if null_rate > 0 else None
    # a NOT NULL draw goes through the nulls-capable writer half the time
    via_nulls = nulls is not None or bool(rng.integers(0, 2))
    nb = np.zeros(n, bool) if nulls is None else nulls
    formats = (1,)
    if enc == "orig":
        if via_nulls:
            s = orc.aocs_encode_orig_nulls(vals, nb)
        else:
            s = orc.aocs_encode(vals)
            formats = (0, 1)
    elif enc == "rle":
        s = (orc.aocs_encode_rle_delta_nulls(vals, nb, delta=0) if via_nulls
             else orc.aocs_encode_rle(vals))
    else:
        s = (orc.aocs_encode_rle_delta_nulls(vals, nb, delta=1) if via_nulls
             else orc.aocs_encode_rle_delta(vals))
    desc = (f"seed={seed} w={width} enc={enc} via_nulls={via_nulls} "
            f"null_rate={null_rate} run_scale={run_scale} span={span} n={n}")
    return s, vals, nulls, formats, desc


@pytest.mark.parametrize("seed", range(40))
def test_codec_fuzz(ctx, orc, seed):
    s, vals, nulls, formats, desc = fuzz_case(orc, seed)
    check_stream(ctx, orc, s, vals, nulls, formats, tag=desc)


# ---------------------------------------------------------------------------
# multi-segfile concatenation, int8
# ---------------------------------------------------------------------------

def test_multi_segfile_concat_int8(ctx, orc):
    rng = np.random.default_rng(43)
    vals = clustered(rng, np.int8, 7000, 9)
    cut = len(vals) // 3
    s = (orc.aocs_encode_rle(vals[:cut]) + orc.aocs_encode_rle(vals[cut:2 * cut])
         + orc.aocs_encode_rle(vals[2 * cut:]))
    t = ctx.bind([(s, 1, len(vals), 1)])
    np.testing.assert_array_equal(t.decode_column(0, np.int8, verify=True), vals)
    gv, gval = t.decode_column_nullable(0, np.int8, verify=True)
    np.testing.assert_array_equal(gv, vals)
    assert gval.all()
    t.free()


# ---------------------------------------------------------------------------
# checksum detection on the directory path (k_verify_crc_dir)
# ---------------------------------------------------------------------------

def block_offsets(stream):
    """(offset, length, logical rows) of every AO block, from the headers."""
    out, off = [], 0
    while off < len(stream):
        b03 = int.from_bytes(stream[off:off + 4], "little")
        b47 = int.from_bytes(stream[off + 4:off + 8], "little")
        kind = (b03 >> 28) & 7
        if kind == 1:
            rows = (b03 & 0x00FFFC00) >> 10
            datalen = ((b03 & 0x3FF) << 11) | ((b47 & 0xFFE00000) >> 21)
        else:
            assert kind == 3
            rows = b47 & 0x3FFFFFFF
            datalen = b03 & 0x1FFFFF
        blen = (24 + datalen + 7) & ~7
        out.append((off, blen, rows))
        off += blen
    assert off == len(stream)
    return out


@pytest.mark.parametrize("dtype", [np.int8, np.int64], ids=["i8", "i64"])
def test_dense_checksum_detected_in_last_block(ctx, orc, dtype):
    """Only the stored block-checksum field of the LAST block is changed: no
    decode kernel reads it, so values stay right and only verify notices."""
    rng = np.random.default_rng(47)
    vals = clustered(rng, dtype, 120000, 3)
    good = orc.aocs_encode_rle(vals)
    blocks = block_offsets(good)
    assert len(blocks) >= 4
    off = blocks[-1][0]
    bad = bytearray(good)
    bad[off + 8] ^= 0x40
    bad = bytes(bad)
    n, width = len(vals), vals.itemsize
    t = ctx.bind([(bad, width, n, 1)])
    with pytest.raises(gx.GxError) as ei:
        t.decode_column(0, dtype, verify=True)
    assert ei.value.status == 4      # GX_ERR_CHECKSUM
    with pytest.raises(gx.GxError) as ei:
        t.decode_column_nullable(0, dtype, verify=True)
    assert ei.value.status == 4
    np.testing.assert_array_equal(t.decode_column(0, dtype, verify=False), vals)
    t.free()
    # the untouched stream verifies
    t = ctx.bind([(good, width, n, 1)])
    np.testing.assert_array_equal(t.decode_column(0, dtype, verify=True), vals)
    t.free()


# ---------------------------------------------------------------------------
# device encoder: every generated table, every column, byte for byte
# ---------------------------------------------------------------------------

def expected_columns(orc, which, sf):
    if which == gx.TPCH_CUSTOMER:
        c = orc.gen_customer(sf)
        return [c["c_custkey"], c["c_mktsegment"].astype(np.int8)]
    if which == gx.TPCH_ORDERS:
        o = orc.gen_orders(sf)
        return [o["o_orderkey"], o["o_custkey"], o["o_orderdate"],
                o["o_shippriority"]]
    if which == gx.TPCH_LINEITEM_Q1:
        q = orc.gen_lineitem_q1(sf)
        return [q["l_returnflag"], q["l_linestatus"], q["l_extendedprice"],
                q["l_discount"], q["l_shipdate"]]
    li = orc.gen_lineitem(sf)
    if which == gx.TPCH_LINEITEM_NUMERIC:
        # llround(x*100) as orc_q3_numeric does; x*100 is within an ulp of
        # an integer, where round-half-away and round-half-even agree
        return [li["l_orderkey"],
                np.rint(li["l_extendedprice"] * 100.0).astype(np.int64),
                np.rint(li["l_discount"] * 100.0).astype(np.int64),
                li["l_shipdate"]]
    return [li["l_orderkey"], li["l_extendedprice"], li["l_discount"],
            li["l_shipdate"]]


# (table, sf with >= 3 blocks in every column, sf with < 10 rows)
ENCODER_TABLES = {
    "customer": (gx.TPCH_CUSTOMER, 0.25, 0.00004),
    "orders": (gx.TPCH_ORDERS, 0.02, 0.000004),
    "lineitem": (gx.TPCH_LINEITEM, 0.01, 0.000001),
    "lineitem_numeric": (gx.TPCH_LINEITEM_NUMERIC, 0.01, 0.000001),
    "lineitem_q1": (gx.TPCH_LINEITEM_Q1, 0.01, 0.000001),
}


@pytest.mark.parametrize("size", ["blocks3", "tiny"])
@pytest.mark.parametrize("name", list(ENCODER_TABLES))
def test_device_encoder_bytes(ctx, orc, name, size):
    which, sf_big, sf_tiny = ENCODER_TABLES[name]
    sf = sf_big if size == "blocks3" else sf_tiny
    cols = expected_columns(orc, which, sf)
    n = len(cols[0])
    if size == "tiny":
        assert 0 < n < 10
    else:
        for c in cols:
            rpb = orc.lib.orc_aocs_rows_per_block(c.itemsize, 32768)
            assert n > 2 * rpb, "every column must span at least 3 blocks"
    t = ctx.tpch_gen(which, sf)
    try:
        assert t.nrows == n
        for ci, c in enumerate(cols):
            assert t.dump_stream(ci) == orc.aocs_encode(c), f"{name} col {ci}"
    finally:
        t.free()


@pytest.mark.parametrize("sf", [0.02, 0.000001], ids=["blocks", "tiny"])
def test_rlekey_host_writer_decodes_on_oracle(ctx, orc, sf):
    """The --rle-keys stream (host_rle_encode, fixed 2-byte counts, so not
    byte-equal to the oracle's writer) fed to the oracle DECODER: the keys
    come back, and every block fits the 32 KiB AO blocksize."""
    want = orc.gen_lineitem(sf)
    n = len(want["l_orderkey"])
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_RLEKEY, sf)
    try:
        assert t.nrows == n
        s = t.dump_stream(0)
        np.testing.assert_array_equal(
            orc.aocs_decode(s, 8, n, np.int64, verify=True), want["l_orderkey"])
        blocks = block_offsets(s)
        assert sum(r for _, _, r in blocks) == n
        assert all(blen <= 32768 for _, blen, _ in blocks)
        if n > 10000:
            assert len(blocks) >= 3
        # the plain columns next to it are the oracle encoder's bytes
        for ci, f in ((1, "l_extendedprice"), (2, "l_discount"), (3, "l_shipdate")):
            assert t.dump_stream(ci) == orc.aocs_encode(want[f]), f
    finally:
        t.free()


# ---------------------------------------------------------------------------
# Q1 against an exact (math.fsum) reference
# ---------------------------------------------------------------------------

Q1_SF = 0.02


@pytest.fixture(scope="module")
def q1_rows(orc):
    return orc.gen_lineitem_q1(Q1_SF)


@pytest.mark.parametrize("vmap", [False, True], ids=["all-visible", "visimap30"])
@pytest.mark.parametrize("cut", ["below", "q1date", "above"])
def test_q1_exact_reference(ctx, orc, q1_rows, cut, vmap):
    """Counts exact.  Sums vs math.fsum of the same terms: all terms are
    positive, so any summation order errs by at most (n_g-1)*2^-53 relative;
    (1-d) and the product add one rounding each (possibly fused).  Hence
    rtol = (n_g+2)*2^-52 from each group's own count — derived, not fitted."""
    li = q1_rows
    ship = li["l_shipdate"]
    cutoff = {"below": int(ship.min()) - 1,
              "q1date": orc.lib.orc_date_adt(1998, 9, 2),
              "above": int(ship.max()) + 1}[cut]
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, Q1_SF)
    try:
        assert t.nrows == len(ship)
        hidden = np.zeros(len(ship), bool)
        if vmap:
            hidden = np.random.default_rng(53).random(len(ship)) < 0.3
            t.set_visimap(hidden)
        got = ctx.q1(t, cutoff)
    finally:
        t.free()
    keep = ~hidden & (ship <= cutoff)
    g = li["l_returnflag"].astype(np.int64) * 2 + li["l_linestatus"]
    price, disc = li["l_extendedprice"], li["l_discount"]
    if cut == "below":
        assert not keep.any()
        assert (got["count"] == 0).all()
        assert (got["sum_price"] == 0.0).all() and (got["sum_revenue"] == 0.0).all()
        return
    if cut == "above" and not vmap:
        assert keep.all()
    for gi in range(6):
        sel = keep & (g == gi)
        ng = int(sel.sum())
        assert int(got["count"][gi]) == ng, f"group {gi}"
        assert ng > 100
        rtol = (ng + 2) * 2.0 ** -52
        want_p = math.fsum(price[sel].tolist())
        want_r = math.fsum((price[sel] * (1.0 - disc[sel])).tolist())
        err_p = abs(got["sum_price"][gi] - want_p) / want_p
        err_r = abs(got["sum_revenue"][gi] - want_r) / want_r
        print(f"q1 {cut} vmap={vmap} g{gi}: n={ng} rtol={rtol:.3e} "
              f"err_price={err_p:.3e} err_rev={err_r:.3e}")
        assert err_p <= rtol, (gi, err_p, rtol)
        assert err_r <= rtol, (gi, err_r, rtol)


# ---------------------------------------------------------------------------
# loud rejection instead of silent mis-addressing.  Every test below ends at
# the pytest.raises; nothing is decoded or scanned afterwards.
# ---------------------------------------------------------------------------

def _raises_invalid(fn):
    with pytest.raises(gx.GxError) as ei:
        fn()
    assert ei.value.status == 3      # GX_ERR_INVALID
    return ei.value


def test_bind_rejects_truncated_orig_stream(ctx, orc):
    vals = np.arange(10000, dtype=np.int64)
    s = orc.aocs_encode(vals)
    _raises_invalid(lambda: ctx.bind([(s[:-8], 8, len(vals))]))


def test_bind_rejects_wrong_width(ctx, orc):
    for n in (3000, 20000):          # one block, and several
        s = orc.aocs_encode(np.arange(n, dtype=np.int32))
        _raises_invalid(lambda: ctx.bind([(s, 8, n)]))


def test_bind_rejects_wrong_nrows_and_blocksize(ctx, orc):
    vals = np.arange(9000, dtype=np.int64)
    s = orc.aocs_encode(vals)
    _raises_invalid(lambda: ctx.bind([(s, 8, len(vals) - 1)]))
    _raises_invalid(lambda: ctx.bind([(s, 8, len(vals) + 1)]))
    _raises_invalid(lambda: ctx.bind([(s, 8, 0)]))
    _raises_invalid(lambda: ctx.bind([(b"", 8, 5)]))
    _raises_invalid(lambda: ctx.bind([(s, 8, len(vals), 0, 0, 8192)]))


def test_bind_concatenated_orig_streams(ctx, orc):
    """Two segment files' Orig streams, the first ending in a partial block:
    O(1) addressing would read wrong rows, so format 0 refuses; the block
    directory (format 1) decodes it."""
    rng = np.random.default_rng(59)
    a = rng.integers(-2**62, 2**62, 4090 + 100, dtype=np.int64)
    b = rng.integers(-2**62, 2**62, 5000, dtype=np.int64)
    s = orc.aocs_encode(a) + orc.aocs_encode(b)
    n = len(a) + len(b)
    _raises_invalid(lambda: ctx.bind([(s, 8, n)]))
    t = ctx.bind([(s, 8, n, 1)])
    np.testing.assert_array_equal(t.decode_column(0, np.int64, verify=True),
                                  np.concatenate([a, b]))
    t.free()


def test_bind_rejects_columns_of_different_nrows(ctx, orc):
    a = orc.aocs_encode(np.arange(100, dtype=np.int64))
    b = orc.aocs_encode(np.arange(101, dtype=np.int64))
    _raises_invalid(lambda: ctx.bind([(a, 8, 100), (b, 8, 101)]))


def test_q1_rejects_wrong_column_shape(ctx, orc):
    """Five width-8 Orig columns of zeros: every read of the unchecked kernel
    would stay inside its stream and land in group 0."""
    n = 1000
    z = orc.aocs_encode(np.zeros(n, np.int64))
    t = ctx.bind([(z, 8, n)] * 5)
    try:
        _raises_invalid(lambda: ctx.q1(t, 0))
    finally:
        t.free()

"""Pin the oracle to the reference: golden vectors (generated from the
reference's own hashfn.c compiled standalone — oracle/gen_golden.py) plus an
independent numpy brute-force of Q3 semantics, plus AOCS codec round-trips."""
import json
import os

import numpy as np
import pytest

from oracle import pyapi as orc

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hash_vectors.json")


# ---------------- hashes vs reference golden vectors ----------------

def _vectors():
    with open(GOLDEN) as f:
        return json.load(f)


def test_hash_bytes_uint32_golden():
    v = _vectors()
    for e in v["hash_bytes_uint32"]:
        assert orc.lib.orc_hash_bytes_uint32(e["k"]) == e["h"]


def test_hashint8_golden():
    v = _vectors()
    for e in v["hashint8"]:
        assert orc.lib.orc_hashint8(e["v"]) == e["h"]


def test_known_answers():
    # SURVEY §8c known answers, produced from the reference in-container.
    assert orc.lib.orc_hash_bytes_uint32(42) == 0x59FCFEC8


def test_hashint8_against_live_reference_if_present():
    """When oracle/_ref/libpgref.so exists (built from /root/reference),
    fuzz the oracle against the real thing beyond the committed vectors."""
    import ctypes
    so = os.path.join(HERE, "..", "oracle", "_ref", "libpgref.so")
    if not os.path.exists(so):
        pytest.skip("reference-compiled hashfn not present")
    ref = ctypes.CDLL(so)
    ref.hash_bytes_uint32.restype = ctypes.c_uint32
    ref.hash_bytes_uint32.argtypes = [ctypes.c_uint32]
    rng = np.random.default_rng(7)
    for v in rng.integers(-2**63, 2**63 - 1, 2000, dtype=np.int64):
        v = int(v)
        lo = v & 0xFFFFFFFF
        hi = (v >> 32) & 0xFFFFFFFF
        lo ^= hi if v >= 0 else (~hi & 0xFFFFFFFF)
        assert orc.lib.orc_hashint8(v) == ref.hash_bytes_uint32(lo)


def test_jump_consistent_hash_properties():
    """cdbhash.c:530-541. Pin with the monotone-split property of the
    Lamping-Veach construction (a key's bucket only ever moves to the NEW
    bucket when nsegs grows) and stability of the full route chain."""
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 2**64 - 1, 500, dtype=np.uint64)
    for k in keys:
        prev = 0
        for n in range(1, 17):
            b = orc.lib.orc_jump_consistent_hash(int(k), n)
            assert 0 <= b < n
            if n > 1:
                assert b == prev or b == n - 1
            prev = b


def test_route_is_jump_of_cdbhash():
    for key in [1, 2, 3, 150000000, -5, 2**40]:
        h = orc.lib.orc_cdbhash_i64(key)
        assert orc.lib.orc_route_i64(key, 8) == orc.lib.orc_jump_consistent_hash(h, 8)
        assert orc.lib.orc_cdbhash_i64(key) == orc.lib.orc_hashint8(key)  # 1-key chain: rot1(0)^h = h


def test_crc32c_standard_vector():
    # "123456789" → CRC-32C 0xE3069283 (finalised); pg state = that ^ 0xFFFFFFFF
    buf = b"123456789"
    state = orc.lib.orc_crc32c(0xFFFFFFFF, buf, len(buf))
    assert state ^ 0xFFFFFFFF == 0xE3069283


# ---------------- dates ----------------

def test_date_adt():
    d = orc.lib.orc_date_adt
    assert d(2000, 1, 1) == 0
    assert d(2000, 1, 2) == 1
    assert d(1999, 12, 31) == -1
    assert d(1995, 3, 15) == -1753
    assert d(1992, 1, 1) - d(1998, 8, 2) == -2405   # orders span
    assert d(1992, 1, 2) - d(1998, 12, 1) == -2525  # shipdate span


# ---------------- datagen invariants ----------------

SF = 0.01


def test_gen_shapes_and_ranges():
    c = orc.gen_customer(SF)
    o = orc.gen_orders(SF)
    li = orc.gen_lineitem(SF)
    assert len(c["c_custkey"]) == 1500
    assert len(o["o_orderkey"]) == 15000
    assert 15000 <= len(li["l_orderkey"]) <= 7 * 15000
    assert c["c_mktsegment"].max() <= 4
    assert (o["o_custkey"] >= 1).all() and (o["o_custkey"] <= 1000).all()
    dlo, dhi = orc.lib.orc_date_adt(1992, 1, 1), orc.lib.orc_date_adt(1998, 8, 2)
    assert o["o_orderdate"].min() >= dlo and o["o_orderdate"].max() <= dhi
    assert (li["l_extendedprice"] >= 900).all() and (li["l_extendedprice"] <= 105000).all()
    assert (li["l_discount"] >= 0).all() and (li["l_discount"] <= 0.10 + 1e-12).all()
    # lineitems are clustered by orderkey, ≤7 per key
    _, counts = np.unique(li["l_orderkey"], return_counts=True)
    assert counts.max() <= 7


def test_gen_sharding_partitions_globally():
    """Union of per-seg shards == global table; each row routed per cdbhash."""
    nsegs = 4
    glob = orc.gen_orders(SF)
    parts = [orc.gen_orders(SF, seg=s, nsegs=nsegs) for s in range(nsegs)]
    tot = sum(len(p["o_orderkey"]) for p in parts)
    assert tot == len(glob["o_orderkey"])
    allk = np.sort(np.concatenate([p["o_orderkey"] for p in parts]))
    assert (allk == np.sort(glob["o_orderkey"])).all()
    for s, p in enumerate(parts):
        for k in p["o_orderkey"][:50]:
            assert orc.lib.orc_route_i64(int(k), nsegs) == s


def test_gen_determinism():
    a = orc.gen_lineitem(SF)
    b = orc.gen_lineitem(SF)
    for f in a:
        assert (a[f] == b[f]).all()


# ---------------- AOCS codec ----------------

def test_aocs_roundtrip_i64():
    rng = np.random.default_rng(3)
    vals = rng.integers(-2**62, 2**62, 10000, dtype=np.int64)
    s = orc.aocs_encode(vals)
    out = orc.aocs_decode(s, 8, len(vals), np.int64)
    assert (out == vals).all()


def test_aocs_roundtrip_i32_and_f64():
    rng = np.random.default_rng(4)
    v32 = rng.integers(-2**30, 2**30, 9001, dtype=np.int32)
    assert (orc.aocs_decode(orc.aocs_encode(v32), 4, len(v32), np.int32) == v32).all()
    vf = rng.random(4091)
    assert (orc.aocs_decode(orc.aocs_encode(vf), 8, len(vf), np.float64) == vf).all()


def test_aocs_block_geometry():
    # reference writer capacity rule at blocksize 32768 (datumstreamblock.c:1508-1560)
    assert orc.lib.orc_aocs_rows_per_block(8, 32768) == 4090
    assert orc.lib.orc_aocs_rows_per_block(4, 32768) == 8181


def test_aocs_header_bitfields():
    """Decode the first block header with the reference's Get macros restated."""
    vals = np.arange(5000, dtype=np.int64)
    s = orc.aocs_encode(vals)
    b03 = int.from_bytes(s[0:4], "little")
    b47 = int.from_bytes(s[4:8], "little")
    assert (b03 >> 28) & 7 == 1            # AoHeaderKind_SmallContent
    assert (b03 >> 27) & 1 == 1            # hasFirstRowNum
    assert (b03 >> 24) & 7 == 1            # AOCSBK_BLOCK
    assert (b03 & 0x00FFFC00) >> 10 == 4090    # rowCount
    datalen = ((b03 & 0x3FF) << 11) | ((b47 & 0xFFE00000) >> 21)
    assert datalen == 16 + 4090 * 8
    assert b47 & 0x1FFFFF == 0             # compressedLength
    assert int.from_bytes(s[16:24], "little") == 1   # firstRowNum
    # Orig datum-stream header at content offset
    assert int.from_bytes(s[24:26], "little") == 0   # version Original
    assert int.from_bytes(s[28:30], "little") == 4090  # ndatum


def test_aocs_checksum_detects_corruption():
    vals = np.arange(100, dtype=np.int64)
    s = bytearray(orc.aocs_encode(vals))
    s[50] ^= 0xFF
    buf = np.frombuffer(bytes(s), np.uint8)
    out = np.zeros(100, np.int64)
    got = orc.lib.orc_aocs_decode(buf.ctypes.data, len(buf), 8, out.ctypes.data, 100, 1)
    assert got == -2


# ---------------- RLE (Dense_Enhanced) codec ----------------

def test_rle_roundtrip_clustered():
    """TPC-H-like clustered keys (≤7 repeats): encode_rle → decode == input,
    with a real compression win."""
    rng = np.random.default_rng(6)
    keys = np.repeat(np.arange(1, 30000, dtype=np.int64),
                     rng.integers(1, 8, 29999))
    s = orc.aocs_encode_rle(keys)
    assert len(s) < len(keys) * 8 / 2   # ≥2x compression
    out = orc.aocs_decode(s, 8, len(keys), np.int64)
    np.testing.assert_array_equal(out, keys)


def test_rle_roundtrip_extremes():
    # all-identical (one giant run), strictly-increasing (no runs), widths 4+8
    one = np.full(100000, 7, np.int64)
    np.testing.assert_array_equal(orc.aocs_decode(orc.aocs_encode_rle(one), 8,
                                                  len(one), np.int64), one)
    asc = np.arange(50000, dtype=np.int32)
    np.testing.assert_array_equal(orc.aocs_decode(orc.aocs_encode_rle(asc), 4,
                                                  len(asc), np.int32), asc)
    # runs crossing varint-length boundaries (63/64, 16383/16384)
    v = np.concatenate([np.full(64, 1), np.full(65, 2), np.full(16384, 3),
                        np.full(16385, 4), np.arange(100)]).astype(np.int64)
    np.testing.assert_array_equal(orc.aocs_decode(orc.aocs_encode_rle(v), 8,
                                                  len(v), np.int64), v)


def test_rle_block_headers_and_checksums():
    keys = np.repeat(np.arange(1, 100000, dtype=np.int64), 5)
    s = orc.aocs_encode_rle(keys)
    b03 = int.from_bytes(s[0:4], "little")
    kind = (b03 >> 28) & 7
    assert kind in (1, 3)
    assert int.from_bytes(s[24:26], "little") == 2    # Dense_Enhanced
    assert int.from_bytes(s[26:28], "little") == 2    # DSB_HAS_RLE_COMPRESSION
    # corruption detection
    bad = bytearray(s)
    bad[60] ^= 0xFF
    buf = np.frombuffer(bytes(bad), np.uint8)
    out = np.zeros(len(keys), np.int64)
    got = orc.lib.orc_aocs_decode(buf.ctypes.data, len(buf), 8,
                                  out.ctypes.data, len(keys), 1)
    assert got == -2


# ---------------- Q3 vs independent numpy brute force ----------------

def brute_force_q3(c, o, li, cutoff):
    seg_ok = c["c_custkey"][c["c_mktsegment"] == 0]
    omask = (o["o_orderdate"] < cutoff) & np.isin(o["o_custkey"], seg_ok)
    okeys = o["o_orderkey"][omask]
    odate = dict(zip(o["o_orderkey"][omask].tolist(), o["o_orderdate"][omask].tolist()))
    oprio = dict(zip(o["o_orderkey"][omask].tolist(), o["o_shippriority"][omask].tolist()))
    lmask = (li["l_shipdate"] > cutoff) & np.isin(li["l_orderkey"], okeys)
    rev = {}
    cnt = {}
    for k, p, d in zip(li["l_orderkey"][lmask].tolist(),
                       li["l_extendedprice"][lmask], li["l_discount"][lmask]):
        rev[k] = rev.get(k, 0.0) + p * (1.0 - d)
        cnt[k] = cnt.get(k, 0) + 1
    keys = sorted(rev)
    return {"l_orderkey": np.array(keys, np.int64),
            "o_orderdate": np.array([odate[k] for k in keys], np.int32),
            "o_shippriority": np.array([oprio[k] for k in keys], np.int32),
            "revenue": np.array([rev[k] for k in keys]),
            "nitems": np.array([cnt[k] for k in keys], np.int64)}


def test_q3_oracle_vs_numpy_bruteforce():
    c = orc.gen_customer(SF)
    o = orc.gen_orders(SF)
    li = orc.gen_lineitem(SF)
    got = orc.q3(c, o, li)
    want = brute_force_q3(c, o, li, orc.CUTOFF_19950315)
    assert (got["l_orderkey"] == want["l_orderkey"]).all()
    assert (got["o_orderdate"] == want["o_orderdate"]).all()
    assert (got["o_shippriority"] == want["o_shippriority"]).all()
    assert (got["nitems"] == want["nitems"]).all()
    np.testing.assert_allclose(got["revenue"], want["revenue"], rtol=1e-12)
    assert len(got["l_orderkey"]) > 50  # non-trivial result


def test_q3_sharded_equals_global():
    """Per-segment Q3 on hash-distributed shards with Motion emulation,
    unioned, == global Q3 — the reference's MPP claim (plan
    shape DESIGN §8e: Motion-1 orders by o_custkey, Motion-2 qualifying
    orders by o_orderkey, one-stage agg co-located with lineitem)."""
    nsegs = 3
    cutoff = orc.CUTOFF_19950315
    c = orc.gen_customer(SF)
    o = orc.gen_orders(SF)
    li = orc.gen_lineitem(SF)
    glob = orc.q3(c, o, li)

    c_route = orc.route(c["c_custkey"], nsegs)          # customer home segs
    o_m1 = orc.route(o["o_custkey"], nsegs)             # Motion 1 target
    o_m2 = orc.route(o["o_orderkey"], nsegs)            # Motion 2 target
    l_route = orc.route(li["l_orderkey"], nsegs)        # lineitem home segs

    # stage 1 on each seg: local BUILDING customers ⋈ Motion-1 orders
    qual_mask = np.zeros(len(o["o_orderkey"]), bool)
    for s in range(nsegs):
        segok = c["c_custkey"][(c_route == s) & (c["c_mktsegment"] == 0)]
        m = (o_m1 == s) & (o["o_orderdate"] < cutoff) & np.isin(o["o_custkey"], segok)
        qual_mask |= m

    # stage 2 on each seg: Motion-2 qualifying orders ⋈ local lineitem + agg
    res = []
    for s in range(nsegs):
        om2 = qual_mask & (o_m2 == s)
        o2 = {f: o[f][om2] for f in o}
        ls = {f: li[f][l_route == s] for f in li}
        # customer filter already applied upstream → pass-through set
        c2 = {"c_custkey": o2["o_custkey"],
              "c_mktsegment": np.zeros(len(o2["o_custkey"]), np.uint8)}
        res.append(orc.q3(c2, o2, ls))
    keys = np.concatenate([r["l_orderkey"] for r in res])
    rev = np.concatenate([r["revenue"] for r in res])
    order = np.argsort(keys)
    assert (keys[order] == glob["l_orderkey"]).all()
    np.testing.assert_allclose(rev[order], glob["revenue"], rtol=1e-9)


# ---------------- numeric(15,2) mode ----------------

def test_q3_numeric_exact_vs_python():
    """Scaled-int64 revenue numerators must be EXACTLY the integer sums a
    pure-python recomputation gives (no tolerance)."""
    c = orc.gen_customer(SF)
    o = orc.gen_orders(SF)
    li = orc.gen_lineitem(SF)
    got = orc.q3_numeric(c, o, li)
    f64 = orc.q3(c, o, li)
    assert (got["l_orderkey"] == f64["l_orderkey"]).all()
    assert (got["nitems"] == f64["nitems"]).all()
    # cross-check vs f64 sums within rounding
    np.testing.assert_allclose(got["revenue_num"] / 1e4, f64["revenue"], rtol=1e-9)
    # exact recomputation for sampled groups
    price_c = np.rint(li["l_extendedprice"] * 100).astype(np.int64)
    disc_c = np.rint(li["l_discount"] * 100).astype(np.int64)
    ok = li["l_shipdate"] > orc.CUTOFF_19950315
    rng = np.random.default_rng(2)
    for i in rng.choice(len(got["l_orderkey"]), 50, replace=False):
        k = got["l_orderkey"][i]
        m = ok & (li["l_orderkey"] == k)
        want = int((price_c[m] * (100 - disc_c[m])).sum())
        assert int(got["revenue_num"][i]) == want


# ---------------- DELTA_RANGE codec ----------------

def test_rle_delta_roundtrips():
    rng = np.random.default_rng(8)
    cases = [
        np.repeat(np.arange(1, 20000, dtype=np.int64), rng.integers(1, 8, 19999)),
        np.cumsum(rng.integers(-100, 100, 40000)).astype(np.int64),
        (-2921 + rng.integers(0, 2526, 50000)).astype(np.int32),
        rng.integers(-2**60, 2**60, 9000).astype(np.int64),      # deltas too wide
        np.cumsum(rng.integers(0, 2**33, 9000)).astype(np.int64),  # mixed
        np.full(100000, 42, np.int64),
        np.array([7], np.int64),
        np.array([0x1FFFFFFF, 2 * 0x1FFFFFFF, 0], np.int64),     # boundary deltas
    ]
    for v in cases:
        s = orc.aocs_encode_rle_delta(v)
        out = orc.aocs_decode(s, v.itemsize, len(v), v.dtype)
        np.testing.assert_array_equal(out, v)


def test_rle_delta_compression_wins():
    rng = np.random.default_rng(9)
    keys = np.repeat(np.arange(1, 50000, dtype=np.int64), rng.integers(1, 8, 49999))
    s_rle = orc.aocs_encode_rle(keys)
    s_rd = orc.aocs_encode_rle_delta(keys)
    assert len(s_rd) < len(s_rle) / 3     # delta on ascending keys ≫ rle alone
    assert len(s_rd) < len(keys) * 8 / 10  # ≥10x total


def test_rle_delta_corruption_detected():
    keys = np.cumsum(np.ones(30000, np.int64))
    s = bytearray(orc.aocs_encode_rle_delta(keys))
    s[70] ^= 0xFF
    buf = np.frombuffer(bytes(s), np.uint8)
    out = np.zeros(len(keys), np.int64)
    assert orc.lib.orc_aocs_decode(buf.ctypes.data, len(buf), 8,
                                   out.ctypes.data, len(keys), 1) == -2


# ---------------- zlib bulk compression ----------------

def test_zlib_roundtrip_and_fallback():
    import ctypes
    lib = orc.lib
    lib.orc_aocs_encode_zlib.restype = ctypes.c_int64
    lib.orc_aocs_encode_zlib.argtypes = [ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int64]
    rng = np.random.default_rng(10)
    for vals in (np.repeat(np.arange(1, 9000, dtype=np.int64), 4),
                 rng.integers(-2**60, 2**60, 15000).astype(np.int64),
                 (-2921 + rng.integers(0, 2526, 30000)).astype(np.int32)):
        w = vals.itemsize
        buf = np.zeros(len(vals) * w + 2**20, np.uint8)
        got = lib.orc_aocs_encode_zlib(vals.ctypes.data, w, len(vals), 1,
                                       32768, 6, buf.ctypes.data, len(buf))
        assert got > 0
        out = np.zeros(len(vals), vals.dtype)
        dec = lib.orc_aocs_decode(buf.ctypes.data, got, w,
                                  out.ctypes.data, len(vals), 1)
        assert dec == len(vals)
        np.testing.assert_array_equal(out, vals)
    # repetitive data must actually shrink
    rep = np.repeat(np.arange(1, 9000, dtype=np.int64), 4)
    buf = np.zeros(len(rep) * 8 + 2**20, np.uint8)
    got = lib.orc_aocs_encode_zlib(rep.ctypes.data, 8, len(rep), 1, 32768, 6,
                                   buf.ctypes.data, len(buf))
    assert got < len(rep) * 8 / 3


def test_crc32c_golden_from_reference():
    """The oracle/GPU CRC32C state (unfinalised, the AO block convention)
    vs the reference's own pg_crc32c_sb8.c compiled standalone."""
    v = _vectors()
    assert "crc32c_state" in v, "regenerate tests/golden via oracle/gen_golden.py"
    for e in v["crc32c_state"]:
        data = bytes.fromhex(e["data"])
        assert orc.lib.orc_crc32c(0xFFFFFFFF, data, len(data)) == e["state"]


def test_zstd_roundtrip():
    rng = np.random.default_rng(11)
    for vals in (np.repeat(np.arange(1, 9000, dtype=np.int64), 4),
                 rng.integers(-2**60, 2**60, 12000).astype(np.int64)):
        s = orc.aocs_encode_zstd(vals)
        buf = np.frombuffer(s, np.uint8)
        out = np.zeros(len(vals), vals.dtype)
        got = orc.lib.orc_aocs_decode_c(buf.ctypes.data, len(buf), vals.itemsize,
                                        out.ctypes.data, len(vals), 1, 2)
        assert got == len(vals)
        np.testing.assert_array_equal(out, vals)


def test_q1_oracle_vs_numpy():
    sf, cut = 0.02, orc.lib.orc_date_adt(1998, 9, 2)
    want = orc.q1(sf, cut)
    li = orc.gen_lineitem(sf)
    # recompute flag/status via the shared generator streams
    o = li["l_orderkey"]
    # line index within order: position among equal keys
    line = np.zeros(len(o), np.int64)
    _, starts = np.unique(o, return_index=True)
    for s in starts:
        k = o[s]
        j = 0
        while s + j < len(o) and o[s + j] == k:
            line[s + j] = j
            j += 1
    flag = np.array([orc.lib.orc_mix(42, 9, int(k) * 8 + int(j)) % 3
                     for k, j in zip(o, line)])
    stat = np.array([orc.lib.orc_mix(42, 10, int(k) * 8 + int(j)) % 2
                     for k, j in zip(o, line)])
    ok = li["l_shipdate"] <= cut
    for g in range(6):
        m = ok & (flag == g // 2) & (stat == g % 2)
        assert want["count"][g] == int(m.sum())
        np.testing.assert_allclose(want["sum_price"][g],
                                   li["l_extendedprice"][m].sum(), rtol=1e-9)


def test_gen_lineitem_q1_matches_q1_and_lineitem():
    """gen_lineitem_q1 materializes the rows orc_q1 aggregates inline: its
    shared columns equal gen_lineitem's, numpy-aggregating it reproduces
    orc_q1's counts exactly, and a shard is the matching slice of rows."""
    sf, seed = 0.02, 42
    q = orc.gen_lineitem_q1(sf, seed)
    li = orc.gen_lineitem(sf, seed)
    for f in ("l_extendedprice", "l_discount", "l_shipdate"):
        np.testing.assert_array_equal(q[f], li[f])
    assert q["l_returnflag"].dtype == np.int8 and q["l_linestatus"].dtype == np.int8
    assert set(np.unique(q["l_returnflag"])) == {0, 1, 2}
    assert set(np.unique(q["l_linestatus"])) == {0, 1}
    g = q["l_returnflag"].astype(np.int64) * 2 + q["l_linestatus"]
    lo, hi = int(q["l_shipdate"].min()), int(q["l_shipdate"].max())
    for cut in (lo - 1, orc.lib.orc_date_adt(1995, 3, 15),
                orc.lib.orc_date_adt(1998, 9, 2), hi):
        want = orc.q1(sf, cut, seed)
        ok = q["l_shipdate"] <= cut
        got = np.bincount(g[ok], minlength=6)
        np.testing.assert_array_equal(got, want["count"])
        for gi in range(6):
            m = ok & (g == gi)
            np.testing.assert_allclose(q["l_extendedprice"][m].sum(),
                                       want["sum_price"][gi], rtol=1e-9)
            np.testing.assert_allclose(
                (q["l_extendedprice"][m] * (1.0 - q["l_discount"][m])).sum(),
                want["sum_revenue"][gi], rtol=1e-9)
    # sharded: same rows as gen_lineitem's shard, and shards partition the table
    tot = 0
    for seg in range(3):
        qs = orc.gen_lineitem_q1(sf, seed, seg, 3)
        ls = orc.gen_lineitem(sf, seed, seg, 3)
        np.testing.assert_array_equal(qs["l_shipdate"], ls["l_shipdate"])
        np.testing.assert_array_equal(qs["l_extendedprice"], ls["l_extendedprice"])
        tot += len(qs["l_returnflag"])
    assert tot == len(q["l_returnflag"])
    assert len(orc.gen_lineitem_q1(0.0)["l_returnflag"]) == 0


# ---------------- REFERENCE-writer parity (the strongest format pin) ----------------

def _ref_fixture_values():
    rng = np.random.default_rng(20260915)
    keys = np.repeat(np.arange(1, 12000, dtype=np.int64),
                     rng.integers(1, 8, 11999))
    zig = np.cumsum(rng.integers(-60, 60, 30000)).astype(np.int32)
    return keys, zig


def test_decode_reference_writer_golden_fixtures():
    """Blocks produced by the REFERENCE's own datumstreamblock.c writer
    (rle_type + delta_range), committed as fixtures — our decoder must
    reproduce the inputs exactly."""
    keys, zig = _ref_fixture_values()
    s = open(os.path.join(HERE, "golden", "refwriter_rle_delta_i64.bin"), "rb").read()
    np.testing.assert_array_equal(orc.aocs_decode(s, 8, len(keys), np.int64), keys)
    s = open(os.path.join(HERE, "golden", "refwriter_rle_delta_i32.bin"), "rb").read()
    np.testing.assert_array_equal(orc.aocs_decode(s, 4, len(zig), np.int32), zig)


def test_decode_reference_writer_live():
    """When oracle/_ref/libpgwriter.so is present, fuzz our decoder against
    the live reference writer across versions/compression modes."""
    if orc.ref_writer() is None:
        pytest.skip("reference writer not built")
    rng = np.random.default_rng(13)
    cases = [
        (np.repeat(np.arange(1, 20000, dtype=np.int64), rng.integers(1, 8, 19999)), 2, 1, 1),
        (np.cumsum(rng.integers(-100, 100, 60000)).astype(np.int64), 2, 1, 1),
        (rng.integers(-2**60, 2**60, 15000).astype(np.int64), 2, 1, 1),
        ((-2921 + rng.integers(0, 2526, 40000)).astype(np.int32), 2, 1, 1),
        (np.full(100000, 7, np.int64), 2, 1, 0),
        (np.arange(30000, dtype=np.int64), 2, 0, 1),
        (rng.integers(0, 2**30, 12000).astype(np.int64), 0, 0, 0),
    ]
    for vals, ver, rle, delta in cases:
        s = orc.ref_writer_stream(vals, version=ver, rle=rle, delta=delta)
        out = orc.aocs_decode(s, vals.itemsize, len(vals), vals.dtype)
        np.testing.assert_array_equal(out, vals)


def test_orig_encoder_byte_exact_vs_reference_writer():
    """Our Orig-format encoder is BYTE-EXACT with the reference's own
    datumstreamblock.c writer (live differential test) for every width."""
    if orc.ref_writer() is None:
        pytest.skip("reference writer not built")
    rng = np.random.default_rng(17)
    cases = [rng.integers(-2**60, 2**60, 23456).astype(np.int64),
             rng.integers(-2**30, 2**30, 30001).astype(np.int32),
             rng.integers(0, 5, 40000).astype(np.int8),
             rng.random(10007).view(np.float64)]
    for vals in cases:
        ours = orc.aocs_encode(vals)
        ref = orc.ref_writer_stream(vals.view((np.int64, np.int32, np.int8)[
            {8: 0, 4: 1, 1: 2}[vals.itemsize]]), version=0, rle=0, delta=0)
        assert ours == ref, f"width {vals.itemsize} diverges"


def test_rle_delta_encoder_byte_exact_vs_reference_writer():
    """Our Dense_Enhanced RLE_TYPE(+DELTA) encoder is BYTE-EXACT with the
    reference's own compiled writer (datumstreamblock.c PutDense/BlockDense
    state machine, incl. lazy repeat-count finalization, the pessimistic
    capacity accounting, and delta-0-after-MAXREPEAT folding)."""
    if orc.ref_writer() is None:
        pytest.skip("reference writer not built")
    rng = np.random.default_rng(7)
    cases = [
        # (vals, delta?)
        (np.repeat(np.arange(1, 12000, dtype=np.int64),
                   rng.integers(1, 8, 11999)), 1),          # TPC-H-like keys
        (np.repeat(np.arange(1, 12000, dtype=np.int64),
                   rng.integers(1, 8, 11999)), 0),          # rle only
        (rng.integers(-2922, -500, 60000).astype(np.int32), 1),
        (np.cumsum(rng.integers(-1000, 1000, 50000)).astype(np.int32), 1),
        (np.full(2_000_000, 42, np.int64), 1),              # one giant run
        (np.arange(100000, dtype=np.int32), 1),             # pure delta
        (rng.integers(-2**62, 2**62, 30000).astype(np.int64), 1),  # delta off
        (np.concatenate([np.full(70000, 5, np.int64),
                         rng.integers(0, 2**40, 30000).astype(np.int64)]), 1),
        (np.array([7], np.int64), 1),
        (rng.integers(0, 3, 100000).astype(np.uint8), 0),   # width-1 rle
    ]
    for vals, delta in cases:
        ours = (orc.aocs_encode_rle_delta(vals) if delta
                else orc.aocs_encode_rle(vals))
        ref = orc.ref_writer_stream(vals, version=2, rle=1, delta=delta)
        assert ours == ref, f"width {vals.itemsize} delta={delta} diverges"
        # and our decoder round-trips the (identical) stream
        out = orc.aocs_decode(bytes(ours), vals.itemsize, len(vals), vals.dtype)
        np.testing.assert_array_equal(out, vals)


def test_null_bitmap_encoders_byte_exact_vs_reference_writer():
    """NULL-bearing blocks: both the Orig and the Dense_Enhanced RLE(+DELTA)
    encoders are BYTE-EXACT with the compiled reference writer (null bitmap
    zero-fill on first null, per-non-repeat-slot bits, HasSpaceNull
    accounting — datumstreamblock.c:1992-2090, 3120-3147), and the nullable
    decoder round-trips values + validity."""
    if orc.ref_writer() is None:
        pytest.skip("reference writer not built")
    rng = np.random.default_rng(11)
    vals64 = np.repeat(np.arange(1, 9000, dtype=np.int64),
                       rng.integers(1, 9, 8999))[:60000]
    n10 = (rng.random(len(vals64)) < 0.1).astype(np.uint8)
    v32 = rng.integers(-3000, 3000, 50000).astype(np.int32)
    n50 = (rng.random(50000) < 0.5).astype(np.uint8)
    vconst = np.full(40000, 7, np.int64)
    nper = np.zeros(40000, np.uint8)
    nper[::97] = 1
    cases = [
        # (vals, nulls, version, delta)
        (vals64, n10, 2, 1),
        (vals64, n10, 2, 0),
        (vals64, n10, 0, 0),
        (v32, n50, 2, 1),
        (v32, n50, 0, 0),
        (np.zeros(30000, np.int64), np.ones(30000, np.uint8), 2, 1),  # all null
        (np.zeros(30000, np.int64), np.ones(30000, np.uint8), 0, 0),
        (vconst, nper, 2, 1),                    # nulls breaking one long run
    ]
    for vals, nulls, ver, delta in cases:
        if ver == 0:
            ours = orc.aocs_encode_orig_nulls(vals, nulls)
            ref = orc.ref_writer_stream(vals, 0, 0, 0, nulls=nulls)
        else:
            ours = orc.aocs_encode_rle_delta_nulls(vals, nulls, delta)
            ref = orc.ref_writer_stream(vals, 2, 1, delta, nulls=nulls)
        assert ours == ref, f"v{ver} delta={delta} diverges"
        out, valid = orc.aocs_decode_nullable(ours, vals.itemsize, len(vals),
                                              vals.dtype)
        np.testing.assert_array_equal(valid, (nulls == 0).astype(np.uint8))
        m = nulls == 0
        np.testing.assert_array_equal(out[m], vals[m])
        assert (out[~m] == 0).all()


def test_plain_decode_refuses_null_blocks():
    """orc_aocs_decode (no validity output) fails loudly on NULL-bearing
    blocks instead of returning garbage."""
    vals = np.arange(1000, dtype=np.int64)
    nulls = np.zeros(1000, np.uint8)
    nulls[5] = 1
    s = orc.aocs_encode_rle_delta_nulls(vals, nulls)
    with pytest.raises(AssertionError):
        orc.aocs_decode(s, 8, 1000, np.int64)
    s0 = orc.aocs_encode_orig_nulls(vals, nulls)
    with pytest.raises(AssertionError):
        orc.aocs_decode(s0, 8, 1000, np.int64)


def test_multi_segfile_stream_concat_decodes():
    """A column scanned across MULTIPLE AO segment files is the
    concatenation of their streams (aocsam.c open_next_scan_seg advances
    through segfiles); the decoder walks block-by-block with a running row
    counter, so concatenated streams decode as one logical column."""
    rng = np.random.default_rng(41)
    vals = np.repeat(np.arange(1, 7000, dtype=np.int64),
                     rng.integers(1, 9, 6999))
    cut = len(vals) // 3
    s = (orc.aocs_encode_rle_delta(vals[:cut])
         + orc.aocs_encode_rle_delta(vals[cut:2 * cut])
         + orc.aocs_encode_rle_delta(vals[2 * cut:]))
    out = orc.aocs_decode(s, 8, len(vals), np.int64)
    np.testing.assert_array_equal(out, vals)
    # Orig segfiles concatenate the same way
    s0 = orc.aocs_encode(vals[:cut]) + orc.aocs_encode(vals[cut:])
    np.testing.assert_array_equal(orc.aocs_decode(s0, 8, len(vals), np.int64),
                                  vals)


def test_empty_and_single_row_tables():
    """Empty AOCS streams (0 blocks) and single-row blocks — the edge cases
    the reference's AO regress tests exercise (uao_* schedules)."""
    empty = np.array([], np.int64)
    for enc in (orc.aocs_encode, orc.aocs_encode_rle, orc.aocs_encode_rle_delta):
        s = enc(empty)
        assert s == b""
        np.testing.assert_array_equal(orc.aocs_decode(s, 8, 0, np.int64), empty)
    one = np.array([42], np.int64)
    for enc in (orc.aocs_encode, orc.aocs_encode_rle, orc.aocs_encode_rle_delta):
        np.testing.assert_array_equal(orc.aocs_decode(enc(one), 8, 1, np.int64),
                                      one)
    # empty inputs through the whole pipeline
    c = {"c_custkey": empty, "c_mktsegment": np.array([], np.uint8)}
    o = {"o_orderkey": empty, "o_custkey": empty,
         "o_orderdate": np.array([], np.int32),
         "o_shippriority": np.array([], np.int32)}
    l = {"l_orderkey": empty, "l_extendedprice": np.array([], np.float64),
         "l_discount": np.array([], np.float64),
         "l_shipdate": np.array([], np.int32)}
    assert len(orc.q3(c, o, l)["l_orderkey"]) == 0


def test_varlena_encoder_byte_exact_vs_reference_writer():
    """Varlena (text) Orig streams: our encoder byte-equals the compiled
    reference writer (short-form conversion <=126 B payload, zero-pad
    alignment for 4-byte headers, NULL bitmap), and the decoder
    round-trips values + validity."""
    if orc.ref_writer() is None:
        pytest.skip("reference writer not built")
    rng = np.random.default_rng(53)
    words = [b"BUILDING", b"AUTOMOBILE", b"MACHINERY", b"HOUSEHOLD",
             b"FURNITURE"]
    strings = [words[i % 5] + b"-" + str(i).encode() for i in range(50000)]
    for i in range(0, 50000, 37):       # long values force 4-byte headers
        strings[i] = bytes(rng.integers(65, 90,
                                        int(rng.integers(127, 400)))
                           .astype(np.uint8))
    strings[7] = b""                     # empty string
    mine = orc.aocs_encode_varlena(strings)
    assert mine == orc.ref_writer_varlena_stream(strings)
    assert orc.aocs_decode_varlena(mine, len(strings)) == strings
    nulls = (rng.random(50000) < 0.12).astype(np.uint8)
    mine2 = orc.aocs_encode_varlena(strings, nulls)
    assert mine2 == orc.ref_writer_varlena_stream(strings, nulls)
    out2 = orc.aocs_decode_varlena(mine2, len(strings))
    assert out2 == [None if nulls[i] else strings[i]
                    for i in range(len(strings))]
    # Dense_Enhanced rle_type varlena (RLE on repeated payloads)
    reps = []
    for i, r in enumerate(rng.integers(1, 60, 2000)):
        reps += [words[i % 5]] * int(r)
    for i in range(0, len(reps), 97):
        reps[i] = bytes(rng.integers(65, 90,
                                     int(rng.integers(127, 300)))
                        .astype(np.uint8))
    mrle = orc.aocs_encode_varlena_rle(reps)
    assert mrle == orc.ref_writer_varlena_stream(reps, version=2, rle=1)
    assert orc.aocs_decode_varlena(mrle, len(reps)) == reps
    nl = (rng.random(len(reps)) < 0.1).astype(np.uint8)
    mrle2 = orc.aocs_encode_varlena_rle(reps, nl)
    assert mrle2 == orc.ref_writer_varlena_stream(reps, nulls=nl,
                                                  version=2, rle=1)
    # one giant run crosses into the NonBulkDense envelope
    big = [b"BUILDING"] * 100000
    mbig = orc.aocs_encode_varlena_rle(big)
    assert mbig == orc.ref_writer_varlena_stream(big, version=2, rle=1)
    assert orc.aocs_decode_varlena(mbig, len(big)) == big


def test_varlena_short_form_boundary():
    """The short-form threshold: payload <= 126 B stores as 1-byte-header
    short varlena, 127 B+ stores aligned with a 4-byte header
    (VARATT_CAN_MAKE_SHORT, varatt.h:261-264).  Byte-exact vs the
    reference writer right at the boundary, both formats."""
    if orc.ref_writer() is None:
        pytest.skip("reference writer not built")
    vals = []
    for ln in (0, 1, 125, 126, 127, 128, 300):
        vals += [bytes([65 + (ln % 26)]) * ln] * 3    # runs of 3 each
    for ver, rle in ((0, 0), (2, 1)):
        if ver == 0:
            ours = orc.aocs_encode_varlena(vals)
        else:
            ours = orc.aocs_encode_varlena_rle(vals)
        ref = orc.ref_writer_varlena_stream(vals, version=ver, rle=rle)
        assert ours == ref, f"v{ver} boundary diverges"
        assert orc.aocs_decode_varlena(ours, len(vals)) == vals


# ---------------- multi-key cdbhash (cdbhash.c:189-247) ----------------

def _py_cdbhash_multi(vals, types, isnull=None, hashfn=None):
    """Independent restatement of the reference rotate-combine loop
    (cdbhash.c:189-216) on top of the golden-pinned per-type hashes."""
    h8 = hashfn or (lambda v: orc.lib.orc_hashint8(int(v)))
    h4 = lambda v: orc.lib.orc_hash_bytes_uint32(np.uint32(np.int32(v)))
    h = 0
    for k, (v, t) in enumerate(zip(vals, types)):
        h = ((h << 1) | (h >> 31)) & 0xFFFFFFFF      # pg_rotate_left32(h, 1)
        if isnull is not None and isnull[k]:
            continue                                  # NULL: rotation only
        h ^= (h4(v) if t == 1 else h8(v))
    return h


def test_cdbhash_multi_matches_independent_restatement():
    rng = np.random.default_rng(31)
    for nkeys in (1, 2, 3, 5):
        vals = rng.integers(-2**62, 2**62, (200, nkeys)).astype(np.int64)
        types = rng.integers(0, 2, nkeys).astype(np.int32)
        # clamp int4-typed attrs into int32 range (widened representation)
        for k in range(nkeys):
            if types[k] == 1:
                vals[:, k] = rng.integers(-2**31, 2**31, 200)
        nulls = (rng.random((200, nkeys)) < 0.2).astype(np.uint8)
        for i in range(200):
            want = _py_cdbhash_multi(vals[i], types, nulls[i])
            got = orc.cdbhash_multi(vals[i], types, nulls[i])
            assert got == want, (i, nkeys)
        # all-NOT-NULL path (isnull omitted)
        for i in range(50):
            want = _py_cdbhash_multi(vals[i], types)
            assert orc.cdbhash_multi(vals[i], types) == want


def test_cdbhash_multi_single_key_equals_route():
    """1-key multi chain must equal the established single-key chain
    (pinned by the reference golden vectors)."""
    rng = np.random.default_rng(32)
    keys = rng.integers(-2**62, 2**62, 500).astype(np.int64)
    types = np.zeros(1, np.int32)
    for nsegs in (2, 8, 64):
        got = orc.route_multi(keys.reshape(-1, 1), types, nsegs)
        want = orc.route(keys, nsegs)
        np.testing.assert_array_equal(got, want)


def test_cdbhash_multi_against_live_reference_if_present():
    """When the compiled reference hashfn.c is present, drive the rotate-
    combine loop with the REFERENCE's own hash function — pins the multi-key
    chain end to end."""
    import ctypes
    ref_so = os.path.join(HERE, "..", "oracle", "_ref", "libpgref.so")
    if not os.path.exists(ref_so):
        pytest.skip("oracle/_ref not built here")
    ref = ctypes.CDLL(ref_so)
    ref.hash_bytes_uint32.restype = ctypes.c_uint32
    ref.hash_bytes_uint32.argtypes = [ctypes.c_uint32]

    def ref_hashint8(v):
        v = int(v)
        lo = v & 0xFFFFFFFF
        hi = (v >> 32) & 0xFFFFFFFF
        lo ^= hi if v >= 0 else (~hi & 0xFFFFFFFF)
        return ref.hash_bytes_uint32(lo)

    rng = np.random.default_rng(33)
    vals = rng.integers(-2**62, 2**62, (100, 3)).astype(np.int64)
    types = np.zeros(3, np.int32)
    for i in range(100):
        want = _py_cdbhash_multi(vals[i], types, hashfn=ref_hashint8)
        assert orc.cdbhash_multi(vals[i], types) == want


def test_route_multi_null_only_rows():
    """An all-NULL key row hashes to 0-rotated-N = 0 -> jump(0, n); matches
    cdbhash semantics where NULLs contribute only rotations."""
    vals = np.zeros((4, 2), np.int64)
    nulls = np.ones((4, 2), np.uint8)
    types = np.zeros(2, np.int32)
    out = orc.route_multi(vals, types, 8, isnull=nulls)
    want = orc.lib.orc_jump_consistent_hash(0, 8)
    assert (out == want).all()


def test_cdbhash_multi_boundary_values():
    """Boundary attributes through the rotate-combine chain: INT32_MIN/MAX
    as int4, INT64_MIN/MAX as int8, zeros, sign boundaries — vs the
    independent restatement."""
    cases = [
        ([0], [0]), ([0], [1]),
        ([-1], [0]), ([-1], [1]),
        ([2**31 - 1], [1]), ([-2**31], [1]),
        ([2**63 - 1], [0]), ([-2**63], [0]),
        ([2**31, -2**31], [0, 1]),
        ([2**63 - 1, -2**63, 0], [0, 0, 1]),
        ([-2**31, 2**31 - 1, -1, 0, 1], [1, 1, 0, 1, 0]),
    ]
    for vals, types in cases:
        v = np.array(vals, np.int64)
        t = np.array(types, np.int32)
        want = _py_cdbhash_multi(v, t)
        got = orc.cdbhash_multi(v, t)
        assert got == want, (vals, types)
        # and the reduce step at several segment counts
        for nsegs in (2, 3, 8, 17, 64):
            r = orc.route_multi(v.reshape(1, -1), t, nsegs)[0]
            assert 0 <= r < nsegs

"""Primary-filter literals at and beyond the column type's range.

A gx_filter literal is an int64 whatever the column width and the reference
evaluates the cross-type operator (int48lt etc.) exactly: `int8col < 300` is
true for every row.  The kernels compare in the column type, so the host
must fold such quals before narrowing the literal; these tests pin that
against numpy on the int64-widened column, on negative int8 values, the
int32 extremes and +-2^62, through gx_scan_filter and every primary Q3
filter role (local, forced-Motion and RLE-fact-key kernels)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

OPS = ["<", ">", "==", "!=", "<=", ">="]
I8, I32, I64 = np.iinfo(np.int8), np.iinfo(np.int32), np.iinfo(np.int64)


def np_cmp(v, op, lit):
    """numpy on the int64-widened column; lit is a Python int within int64."""
    v = v.astype(np.int64)
    lit = np.int64(lit)
    return {"<": v < lit, ">": v > lit, "==": v == lit, "!=": v != lit,
            "<=": v <= lit, ">=": v >= lit}[op]


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


def edge_column(rng, dtype, n, extra):
    """Full-range values, a cluster near zero, and the planted edges."""
    ii = np.iinfo(dtype)
    v = rng.integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
    v[: n // 3] = rng.integers(-400 if ii.min < -400 else ii.min,
                               400 if ii.max > 400 else ii.max, n // 3)
    rng.shuffle(v)
    plant = np.array([ii.min, ii.max, ii.min + 1, ii.max - 1, 0, -1, 1] + extra)
    pos = rng.choice(n, len(plant), replace=False)
    pos[0], pos[1] = 0, n - 1              # extremes in the first and last block
    v[pos] = plant.astype(dtype)
    return v


# literals whose low bits alias an in-range value: 300 -> 44, -300 -> -44,
# 2^32+5 -> 5, 3e9 -> -1294967296, 2^31 -> INT32_MIN, -2^31-1 -> INT32_MAX
LITS = {
    1: [I8.min, I8.max, I8.min - 1, I8.max + 1, I8.min + 1, I8.max - 1,
        300, -300, 256, -256, 44, -44, 0, 2**31, 2**32 + 5, -2**62],
    4: [I32.min, I32.max, I32.min - 1, I32.max + 1, I32.min + 1, I32.max - 1,
        2**31, -2**31 - 1, 3 * 10**9, -3 * 10**9, 2**32 + 5, 5,
        -1294967296, 0, 2**62, I64.min],
    8: [I64.min, I64.max, I64.min + 1, I64.max - 1, 2**62, -2**62,
        2**62 + 1, -2**62 - 1, 0],
}


@pytest.fixture(scope="module")
def scan_table(ctx, orc):
    """8 KiB blocks: 9000 rows cross a block boundary in every column
    (8151 / 2037 / 1018 rows per block)."""
    rng = np.random.default_rng(71)
    n, bs = 9000, 8192
    cols = [edge_column(rng, np.int8, n, [44, -44]),
            edge_column(rng, np.int32, n, [5, -1294967296]),
            edge_column(rng, np.int64, n, [2**62, -2**62, 2**62 + 1, -2**62 - 1])]
    for c in cols:
        assert n > orc.lib.orc_aocs_rows_per_block(c.itemsize, bs)
    t = ctx.bind([(orc.aocs_encode(c, bs), c.itemsize, n, 0, 0, bs) for c in cols])
    yield t, cols
    t.free()


@pytest.mark.parametrize("col", [0, 1, 2], ids=["i8", "i32", "i64"])
def test_scan_filter_edge_literals(scan_table, col):
    t, cols = scan_table
    v = cols[col]
    bad = []
    for lit in LITS[v.itemsize]:
        for op in OPS:
            got, _ = t.scan_filter(col, op, lit)
            want = int(np_cmp(v, op, lit).sum())
            if got != want:
                bad.append((op, lit, got, want))
    assert not bad, f"(op, literal, got, want): {bad}"


def test_scan_filter_edge_literals_with_visimap(scan_table):
    t, cols = scan_table
    hidden = np.random.default_rng(73).random(len(cols[0])) < 0.3
    t.set_visimap(hidden)
    try:
        for col, lit in ((0, 300), (0, -129), (1, 3 * 10**9), (1, -2**31 - 1)):
            for op in OPS:
                got, _ = t.scan_filter(col, op, lit)
                want = int((np_cmp(cols[col], op, lit) & ~hidden).sum())
                assert got == want, (col, op, lit)
    finally:
        t.set_visimap(None)


def test_scan_filter_rejects_bad_op(scan_table):
    t, _ = scan_table
    for op in (6, -1, 7):
        with pytest.raises(gx.GxError) as ei:
            t.scan_filter(0, op, 0)
        assert ei.value.status == 3          # GX_ERR_INVALID


# ---------------------------------------------------------------------------
# Q3 descriptor: the three primary filters
# ---------------------------------------------------------------------------

class Q3Tables:
    def __init__(self, ctx, orc, rle_fact_key=False):
        rng = np.random.default_rng(79)
        nc, no, nl = 17000, 9000, 20000      # i8 / i32 columns cross a block
        self.c_keys = np.arange(1, nc + 1, dtype=np.int64)
        self.c_seg = edge_column(rng, np.int8, nc, [44, -44])
        self.o_keys = np.arange(1, no + 1, dtype=np.int64)
        self.o_cust = rng.integers(1, nc + 1, no).astype(np.int64)
        self.o_date = edge_column(rng, np.int32, no, [5, -1294967296])
        self.o_prio = rng.integers(0, 5, no).astype(np.int32)
        self.li_keys = np.sort(rng.integers(1, no + 1, nl)).astype(np.int64)
        self.price = rng.uniform(1, 50, nl)
        self.disc = rng.integers(0, 11, nl) / 100.0
        self.ship = edge_column(rng, np.int32, nl, [5, 1294967296])
        assert nc > orc.lib.orc_aocs_rows_per_block(1, 32768)
        assert no > orc.lib.orc_aocs_rows_per_block(4, 32768)
        enc = orc.aocs_encode
        self.cust = ctx.bind([(enc(self.c_keys), 8, nc), (enc(self.c_seg), 1, nc)])
        self.ordr = ctx.bind([(enc(self.o_keys), 8, no), (enc(self.o_cust), 8, no),
                              (enc(self.o_date), 4, no), (enc(self.o_prio), 4, no)])
        key = ((orc.aocs_encode_rle(self.li_keys), 8, nl, 1) if rle_fact_key
               else (enc(self.li_keys), 8, nl))
        self.li = ctx.bind([key, (enc(self.price), 8, nl), (enc(self.disc), 8, nl),
                            (enc(self.ship), 4, nl)])

    def free(self):
        self.li.free(); self.ordr.free(); self.cust.free()

    def desc(self, dim_f, mid_f, fact_f):
        return {"dim": self.cust, "dim_key_col": 0, "dim_filter": (1,) + dim_f,
                "mid": self.ordr, "mid_key_col": 0, "mid_fk_col": 1,
                "mid_attr1_col": 2, "mid_attr2_col": 3,
                "mid_filter": (2,) + mid_f,
                "fact": self.li, "fact_key_col": 0, "fact_a_col": 1,
                "fact_b_col": 2, "fact_filter": (3,) + fact_f}

    def expect(self, dim_f, mid_f, fact_f):
        """the numpy evaluation test_q3_desc_fuzz uses"""
        segok = self.c_keys[np_cmp(self.c_seg, *dim_f)]
        om = np_cmp(self.o_date, *mid_f) & np.isin(self.o_cust, segok)
        lm = np_cmp(self.ship, *fact_f) & np.isin(self.li_keys, self.o_keys[om])
        keys, inv, counts = np.unique(self.li_keys[lm], return_inverse=True,
                                      return_counts=True)
        rev = np.zeros(len(keys))
        np.add.at(rev, inv, self.price[lm] * (1.0 - self.disc[lm]))
        return keys, counts, rev

    def check(self, ctx, dim_f, mid_f, fact_f, tag=""):
        got = ctx.q3_desc(self.desc(dim_f, mid_f, fact_f)).run().result()
        keys, counts, rev = self.expect(dim_f, mid_f, fact_f)
        msg = f"{tag} dim{dim_f} mid{mid_f} fact{fact_f}"
        np.testing.assert_array_equal(got["l_orderkey"], keys, err_msg=msg)
        np.testing.assert_array_equal(got["nitems"], counts, err_msg=msg)
        # positive terms, n <= 20 per group: (n+2)*2^-52 < 5e-15 covers any
        # summation order plus the two roundings of p*(1-d)
        np.testing.assert_allclose(got["revenue"], rev, rtol=1e-13, err_msg=msg)
        return len(keys)


@pytest.fixture(scope="module")
def q3t(ctx, orc):
    t = Q3Tables(ctx, orc)
    yield t
    t.free()


# neutral (in-range, selective) filters for the roles not under test
NEUTRAL = {"dim": ("<", 64), "mid": ("<", 200), "fact": (">", -200)}

# (op, literal, kind): T always true, F always false, B boundary (in range)
DIM_CASES = [("<", 300, "T"), (">", 300, "F"), ("==", 300, "F"),
             ("!=", -300, "T"), ("<=", -300, "F"), (">=", -300, "T"),
             (">=", 128, "F"), ("<", 128, "T"), (">", -129, "T"),
             ("<=", -129, "F"), ("==", 2**32 + 44, "F"),
             ("<=", 127, "B"), ("<", -128, "B"), ("==", -128, "B"),
             (">", 126, "B"), ("!=", 127, "B"), (">=", -127, "B")]
I32_CASES = [("<", 3 * 10**9, "T"), (">", 3 * 10**9, "F"),
             ("==", 2**32 + 5, "F"), ("!=", 2**32 + 5, "T"),
             ("<=", -2**31 - 1, "F"), (">=", -2**31 - 1, "T"),
             (">=", 2**31, "F"), ("<", 2**31, "T"), (">", -3 * 10**9, "T"),
             ("<=", -3 * 10**9, "F"),
             ("<=", I32.max, "B"), ("<", I32.min, "B"), ("==", I32.min, "B"),
             (">", I32.max - 1, "B"), ("!=", I32.max, "B"),
             (">=", I32.min + 1, "B")]
ROLE_CASES = ([("dim",) + c for c in DIM_CASES] +
              [("mid",) + c for c in I32_CASES] +
              [("fact",) + c for c in I32_CASES])


def test_role_cases_cover_every_op_and_kind():
    for role in ("dim", "mid", "fact"):
        mine = [c for c in ROLE_CASES if c[0] == role]
        assert {c[1] for c in mine} == set(OPS)
        assert {c[3] for c in mine} == {"T", "F", "B"}


@pytest.mark.parametrize("role,op,lit,kind", ROLE_CASES,
                         ids=[f"{r}{o}{l}" for r, o, l, _ in ROLE_CASES])
def test_q3_primary_filter_edge_literals(ctx, q3t, role, op, lit, kind):
    f = dict(NEUTRAL)
    f[role] = (op, lit)
    ngroups = q3t.check(ctx, f["dim"], f["mid"], f["fact"])
    col = {"dim": q3t.c_seg, "mid": q3t.o_date, "fact": q3t.ship}[role]
    m = np_cmp(col, op, lit)
    if kind == "T":
        assert m.all() and ngroups > 0
    elif kind == "F":
        assert not m.any() and ngroups == 0
    else:
        assert I8.min <= lit <= I8.max or I32.min <= lit <= I32.max


# every role out of range at once, each literal aliasing a selective in-range
# value when truncated (!= 44, < -1294967296, > 1294967296)
ALL_OUT = (("!=", 300), ("<", 3 * 10**9), (">", -3 * 10**9))


def test_q3_edge_literals_forced_motion(ctx, q3t):
    """the Motion kernels (k_ord_m1_hist, k_ord_m1_emit) take the same folded
    literals"""
    try:
        ctx.comm_init(ctx.comm_unique_id())
    except gx.GxError:
        pass    # communicator may already exist
    os.environ["GX_FORCE_MOTION"] = "1"
    try:
        assert q3t.check(ctx, *ALL_OUT, tag="motion") > 0
        assert q3t.check(ctx, ("<", 64), ("<=", I32.max), (">=", -2**31 - 1),
                         tag="motion") > 0
    finally:
        del os.environ["GX_FORCE_MOTION"]


def test_q3_edge_literals_rle_fact_key(ctx, orc):
    """the fused RLE fact-key probe kernel"""
    t = Q3Tables(ctx, orc, rle_fact_key=True)
    try:
        assert t.check(ctx, *ALL_OUT, tag="rle") > 0
        assert t.check(ctx, ("<", 64), ("<", 200), (">=", -2**31 - 1), tag="rle") > 0
        assert t.check(ctx, ("<", 64), ("<", 200), (">=", 2**31), tag="rle") == 0
    finally:
        t.free()


@pytest.mark.parametrize("role", ["dim", "mid", "fact"])
@pytest.mark.parametrize("op", [6, -1])
def test_q3_primary_filter_op_validated(ctx, q3t, role, op):
    f = dict(NEUTRAL)
    f[role] = (op, 0)
    with pytest.raises(gx.GxError) as ei:
        ctx.q3_desc(q3t.desc(f["dim"], f["mid"], f["fact"]))
    assert ei.value.status == 3              # GX_ERR_INVALID at prepare

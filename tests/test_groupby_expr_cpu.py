"""CPU-side checks of the descriptor GROUP BY's float8 expressions and float8
quals (gx_groupby_expr): the ctypes mirrors match the C structs, and the host
restatements of the expression value and of the float8 comparison, which run
through the same functions the scan kernel calls, agree with numpy's IEEE
doubles and with a Python restatement of float8_cmp_internal."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(ROOT, "cloudberry_amd", "libgpuexec.so")


@pytest.fixture(scope="module")
def gx():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()
    import cloudberry_amd
    return cloudberry_amd


def test_groupby_expr_symbols_exported(gx):
    lib = gx.lib()
    for n in ("gx_groupby_expr", "gx_groupby_expr_dist", "gx_test_groupby_expr",
              "gx_selftest_expr_eval", "gx_selftest_fqual"):
        assert hasattr(lib, n), f"symbol {n} not exported"


def test_gb_ext_ctypes_sizes_match_c(gx):
    lib = gx.lib()
    lib.gx_abi_sizeof.restype = ctypes.c_int64
    lib.gx_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.gx_abi_sizeof(13) == ctypes.sizeof(gx._GbExt)
    assert lib.gx_abi_sizeof(14) == ctypes.sizeof(gx._Expr) == 8 + 3 * 8
    assert lib.gx_abi_sizeof(15) == ctypes.sizeof(gx._FQual) == 16
    assert ctypes.sizeof(gx._Factor) == 8
    # 2 i32 + 8 exprs + 8 i32 + 4 fquals
    assert ctypes.sizeof(gx._GbExt) == 8 + 8 * 32 + 32 + 4 * 16
    # the kinds before it keep their meaning; 12 stays unknown
    assert lib.gx_abi_sizeof(12) == -1
    assert lib.gx_abi_sizeof(8) == ctypes.sizeof(gx._GbDesc) == 240
    assert lib.gx_abi_sizeof(10) == ctypes.sizeof(gx._Agg) == 16
    assert (gx.GB_MAX_FACTORS, gx.GB_MAX_FQUALS, gx.GB_MAX_OPERANDS) == (3, 4, 8)


# ---------------- gx_selftest_expr_eval ----------------

def _doubles(rng, n):
    """n doubles over the whole format: random bit patterns (full mantissas,
    every exponent, NaNs among them), moderate values whose products stay
    finite, subnormals, and the special values"""
    bits = rng.integers(0, 2**64, n, dtype=np.uint64)
    v = bits.view(np.float64).copy()
    third = n // 3
    v[:third] = rng.standard_normal(third) * 10.0 ** rng.integers(-3, 4, third)
    sub = rng.integers(1, 2**52, n // 20, dtype=np.uint64).view(np.float64)
    v[third:third + len(sub)] = sub * rng.choice([-1.0, 1.0], len(sub))
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324,
                        1.0, -1.0, 2.2250738585072014e-308,
                        1.7976931348623157e308])
    v[-len(special):] = special
    rng.shuffle(v)
    return v


def _np_factor(c, form):
    return {"": c, "1-": 1.0 - c, "1+": 1.0 + c}[form]


FORMS = ["", "1-", "1+"]
SHAPES = ([[f] for f in FORMS] +
          [[f, g] for f in FORMS for g in FORMS] +
          [["", "1-", "1+"], ["1+", "", "1-"], ["1-", "1-", "1-"],
           ["", "", ""], ["1+", "1+", ""]])


@pytest.mark.parametrize("forms", SHAPES, ids=lambda f: "*".join(x or "c" for x in f))
def test_expr_eval_is_bit_equal_to_numpy(gx, forms):
    rng = np.random.default_rng(len(forms) * 100 + sum(FORMS.index(f) for f in forms))
    n = 10000
    vals = np.stack([_doubles(rng, n) for _ in range(4)], axis=1)
    for special in (0.0, -0.0, np.inf, -np.inf, 5e-324):
        assert (vals.view(np.uint64) == np.float64(special).view(np.uint64)).any()
    assert np.isnan(vals).any()
    isnull = rng.random(vals.shape) < 0.1
    cols = [3, 0, 2][:len(forms)]              # not the identity mapping
    factors = [c if f == "" else (f, c) for f, c in zip(forms, cols)]
    got, got_null = gx.selftest_expr_eval(factors, vals, isnull)
    with np.errstate(all="ignore"):
        want = _np_factor(vals[:, cols[0]], forms[0])
        for f, c in zip(forms[1:], cols[1:]):
            want = want * _np_factor(vals[:, c], f)   # ((f0 * f1) * f2)
    want_null = isnull[:, cols].any(axis=1)
    np.testing.assert_array_equal(got_null, want_null)
    ok = ~want_null
    gb, wb = got[ok].view(np.uint64), want[ok].view(np.uint64)
    nan = np.isnan(want[ok])
    np.testing.assert_array_equal(np.isnan(got[ok]), nan)
    np.testing.assert_array_equal(gb[~nan], wb[~nan])          # bit for bit
    assert (got[want_null] == 0).all()
    # no NULL array: nothing is NULL
    got2, null2 = gx.selftest_expr_eval(factors, vals)
    assert not null2.any()
    np.testing.assert_array_equal(got2[ok].view(np.uint64)[~nan], wb[~nan])


def test_expr_eval_the_q1_expression(gx):
    vals = np.array([[100.25, 0.25, 0.125], [3.0, 0.0, 0.5]])
    got, nl = gx.selftest_expr_eval([0, ("1-", 1), ("1+", 2)], vals)
    assert got.tolist() == [(100.25 * (1 - 0.25)) * (1 + 0.125), 3.0 * 1.5]
    assert not nl.any()


def test_expr_eval_rejects_bad_arguments(gx):
    vals = np.zeros((4, 2))
    for factors in ([], [0, 0, 0, 0], [(3, 0)], [(-1, 0)], [2], [-1], [0, ("1-", 2)]):
        with pytest.raises(ValueError, match=r"bad arguments \(1\)"):
            gx.selftest_expr_eval(factors, vals)
    got, _ = gx.selftest_expr_eval([(2, 1)], vals)     # raw form code 2 = 1 + c
    assert got.tolist() == [1.0] * 4


# ---------------- gx_selftest_fqual ----------------

def _float8_cmp_internal(a, b):
    """float.c: NaNs are equal to each other and greater than everything"""
    if np.isnan(a):
        return 0 if np.isnan(b) else 1
    if np.isnan(b):
        return -1
    if a > b:
        return 1
    if a < b:
        return -1
    return 0


_CMP_OPS = {"<": lambda c: c < 0, ">": lambda c: c > 0, "==": lambda c: c == 0,
            "!=": lambda c: c != 0, "<=": lambda c: c <= 0, ">=": lambda c: c >= 0}
GRID = [-np.inf, -1.5, -0.0, 0.0, 2.25, np.inf, np.nan]


@pytest.mark.parametrize("op", list(_CMP_OPS))
def test_fqual_matches_float8_cmp_internal(gx, op):
    for x in GRID:
        for lit in GRID:
            want = int(_CMP_OPS[op](_float8_cmp_internal(x, lit)))
            assert gx.selftest_fqual(op, x, lit) == want, (op, x, lit)


def test_fqual_named_edges(gx):
    nan, inf = np.nan, np.inf
    neg_nan = np.array([0xFFF8000000000001], np.uint64).view(np.float64)[0]
    assert gx.selftest_fqual("==", -0.0, 0.0) == 1
    assert gx.selftest_fqual("==", 0.0, -0.0) == 1
    assert gx.selftest_fqual("<", -0.0, 0.0) == 0
    assert gx.selftest_fqual("==", nan, nan) == 1
    assert gx.selftest_fqual("==", neg_nan, nan) == 1
    assert gx.selftest_fqual(">", nan, inf) == 1
    assert gx.selftest_fqual(">", neg_nan, inf) == 1
    for x in GRID[:-1]:
        assert gx.selftest_fqual("<", x, nan) == 1
        assert gx.selftest_fqual(">=", x, nan) == 0
    assert gx.selftest_fqual("<", 5e-324, 1e-323) == 1
    assert gx.selftest_fqual("<", -1e-323, -5e-324) == 1
    assert gx.selftest_fqual(6, 1.0, 1.0) == -1
    assert gx.selftest_fqual(-1, 1.0, 1.0) == -1

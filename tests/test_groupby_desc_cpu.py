"""CPU-side checks of the descriptor-form GROUP BY (gx_groupby_desc): the
ctypes mirrors match the C structs, the host-side result ordering agrees with
numpy, and the exported LDS capacity behaves as the GPU tests assume."""
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


def test_groupby_desc_symbols_exported(gx):
    lib = gx.lib()
    for n in ("gx_groupby_desc", "gx_gb_result_free", "gx_gb_lds_groups",
              "gx_test_groupby_desc", "gx_selftest_gb_sort"):
        assert hasattr(lib, n), f"symbol {n} not exported"


def test_gb_desc_ctypes_sizes_match_c(gx):
    lib = gx.lib()
    lib.gx_abi_sizeof.restype = ctypes.c_int64
    lib.gx_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.gx_abi_sizeof(8) == ctypes.sizeof(gx._GbDesc)
    assert lib.gx_abi_sizeof(9) == ctypes.sizeof(gx._GbResult) == 48
    assert lib.gx_abi_sizeof(10) == ctypes.sizeof(gx._Agg) == 16
    assert lib.gx_abi_sizeof(11) == ctypes.sizeof(gx._GbdStats) == 48
    # 8 t + (1 + 4) i32 + 1 i32 + 8 aggs + nquals (+ pad) + 4 filters + i64
    assert ctypes.sizeof(gx._GbDesc) == 8 + 20 + 4 + 8 * 16 + 8 + 4 * 16 + 8
    assert lib.gx_abi_sizeof(12) == -1


def _lexsort_nulls_last(keys, key_null):
    """numpy's order over (key_null, key) pairs, first column most significant;
    lexsort is stable and takes its LAST key as the primary one."""
    cols = []
    for k in range(keys.shape[1] - 1, -1, -1):
        cols.append(keys[:, k])
        cols.append(key_null[:, k])
    return np.lexsort(cols)


@pytest.mark.parametrize("nkeys", [1, 2, 3, 4])
def test_gb_sort_matches_lexsort(gx, nkeys):
    rng = np.random.default_rng(100 + nkeys)
    n = 3000
    # few distinct values: many ties in the leading columns and duplicate rows
    keys = rng.integers(-3, 4, (n, nkeys)).astype(np.int64)
    keys[rng.random((n, nkeys)) < 0.05] = -2**63
    keys[rng.random((n, nkeys)) < 0.05] = 2**63 - 1
    key_null = (rng.random((n, nkeys)) < 0.15).astype(np.uint8)
    keys[key_null == 1] = 0                     # as the executor returns them
    assert len(np.unique(np.concatenate([keys, key_null], axis=1), axis=0)) < n
    perm = gx.gb_sort(keys, key_null)
    np.testing.assert_array_equal(perm, _lexsort_nulls_last(keys, key_null))
    # NULLS LAST in the leading column
    lead = key_null[perm, 0]
    assert (np.diff(lead.astype(np.int8)) >= 0).all()


def test_gb_sort_all_null_column_and_edges(gx):
    rng = np.random.default_rng(7)
    n = 500
    keys = rng.integers(-5, 6, (n, 3)).astype(np.int64)
    key_null = np.zeros((n, 3), np.uint8)
    key_null[:, 1] = 1                          # an all-NULL column
    keys[:, 1] = 0
    perm = gx.gb_sort(keys, key_null)
    np.testing.assert_array_equal(perm, _lexsort_nulls_last(keys, key_null))
    # no rows; and bad arguments are refused, not crashed on
    assert len(gx.gb_sort(np.zeros((0, 2), np.int64), np.zeros((0, 2), np.uint8))) == 0
    lib = gx.lib()
    out = np.zeros(4, np.int64)
    assert lib.gx_selftest_gb_sort(None, None, 4, 1, out.ctypes.data) == 1
    assert lib.gx_selftest_gb_sort(None, None, 0, 5, out.ctypes.data) == 1
    assert lib.gx_selftest_gb_sort(None, None, 0, 0, out.ctypes.data) == 1


def test_gb_lds_groups_positive_and_non_increasing(gx):
    caps = [gx.gb_lds_groups(n) for n in range(1, 9)]
    assert all(c > 0 for c in caps)
    assert all(a >= b for a, b in zip(caps, caps[1:]))
    # the worst slot (two words per aggregate, an 8-byte row word) of a full
    # table leaves room for at least two workgroups on a 160-KiB CU
    for n, c in zip(range(1, 9), caps):
        assert c * (16 * n + 8) * 2 <= 160 * 1024
    assert gx.gb_lds_groups(0) == 0 and gx.gb_lds_groups(9) == 0

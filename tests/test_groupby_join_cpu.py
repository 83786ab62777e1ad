"""CPU-side checks of the descriptor GROUP BY over a join (gx_groupby_join):
the ctypes mirrors match the C structs, and the host restatement of the join
table, a serial build and probe through the hash, slot and compare functions
the kernels call, agrees with a Python dict join."""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(ROOT, "cloudberry_amd", "libgpuexec.so")

INT64_MIN, INT64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module")
def gx():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()
    import cloudberry_amd
    return cloudberry_amd


def test_groupby_join_symbols_exported(gx):
    lib = gx.lib()
    for n in ("gx_groupby_join", "gx_groupby_join_dist", "gx_test_groupby_join",
              "gx_test_gbj_partial", "gx_selftest_gbj_join",
              "gx_selftest_gbj_slots"):
        assert hasattr(lib, n), f"symbol {n} not exported"


def test_gbj_ctypes_sizes_match_c(gx):
    lib = gx.lib()
    lib.gx_abi_sizeof.restype = ctypes.c_int64
    lib.gx_abi_sizeof.argtypes = [ctypes.c_int]
    # pointer + 4 i32 + 4 filters of 16 bytes
    assert lib.gx_abi_sizeof(16) == ctypes.sizeof(gx._GbJoin) == 8 + 16 + 4 * 16
    # 2 i32 + 2 joins + 4 i32 + 8 i32
    assert lib.gx_abi_sizeof(17) == ctypes.sizeof(gx._GbjExt) == 8 + 2 * 88 + 16 + 32
    # 2 doubles + 6 i64 + 2 i64
    assert lib.gx_abi_sizeof(18) == ctypes.sizeof(gx._GbjStats) == 80
    assert gx.GBJ_MAX_JOINS == 2
    # the kinds before them keep their meaning; 12 stays unknown
    assert lib.gx_abi_sizeof(12) == -1
    assert lib.gx_abi_sizeof(19) == -1
    assert lib.gx_abi_sizeof(8) == ctypes.sizeof(gx._GbDesc) == 240
    assert lib.gx_abi_sizeof(13) == ctypes.sizeof(gx._GbExt)
    assert lib.gx_abi_sizeof(11) == ctypes.sizeof(gx._GbdStats) == 48


# ---------------- gx_selftest_gbj_join ----------------

def _dict_join(dim_keys, fact_keys, dim_null=None, fact_null=None):
    table = {}
    for r, k in enumerate(dim_keys):
        if dim_null is None or not dim_null[r]:
            assert int(k) not in table
            table[int(k)] = r
    return np.array([-1 if (fact_null is not None and fact_null[i])
                     else table.get(int(k), -1)
                     for i, k in enumerate(fact_keys)], np.int64)


def test_join_key_edges(gx):
    """0, -1, both extremes, multiples of 2^32 and keys that differ only above
    bit 32 are all distinct keys, each found at its own row"""
    dim = np.array([0, -1, INT64_MIN, INT64_MAX, 2**32, 2 * 2**32, -2**32,
                    5, 5 + 2**32, 5 + 2**33, 5 - 2**32, 2**63 - 2**32, 1, 2**31,
                    -2**31], np.int64)
    assert len(set(dim.tolist())) == len(dim)
    assert len(set((dim & 0xFFFFFFFF).tolist())) < len(dim)     # low words repeat
    miss = np.array([2, -2, INT64_MIN + 1, INT64_MAX - 1, 3 * 2**32, 5 + 2**34,
                     2**32 - 1], np.int64)
    assert not set(miss.tolist()) & set(dim.tolist())
    fact = np.concatenate([dim[::-1], miss, dim])
    rows, dup = gx.selftest_gbj_join(dim, fact)
    assert dup is None
    want = _dict_join(dim, fact)
    np.testing.assert_array_equal(rows, want)
    assert (want >= 0).sum() == 2 * len(dim) and (want < 0).sum() == len(miss)


def test_join_random_and_nulls(gx):
    rng = np.random.default_rng(1601)
    nd, nf = 5000, 20000
    dim = rng.permutation(np.arange(-4000, 4000, dtype=np.int64))[:nd] * 7919
    dim_null = rng.random(nd) < 0.1
    fact = rng.integers(-4100, 4100, nf).astype(np.int64) * 7919
    fact_null = rng.random(nf) < 0.1
    # a NULL dimension key whose value a fact row carries is still no match,
    # and a NULL fact key whose value the dimension holds matches nothing
    live = set(dim[~dim_null].tolist())
    dead = set(dim[dim_null].tolist()) - live
    assert any(int(k) in dead for k in fact[~fact_null])
    assert any(int(k) in live for k in fact[fact_null])
    rows, dup = gx.selftest_gbj_join(dim, fact, dim_null, fact_null)
    assert dup is None
    want = _dict_join(dim, fact, dim_null, fact_null)
    np.testing.assert_array_equal(rows, want)
    assert (want >= 0).any() and (want[~fact_null] < 0).any()
    assert (rows[fact_null] == -1).all()
    assert not dim_null[rows[rows >= 0]].any()
    # the Context method is the same function
    ctx_rows, _ = gx.Context.selftest_gbj_join(None, dim, fact, dim_null, fact_null)
    np.testing.assert_array_equal(ctx_rows, want)
    # no NULL arrays, empty sides
    rows, _ = gx.selftest_gbj_join(dim[~dim_null], fact)
    np.testing.assert_array_equal(rows, _dict_join(dim[~dim_null], fact))
    rows, dup = gx.selftest_gbj_join(np.zeros(0, np.int64), fact[:10])
    assert dup is None and (rows == -1).all()
    rows, dup = gx.selftest_gbj_join(dim[~dim_null], np.zeros(0, np.int64))
    assert dup is None and len(rows) == 0


def test_join_full_collision(gx):
    """3000 keys that all hash to ONE home slot of the minimal table (8192
    slots for 3000 rows): every insert and every probe walks the whole run"""
    nd = 3000
    keys, home = [], None
    for base in range(0, 64 * 2**20, 2**20):
        cand = np.arange(base, base + 2**20, dtype=np.int64) * 2654435761 - 2**40
        slot, nslots = gx.selftest_gbj_slots(cand, nd)
        assert nslots == 8192 and slot.max() < nslots
        if home is None:
            home = int(slot[0])
        keys.extend(cand[slot == home].tolist())
        if len(keys) >= nd + 50:
            break
    assert len(keys) >= nd + 50
    keys = np.array(keys, np.int64)
    assert len(np.unique(keys)) == len(keys)
    slot, _ = gx.selftest_gbj_slots(keys, nd)
    assert (slot == home).all()                     # really one home slot
    dim, miss = keys[:nd], keys[nd:]                # the misses walk the run too
    fact = np.concatenate([dim[::-1], miss])
    rows, dup = gx.selftest_gbj_join(dim, fact)
    assert dup is None
    np.testing.assert_array_equal(rows, _dict_join(dim, fact))
    assert (rows[:nd] == np.arange(nd)[::-1]).all() and (rows[nd:] == -1).all()


def test_join_duplicate_report(gx):
    rng = np.random.default_rng(1602)
    dim = rng.permutation(20000)[:4000].astype(np.int64) - 10000
    fact = dim[:100]
    bad = dim.copy()
    bad[3777] = bad[12]                             # one duplicated key
    rows, dup = gx.selftest_gbj_join(bad, fact)
    assert rows is None and dup == bad[12]
    # INT64_MIN and 0 are reported like any other key
    for k in (INT64_MIN, 0):
        rows, dup = gx.selftest_gbj_join(np.array([7, k, 9, k], np.int64), fact)
        assert rows is None and dup == k
    # a duplicate under a NULL flag takes no part: legal
    dn = np.zeros(len(bad), np.uint8)
    dn[3777] = 1
    rows, dup = gx.selftest_gbj_join(bad, fact, dn)
    assert dup is None
    np.testing.assert_array_equal(rows, _dict_join(bad, fact, dn))
    # two NULL keys with equal values are no duplicate either
    dn[12] = 1
    rows, dup = gx.selftest_gbj_join(bad, fact, dn)
    assert dup is None and rows[12] == -1


def test_join_bad_arguments(gx):
    lib = gx.lib()
    k = np.arange(4, dtype=np.int64)
    out = np.zeros(4, np.int64)
    dup = ctypes.c_int64()
    good = (k.ctypes.data, None, 4, k.ctypes.data, None, 4, out.ctypes.data,
            ctypes.byref(dup))
    assert lib.gx_selftest_gbj_join(*good) == 0

    def bent(i, v):
        a = list(good)
        a[i] = v
        return lib.gx_selftest_gbj_join(*a)
    assert bent(2, -1) == -1                        # negative counts
    assert bent(5, -1) == -1
    assert bent(0, None) == -1                      # missing arrays
    assert bent(3, None) == -1
    assert bent(6, None) == -1
    assert bent(7, None) == -1
    assert bent(2, 2**32 - 1) == -1                 # rows past the u32 slot word
    with pytest.raises(ValueError):
        gx.selftest_gbj_slots(k, -1)
    with pytest.raises(ValueError):
        gx.selftest_gbj_slots(k, 2**32 - 1)

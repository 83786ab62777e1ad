"""CPU checks of the two pure host helpers of the multi-segment Q3 path, run
through the no-GPU symbol gx_selftest_motion_layout: the send/receive
bookkeeping over the all-gathered n×n count matrix, and the layout of the
join table built from received rows.  The same helpers are what gx_q3_run
calls at nsegs > 1."""
import ctypes

import numpy as np
import pytest

import cloudberry_amd as gx


def _want_layout(c, seg):
    n = c.shape[0]
    scnt, rcnt = c[seg, :], c[:, seg]
    soff = np.concatenate([[0], np.cumsum(scnt)]).astype(np.uint64)
    roff = np.concatenate([[0], np.cumsum(rcnt)]).astype(np.uint64)
    assert len(soff) == n + 1
    return scnt, soff, rcnt, roff


def _check_every_seg(c):
    for seg in range(c.shape[0]):
        got = gx.motion_exchange_layout(c, seg)
        for g, w in zip(got, _want_layout(c, seg)):
            np.testing.assert_array_equal(g, w)


@pytest.mark.parametrize("n", range(1, 17))
def test_exchange_layout_random_matrix(n):
    rng = np.random.default_rng(100 + n)
    # asymmetric on purpose: row and column sums differ, so a transposed
    # index (cnts_all[i*n + seg] for the send side) cannot pass
    c = rng.integers(0, 1 << 33, (n, n)).astype(np.uint64)
    if n > 1:
        assert not (c == c.T).all()
    _check_every_seg(c)


@pytest.mark.parametrize("n", [1, 2, 3, 8, 16])
def test_exchange_layout_zero_rows_and_columns(n):
    rng = np.random.default_rng(200 + n)
    base = rng.integers(1, 1000, (n, n)).astype(np.uint64)
    _check_every_seg(np.zeros((n, n), np.uint64))
    for k in sorted({0, n // 2, n - 1}):
        c = base.copy()
        c[k, :] = 0                 # rank k sends nothing
        _check_every_seg(c)
        c = base.copy()
        c[:, k] = 0                 # rank k receives nothing
        _check_every_seg(c)
        c = base.copy()
        c[k, :] = 0
        c[:, (k + 1) % n] = 0
        _check_every_seg(c)


def test_exchange_layout_rejects_bad_seg():
    c = np.ones((3, 3), np.uint64)
    for seg in (-1, 3):
        with pytest.raises(ValueError):
            gx.motion_exchange_layout(c, seg)


def _is_pow2(v):
    return v > 0 and v & (v - 1) == 0


def _table_cases():
    rng = np.random.default_rng(7)
    cases = [(0, 2**64 - 1, 0), (1, 1, 1), (1, 2**32 - 1, 2**32 - 1),
             (1, 2**32, 2**32), (1000, 1, 1000), (1000, 2**32 - 1000, 2**32 - 1),
             (1000, 2**32 - 500, 2**32 + 499), (5, 1, 2**62)]
    for _ in range(40):
        qual = int(rng.integers(1, 200000))
        kmin = int(rng.integers(1, 2**40))
        span = int(rng.integers(qual, qual * 4096))
        cases.append((qual, kmin, kmin + span - 1))
    return cases


@pytest.mark.parametrize("nsegs", [1, 2, 8, 16])
@pytest.mark.parametrize("tf", [300, 100, 50, 0])
def test_table_layout_properties(nsegs, tf):
    for qual, kmin, kmax in _table_cases():
        lay = gx.motion_table_layout(qual, kmin, kmax, nsegs, tf)
        what = (qual, kmin, kmax, nsegs, tf, lay)
        assert _is_pow2(lay["slots"]) and lay["slots"] > qual, what
        assert lay["slots"] >= qual * tf // 100 + 1, what
        assert lay["key_width"] == (4 if kmax < 2**32 else 8), what
        mask = lay["slots"] - 1
        if qual > 0:
            assert lay["slot_kmin"] <= mask and lay["slot_kmax"] <= mask, what
            assert lay["kmin"] == kmin, what
        else:
            assert lay["scale"] < 0 and lay["interpolated"] == 0, what
        assert lay["interpolated"] == (1 if lay["scale"] >= 0 else 0), what
        if lay["interpolated"]:
            # order preserving: the extreme keys land at the two ends
            assert lay["slot_kmin"] == 0, what
            assert lay["slot_kmin"] <= lay["slot_kmax"], what


def test_table_layout_key_width_edge():
    assert gx.motion_table_layout(10, 1, 2**32 - 1, 2)["key_width"] == 4
    assert gx.motion_table_layout(10, 1, 2**32, 2)["key_width"] == 8


@pytest.mark.parametrize("nsegs", [1, 2, 8])
def test_table_layout_density_rule(nsegs):
    """Interpolated exactly when qual >= range / (64 * nsegs)."""
    qual = 1000
    edge = qual * 64 * nsegs            # the largest range still dense
    lay = gx.motion_table_layout(qual, 5, 5 + edge - 1, nsegs)
    assert lay["interpolated"] == 1 and lay["scale"] == lay["slots"] / edge
    lay = gx.motion_table_layout(qual, 5, 5 + edge, nsegs)
    assert lay["interpolated"] == 0 and lay["scale"] < 0
    assert gx.motion_table_layout(0, 2**64 - 1, 0, nsegs)["scale"] < 0


def test_numpy_mirrors_match_c_structs():
    lib = gx.lib()
    lib.gx_abi_sizeof.restype = ctypes.c_int64
    lib.gx_abi_sizeof.argtypes = [ctypes.c_int]
    assert lib.gx_abi_sizeof(7) == ctypes.sizeof(gx._TblLayout) == 48
    assert lib.gx_abi_sizeof(1) == gx.Q3_GROUP_DTYPE.itemsize
    assert gx.ORD_ROW_DTYPE.itemsize == 24 and gx.QUAL_ROW_DTYPE.itemsize == 16

"""CPU-side checks of the two-stage descriptor GROUP BY (gx_groupby_desc_dist):
the wire-row stride and its numpy mirror, and the owner routing restated on
the host through the same functions the partition kernel calls, held against
the oracle's bit-exact Motion routing."""
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(ROOT, "cloudberry_amd", "libgpuexec.so")

INT64_MIN = -2**63


@pytest.fixture(scope="module")
def gx():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()
    import cloudberry_amd
    return cloudberry_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


def test_dist_symbols_exported(gx):
    lib = gx.lib()
    for n in ("gx_groupby_desc_dist", "gx_gbd_wire_stride", "gx_test_gbd_partial",
              "gx_test_gbd_combine", "gx_selftest_gbd_route"):
        assert hasattr(lib, n), f"symbol {n} not exported"


# ---------------- wire stride ----------------

MINMAX8 = [("min", 0), ("max", 0), ("min", 1, True), ("max", 1, True)] * 2


def test_wire_stride(gx):
    assert gx.gbd_wire_stride([], [("count*", None)]) == 8
    assert gx.gbd_wire_stride([0, 1, 2, 3], MINMAX8) == 168
    assert gx.gbd_wire_stride([0], [("sum", 1, True), ("count*", None)]) == 40
    # COUNT(col) is one word too; is_f64 does not change the word count
    assert gx.gbd_wire_stride([0, 1], [("count", 2), ("sum", 2)]) == 8 * (3 + 3)


def test_wire_stride_rejects_bad_descriptors(gx):
    assert gx.gbd_wire_stride([0], []) == -1                      # naggs = 0
    assert gx.gbd_wire_stride([0] * 5, [("count*", None)]) == -1  # nkeys = 5
    assert gx.gbd_wire_stride([0], [(5, 0)]) == -1                # unknown fn
    assert gx.gbd_wire_stride([0], [(-1, 0)]) == -1
    assert gx.gbd_wire_stride([0], [("count*", None)] * 9) == -1  # naggs = 9
    assert gx.lib().gx_gbd_wire_stride(None) == -1
    with pytest.raises(ValueError):
        gx.gbd_wire_dtype([0], [(5, 0)])


@pytest.mark.parametrize("keys,aggs", [
    ([], [("count*", None)]),
    ([0, 1, 2, 3], MINMAX8),
    ([0], [("sum", 1, True), ("count*", None)]),
    ([2, 0, 1], [("count", 3), ("min", 3)]),
])
def test_wire_dtype_mirrors_the_stride(gx, keys, aggs):
    dt = gx.gbd_wire_dtype(keys, aggs)
    assert dt.itemsize == gx.gbd_wire_stride(keys, aggs)
    assert dt.names[-1] == "acc"
    assert dt.fields["acc"][1] + dt["acc"].itemsize == dt.itemsize
    if keys:
        assert dt.names == ("keys", "key_null", "_pad", "acc")
        assert dt["keys"].shape == (len(keys),)
        assert dt.fields["key_null"][1] == 8 * len(keys)
        assert dt.fields["acc"][1] == 8 * len(keys) + 8
    else:
        assert dt.names == ("acc",)


# ---------------- routing ----------------

WIDTHS = [(8,), (4,), (1, 2), (8, 4, 2, 1)]
NSEGS = [1, 2, 3, 7, 16, 2048]


def _route_input(widths):
    rng = np.random.default_rng(900 + sum(widths) + len(widths))
    n = 2000
    cols = []
    for w in widths:
        lo, hi = -2**(8 * w - 1), 2**(8 * w - 1) - 1
        v = rng.integers(lo, hi, n, dtype=np.int64, endpoint=True)
        v[rng.random(n) < 0.3] //= 2**(8 * w - 4)      # small values as well
        if w == 8:
            v[:4] = [0, INT64_MIN, -1, 2**63 - 1]
        else:
            v[:4] = [lo, -1, 0, hi]
        cols.append(v)
    keys = np.stack(cols, axis=1)
    null = rng.random((n, len(widths))) < 0.15
    null[:4] = False
    null[10:20] = True                                 # NULL in every column
    return keys, null


@pytest.mark.parametrize("widths", WIDTHS)
def test_route_matches_oracle(gx, orc, widths):
    keys, null = _route_input(widths)
    for w, c in zip(widths, range(len(widths))):
        if w < 8:
            assert (keys[:, c] < 0).any()
    assert null.all(axis=1).any() and (keys[~null] == 0).any()
    types = [0 if w == 8 else 1 for w in widths]
    for nsegs in NSEGS:
        got = gx.gbd_route(keys, null, widths, nsegs)
        want = orc.route_multi(np.where(null, 0, keys), types, nsegs, isnull=null)
        np.testing.assert_array_equal(got, want)
        assert got.min() >= 0 and got.max() < nsegs
        if nsegs > 1:
            assert len(np.unique(got)) > 1
    # the value under a NULL never reaches the hash
    junk = np.where(null, 12345, keys)
    np.testing.assert_array_equal(gx.gbd_route(junk, null, widths, 7),
                                  gx.gbd_route(keys, null, widths, 7))


def test_single_wide_column_is_the_plain_route(gx, orc):
    keys, null = _route_input((8,))
    none = np.zeros_like(null)
    for nsegs in NSEGS:
        np.testing.assert_array_equal(gx.gbd_route(keys, none, (8,), nsegs),
                                      orc.route(keys[:, 0], nsegs))


def test_null_and_zero_route_apart(gx):
    """(NULL, 1) and (0, 1) are different groups and hash differently: over
    enough segments they land on different ones"""
    keys = np.array([[0, 1], [0, 1]], np.int64)
    null = np.array([[1, 0], [0, 0]], np.uint8)
    d = gx.gbd_route(keys, null, (8, 4), 2048)
    assert d[0] != d[1]


def test_plain_aggregate_routes_to_segment_zero(gx):
    for nsegs in NSEGS:
        out = gx.gbd_route(np.zeros((5, 0), np.int64), np.zeros((5, 0), np.uint8),
                           [], nsegs)
        assert (out == 0).all() and len(out) == 5


def test_route_rejects_bad_arguments(gx):
    lib = gx.lib()
    k = np.zeros((4, 1), np.int64)
    nl = np.zeros((4, 1), np.uint8)
    w8 = np.array([8], np.int32)
    out = np.zeros(4, np.int32)
    ok = (k.ctypes.data, nl.ctypes.data, w8.ctypes.data, 1, 4, 3, out.ctypes.data)
    assert lib.gx_selftest_gbd_route(*ok) == 0

    def bad(**kw):
        names = ("keys", "key_null", "widths", "nkeys", "n", "nsegs", "out")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.gx_selftest_gbd_route(*[args[x] for x in names])
    assert bad(nsegs=0) == 1
    assert bad(nkeys=5) == 1
    assert bad(nkeys=-1) == 1
    assert bad(n=-1) == 1
    assert bad(keys=None) == 1
    assert bad(key_null=None) == 1
    assert bad(widths=None) == 1
    assert bad(out=None) == 1
    w3 = np.array([3], np.int32)
    assert bad(widths=w3.ctypes.data) == 1
    with pytest.raises(ValueError):
        gx.gbd_route(k, nl, (3,), 3)

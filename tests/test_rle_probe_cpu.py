"""CPU checks of bind's per-block routing for the fused RLE fact-key probe
(rle_block_class through gx_selftest_rle_block_class; gx_table_bind stores the
same values in the block directory the kernel reads).  The inputs are the
oracle writer's streams for the key shapes test_rle_probe_gpu.py runs, and the
expectation is derived from the headers by an independent walker: the parallel
count decode may be chosen only when every repeat count is 2 bytes long, and a
block the kernel cannot read must route the column to materialize."""
import numpy as np
import pytest

import cloudberry_amd as gx
import rle_shapes as S
from oracle import pyapi as orc


def want_class(b):
    if b["version"] not in (1, 2) or b["flags"] & 5 or b["phys"] > 4096:
        return gx.RLEBLK_UNFUSED
    if not b["flags"] & 2:
        return gx.RLEBLK_NOBITMAP
    return (gx.RLEBLK_FIXED2 if set(b["cnt_lens"]) == {2}
            else gx.RLEBLK_VARINT)


def check(stream, want):
    blocks = S.walk_blocks(stream)
    got = gx.rle_block_classes(stream)
    assert list(got) == [want_class(b) for b in blocks]
    assert list(got) == want
    return blocks


def test_distinct_keys_have_no_bitmap():                       # case a
    blocks = check(orc.aocs_encode_rle(S.shape_a()), [gx.RLEBLK_NOBITMAP] * 3)
    assert [(b["flags"], b["phys"]) for b in blocks] == \
        [(0, 4090), (0, 4090), (0, 820)]


def test_canonical_two_byte_counts_are_fixed2():               # case c
    blocks = check(orc.aocs_encode_rle(S.shape_c()), [gx.RLEBLK_FIXED2])
    b = blocks[0]
    assert b["flags"] == 2 and b["phys"] == b["ncnt"] == 301
    assert b["csize"] == 2 * b["ncnt"] and b["phys"] % 8 != 0


@pytest.mark.parametrize("variant", ["fwd", "rev", "tail"])
def test_one_and_three_byte_counts_are_not_fixed2(variant):    # case e
    """csize == 2 * ncnt holds (1 + 3 bytes) and must not pick the fixed
    stride"""
    blocks = check(orc.aocs_encode_rle(S.shape_e(variant)), [gx.RLEBLK_VARINT])
    b = blocks[0]
    assert b["csize"] == 2 * b["ncnt"] == 4
    assert sorted(b["cnt_lens"]) == [1, 3]


def test_mixed_count_lengths_are_varint():                     # cases b, d
    b = check(orc.aocs_encode_rle(S.shape_b()), [gx.RLEBLK_VARINT])[0]
    assert set(b["cnt_lens"]) == {1, 2}
    d = check(orc.aocs_encode_rle(S.shape_d()), [gx.RLEBLK_VARINT])[0]
    assert sorted(d["cnt_lens"]) == [1, 2, 3] and d["kind"] == 3


def test_delta_block_is_unfused():                             # case g
    g = check(orc.aocs_encode_rle_delta(S.shape_g()), [gx.RLEBLK_UNFUSED])
    assert g[0]["flags"] & 4 and not g[0]["flags"] & 1


def test_orig_block_is_unfused():                              # case h
    k = S.shape_a()
    h = check(orc.aocs_encode(k[:3000]) + orc.aocs_encode_rle(S.shape_b()),
              [gx.RLEBLK_UNFUSED, gx.RLEBLK_VARINT])
    assert h[0]["version"] == 0


def test_block_of_over_4096_datums_is_unfused():               # case i
    i = check(orc.aocs_encode_rle(S.shape_i(), 65536), [gx.RLEBLK_UNFUSED])
    assert i[0]["phys"] > 4096 and i[0]["flags"] == 2


def test_header_that_overruns_its_block_is_unfused():
    """a count section longer than the block cannot be walked on the host, so
    the block is not offered to the fused scan"""
    s = bytearray(orc.aocs_encode_rle(S.shape_c()))
    assert gx.rle_block_classes(bytes(s))[0] == gx.RLEBLK_FIXED2
    s[24 + 28:24 + 32] = np.int32(1 << 20).tobytes()           # csize
    assert gx.rle_block_classes(bytes(s))[0] == gx.RLEBLK_UNFUSED


def test_bad_stream_is_refused():
    with pytest.raises(ValueError):
        gx.rle_block_classes(b"\x01" * 64)

"""Key-column shapes for the fused RLE fact-key probe tests, and a header
walker that states what each stream really contains (shared by
test_rle_probe_cpu.py and test_rle_probe_gpu.py; not a test module).

Every shape is an int64 key column whose equal keys are contiguous.  The
header expectations are asserted by the tests, so a writer change cannot
silently move a case off the block layout it is meant to cover."""
import struct

import numpy as np


def walk_blocks(stream):
    """One dict per AO block of an uncompressed AOCS stream: envelope kind (1
    small content, 3 large content) and row count, DatumStreamBlock version,
    flags (1 NULL bitmap, 2 RLE, 4 DELTA), logical, phys and, for RLE blocks,
    ncnt, csize and the byte length of every repeat count."""
    out, off = [], 0
    while off + 24 <= len(stream):
        b03, b47 = struct.unpack_from("<II", stream, off)
        if b03 == 0 and b47 == 0:
            break
        kind = (b03 >> 28) & 7
        if kind == 1:
            rows = (b03 & 0x00FFFC00) >> 10
            datalen = ((b03 & 0x3FF) << 11) | ((b47 & 0xFFE00000) >> 21)
            assert b47 & 0x1FFFFF == 0, "compressed block"
        else:
            assert kind == 3, kind
            rows = b47 & 0x3FFFFFFF
            datalen = b03 & 0x1FFFFF
        c = off + 24
        version, flags = struct.unpack_from("<hh", stream, c)
        b = {"kind": kind, "rows": rows, "version": version, "flags": flags}
        if version == 0:                    # Orig: int16 ndatum at +4
            b["logical"] = struct.unpack_from("<h", stream, c + 4)[0]
            b["phys"] = b["logical"]
        else:
            b["logical"], b["phys"] = struct.unpack_from("<ii", stream, c + 4)
        if version != 0 and flags & 2:
            _, bmbits, ncnt, csize = struct.unpack_from("<iiii", stream, c + 16)
            if flags & 1:                   # NULL bitmap sits before the RLE one
                raise AssertionError("NULL-bearing block")
            p = c + 32 + (12 if flags & 4 else 0)
            cnts = stream[p + ((bmbits + 7) >> 3):][:csize]
            lens, i = [], 0
            while i < csize:
                lens.append((cnts[i] >> 6) + 1)
                i += lens[-1]
            assert i == csize and len(lens) == ncnt
            b.update(bmbits=bmbits, ncnt=ncnt, csize=csize, cnt_lens=lens)
        out.append(b)
        off += (24 + datalen + 7) & ~7
    return out


def runs(keys, lens):
    return np.repeat(np.asarray(keys, np.int64), np.asarray(lens, np.int64))


# ---- the key columns of cases a-f and i (g, h, j differ only in the writer) ----

def shape_a():
    """all-distinct keys over 3 blocks: no repeat bitmap at all"""
    return np.arange(3, 3 + 9000, dtype=np.int64)


def shape_b():
    """runs of 64, 65, 66 rows (counts 63, 64, 65: the 1 -> 2-byte varint
    boundary) beside runs of 1..7 rows"""
    rng = np.random.default_rng(101)
    lens = np.concatenate([[64, 65, 66, 1, 2, 66, 65, 64, 7, 1],
                           rng.integers(1, 8, 150), [65, 64, 66, 3]])
    rng.shuffle(lens[10:])
    return runs(10 + 3 * np.arange(len(lens)), lens)


def shape_c():
    """every run 65..16384 rows: the reference itself writes all-2-byte
    counts; one run of exactly 16384 (count 0x3FFF, the largest 2-byte one)"""
    rng = np.random.default_rng(103)
    lens = rng.integers(65, 110, 301)
    lens[137] = 16384
    return runs(1000 + 2 * np.arange(len(lens)), lens)


def shape_d():
    """16384 rows (largest 2-byte count) next to 16385 (smallest 3-byte)"""
    return runs([21, 22, 23, 24], [16384, 16385, 3, 1])


def shape_e(variant):
    """finding 1: one 3-byte and one 1-byte count, csize == 2 * ncnt"""
    if variant == "fwd":
        return runs([7, 8], [20000, 2])
    if variant == "rev":
        return runs([8, 7], [2, 20000])
    assert variant == "tail"
    return np.concatenate([runs([7, 8], [20000, 2]),
                           np.arange(100, 130, dtype=np.int64)])


def shape_f(variant):
    if variant == "split":      # distinct keys fill block 0; the key that
        k = np.arange(1, 4091, dtype=np.int64)    # ends it runs on into block 1
        return np.concatenate([k, runs([4090, 5000, 5001], [9, 4, 1])])
    if variant == "one_row":
        return np.array([77], np.int64)
    if variant == "one_run":
        return runs([77], [300])
    assert variant == "last_block_one_row"
    return np.arange(1, 4090 + 2, dtype=np.int64)


def shape_g():
    """sorted keys with duplicates: what the reference delta-compresses"""
    rng = np.random.default_rng(107)
    return np.sort(rng.integers(1, 4000, 12000)).astype(np.int64)


def shape_i():
    """over 4096 distinct keys in one 64 KiB block, then short runs"""
    rng = np.random.default_rng(109)
    return np.concatenate([np.arange(1, 6001, dtype=np.int64),
                           runs(7000 + np.arange(500), rng.integers(1, 5, 500))])

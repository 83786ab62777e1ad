"""Host rule that lets Q3 sizing pick the rank form of the join/agg table
(gx_selftest_rank_eligible): no GPU needed."""
import pytest

gx = pytest.importorskip("cloudberry_amd")


@pytest.mark.parametrize("n", [1, 10, 14_600_000])
@pytest.mark.parametrize("kmin", [1, 100, 2**40 + 5])
def test_density_boundary(n, kmin):
    """range = kmax - kmin + 1 <= 64 n"""
    assert gx.rank_eligible(n, kmin, kmin + 64 * n - 1)
    assert not gx.rank_eligible(n, kmin, kmin + 64 * n)
    assert gx.rank_eligible(n, kmin, kmin)              # duplicates of one key


def test_no_rows_sparse_keys_and_switch():
    assert not gx.rank_eligible(0, 1, 1)
    assert not gx.rank_eligible(0, 2**64 - 1, 0)        # sizing's empty stats
    assert not gx.rank_eligible(2, 1, 10**9)
    assert not gx.rank_eligible(5, 10, 9)               # inverted stats
    assert not gx.rank_eligible(10, 1, 640, enabled=False)
    assert gx.rank_eligible(10, 1, 640)


def test_row_count_limit_and_full_span():
    """prefix counts are u32: fewer than 2^32 rows; a span of all 2^64 keys
    must not wrap into a small range"""
    assert gx.rank_eligible(2**32 - 1, 1, 2**32 - 1)
    assert not gx.rank_eligible(2**32, 1, 2**32)
    assert not gx.rank_eligible(1000, 0, 2**64 - 1)


def test_scan_block_is_whole_words():
    b = gx.rank_scan_block_keys()
    assert b > 0 and b % 64 == 0

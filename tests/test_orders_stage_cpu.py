"""The rule that picks the form of the rank-form orders stage
(gx_selftest_orders_staged): staged iff qual * K <= nrows unless
GX_ORDERS_STAGED forces a form; and the staged filter grid.  No GPU needed."""
import pytest

gx = pytest.importorskip("cloudberry_amd")


def test_k_is_a_small_positive_integer():
    assert 1 <= gx.orders_stage_k() <= 64


@pytest.mark.parametrize("qual", [1, 7, 1000, 14_500_000])
def test_boundary(qual):
    K = gx.orders_stage_k()
    assert gx.orders_staged(qual, qual * K) is True        # qual * K == nrows
    assert gx.orders_staged(qual, qual * K + 1) is True
    assert gx.orders_staged(qual, qual * K - 1) is False
    assert gx.orders_staged(qual + 1, qual * K) is False


def test_qual_zero_takes_the_rule():
    assert gx.orders_staged(0, 0) is True
    assert gx.orders_staged(0, 1) is True
    assert gx.orders_staged(0, 150_000_000) is True


@pytest.mark.parametrize("qual,nrows", [(0, 0), (1, 1), (1, 10**6), (10**6, 10**6)])
def test_forced_values_override_the_rule(qual, nrows):
    assert gx.orders_staged(qual, nrows, env=0) is False
    assert gx.orders_staged(qual, nrows, env=1) is True


def test_no_overflow_near_2p40_and_beyond():
    K = gx.orders_stage_k()
    n = 2**40
    assert gx.orders_staged(n // K, n) is True
    assert gx.orders_staged(n // K + 1, n) is False
    assert gx.orders_staged(n, n) is (K == 1)
    # a product qual * K would wrap int64 here
    big = 2**62
    assert gx.orders_staged(big, big) is (K == 1)
    assert gx.orders_staged(big // K, big) is True
    assert gx.orders_staged(big // K + 1, big) is False


def test_wave_segment_fits_the_lds_budget():
    """4 waves x W records x 16 B stay within 20 KiB: 8 blocks per CU"""
    W = gx.orders_stage_wave_records()
    assert W >= 64 and W % 64 == 0
    assert 4 * W * 16 <= 20 * 1024


def test_grid_follows_the_selectivity():
    W = gx.orders_stage_wave_records()
    n = 150_000_000
    rowblocks = (n + 255) // 256
    # 10 %: 0.75 W records over 6.4 per iteration (30 iterations at W = 256)
    iters = (3 * W * 10) // (4 * 64)
    assert gx.orders_stage_grid(n // 10, n) == -(-rowblocks // iters)
    # very few qualify: never fewer than 8192 blocks on a large table
    assert gx.orders_stage_grid(10, n) == 8192
    assert gx.orders_stage_grid(0, n) == 8192
    # everything qualifies: 0.75 W / 64 iterations per wave, at least one
    assert gx.orders_stage_grid(n, n) == -(-rowblocks // max(3 * W // 256, 1))
    # never more than 2^20 blocks
    assert gx.orders_stage_grid(2**40, 2**40) == 2**20
    # small tables: no more blocks than rows need
    assert gx.orders_stage_grid(100, 1000) == 4
    assert gx.orders_stage_grid(0, 0) == 1
    assert gx.orders_stage_grid(1, 1) == 1

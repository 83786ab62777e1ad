"""Staged form of the rank-form orders stage: the filter kernel compacts
{key, attr1, attr2} of the qualifying mid rows through per-wave LDS segments
of W records into a staging array, and the fill reads those records instead
of walking the mid table again.

Results are checked against the numpy brute force of test_rank_table_gpu
(keys, attrs and counts bit-equal, revenue within rtol=1e-6).  Every case
pins table_mode() and orders_mode().  Unless a case says otherwise it forces
GX_ORDERS_STAGED=1 and a one-block filter grid through the test seam: with
256 threads per block, wave w then owns the 64-row chunks c with c % 4 == w,
so a table of a few thousand rows reaches many iterations per wave, the
segment-overflow flush and the block-end claim.  The number of mid-loop
flushes is checked against a host simulation of the rule (a wave flushes
when its segment cannot take the iteration's records)."""
import numpy as np
import pytest

from test_rank_table_gpu import Plan, facts_for, _assert_q3

pytestmark = pytest.mark.gpu

gx = pytest.importorskip("cloudberry_amd")

TPB = 256


@pytest.fixture(scope="module")
def ctx():
    c = gx.Context(device=0, seg=0, nsegs=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def orc():
    from oracle import pyapi
    return pyapi


@pytest.fixture(scope="module")
def W():
    return gx.orders_stage_wave_records()


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    for v in ("GX_RANK_TABLE", "GX_DIM_BITMAP", "GX_FORCE_MOTION",
              "GX_TABLE_FACTOR_PCT"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("GX_ORDERS_STAGED", "1")


def flushes_expected(om, grid, W):
    """mid-loop flushes of the staged filter kernel over the qualifying-row
    mask om with `grid` blocks of four waves"""
    om = np.asarray(om, bool)
    chunks = (len(om) + 63) // 64
    per_chunk = [int(om[c * 64:(c + 1) * 64].sum()) for c in range(chunks)]
    waves = 4 * grid
    fl = 0
    for v in range(waves):
        wn = 0
        for c in range(v, chunks, waves):
            cnt = per_chunk[c]
            if cnt == 0:
                continue
            if wn + cnt > W:
                fl += 1
                wn = 0
            wn += cnt
    return fl


def run_plan(p, W, grid=1, runs=1, dim_join="semi", want=None, mode=1):
    """run p's q `runs` times at the given filter grid; every run is checked"""
    want = p.brute(dim_join) if want is None else want
    q = p.q(dim_join)
    q._test_set_orders_grid(grid)
    try:
        for _ in range(runs):
            got = q.run().result()
            assert q.table_mode() == 1
            assert q.orders_mode() == mode
            _assert_q3(got, want)
            if mode == 1:
                blocks, fl, recs = q.orders_stage_claims()
                om = p.qual_rows(dim_join)
                g = grid if grid else gx.orders_stage_grid(int(om.sum()),
                                                           len(p.o_keys))
                assert blocks == g
                assert fl == flushes_expected(om, g, W)
                assert recs == om.sum()
    finally:
        q.free()
    return want


def dense(seed, n, frac, kmin=1):
    rng = np.random.default_rng(seed)
    keys = kmin + np.arange(n, dtype=np.int64)
    qual = rng.random(n) < frac
    qual[0] = qual[-1] = True
    return rng, keys, qual


# ---------------- 1. many iterations ----------------

@pytest.fixture(scope="module")
def case1(ctx, orc):
    rng, keys, qual = dense(101, 64 * 300 + 5, 0.10, kmin=1000)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, [999, 1000 + len(keys)]),
             ship_all=True)
    yield p, p.brute()
    p.free()


@pytest.mark.parametrize("grid", [1, 3])
def test_many_iterations_three_runs(case1, W, grid):
    """64 * 300 + 5 rows, ~10 % qualify, three runs of one q: the cursor
    reset leaves nothing behind.  One block gives each wave 75 iterations
    and ~480 records, so at W = 256 every wave also flushes once mid-loop;
    three blocks give ~160 per wave, many iterations and no overflow."""
    p, want = case1
    assert len(want["l_orderkey"]) > 1500
    fl = flushes_expected(p.qual_rows(), grid, W)
    if grid == 3 and W >= 256:
        assert fl == 0
    run_plan(p, W, grid=grid, runs=3, want=want)


# ---------------- 2. every row qualifies ----------------

def test_every_row_qualifies(ctx, orc, W):
    """n = 4 (3 W + 17), not a multiple of 64: each wave flushes mid-loop
    several times and the block once at the end"""
    n = 4 * (3 * W + 17)
    assert n % 64 != 0
    rng = np.random.default_rng(103)
    keys = 7 + np.arange(n, dtype=np.int64)
    qual = np.ones(n, bool)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, [6, 7 + n], extra=500),
             ship_all=True)
    try:
        assert flushes_expected(qual, 1, W) >= 8
        want = run_plan(p, W, runs=2)
        np.testing.assert_array_equal(want["l_orderkey"], keys)
    finally:
        p.free()


# ---------------- 3. segment edges ----------------

@pytest.mark.parametrize("off", ["W-64", "W-63", "W-1", "W", "W+1", "2W"])
def test_segment_edges(ctx, orc, W, off):
    """only wave 0's chunks hold qualifying rows; the other three waves end
    with zero records beside a full one"""
    count = {"W-64": W - 64, "W-63": W - 63, "W-1": W - 1, "W": W,
             "W+1": W + 1, "2W": 2 * W}[off]
    rng = np.random.default_rng(107)
    chunks0 = (2 * W) // 64 + 4                  # wave-0 chunks
    n = 64 * 4 * chunks0
    keys = 11 + np.arange(n, dtype=np.int64)
    rows0 = np.flatnonzero((np.arange(n) // 64) % 4 == 0)
    qual = np.zeros(n, bool)
    qual[rng.choice(rows0, count, replace=False)] = True
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, extra=500), ship_all=True)
    try:
        assert p.qual_rows().sum() == count
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual])
    finally:
        p.free()


def test_segment_exactly_full_then_one_more(ctx, orc, W):
    """wave 0 fills its segment to exactly W with whole chunks, then meets
    one more record: the flush moves W records and the segment restarts"""
    full = W // 64
    n = 64 * 4 * (full + 2)
    keys = 3 + np.arange(n, dtype=np.int64)
    qual = np.zeros(n, bool)
    for c in range(full):
        qual[64 * 4 * c:64 * 4 * c + 64] = True
    qual[64 * 4 * (full + 1) + 5] = True
    rng = np.random.default_rng(109)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, extra=500), ship_all=True)
    try:
        assert flushes_expected(qual, 1, W) == 1
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual])
    finally:
        p.free()


# ---------------- 4. tiny and ragged inputs ----------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tiny_tables(ctx, orc, W, n):
    rng, keys, qual = dense(113 + n, n, 0.5, kmin=21)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, [20, 21 + n], extra=50),
             ship_all=True)
    try:
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual])
        run_plan(p, W, grid=0, want=want)
    finally:
        p.free()


@pytest.mark.parametrize("where", ["middle", "first", "last_partial_chunk"])
def test_one_qualifying_row(ctx, orc, W, where):
    n = 64 * 47 + 3
    at = {"middle": 1234, "first": 0, "last_partial_chunk": n - 1}[where]
    rng = np.random.default_rng(127)
    keys = 5 + np.arange(n, dtype=np.int64)
    qual = np.zeros(n, bool)
    qual[at] = True
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, extra=300), ship_all=True)
    try:
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], [5 + at])
        run_plan(p, W, grid=0, want=want)
    finally:
        p.free()


def test_rows_in_the_last_partial_chunk(ctx, orc, W):
    """the last chunk has 3 rows, all qualifying, among ~10 % elsewhere"""
    rng, keys, qual = dense(131, 64 * 40 + 3, 0.10)
    qual[-3:] = True
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys, extra=300), ship_all=True)
    try:
        want = run_plan(p, W)
        assert set(keys[-3:].tolist()) <= set(want["l_orderkey"].tolist())
    finally:
        p.free()


def test_none_qualifying(ctx, orc):
    """no qualifying row: sizing refuses the rank form, as
    test_no_qualifying_order expects, and the hash form runs"""
    rng = np.random.default_rng(137)
    keys = np.arange(1, 3001, dtype=np.int64)
    p = Plan(ctx, orc, keys, np.zeros(3000, bool), facts_for(rng, keys))
    try:
        q = p.q()
        q._test_set_orders_grid(1)
        got = q.run().result()
        assert q.table_mode() == 0
        assert q.orders_mode() == 0
        assert len(got["l_orderkey"]) == 0
        q.free()
    finally:
        p.free()


# ---------------- 5. grids ----------------

@pytest.mark.parametrize("grid", [1, 2, 7, 0], ids=["g1", "g2", "g7", "rule"])
def test_grids(case1, W, grid):
    """the case-1 data at one, two and seven blocks and at the production
    rule: the same result each time"""
    p, want = case1
    run_plan(p, W, grid=grid, want=want)


# ---------------- 6. the other instantiations, forced staged ----------------

def test_visimap_on_mid_hides_qualifying_rows(ctx, orc, W):
    rng, keys, qual = dense(139, 64 * 150 + 9, 0.4)
    hidden = rng.random(len(keys)) < 0.3
    hidden[0] = True
    assert (qual & hidden).sum() > 100
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys), o_hidden=hidden,
             ship_all=True)
    try:
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual & ~hidden])
    finally:
        p.free()


@pytest.mark.parametrize("dim_join", ["anti", "anti_notin"])
def test_anti_joins(ctx, orc, W, dim_join):
    rng, keys, qual = dense(149, 64 * 150 + 9, 0.4)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys))
    try:
        want = run_plan(p, W, dim_join=dim_join)
        assert len(want["l_orderkey"]) > 1000
    finally:
        p.free()


def test_hash_dim_set(ctx, orc, W, monkeypatch):
    """GX_DIM_BITMAP=0: the bloom + hash-set instantiation (BM off)"""
    monkeypatch.setenv("GX_DIM_BITMAP", "0")
    rng, keys, qual = dense(151, 64 * 150 + 9, 0.4)
    p = Plan(ctx, orc, keys, qual, facts_for(rng, keys))
    try:
        q = p.q()
        q._test_set_orders_grid(1)
        q.run()
        assert (q.dim_mode(), q.table_mode(), q.orders_mode()) == (0, 1, 1)
        _assert_q3(q.result(), p.brute())
        om = p.qual_rows()
        assert q.orders_stage_claims() == (1, flushes_expected(om, 1, W), om.sum())
        q.free()
    finally:
        p.free()


def test_u64_keys(ctx, orc, W):
    rng, keys, qual = dense(157, 64 * 150 + 9, 0.4, kmin=2**40 + 5)
    li = facts_for(rng, keys, [2**40 + 4, 2**40 + 5 + len(keys), 5])
    p = Plan(ctx, orc, keys, qual, li, ship_all=True)
    try:
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual])
    finally:
        p.free()


@pytest.mark.parametrize("order", ["asc", "desc", "shuffled"])
def test_mid_row_order(ctx, orc, W, order):
    rng, keys, qual = dense(163, 64 * 150 + 9, 0.3, kmin=1000)
    n = len(keys)
    idx = {"asc": np.arange(n), "desc": np.arange(n)[::-1],
           "shuffled": np.random.default_rng(167).permutation(n)}[order]
    li = rng.permutation(facts_for(rng, keys, [999, 1000 + n]))
    p = Plan(ctx, orc, keys[idx], qual[idx], li, ship_all=True)
    try:
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[qual])
    finally:
        p.free()


@pytest.mark.parametrize("order", ["adjacent", "shuffled"])
def test_qualifying_rows_duplicated_verbatim(ctx, orc, W, order):
    """a key on two identical qualifying rows stores twice to one slot and
    still yields one group"""
    rng, keys, qual = dense(173, 5000, 0.4)
    li = rng.permutation(facts_for(rng, keys))
    p = Plan(ctx, orc, keys, qual, li, ship_all=True)
    idx = np.repeat(np.arange(len(keys)), 1 + qual)
    if order == "shuffled":
        idx = np.random.default_rng(179).permutation(idx)
    enc = orc.aocs_encode
    m = len(idx)
    ordr2 = ctx.bind([(enc(p.o_keys[idx]), 8, m), (enc(p.o_cust[idx]), 8, m),
                      (enc(p.o_date[idx]), 4, m), (enc(p.o_prio[idx]), 4, m)])
    try:
        want = p.brute()
        fl = flushes_expected(p.qual_rows()[idx], 1, W)
        p.ordr.free()
        p.ordr = ordr2
        q = p.q()
        q._test_set_orders_grid(1)
        got = q.run().result()
        assert (q.table_mode(), q.orders_mode()) == (1, 1)
        _assert_q3(got, want)
        assert q.orders_stage_claims() == (1, fl, p.qual_rows()[idx].sum())
        q.free()
    finally:
        p.free()


def test_key_on_a_qualifying_and_a_failing_row(ctx, orc, W):
    """every key twice, one row failing the filter with other attrs: the
    record carries the qualifying row's attrs whichever row comes first"""
    rng = np.random.default_rng(181)
    n = 4000
    keys = 1 + np.arange(n, dtype=np.int64)
    both = np.concatenate([keys, keys])
    qual = np.concatenate([np.ones(n, bool), np.zeros(n, bool)])
    perm = rng.permutation(2 * n)
    both, qual = both[perm], qual[perm]
    drop = rng.random(n) < 0.5
    qual &= ~drop[both - 1]
    p = Plan(ctx, orc, both, qual, facts_for(rng, keys), ship_all=True)
    try:
        want = run_plan(p, W)
        np.testing.assert_array_equal(want["l_orderkey"], keys[~drop])
    finally:
        p.free()


# ---------------- 7. form switching on one q ----------------

def test_staged_twopass_staged_on_one_q(case1, W, monkeypatch):
    """each form's first run allocates its own buffers (staging records;
    row mask) and leaves the other's valid"""
    p, want = case1
    q = p.q()
    q._test_set_orders_grid(1)
    try:
        for force, mode in (("1", 1), ("0", 0), ("1", 1)):
            monkeypatch.setenv("GX_ORDERS_STAGED", force)
            got = q.run().result()
            assert (q.table_mode(), q.orders_mode()) == (1, mode)
            _assert_q3(got, want)
        # and a q whose first run is two-pass
        q2 = p.q()
        for force, mode in (("0", 0), ("1", 1), ("0", 0)):
            monkeypatch.setenv("GX_ORDERS_STAGED", force)
            got = q2.run().result()
            assert (q2.table_mode(), q2.orders_mode()) == (1, mode)
            _assert_q3(got, want)
        q2.free()
    finally:
        q.free()


# ---------------- 8. the default plan ----------------

def test_default_q3_rule_and_both_forms(ctx, orc, monkeypatch):
    """TPC-H SF 0.01 against the oracle with nothing forced: the form is the
    one the rule gives for the oracle's own qualifying count; then each form
    forced"""
    sf = 0.01
    c, o, li = orc.gen_customer(sf), orc.gen_orders(sf), orc.gen_lineitem(sf)
    want = orc.q3(c, o, li)
    nq = int(((o["o_orderdate"] < gx.CUTOFF_19950315) &
              np.isin(o["o_custkey"], c["c_custkey"][c["c_mktsegment"] == 0])).sum())
    nrows = len(o["o_orderdate"])
    assert 0 < nq < nrows
    predicted = 1 if nq * gx.orders_stage_k() <= nrows else 0
    t = (ctx.tpch_gen(gx.TPCH_CUSTOMER, sf), ctx.tpch_gen(gx.TPCH_ORDERS, sf),
         ctx.tpch_gen(gx.TPCH_LINEITEM, sf))
    q = ctx.q3(*t)
    try:
        for force, mode in ((None, predicted), ("0", 0), ("1", 1), (None, predicted)):
            if force is None:
                monkeypatch.delenv("GX_ORDERS_STAGED", raising=False)
            else:
                monkeypatch.setenv("GX_ORDERS_STAGED", force)
            _assert_q3(q.run().result(), want)
            assert (q.table_mode(), q.orders_mode()) == (1, mode)
            if mode == 1:
                blocks, fl, recs = q.orders_stage_claims()
                assert blocks == gx.orders_stage_grid(nq, nrows)
                assert (fl, recs) == (0, nq)
    finally:
        q.free()
        for x in reversed(t):
            x.free()

#!/usr/bin/env python3
"""Stage timing of the two-stage descriptor GROUP BY (gx_groupby_desc_dist) on
ONE GPU through the forced-motion branch (GX_FORCE_MOTION=1: a one-rank
self-exchange, the only form one GPU can time).  One process per case; the
result is compared with gx_groupby_desc before anything is timed.  Recorded,
not gated.

  low   GX_TPCH_LINEITEM_Q1 at --sf: GROUP BY (returnflag, linestatus) WHERE
        shipdate <= cutoff, COUNT(*) + SUM(price), max_groups = --low-bound
        (the planner's bound: six groups exist).
  high  --rows rows over about --keys distinct int64 keys, SUM(float8) +
        COUNT(*), alternated with gx_groupby_dist (unchanged code, the
        yardstick) on the same bound table in the same process.

    python tools/gb_desc_dist_time.py --case low|high [--runs R] [--out F]

The four stage times are gx_gb_stats' HIP-event spans.  ms_partial of
gx_groupby_desc_dist is scan + extract (its table clear is enqueued before the
first event); gx_groupby_dist's is table clear + scan (its partition kernels
read the table slots, so it has no extract).  Each case updates its own key of
the JSON file."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cloudberry_amd as gx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--case", required=True, choices=["low", "high"])
ap.add_argument("--sf", type=float, default=100.0)
ap.add_argument("--low-bound", type=int, default=64)
ap.add_argument("--rows", type=float, default=100e6)
ap.add_argument("--keys", type=float, default=10e6)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                              "groupby_desc_dist.json"))
args = ap.parse_args()
assert args.runs >= 5, "report the median of at least 5 runs"
STAGES = ("ms_partial", "ms_partition", "ms_exchange", "ms_combine")
COUNTERS = ("rows_in", "partial_groups", "sent_rows", "recv_rows", "final_groups")


def summary(xs):
    xs = [float(x) for x in xs]
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "all": xs}


def same(a, b):
    assert a["ngroups"] == b["ngroups"], "group count differs"
    for f in ("keys", "key_null", "agg_null"):
        assert (a[f] == b[f]).all(), f"{f} differ"
    for x, y in zip(a["aggs"], b["aggs"]):
        assert x.tobytes() == y.tobytes(), "aggregates differ"


def desc_dist_stats(ctx, t, keys, aggs, quals, max_groups):
    """one timed call: the C entry point alone, result freed unconverted"""
    d = ctx._gb_desc(t, keys, aggs, quals, max_groups)
    res, st = gx._GbResult(), gx._GbStats()
    w0 = time.perf_counter()
    ctx._chk(ctx._lib.gx_groupby_desc_dist(ctx._h, ctypes.byref(d),
                                           ctypes.byref(res), ctypes.byref(st)))
    wall = (time.perf_counter() - w0) * 1e3
    ctx._lib.gx_gb_result_free(ctypes.byref(res))
    out = {f: getattr(st, f) for f, _ in st._fields_}
    out["wall_ms"] = wall
    return out


def dist_stats(ctx, t):
    gp, n, st = ctypes.POINTER(gx._KvGroup)(), ctypes.c_int64(), gx._GbStats()
    w0 = time.perf_counter()
    ctx._chk(ctx._lib.gx_groupby_dist(ctx._h, t._t, 0, 1, ctypes.byref(gp),
                                      ctypes.byref(n), ctypes.byref(st)))
    wall = (time.perf_counter() - w0) * 1e3
    ctx._lib.gx_free(gp)
    out = {f: getattr(st, f) for f, _ in st._fields_}
    out["wall_ms"] = wall
    return out


def stage_summary(stats):
    return {f: summary([s[f] for s in stats]) for f in STAGES + ("wall_ms",)}


def below_partial(stats):
    med = {f: statistics.median([s[f] for s in stats]) for f in STAGES}
    return {"partition_below_partial": med["ms_partition"] < med["ms_partial"],
            "combine_below_partial": med["ms_combine"] < med["ms_partial"]}


def case_low(ctx):
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, args.sf)
    keys, aggs = [0, 1], [("count*", None), ("sum", 2, True)]
    quals = [(4, "<=", gx.CUTOFF_19950315)]
    mg = args.low_bound
    want = ctx.groupby_desc(t, keys, aggs, quals=quals, max_groups=mg)
    got = ctx.groupby_desc_dist(t, keys, aggs, quals=quals, max_groups=mg)
    # six groups of ~10^8 rows each: the float8 sums depend on arrival order
    assert want["ngroups"] == got["ngroups"]
    assert (want["keys"] == got["keys"]).all()
    assert (want["aggs"][0] == got["aggs"][0]).all()
    np.testing.assert_allclose(got["aggs"][1], want["aggs"][1], rtol=1e-6)
    print(f"low: sf {args.sf}, {t.nrows} rows, {got['ngroups']} groups, agrees "
          "with gx_groupby_desc", flush=True)
    stats = []
    for i in range(args.warmup + args.runs):
        s = desc_dist_stats(ctx, t, keys, aggs, quals, mg)
        if i >= args.warmup:
            stats.append(s)
        print(f"low: pass {i} {s}", flush=True)
    n = t.nrows
    t.free()
    return {
        "what": "GROUP BY (returnflag, linestatus) WHERE shipdate <= cutoff, "
                "COUNT(*) + SUM(price) through gx_groupby_desc_dist, 1 GPU, "
                "GX_FORCE_MOTION=1 (one-rank self-exchange)",
        "sf": args.sf, "rows": n, "max_groups": mg,
        "runs": args.runs, "warmup": args.warmup,
        "stage_ms": stage_summary(stats),
        "counters": {f: stats[-1][f] for f in COUNTERS},
        **below_partial(stats),
    }


def case_high(ctx):
    from oracle import pyapi as orc
    nrows, nkeys = int(args.rows), int(args.keys)
    t0 = time.time()
    rng = np.random.default_rng(3)              # tools/gb_dist_time.py's input
    keys = rng.integers(1, nkeys + 1, nrows).astype(np.int64)
    vals = rng.integers(-1000, 1001, nrows).astype(np.float64)
    kstream, vstream = orc.aocs_encode(keys), orc.aocs_encode(vals)
    del keys, vals
    print(f"high: host gen+encode {nrows} rows: {time.time() - t0:.1f}s", flush=True)
    t = ctx.bind([(kstream, 8, nrows), (vstream, 8, nrows)])
    del kstream, vstream
    aggs = [("sum", 1, True), ("count*", None)]
    want = ctx.groupby_desc(t, [0], aggs)
    got = ctx.groupby_desc_dist(t, [0], aggs)
    same(got, want)                             # integer-valued sums: exact
    ng = got["ngroups"]
    print(f"high: {ng} groups, identical to gx_groupby_desc", flush=True)
    del want, got
    new, old = [], []
    for i in range(args.warmup + args.runs):    # alternated
        a = desc_dist_stats(ctx, t, [0], aggs, [], 0)
        b = dist_stats(ctx, t)
        if i >= args.warmup:
            new.append(a)
            old.append(b)
        print(f"high: pass {i} desc_dist {a} dist {b}", flush=True)
    t.free()
    return {
        "what": "one int64 key, SUM(float8) + COUNT(*): gx_groupby_desc_dist "
                "alternated with gx_groupby_dist (unchanged, the yardstick) on "
                "the same bound table, 1 GPU, GX_FORCE_MOTION=1 (one-rank "
                "self-exchange)",
        "rows": nrows, "distinct_keys_requested": nkeys, "groups": ng,
        "runs": args.runs, "warmup": args.warmup,
        "wire_row_bytes": {"groupby_desc_dist": gx.gbd_wire_stride([0], aggs),
                           "groupby_dist": gx.KV_GROUP_DTYPE.itemsize},
        "groupby_desc_dist": {"stage_ms": stage_summary(new),
                              "counters": {f: new[-1][f] for f in COUNTERS},
                              **below_partial(new)},
        "groupby_dist": {"stage_ms": stage_summary(old),
                         "counters": {f: old[-1][f] for f in COUNTERS},
                         **below_partial(old)},
    }


path = os.path.abspath(args.out)
out = {}
if os.path.exists(path):
    with open(path) as f:
        out = json.load(f)
ctx = gx.Context(device=0, seg=0, nsegs=1)
ctx.comm_init(ctx.comm_unique_id())
os.environ["GX_FORCE_MOTION"] = "1"
key = {"low": "low_cardinality", "high": "high_cardinality"}[args.case]
out[key] = case_low(ctx) if args.case == "low" else case_high(ctx)
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out[key]), flush=True)
ctx.close()

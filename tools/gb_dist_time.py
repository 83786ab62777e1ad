#!/usr/bin/env python3
"""Stage timing of the two-stage GROUP BY (gx_groupby_dist) on ONE GPU
through the forced-motion branch (self-exchange), next to the wall time of
the one-stage gx_groupby on the same bound table.

The two-stage path does strictly more work than the one-stage reference:
the same partial agg, plus the partition, the exchange and a combine over
the partial groups.  Recorded, not gated.  Default input: 100M rows, 10M
distinct keys, integer-valued f64 measure (sums are exact, so the two
results are compared bit-for-bit before anything is timed).

    python tools/gb_dist_time.py [--rows N] [--keys K] [--runs R] [--out F]
"""
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
from oracle import pyapi as orc  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=float, default=100e6)
ap.add_argument("--keys", type=float, default=10e6)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gb_dist_r3.json"))
args = ap.parse_args()
NROWS, NKEYS = int(args.rows), int(args.keys)
assert args.runs >= 5, "report the median of at least 5 runs"

t0 = time.time()
rng = np.random.default_rng(3)
keys = rng.integers(1, NKEYS + 1, NROWS).astype(np.int64)
vals = rng.integers(-1000, 1001, NROWS).astype(np.float64)
kstream, vstream = orc.aocs_encode(keys), orc.aocs_encode(vals)
del keys, vals
print(f"host gen+encode {NROWS} rows: {time.time() - t0:.1f}s", flush=True)

ctx = gx.Context(device=0, seg=0, nsegs=1)
ctx.comm_init(ctx.comm_unique_id())
t = ctx.bind([(kstream, 8, NROWS), (vstream, 8, NROWS)])
del kstream, vstream
lib = ctx._lib


def one_stage():
    """wall ms of the C call alone (result freed, no Python conversion)"""
    gp, n = ctypes.POINTER(gx._KvGroup)(), ctypes.c_int64()
    w0 = time.perf_counter()
    ctx._chk(lib.gx_groupby(ctx._h, t._t, 0, 1, ctypes.byref(gp), ctypes.byref(n)))
    ms = (time.perf_counter() - w0) * 1e3
    return ms, gp, n.value


def two_stage():
    gp, n, st = ctypes.POINTER(gx._KvGroup)(), ctypes.c_int64(), gx._GbStats()
    w0 = time.perf_counter()
    ctx._chk(lib.gx_groupby_dist(ctx._h, t._t, 0, 1, ctypes.byref(gp),
                                 ctypes.byref(n), ctypes.byref(st)))
    ms = (time.perf_counter() - w0) * 1e3
    return ms, gp, n.value, {f: getattr(st, f) for f, _ in st._fields_}


def as_array(gp, n):
    a = np.frombuffer(ctypes.string_at(gp, n * 32), gx.KV_GROUP_DTYPE)
    lib.gx_free(gp)
    return a


os.environ["GX_FORCE_MOTION"] = "1"

# results must agree before a time means anything
_, gp1, n1 = one_stage()
_, gp2, n2, _ = two_stage()
a1, a2 = as_array(gp1, n1), as_array(gp2, n2)
assert n1 == n2 and a1.tobytes() == a2.tobytes(), "two-stage result differs"
print(f"results identical: {n1} groups", flush=True)
del a1, a2

for _ in range(args.warmup):
    lib.gx_free(one_stage()[1])
    lib.gx_free(two_stage()[1])

# alternate the two paths so drift on a shared host hits both alike
w_one, w_two, stats = [], [], []
for _ in range(args.runs):
    ms, gp, _ = one_stage()
    lib.gx_free(gp)
    w_one.append(ms)
    ms, gp, _, st = two_stage()
    lib.gx_free(gp)
    w_two.append(ms)
    stats.append(st)


def med(xs):
    return float(statistics.median(xs))


stage = {f: med([s[f] for s in stats])
         for f in ("ms_partial", "ms_partition", "ms_exchange", "ms_combine")}
res = {
    "what": "gx_groupby_dist, 1 GPU, GX_FORCE_MOTION=1 (self-exchange) vs "
            "gx_groupby on the same bound table",
    "rows": NROWS, "distinct_keys_requested": NKEYS,
    "runs": args.runs, "warmup": args.warmup, "statistic": "median",
    "stage_ms": stage,
    "stage_ms_all_runs": [{f: s[f] for f in stage} for s in stats],
    "counters": {f: stats[-1][f] for f in ("rows_in", "partial_groups",
                                           "sent_rows", "recv_rows",
                                           "final_groups")},
    "wall_ms_groupby_dist": med(w_two),
    "wall_ms_groupby_dist_all_runs": w_two,
    "wall_ms_groupby_one_stage": med(w_one),
    "wall_ms_groupby_one_stage_all_runs": w_one,
    "note": "wall times include the device-to-host copy of the groups and "
            "the host sort in both paths; stage_ms are HIP-event times",
}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res), flush=True)
t.free()
ctx.close()

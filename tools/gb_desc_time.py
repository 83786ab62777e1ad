#!/usr/bin/env python3
"""Kernel timing of the descriptor-form GROUP BY (gx_groupby_desc) on ONE GPU
against the two kernels that stay beside it, each on the same bound table in
the same process, variants alternated, results compared before anything is
timed.  Recorded, not gated.

  low   GX_TPCH_LINEITEM_Q1 at --sf: GROUP BY (returnflag, linestatus) WHERE
        shipdate <= cutoff, COUNT(*) + SUM(price), against gx_q1's ms_out
        (the hand-specialised kernel: 22 B/row, this plan reads 14 B/row).
  lds0  the same query with GX_GB_LDS=0 alternated with the default, at
        --lds0-sf: six-address global atomics, so keep the scale factor small
        and give the run its own time limit.
  high  --rows rows over about --keys distinct int64 keys, SUM(float8) +
        COUNT(*), LDS on and off, against the one-stage gx_groupby
        (gx_groupby_dist's ms_partial at nsegs == 1: table clear + k_groupby
        + extract between two HIP events; gx_groupby_desc's ms_kernel is the
        scan kernel alone, so its own clear + extract span is not in it).
  q1rev GX_TPCH_LINEITEM_Q1 at --sf: the same GROUP BY with COUNT(*) +
        SUM(price) + SUM(price * (1 - disc)) through gx_groupby_expr (the
        22 B/row k_q1_agg reads), alternated with gx_q1 and with the
        two-aggregate gx_groupby_desc call of `low`.
  low with --parent-root DIR (a built checkout of the parent commit): `low`
        run by one fresh process per round from DIR and from this tree,
        alternated --rounds times, to see whether the scan kernel that takes
        no expressions moved.

    python tools/gb_desc_time.py [--cases low,lds0,high,q1rev] [--runs R] [--out F]

Each case updates its own key of the JSON file, so cases may run in separate
processes."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cloudberry_amd as gx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", default="low,lds0,high")
ap.add_argument("--sf", type=float, default=100.0)
ap.add_argument("--lds0-sf", type=float, default=1.0)
ap.add_argument("--rows", type=float, default=100e6)
ap.add_argument("--keys", type=float, default=10e6)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupby_desc.json"))
args = ap.parse_args()
assert args.runs >= 5, "report the median of at least 5 runs"
CASES = args.cases.split(",")
STREAM_TBS = (5.8, 6.6)          # measured stream ceiling, TB/s


def summary(xs):
    xs = [float(x) for x in xs]
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "all": xs}


def set_lds(on):
    if on:
        os.environ.pop("GX_GB_LDS", None)
    else:
        os.environ["GX_GB_LDS"] = "0"


def slots_pow2(want):
    s = 1024
    while s < want:
        s <<= 1
    return s


Q1_AGGS = [("count*", None), ("sum", 2, True)]


def q1_desc(ctx, t, lds=True):
    set_lds(lds)
    try:
        return ctx.groupby_desc(t, [0, 1], Q1_AGGS,
                                quals=[(4, "<=", gx.CUTOFF_19950315)], stats=True)
    finally:
        set_lds(True)


def check_q1(res, q1):
    slot = res["keys"][:, 0] * 2 + res["keys"][:, 1]
    want = np.nonzero(q1["count"])[0]
    assert (slot == want).all(), "group set differs from gx_q1"
    assert (res["aggs"][0] == q1["count"][want]).all(), "counts differ from gx_q1"
    np.testing.assert_allclose(res["aggs"][1], q1["sum_price"][want], rtol=1e-6)


def case_low(ctx, sf):
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, sf)
    n = t.nrows
    q1 = ctx.q1(t, gx.CUTOFF_19950315)
    res, st = q1_desc(ctx, t)
    check_q1(res, q1)
    print(f"low: sf {sf}, {n} rows, results agree with gx_q1", flush=True)
    for _ in range(args.warmup):
        ctx.q1(t, gx.CUTOFF_19950315)
        q1_desc(ctx, t)
    ms_q1, ms_desc = [], []
    for _ in range(args.runs):                  # alternated
        ms_q1.append(ctx.q1(t, gx.CUTOFF_19950315)["ms"])
        ms_desc.append(q1_desc(ctx, t)[1]["ms_kernel"])
    t.free()
    md, mq = statistics.median(ms_desc), statistics.median(ms_q1)
    return {
        "what": "GROUP BY (returnflag, linestatus) WHERE shipdate <= cutoff, "
                "COUNT(*) + SUM(price): k_groupby_desc (ms_kernel) against "
                "gx_q1's k_q1_agg (ms_out), same table, alternated",
        "sf": sf, "rows": n, "rows_pass": st["rows_pass"],
        "rows_lds": st["rows_lds"], "rows_global": st["rows_global"],
        "runs": args.runs, "warmup": args.warmup,
        "ms_groupby_desc": summary(ms_desc), "ms_q1": summary(ms_q1),
        "ratio_desc_over_q1": md / mq,
        "bytes_per_row": {"groupby_desc": 14, "q1": 22},
        "tb_per_s": {"groupby_desc": 14 * n / md / 1e9, "q1": 22 * n / mq / 1e9},
        "stream_ceiling_tb_per_s": STREAM_TBS,
    }


def case_low_vs_parent(parent_root, sf, rounds):
    """`low` in fresh processes, the parent commit's tree and this one
    alternated; each child checks its result against gx_q1 before timing"""
    got = {"parent": [], "this": []}
    for r in range(rounds):
        for name, root in (("parent", parent_root), ("this", ROOT)):
            with tempfile.TemporaryDirectory() as tmp:
                f = os.path.join(tmp, "low.json")
                subprocess.run(
                    [sys.executable, os.path.join(root, "tools", "gb_desc_time.py"),
                     "--cases", "low", "--sf", str(sf), "--runs", str(args.runs),
                     "--warmup", str(args.warmup), "--out", f],
                    check=True, cwd=root, stdout=subprocess.DEVNULL, timeout=300)
                with open(f) as fh:
                    low = json.load(fh)["low_cardinality"]
            got[name].append({k: low[k] for k in ("ms_groupby_desc", "ms_q1")})
            print(f"low: round {r} {name} "
                  f"{low['ms_groupby_desc']['median']:.3f} ms", flush=True)
    meds = {k: [x["ms_groupby_desc"]["median"] for x in v] for k, v in got.items()}
    return {
        "what": "case `low` (k_groupby_desc without expressions), one fresh "
                "process per round from the parent commit's build and from "
                "this one, alternated; ms_kernel median of each process",
        "sf": sf, "rounds": rounds, "runs": args.runs, "warmup": args.warmup,
        "parent": got["parent"], "this": got["this"],
        "ms_parent": summary(meds["parent"]), "ms_this": summary(meds["this"]),
        "every_new_above_every_parent": min(meds["this"]) > max(meds["parent"]),
    }


Q1REV_AGGS = [("count*", None), ("sum", 2, True), ("sum", [2, ("1-", 3)])]


def q1_expr(ctx, t):
    return ctx.groupby_expr(t, [0, 1], Q1REV_AGGS,
                            quals=[(4, "<=", gx.CUTOFF_19950315)], stats=True)


def case_q1rev(ctx, sf):
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, sf)
    n = t.nrows
    q1 = ctx.q1(t, gx.CUTOFF_19950315)
    res, st = q1_expr(ctx, t)
    check_q1(res, q1)
    want = np.nonzero(q1["count"])[0]
    np.testing.assert_allclose(res["aggs"][2], q1["sum_revenue"][want], rtol=1e-6)
    check_q1(q1_desc(ctx, t)[0], q1)
    print(f"q1rev: sf {sf}, {n} rows, results agree with gx_q1", flush=True)
    for _ in range(args.warmup):
        ctx.q1(t, gx.CUTOFF_19950315)
        q1_desc(ctx, t)
        q1_expr(ctx, t)
    ms_q1, ms_desc, ms_expr = [], [], []
    for _ in range(args.runs):                  # alternated
        ms_q1.append(ctx.q1(t, gx.CUTOFF_19950315)["ms"])
        ms_desc.append(q1_desc(ctx, t)[1]["ms_kernel"])
        ms_expr.append(q1_expr(ctx, t)[1]["ms_kernel"])
    t.free()
    me, md, mq = (statistics.median(x) for x in (ms_expr, ms_desc, ms_q1))
    return {
        "what": "GROUP BY (returnflag, linestatus) WHERE shipdate <= cutoff, "
                "COUNT(*) + SUM(price) + SUM(price * (1 - disc)): "
                "gx_groupby_expr (ms_kernel) against gx_q1's k_q1_agg (ms_out) "
                "and against gx_groupby_desc's COUNT(*) + SUM(price), same "
                "table, alternated",
        "sf": sf, "rows": n, "rows_pass": st["rows_pass"],
        "rows_lds": st["rows_lds"], "rows_global": st["rows_global"],
        "runs": args.runs, "warmup": args.warmup,
        "ms_groupby_expr": summary(ms_expr), "ms_groupby_desc": summary(ms_desc),
        "ms_q1": summary(ms_q1),
        "ratio_expr_over_q1": me / mq, "ratio_desc_over_q1": md / mq,
        "ratio_expr_over_desc": me / md,
        "bytes_per_row": {"groupby_expr": 22, "groupby_desc": 14, "q1": 22},
        "tb_per_s": {"groupby_expr": 22 * n / me / 1e9,
                     "groupby_desc": 14 * n / md / 1e9, "q1": 22 * n / mq / 1e9},
        "stream_ceiling_tb_per_s": STREAM_TBS,
    }


def case_lds0(ctx, sf):
    t = ctx.tpch_gen(gx.TPCH_LINEITEM_Q1, sf)
    n = t.nrows
    q1 = ctx.q1(t, gx.CUTOFF_19950315)
    on, st_on = q1_desc(ctx, t)
    off, st_off = q1_desc(ctx, t, lds=False)
    check_q1(on, q1)
    check_q1(off, q1)
    assert st_off["rows_lds"] == 0 and st_on["rows_global"] == 0
    print(f"lds0: sf {sf}, {n} rows, both agree with gx_q1", flush=True)
    ms_on, ms_off = [], []
    for i in range(args.warmup + args.runs):    # alternated
        a = q1_desc(ctx, t)[1]["ms_kernel"]
        b = q1_desc(ctx, t, lds=False)[1]["ms_kernel"]
        if i >= args.warmup:
            ms_on.append(a)
            ms_off.append(b)
    t.free()
    return {
        "what": "the low-cardinality query with the LDS stage (default) and "
                "with GX_GB_LDS=0 (every row's atomics on six global slots)",
        "sf": sf, "rows": n, "runs": args.runs, "warmup": args.warmup,
        "ms_lds_on": summary(ms_on), "ms_lds_off": summary(ms_off),
        "ratio_off_over_on": statistics.median(ms_off) / statistics.median(ms_on),
    }


def case_high(ctx, nrows, nkeys):
    from oracle import pyapi as orc
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

    def desc(lds, max_groups=0, giveup=None):
        set_lds(lds)
        if giveup is not None:
            os.environ["GX_GB_GIVEUP_ROWS"] = str(giveup)
        try:
            return ctx.groupby_desc(t, [0], aggs, max_groups=max_groups, stats=True)
        finally:
            set_lds(True)
            os.environ.pop("GX_GB_GIVEUP_ROWS", None)

    old, old_st = ctx.groupby_dist(t, 0, 1, stats=True)     # one-stage plan
    ng = len(old["key"])
    for lds in (True, False):
        res, st = desc(lds)
        assert res["ngroups"] == ng and (res["keys"][:, 0] == old["key"]).all()
        assert (res["aggs"][1] == old["count"]).all()
        assert res["aggs"][0].tobytes() == old["sum"].tobytes(), "sums differ"
    res, _ = desc(True, max_groups=ng)
    assert res["aggs"][0].tobytes() == old["sum"].tobytes()
    print(f"high: {ng} groups, results identical to gx_groupby", flush=True)
    del res, old
    ms = {"old": [], "on": [], "off": [], "on_bound": [], "on_never": [],
          "on_1024": []}
    lds_rows = {}
    for i in range(args.warmup + args.runs):    # alternated
        got = {"old": ctx.groupby_dist(t, 0, 1, stats=True)[1]["ms_partial"]}
        for name, (lds, mg, gu) in (("on", (True, 0, None)),
                                    ("off", (False, 0, None)),
                                    ("on_bound", (True, ng, None)),
                                    ("on_never", (True, 0, 0)),
                                    ("on_1024", (True, 0, 1024))):
            st = desc(lds, mg, gu)[1]
            got[name] = st["ms_kernel"]
            lds_rows[name] = st["rows_lds"]
        if i >= args.warmup:
            for k, v in got.items():
                ms[k].append(v)
        print(f"high: pass {i} {got}", flush=True)
    t.free()
    med = {k: statistics.median(v) for k, v in ms.items()}
    words = 3                                   # sum, its input count, count(*)
    return {
        "what": "one int64 key, SUM(float8) + COUNT(*): k_groupby_desc "
                "(ms_kernel, scan kernel alone) with the LDS stage on and "
                "off, against the one-stage gx_groupby (ms_partial = table "
                "clear + k_groupby + extract), same table, alternated",
        "rows": nrows, "distinct_keys_requested": nkeys, "groups": ng,
        "runs": args.runs, "warmup": args.warmup,
        "ms_groupby_one_stage_partial": summary(ms["old"]),
        "ms_groupby_desc_lds_on": summary(ms["on"]),
        "ms_groupby_desc_lds_off": summary(ms["off"]),
        "ms_groupby_desc_lds_on_max_groups_true": summary(ms["on_bound"]),
        "ms_groupby_desc_lds_on_never_give_up": summary(ms["on_never"]),
        "ms_groupby_desc_lds_on_give_up_after_1024": summary(ms["on_1024"]),
        "rows_lds": lds_rows,
        "ratio_lds_on_over_one_stage": med["on"] / med["old"],
        "ratio_lds_off_over_one_stage": med["off"] / med["old"],
        "ratio_lds_on_over_off": med["on"] / med["off"],
        "table_bytes": {
            "groupby_desc_bound_nrows": slots_pow2(2 * nrows) * (4 + 8 * words),
            "groupby_desc_max_groups_true": slots_pow2(2 * ng) * (4 + 8 * words),
            "gx_groupby_2x_nrows": slots_pow2(2 * nrows) * 24,
        },
    }


path = os.path.abspath(args.out)
out = {}
if os.path.exists(path):
    with open(path) as f:
        out = json.load(f)
ctx = None
for case in CASES:
    if case == "low" and args.parent_root:      # children only: no context here
        out["low_cardinality_vs_parent"] = case_low_vs_parent(
            os.path.abspath(args.parent_root), args.sf, args.rounds)
    else:
        ctx = ctx or gx.Context(device=0, seg=0, nsegs=1)
    if case == "low" and args.parent_root:
        pass
    elif case == "low":
        out["low_cardinality"] = case_low(ctx, args.sf)
    elif case == "q1rev":
        out["q1_revenue"] = case_q1rev(ctx, args.sf)
    elif case == "lds0":
        out["low_cardinality_lds_off"] = case_lds0(ctx, args.lds0_sf)
    elif case == "high":
        out["high_cardinality"] = case_high(ctx, int(args.rows), int(args.keys))
    else:
        raise SystemExit(f"unknown case {case}")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out), flush=True)
if ctx:
    ctx.close()

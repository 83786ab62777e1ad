#!/usr/bin/env python3
"""Kernel timing of the descriptor GROUP BY over a join (gx_groupby_join) on
ONE GPU against the two paths that bracket it, each on the same bound tables
in the same process, variants alternated, results compared before anything is
timed.  Recorded, not gated.

  q3ish  the generated TPC-H tables at --sf:
           lineitem JOIN orders ON l_orderkey = o_orderkey
           WHERE o_orderdate < cutoff AND l_shipdate > cutoff
           GROUP BY o_shippriority, COUNT(*), SUM(price * (1 - disc))
         through gx_groupby_join (ms_build + ms_kernel), beside
         - gx_q3_run's ms_orders_build + ms_probe_agg on the same tables with
           a customer filter that passes every row: the hand-specialised join
           over the same columns (it groups by the join key, so it also keeps
           one slot per order), and
         - gx_groupby_expr with the same aggregates and the same lineitem qual
           over lineitem alone (one group): the scan floor.
         Before timing: the COUNT(*) total equals Q3's probe_hits and the
         revenue total the sum of Q3's group revenues to 1e-6 relative.

    python tools/gb_join_time.py [--sf S] [--runs R] [--out F]

The case updates its own key of the JSON file.  The parent-versus-this
comparison of the join-free scan kernel is tools/gb_desc_time.py --cases low
--parent-root DIR --out <the same file>."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cloudberry_amd as gx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sf", type=float, default=10.0)
ap.add_argument("--runs", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupby_join.json"))
args = ap.parse_args()
assert args.runs >= 5, "report the median of at least 5 runs"

CUT = gx.CUTOFF_19950315
AGGS = [("count*", None), ("sum", [1, ("1-", 2)])]
LI_QUALS = [(3, ">", CUT)]


def summary(xs):
    xs = [float(x) for x in xs]
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs),
            "all": xs}


def case_q3ish(ctx, sf):
    cust = ctx.tpch_gen(gx.TPCH_CUSTOMER, sf)
    ordr = ctx.tpch_gen(gx.TPCH_ORDERS, sf)
    li = ctx.tpch_gen(gx.TPCH_LINEITEM, sf)
    q3 = ctx.q3_desc({"dim": cust, "dim_key_col": 0, "dim_filter": (1, ">=", 0),
                      "mid": ordr, "mid_key_col": 0, "mid_fk_col": 1,
                      "mid_attr1_col": 2, "mid_attr2_col": 3,
                      "mid_filter": (2, "<", CUT),
                      "fact": li, "fact_key_col": 0, "fact_a_col": 1,
                      "fact_b_col": 2, "fact_filter": (3, ">", CUT)})

    def join():
        return ctx.groupby_join(li, [gx.DimCol(0, 3)], AGGS,
                                [(ordr, 0, 0, [(2, "<", CUT)])], quals=LI_QUALS,
                                stats=True)

    def floor():
        return ctx.groupby_expr(li, [], AGGS, quals=LI_QUALS, stats=True)

    def q3_ms():
        st = q3.run().stats()
        return st["ms_orders_build"] + st["ms_probe_agg"], st

    _, q3st = q3_ms()
    groups = q3.result()
    res, st = join()
    assert int(res["aggs"][0].sum()) == q3st["probe_hits"], "joined rows differ from Q3"
    np.testing.assert_allclose(res["aggs"][1].sum(), groups["revenue"].sum(), rtol=1e-6)
    assert st["rows_pass"] == q3st["probe_hits"]
    fl, fst = floor()
    assert fst["rows_pass"] == st["rows_probed"]
    print(f"q3ish: sf {sf}, {li.nrows} lineitem rows, {st['dim_rows'][0]} orders in "
          f"the join table, {st['rows_pass']} joined rows, {res['ngroups']} groups; "
          f"totals agree with gx_q3_run", flush=True)
    del groups
    for _ in range(args.warmup):
        q3_ms()
        join()
        floor()
    ms_q3, ms_q3_build, ms_join, ms_join_build, ms_join_kernel, ms_floor = ([] for _ in range(6))
    for _ in range(args.runs):                  # alternated
        m, s = q3_ms()
        ms_q3.append(m)
        ms_q3_build.append(s["ms_orders_build"])
        s = join()[1]
        ms_join.append(s["ms_build"] + s["ms_kernel"])
        ms_join_build.append(s["ms_build"])
        ms_join_kernel.append(s["ms_kernel"])
        ms_floor.append(floor()[1]["ms_kernel"])
    table_mode = q3.table_mode()
    out = {
        "what": "lineitem JOIN orders ON l_orderkey = o_orderkey WHERE o_orderdate "
                "< cutoff AND l_shipdate > cutoff GROUP BY o_shippriority, COUNT(*), "
                "SUM(price * (1 - disc)): gx_groupby_join (ms_build + ms_kernel) "
                "against gx_q3_run (ms_orders_build + ms_probe_agg, customer filter "
                "passing every row) and against gx_groupby_expr over lineitem alone "
                "(ms_kernel), same tables, alternated",
        "sf": sf, "lineitem_rows": li.nrows, "orders_rows": ordr.nrows,
        "join_table_rows": st["dim_rows"][0], "rows_probed": st["rows_probed"],
        "rows_joined": st["rows_pass"], "groups": res["ngroups"],
        "q3_groups": q3st["groups"], "q3_table_mode": table_mode,
        "runs": args.runs, "warmup": args.warmup,
        "ms_groupby_join": summary(ms_join),
        "ms_groupby_join_build": summary(ms_join_build),
        "ms_groupby_join_kernel": summary(ms_join_kernel),
        "ms_q3_build_plus_probe": summary(ms_q3),
        "ms_q3_orders_build": summary(ms_q3_build),
        "ms_groupby_expr_scan_floor": summary(ms_floor),
        "ratio_join_over_q3": statistics.median(ms_join) / statistics.median(ms_q3),
        "ratio_join_kernel_over_floor":
            statistics.median(ms_join_kernel) / statistics.median(ms_floor),
    }
    q3.free()
    for t in (li, ordr, cust):
        t.free()
    return out


path = os.path.abspath(args.out)
out = {}
if os.path.exists(path):
    with open(path) as f:
        out = json.load(f)
ctx = gx.Context(device=0, seg=0, nsegs=1)
out["q3ish"] = case_q3ish(ctx, args.sf)
ctx.close()
os.makedirs(os.path.dirname(path), exist_ok=True)
with open(path, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out), flush=True)

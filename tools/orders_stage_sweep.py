#!/usr/bin/env python3
"""Sweep the two forms of the rank-form orders stage (GX_ORDERS_STAGED=0
two-pass, =1 staged) over the selectivity of the mid table at SF100: the
threshold K of the rule `staged iff qual * K <= nrows` sits where the staged
form stops winning.  The selectivity moves with the date literal and the
anti join: ~0 % (ends in the hash form: skipped), ~7 %, the default ~10 %,
all dates ~20 %, anti + default ~40 %, anti + all dates ~80 %.  AB_POINTS
picks points by name.  At each point the staged form also runs with the
filter grid of the two-pass form (32768 blocks) instead of the one sized from
the selectivity.  Prints one JSON line at the end."""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import cloudberry_amd as gx  # noqa: E402

SF = float(os.environ.get("AB_SF", "100"))
REPS = int(os.environ.get("AB_REPS", "8"))
POINTS = [                       # name, mid date literal (o_orderdate < lit), dim join
    # ~0 % is no rank-form run: the rank table needs key range <= 64 x
    # qualifying rows, which TPC-H orderkeys meet only above 6.3 %; a point
    # that ends in the hash form is reported as skipped
    ("near0", -2920, "semi"),    # one day of orders
    ("low", -2079, "semi"),      # 35 % of the dates x 20 %: ~7 %
    ("default", gx.CUTOFF_19950315, "semi"),
    ("all_dates", 0, "semi"),
    ("anti_default", gx.CUTOFF_19950315, "anti"),
    ("anti_all_dates", 0, "anti"),
]


def main():
    ctx = gx.Context(device=0, seg=0, nsegs=1)
    cust = ctx.tpch_gen(gx.TPCH_CUSTOMER, SF)
    ordr = ctx.tpch_gen(gx.TPCH_ORDERS, SF)
    li = ctx.tpch_gen(gx.TPCH_LINEITEM, SF)
    nrows = ordr.nrows
    only = os.environ.get("AB_POINTS")
    out = {"sf": SF, "reps": REPS, "mid_rows": nrows, "K": gx.orders_stage_k(),
           "points": []}
    for name, lit, join in POINTS:
        if only and name not in only.split(","):
            continue
        desc = {"dim": cust, "dim_key_col": 0, "dim_filter": (1, "==", 0),
                "mid": ordr, "mid_key_col": 0, "mid_fk_col": 1,
                "mid_attr1_col": 2, "mid_attr2_col": 3,
                "mid_filter": (2, "<", lit),
                "fact": li, "fact_key_col": 0, "fact_a_col": 1, "fact_b_col": 2,
                "fact_filter": (3, ">", gx.CUTOFF_19950315),
                "dim_join": join}
        row = {"point": name, "literal": lit, "dim_join": join}
        groups = None
        for label, env, grid in (("two_pass", "0", 0), ("staged", "1", 0),
                                 ("staged_grid32768", "1", 32768)):
            os.environ["GX_ORDERS_STAGED"] = env
            q = ctx.q3_desc(desc)
            q._test_set_orders_grid(grid)
            ms = []
            q.run()
            if q.table_mode() != 1:           # nothing qualifies: hash form
                row["skipped"] = "no rank-form run at this literal"
                q.free()
                break
            for _ in range(REPS + 1):
                q.run()
                ms.append(q.stats()["ms_orders_build"])
            ms = ms[1:]                       # the first run allocates
            st = q.stats()
            assert q.table_mode() == 1 and q.orders_mode() == int(env)
            if groups is None:
                groups = st["groups"]
                row["groups"] = groups
            assert st["groups"] == groups, (name, label, st["groups"], groups)
            row[label] = {"ms_orders_build_min": round(min(ms), 3),
                          "ms_orders_build_median": round(statistics.median(ms), 3)}
            if env == "1":
                blocks, flushes, recs = q.orders_stage_claims()
                row[label].update(blocks=blocks, midloop_flushes=flushes)
                row["qualifying_rows"] = recs
                row["selectivity"] = round(recs / nrows, 4)
            q.free()
            print(name, label, row[label], flush=True)
        out["points"].append(row)
    os.environ.pop("GX_ORDERS_STAGED", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""PMC side-run for bench.py's roofline.traffic.

Runs a short Q3 bench under `rocprofv3 --pmc FETCH_SIZE` (counters-only —
never combined with trace domains, per the pool rule), parses the counter
CSV, and returns the corrected HBM read bytes per dominant-kernel launch:

    traffic = FETCH_SIZE_KB * 1024 * 2

The x2 is the documented gfx950 correction (MI355X_MICROARCH.md §HBM:
FETCH_SIZE tallies 128-B requests at 64 B for wide coalesced streams; the
r1 calibration on this kernel's mix is in profiles/rocprof_r01_q3_sf100.txt
— 6.38 GB counted vs 16.8 GB algorithmic with the u32 probe table largely
served from Infinity Cache, i.e. ~12.8 GB corrected DRAM-side reads).

Fail-soft by design: any error returns None and the bench line carries
traffic: null.
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile


def probe_kernel_fetch_bytes(sf, steps=2, timeout=480):
    """Return (corrected_bytes_per_launch, raw_kb, ndispatch) for the
    lineitem probe kernel, or None."""
    rocprof = "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(rocprof):
        return None
    bench = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "bench.py")
    outdir = tempfile.mkdtemp(prefix="gxpmc_", dir="/tmp")
    env = dict(os.environ)
    env["TMPDIR"] = "/tmp"
    cmd = [rocprof, "--pmc", "FETCH_SIZE", "--output-format", "csv",
           "-d", outdir, "-o", "t",
           "--", sys.executable, bench, "--steps", str(steps),
           "--warmup", "1", "--sf", str(sf),
           "--no-cpu-baseline", "--no-traffic"]
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, timeout=timeout,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       check=True)
    except Exception:
        return None
    files = glob.glob(os.path.join(outdir, "**", "*counter_collection.csv"),
                      recursive=True)
    if not files:
        return None
    total_kb, n = 0.0, 0
    try:
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                kname = row.get("Kernel_Name", "")
                cname = row.get("Counter_Name", "")
                if "k_li_probe_agg" in kname and cname == "FETCH_SIZE":
                    total_kb += float(row.get("Counter_Value", 0))
                    n += 1
    except Exception:
        return None
    if n == 0:
        return None
    kb_per_launch = total_kb / n
    return (kb_per_launch * 1024.0 * 2.0, kb_per_launch, n)


if __name__ == "__main__":
    print(probe_kernel_fetch_bytes(float(sys.argv[1]) if len(sys.argv) > 1
                                   else 100.0))

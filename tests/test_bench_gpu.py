"""bench.py end to end on the GPU at a tiny SF: the result line's contract
fields and --dump-outputs (what the timed path computed, checked against
the oracle on the same seeded inputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SF = 0.01


def _bench(outdir):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"),
                        "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--sf", str(SF), "--dump-outputs", str(outdir)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_line_and_dump_outputs(tmp_path):
    from oracle import pyapi as orc
    out = _bench(tmp_path / "a")
    assert out["metric"] == "tpch_q3_rows_per_sec" and out["unit"] == "rows/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    # value = rows / step time; ms_per_step is printed rounded to 0.001 ms
    assert out["value"] == pytest.approx(
        out["config"]["lineitem_rows"] / (out["ms_per_step"] / 1e3),
        rel=0.0006 / out["ms_per_step"] + 1e-6)
    # a plain run leaves the --full legs out
    assert out["cpu_baseline"] is None
    assert out["roofline"]["traffic"] is None
    assert out["config"]["scan_filter_kernel_gbps"] is None

    got = {f[:-4]: np.load(tmp_path / "a" / f)
           for f in os.listdir(tmp_path / "a")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 * 2**20
    want = orc.q3(orc.gen_customer(SF), orc.gen_orders(SF), orc.gen_lineitem(SF))
    n = len(want["l_orderkey"])
    assert got["ngroups"][0] == n == out["config"]["groups"]
    np.testing.assert_array_equal(got["sample_index"], np.arange(n))
    for f in ("l_orderkey", "o_orderdate", "o_shippriority", "nitems"):
        np.testing.assert_array_equal(got[f], want[f].astype(np.float64))
    np.testing.assert_allclose(got["revenue"], want["revenue"], rtol=1e-9)

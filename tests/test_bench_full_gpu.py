"""bench.py --full: a plain run prints the result line's own fields and measures nothing else; --full adds the measurements
that take runs of their own (here the CPU baseline, the cheapest of them at config c1)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = ("roofline", "roofline_kernels", "roofline_symbols", "roofline_family", "roofline_step", "roofline_isolated",
         "roofline_pool", "cpu_baseline", "extra_points")


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", "2", "--warmup", "1", *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_plain_run_measures_only_the_result_line_and_full_adds_the_rest():
    plain = _bench()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in plain, k
    assert plain["value"] > 0 and plain["steps"] == 2 and plain["higher_is_better"] is True
    assert not [k for k in EXTRA if k in plain]
    full = _bench("--full", "--no-roofline")
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["unit"] == "encoder frames/s"
    assert not [k for k in EXTRA if k in full and k != "cpu_baseline"]

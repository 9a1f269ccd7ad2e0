"""bench.py --dump-outputs: what the timed steps computed, written after the last of them.  The same arguments give the same
inputs, so two runs dump the same bits; --steps sets how many steps ran before the dump."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, steps):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", str(steps), "--warmup", "1",
                        "--no-cpu-baseline", "--no-roofline", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["steps"] == steps
    return {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}


def test_dump_outputs_of_the_training_step(tmp_path):
    a, b, c = _bench(tmp_path / "a", 2), _bench(tmp_path / "b", 2), _bench(tmp_path / "c", 3)
    assert sorted(a) == ["encoder_out", "gradients", "parameters"]
    assert a["encoder_out"].shape == (2, 50, 144)                     # config c1: B = 2 utterances of T = 50 frames, d_model 144
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all()
        assert np.array_equal(a[k], b[k]), f"{k}: two runs of one command differ"
    assert not np.array_equal(a["parameters"], c["parameters"]), "a third timed step did not move the dumped weights"

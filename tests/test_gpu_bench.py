"""bench.py end to end on the device, at a small batch: a plain run prints one JSON line with the
headline fields and nothing that belongs to --full, --steps sets the timed steps, and
--dump-outputs writes the last step's arrays, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"loss", "params", "bn_buffers", "grads", "adam_exp_avg", "adam_exp_avg_sq"}


def _run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", "192", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {n: np.load(os.path.join(out_dir, n + ".npy")) for n in NAMES}


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    d, a = _run(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False and d["higher_is_better"] is True
    assert d["unit"] == "trials/s" and d["dtype"] == "fp32" and d["n_gpus"] == 1
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(192 / (d["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("roofline", "cpu_baseline", "cfg4_dp", "cfg5_train", "cfg5_infer_bf16", "cfg2_eval_fp32",
              "real_protocol_folds"):
        assert d[k] is None
    assert d["kernels"] == {}
    assert {os.path.splitext(f)[0] for f in os.listdir(tmp_path / "a")} == NAMES
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["params"].shape == a["grads"].shape == a["adam_exp_avg"].shape == a["adam_exp_avg_sq"].shape
    assert float(a["loss"][0]) == pytest.approx(d["final_loss"], abs=1e-5)
    assert np.abs(a["grads"]).max() > 0 and np.abs(a["adam_exp_avg_sq"]).max() > 0
    _, b = _run(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n

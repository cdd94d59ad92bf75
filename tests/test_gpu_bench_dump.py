"""bench.py --dump-outputs on the device.  The step before the dumped one restarts from the run's initial state, so the dump
depends on the arguments alone: on the ordered-reduction build (DWN_DETERMINISTIC=1) bit for bit, whatever --steps / --warmup
came before the restore; on the normal build up to the rounding of its float atomics (one backward + AdamW step of them, then
the dumped forward)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
# normal build, two runs: relative L2 of the predictions 4.4e-3 ... 5.9e-3 and of the loss 0.9e-4 ... 2.7e-4 measured (B=32 T=32
# 36x64 bf16); the dumped step's one backward + AdamW step moves the loss by ~36 % from the initial forward's, so a broken
# backward or optimizer kernel stands far outside these bounds
PRED_BOUND, LOSS_BOUND = 2e-2, 1e-3


def _dump(tmp, name, steps, warmup, deterministic):
    env = dict(os.environ, DWN_DETERMINISTIC="1" if deterministic else "0")
    env.pop("DWN_LIB_PATH", None)
    out = tmp / name
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out)], cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == steps and line["warmup"] == warmup
    return {p.stem: np.load(p) for p in sorted(out.glob("*.npy"))}


def _rel(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(a))


def test_deterministic_build_dump_is_fixed_by_the_arguments(tmp_path):
    a = _dump(tmp_path, "a", 3, 1, True)
    b = _dump(tmp_path, "b", 2, 0, True)
    assert sorted(a) == ["loss", "prediction_0"] and a["prediction_0"].shape == (32, 7863, 32)
    assert a["loss"].dtype == np.float64 and a["prediction_0"].dtype == np.float32
    assert np.isfinite(a["prediction_0"]).all()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_normal_build_dumps_agree_between_runs(tmp_path):
    a = _dump(tmp_path, "a", 2, 0, False)
    b = _dump(tmp_path, "b", 2, 0, False)
    c = _dump(tmp_path, "c", 6, 2, False)
    rb, rc = _rel(a["prediction_0"], b["prediction_0"]), _rel(a["prediction_0"], c["prediction_0"])
    lb, lc = _rel(a["loss"], b["loss"]), _rel(a["loss"], c["loss"])
    print(f"normal build, dump noise: predictions {rb:.2e} / {rc:.2e}, loss {lb:.2e} / {lc:.2e}")
    assert max(rb, rc) < PRED_BOUND and max(lb, lc) < LOSS_BOUND

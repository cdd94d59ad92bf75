"""Determinism of the parametric-fit kernels: they use no atomic, every sum is closed by a fixed butterfly
and every decision is taken on bits all lanes share, so two runs in this process give the same bits, and a fresh child process on
the ordered-reduction build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) gives THE SAME BITS as the product library here — the
params, table and start vectors of three grids through a row table and with other options, and their profiles, compared through one
digest."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
TENSORS = 24


def test_two_runs_give_the_same_bits():
    from tests.test_gpu_rf_fit import rf_fit_digest
    a, b = rf_fit_digest(), rf_fit_digest()
    print(f"run 1: tensors={a[0]} digest={a[1]}\nrun 2: tensors={b[0]} digest={b[1]}")
    assert a == b and a[0] == TENSORS


def test_deterministic_build_gives_the_bits_of_the_product_build():
    import sensorium_amd._lib as L
    from tests.test_gpu_rf_fit import rf_fit_digest
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    assert L.LIB_PATH.name == "libdwiseneuro_hip.so" or os.environ.get("DWN_LIB_PATH") or L.DETERMINISTIC
    tensors, digest = rf_fit_digest()
    env = dict(os.environ, DWN_DETERMINISTIC="1")
    env.pop("DWN_LIB_PATH", None)
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "det_rf_fit_worker.py")], cwd=str(ROOT), env=env, capture_output=True,
                         text=True, timeout=300)
    m = re.search(r"DET_RF_FIT deterministic=(\d) lib=(\S+) tensors=(\d+) digest=([0-9a-f]{64})", res.stdout)
    assert res.returncode == 0 and m, res.stdout[-2000:] + res.stderr[-3000:]
    print(m.group(0))
    print(f"this process ({L.LIB_PATH.name}): tensors={tensors} digest={digest}")
    assert m.group(1) == "1" and m.group(2) == "libdwiseneuro_hip_det.so"
    assert int(m.group(3)) == tensors == TENSORS
    assert m.group(4) == digest, "the deterministic build and the product build disagree in at least one bit"

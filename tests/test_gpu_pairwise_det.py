"""The ordered-reduction build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) on the population-structure kernels: they use no
atomic and no grid that depends on the build, so a fresh child process on the deterministic library must produce THE SAME BITS as
the product library in this process — states, matrices and comparison of the fixed cases of tests/test_gpu_pairwise.py, compared
through one digest."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_deterministic_build_gives_the_bits_of_the_product_build():
    import sensorium_amd._lib as L
    from tests.test_gpu_pairwise import pairwise_digest
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    assert L.LIB_PATH.name == "libdwiseneuro_hip.so" or os.environ.get("DWN_LIB_PATH") or L.DETERMINISTIC
    tensors, digest = pairwise_digest()
    env = dict(os.environ, DWN_DETERMINISTIC="1")
    env.pop("DWN_LIB_PATH", None)
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "det_pairwise_worker.py")], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=300)
    m = re.search(r"DET_PAIRWISE deterministic=(\d) lib=(\S+) tensors=(\d+) digest=([0-9a-f]{64})", res.stdout)
    assert res.returncode == 0 and m, res.stdout[-2000:] + res.stderr[-3000:]
    print(m.group(0))
    print(f"this process ({L.LIB_PATH.name}): tensors={tensors} digest={digest}")
    assert m.group(1) == "1" and m.group(2) == "libdwiseneuro_hip_det.so"
    assert int(m.group(3)) == tensors == 16
    assert m.group(4) == digest, "the deterministic build and the product build disagree in at least one bit"

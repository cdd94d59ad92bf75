"""The retinotopic-readout-gain kernels use no atomics and their grids depend on the geometry alone: the ordered-
reduction build (-DDWN_DETERMINISTIC) must return the very bits of the product build, launch after launch, on three shapes."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

from tests.test_gpu_spatial_gain import DIGEST_CASES, spatial_digest  # noqa: E402


def test_deterministic_build_gives_the_product_build_bits():
    import sensorium_amd._lib as L
    if L.DETERMINISTIC:
        pytest.skip("this process already runs the deterministic build")
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    digest, tensors, differing = spatial_digest()
    assert len(DIGEST_CASES) == 3 and tensors == 6 * len(DIGEST_CASES) and differing == 0
    env = dict(os.environ, DWN_DETERMINISTIC="1")
    env.pop("DWN_LIB_PATH", None)
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "det_spatial_worker.py")], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=300)
    m = re.search(r"DET_SPATIAL deterministic=(\d) lib=(\S+) digest=([0-9a-f]{64}) tensors=(\d+) differing=(\d+)", res.stdout)
    assert res.returncode == 0 and m, res.stdout[-2000:] + res.stderr[-3000:]
    print(m.group(0))
    assert m.group(1) == "1" and m.group(2) == "libdwiseneuro_hip_det.so"
    assert int(m.group(4)) == tensors and int(m.group(5)) == 0
    assert m.group(3) == digest

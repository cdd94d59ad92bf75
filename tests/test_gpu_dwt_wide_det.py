"""The ordered-reduction build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) on the temporal depth-wise kernels of size 7 and 9:
two launches of each direction on the same operands must agree BIT FOR BIT in every output, the atomically accumulated weight
gradient and BatchNorm sums included (the DET_* bracketing of the statistics and dW flushes in csrc/dwn_dwconv.hip) — the form of
tests/test_gpu_dws_ks_det.py."""
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_deterministic_build_repeats_kt7_kt9_kernels_bit_for_bit():
    env = dict(os.environ, DWN_DETERMINISTIC="1")
    env.pop("DWN_LIB_PATH", None)
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "det_dwt_wide_worker.py")], cwd=str(ROOT), env=env, capture_output=True,
                         text=True, timeout=600)
    m = re.search(r"DET_DWT_WIDE deterministic=(\d) lib=(\S+) tensors=(\d+) differing=(\d+)", res.stdout)
    assert res.returncode == 0 and m, res.stdout[-2000:] + res.stderr[-3000:]
    assert m.group(1) == "1" and m.group(2) == "libdwiseneuro_hip_det.so"
    assert int(m.group(3)) == 56          # 2 sizes x 2 shapes x 2 storage types x 7 tensors
    assert int(m.group(4)) == 0, f"{m.group(4)} of {m.group(3)} outputs differ between two launches of the deterministic build"

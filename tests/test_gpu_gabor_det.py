"""The ordered-reduction build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) on the drifting-Gabor kernels: they use no atomic and
no grid that depends on the build, so a fresh child process on the deterministic library must produce THE SAME BITS as the product
library in this process — out and dparams of the fixed cases of tests/test_gpu_gabor.py, compared through one digest."""
import os

import pytest

from tests.det_child import deterministic_child

pytestmark = pytest.mark.gpu


def test_deterministic_build_gives_the_bits_of_the_product_build():
    import sensorium_amd._lib as L
    from tests.test_gpu_gabor import DIGEST_CASES, gabor_digest
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    assert L.LIB_PATH.name == "libdwiseneuro_hip.so" or os.environ.get("DWN_LIB_PATH") or L.DETERMINISTIC
    tensors, digest = gabor_digest()
    deterministic, lib, (child_tensors, child_digest) = deterministic_child("tests.test_gpu_gabor:gabor_digest")
    print(f"this process ({L.LIB_PATH.name}): tensors={tensors} digest={digest}")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    assert child_tensors == tensors == 2 * len(DIGEST_CASES)
    assert child_digest == digest, "the deterministic build and the product build disagree in at least one bit"

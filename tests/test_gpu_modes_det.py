"""The ordered-reduction build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) on the population-modes kernels: they use no atomic
and no split that depends on the build, so a fresh child process on the deterministic library must produce THE SAME BITS as the
product library in this process, compared through one digest over the fixed cases of tests/test_gpu_modes.py."""
import os

import pytest

from tests.det_child import deterministic_child

pytestmark = pytest.mark.gpu


def test_deterministic_build_gives_the_bits_of_the_product_build():
    import sensorium_amd._lib as L
    from tests.test_gpu_modes import modes_digest
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    assert L.LIB_PATH.name == "libdwiseneuro_hip.so" or os.environ.get("DWN_LIB_PATH") or L.DETERMINISTIC
    tensors, digest = modes_digest()
    deterministic, lib, (child_tensors, child_digest) = deterministic_child("tests.test_gpu_modes:modes_digest")
    print(f"this process ({L.LIB_PATH.name}): tensors={tensors} digest={digest}")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    assert child_tensors == tensors == 27
    assert child_digest == digest, "the deterministic build and the product build disagree in at least one bit"

"""Determinism of the receptive-field kernels: they use no atomic and no grid that depends on the build
or on what the runtime reports, so two runs in this process give the same bits, and a fresh child process on the ordered-reduction
build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) gives THE SAME BITS as the product library here — the noise of every
geometry and kind of tests/test_gpu_rf.py and the state, cov, z and summary of two accumulator cases, compared through one digest."""
import os

import pytest

from tests.det_child import deterministic_child

pytestmark = pytest.mark.gpu


def test_two_runs_give_the_same_bits():
    from tests.test_gpu_rf import rf_digest
    a, b = rf_digest(), rf_digest()
    print(f"run 1: tensors={a[0]} digest={a[1]}\nrun 2: tensors={b[0]} digest={b[1]}")
    assert a == b and a[0] == 18


def test_deterministic_build_gives_the_bits_of_the_product_build():
    import sensorium_amd._lib as L
    from tests.test_gpu_rf import rf_digest
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    assert L.LIB_PATH.name == "libdwiseneuro_hip.so" or os.environ.get("DWN_LIB_PATH") or L.DETERMINISTIC
    tensors, digest = rf_digest()
    deterministic, lib, (child_tensors, child_digest) = deterministic_child("tests.test_gpu_rf:rf_digest")
    print(f"this process ({L.LIB_PATH.name}): tensors={tensors} digest={digest}")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    assert child_tensors == tensors == 18
    assert child_digest == digest, "the deterministic build and the product build disagree in at least one bit"

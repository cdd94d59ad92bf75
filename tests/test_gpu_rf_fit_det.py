"""Determinism of the parametric-fit kernels: they use no atomic, every sum is closed by a fixed butterfly
and every decision is taken on bits all lanes share, so two runs in this process give the same bits, and a fresh child process on
the ordered-reduction build (libdwiseneuro_hip_det.so, DWN_DETERMINISTIC=1) gives THE SAME BITS as the product library here — the
params, table and start vectors of three grids through a row table and with other options, and their profiles, compared through one
digest."""
import os

import pytest

from tests.det_child import deterministic_child

pytestmark = pytest.mark.gpu
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
    deterministic, lib, (child_tensors, child_digest) = deterministic_child("tests.test_gpu_rf_fit:rf_fit_digest")
    print(f"this process ({L.LIB_PATH.name}): tensors={tensors} digest={digest}")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    assert child_tensors == tensors == TENSORS
    assert child_digest == digest, "the deterministic build and the product build disagree in at least one bit"

"""The retinotopic-readout-gain kernels use no atomics and their grids depend on the geometry alone: the ordered-
reduction build (-DDWN_DETERMINISTIC) must return the very bits of the product build, launch after launch, on three shapes."""
import pytest

pytestmark = pytest.mark.gpu

from tests.det_child import deterministic_child  # noqa: E402
from tests.test_gpu_spatial_gain import DIGEST_CASES, spatial_digest  # noqa: E402


def test_deterministic_build_gives_the_product_build_bits():
    import sensorium_amd._lib as L
    if L.DETERMINISTIC:
        pytest.skip("this process already runs the deterministic build")
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    digest, tensors, differing = spatial_digest()
    assert len(DIGEST_CASES) == 3 and tensors == 6 * len(DIGEST_CASES) and differing == 0
    deterministic, lib, (child_digest, child_tensors, child_differing) = deterministic_child("tests.test_gpu_spatial_gain:spatial_digest")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    assert child_tensors == tensors and child_differing == 0
    assert child_digest == digest

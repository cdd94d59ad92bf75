"""Child process of tests/test_gpu_spatial_gain_det.py: the retinotopic-readout-gain kernels launched twice on fixed inputs with
whatever library DWN_DETERMINISTIC selects; prints a digest of every output and whether the two launches agreed bit for bit."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import sensorium_amd._lib as L  # noqa: E402
from tests.test_gpu_spatial_gain import spatial_digest  # noqa: E402


def main():
    digest, tensors, differing = spatial_digest()
    print(f"DET_SPATIAL deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} digest={digest} "
          f"tensors={tensors} differing={differing}")


if __name__ == "__main__":
    main()

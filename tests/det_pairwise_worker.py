"""Child process of tests/test_gpu_pairwise_det.py: the population-structure kernels on the fixed cases of
tests/test_gpu_pairwise.py with whatever library DWN_DETERMINISTIC selects; prints the digest of every output."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import sensorium_amd._lib as L  # noqa: E402
from tests.test_gpu_pairwise import pairwise_digest  # noqa: E402


def main():
    tensors, digest = pairwise_digest()
    print(f"DET_PAIRWISE deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} tensors={tensors} digest={digest}")


if __name__ == "__main__":
    main()

"""Child process of tests/test_gpu_modulator_det.py: the behaviour-modulator kernels launched twice on fixed inputs with whatever
library DWN_DETERMINISTIC selects; prints a digest of every output and whether the two launches agreed bit for bit."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import sensorium_amd._lib as L  # noqa: E402
from tests.test_gpu_modulator import modulator_digest  # noqa: E402


def main():
    digest, tensors, differing = modulator_digest()
    print(f"DET_MODULATOR deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} digest={digest} "
          f"tensors={tensors} differing={differing}")


if __name__ == "__main__":
    main()

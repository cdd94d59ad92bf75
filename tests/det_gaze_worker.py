"""Child process of tests/test_gpu_gaze_shift.py: the gaze-shift kernels and the plane mean launched twice on the same inputs with
whatever library DWN_DETERMINISTIC selects; prints whether every output came out bit for bit the same."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import sensorium_amd._lib as L  # noqa: E402
from tests.test_gpu_gaze_shift import repeat_report  # noqa: E402


def main():
    tensors, differing = repeat_report()
    print(f"DET_GAZE deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} tensors={tensors} "
          f"differing={differing}")


if __name__ == "__main__":
    main()

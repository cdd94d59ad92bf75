"""Child process of tests/test_gpu_model_mei.py: the bit-for-bit statements about most_exciting_input (plain path against its
verbatim copy, graph replay against the eager loop, five calls of one step against one call of five) with whatever library
DWN_DETERMINISTIC selects; prints one name=0/1 pair per statement."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401,E402

import sensorium_amd._lib as L  # noqa: E402
from tests.test_gpu_model_mei import bitwise_report  # noqa: E402


def main():
    report = bitwise_report()
    print(f"DET_MEI_MODEL deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} "
          + " ".join(f"{k}={int(v)}" for k, v in report.items()))


if __name__ == "__main__":
    main()

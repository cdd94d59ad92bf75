"""Child process of tests/test_gpu_dws_ks_det.py: the depth-wise spatial kernels of size 5 and 7 launched twice on the same operands
with whatever library DWN_DETERMINISTIC selects; prints whether every output — y2, dh1, and the atomically accumulated dW and
BatchNorm sums — came out bit for bit the same."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sensorium_amd._lib as L
from tests.test_gpu_dws_ks import BF, Case

F32 = torch.float32


def main():
    tensors = differing = 0
    for ks in (5, 7):
        for stride in (1, 2):
            for dtype in (BF, F32):
                case = Case(130, 9, 16, 200, stride, ks, dtype, seed=3)          # ragged slice; more planes than the resident grid
                runs = []
                for _ in range(2):
                    y2, st_f = case.forward()
                    dh1, dw, st_b = case.backward()
                    runs.append([y2.float(), st_f[0], st_f[1], dh1.float(), dw, st_b[0], st_b[1]])
                for a, b in zip(*runs):
                    tensors += 1
                    differing += 0 if torch.equal(a, b) else 1
    print(f"DET_DWS_KS deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} tensors={tensors} "
          f"differing={differing}")


if __name__ == "__main__":
    main()

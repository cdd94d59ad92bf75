"""Child process of tests/test_gpu_dwt_wide_det.py: the temporal depth-wise kernels of size 7 and 9 launched twice on the same operands
with whatever library DWN_DETERMINISTIC selects; prints whether every output — y3, dh2, and the atomically accumulated dW and
BatchNorm sums — came out bit for bit the same."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import sensorium_amd._lib as L
from tests.test_gpu_dwt_wide import BF, F32, WideCase


def main():
    tensors = differing = 0
    for kt in (7, 9):
        for shape in ((2, 13, 35, 72), (3, 9, 576, 72)):      # ragged slice, T off the batch; more positions than one grid stride
            for dtype in (BF, F32):
                case = WideCase(*shape, kt, dtype, seed=3)
                runs = []
                for _ in range(2):
                    y3, st_f = case.forward()
                    dh2, dw, st_b = case.backward()
                    runs.append([y3.float(), st_f[0], st_f[1], dh2.float(), dw, st_b[0], st_b[1]])
                for a, b in zip(*runs):
                    tensors += 1
                    differing += 0 if torch.equal(a, b) else 1
    print(f"DET_DWT_WIDE deterministic={os.environ.get('DWN_DETERMINISTIC', '0')} lib={L.LIB_PATH.name} tensors={tensors} "
          f"differing={differing}")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Host answers of the block composite, one line per argument set (development tool; no device needed).

Replays the grid of tests/test_host_block_plan.py plus ragged and refused arguments and prints, for each, the forward and
backward dwn_block_workspace_bytes, dwn_block_forward_writes and the (rc, message) of dwn_block_backward's device-free checks.
Run once per library (DWN_LIB_PATH, DWN_DETERMINISTIC) and `diff` the outputs: a host-only change of csrc/dwn_api.hip leaves no
differing line.

usage: block_plan_replay.py > answers.txt
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sensorium_amd._lib as L
from tests.test_host_block_plan import answers, block_args, grid


def backward_check(a):
    """dwn_block_backward answers its argument checks before it enters a device; an argument set that passes them is reported as
    such, not by what the device (or its absence) answers next"""
    rc = L.lib.dwn_block_backward(C.byref(a), 0, None)
    refused = rc in (-2, -4, -7) and b"block" in L.lib.dwn_last_error()
    return (rc, L.lib.dwn_last_error().decode()) if refused else ("passed", "")


def line(tag, a):
    fields = "dtype training B T Hin Win Hout Wout Cin Cmid Cout stride ks kt se_r y1_mode pwl_bwd".split()
    return f"{tag} {' '.join(str(getattr(a, f)) for f in fields)} -> {answers(L, a)} {backward_check(a)}"


def main():
    n = 0
    for case, dtype, mode, y1_mode, pwl_bwd in grid():
        print(line("grid", block_args(L, case, dtype, mode, y1_mode, pwl_bwd)))
        n += 1
    base = (64, 64, 1, 7, 32, 2, 4, 8, 16)
    for dtype in (L.DWN_F32, L.DWN_BF16):
        for mode in (L.BN_EVAL, L.BN_TRAIN, L.BN_FROZEN):
            def odd(**kw):
                a = block_args(L, base, dtype, mode)
                for k, v in kw.items():
                    setattr(a, k, v)
                return a
            ragged = [odd(Cin=60), odd(Cmid=452), odd(Cout=68), odd(Cin=12, Cmid=36, Cout=20), odd(Cin=72, Cmid=504, Cout=72)]
            ragged += [odd(ks=k) for k in (1, 2, 4, 5, 7, 9)] + [odd(kt=k) for k in (1, 2, 3, 4, 7, 9, 11)]
            ragged += [odd(Hout=7), odd(Wout=8), odd(stride=2), odd(stride=2, Hout=4, Wout=8), odd(Hin=9, Win=17, stride=2, Hout=5, Wout=8)]
            ragged += [odd(Win=12, Wout=12), odd(Win=130, Wout=130), odd(Cin=128, Cmid=896, Cout=128), odd(Cin=128, Cmid=896, y1_mode=2)]
            for a in ragged:
                print(line("ragged", a))
                n += 1
    print(f"tuples {n}")


if __name__ == "__main__":
    main()

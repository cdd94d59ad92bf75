#!/usr/bin/env python3
"""Host answers of the model's composites, one line per argument set (development tool; no device needed).

Replays the grid of tests/test_host_block_plan.py plus ragged and refused arguments and prints, for each, the forward and
backward dwn_block_workspace_bytes, dwn_block_forward_writes and the (rc, message) of dwn_block_backward's device-free checks;
then the size entries of the stem, the cortex, the readout and conv_pw's backward over the same block shapes, the benchmarked
model's and the model tests' cortex and readout widths and the ten-readout configuration (lines tagged `size`).
Run once per library (DWN_LIB_PATH, DWN_DETERMINISTIC) and `diff` the outputs: a host-only change of csrc/dwn_api.hip leaves no
differing line among the `grid` and `size` lines (valid arguments); the `ragged` lines also show what a refused geometry answers.

usage: block_plan_replay.py > answers.txt
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sensorium_amd._lib as L
import bench
from tests.test_gpu_block import CASES
from tests.test_host_block_plan import answers, bench_cases, block_args, grid


def backward_check(a):
    """dwn_block_backward answers its argument checks before it enters a device; an argument set that passes them is reported as
    such, not by what the device (or its absence) answers next"""
    rc = L.lib.dwn_block_backward(C.byref(a), 0, None)
    refused = rc in (-2, -4, -7) and b"block" in L.lib.dwn_last_error()
    return (rc, L.lib.dwn_last_error().decode()) if refused else ("passed", "")


def line(tag, a):
    fields = "dtype training B T Hin Win Hout Wout Cin Cmid Cout stride ks kt se_r y1_mode pwl_bwd".split()
    return f"{tag} {' '.join(str(getattr(a, f)) for f in fields)} -> {answers(L, a)} {backward_check(a)}"


def sizes():
    """the stem, cortex, readout and conv_pw-backward size entries; returns the number of lines"""
    lib, n = L.lib, 0
    dtypes, modes = (L.DWN_F32, L.DWN_BF16), (L.BN_EVAL, L.BN_TRAIN, L.BN_FROZEN)
    for cin, _, _, exp, _, B, T, H, W in CASES + bench_cases():
        for dtype in dtypes:
            for mode in modes:      # the stem in front of a first block of this shape
                s = L.StemArgs(); s.dtype = dtype; s.training = mode; s.B = B; s.Cin = 5; s.C0 = cin; s.S = T * H * W
                print(f"size stem {dtype} {mode} {B} 5 {cin} {s.S} -> {lib.dwn_stem_workspace_bytes(C.byref(s))}")
            print(f"size pw_backward {dtype} {cin * exp} {cin} -> {lib.dwn_pw_backward_workspace_bytes(cin * exp, cin, dtype)}")
            n += len(modes) + 1
    # (last core width, cortex widths): the model tests' tiny configuration and the benchmarked one
    tiny, full = (16, (32, 64)), (bench.CORE_FEATURES[-1], bench.model_params()["nn_module"][1]["cortex_features"])
    for (first, widths), shapes, readouts in ((tiny, ((2, 6), (3, 5)), (7, 10)), (full, ((32, 32), (2, 8)), bench.NUM_NEURONS_ALL)):
        for B, T in shapes:
            for dtype in dtypes:
                for cin, cout in zip((first,) + tuple(widths), widths):
                    for mode in modes:
                        c = L.CortexArgs(); c.dtype = dtype; c.training = mode; c.B = B; c.T = T; c.Cin = cin; c.C = cout; c.groups = 2
                        print(f"size cortex {dtype} {mode} {B} {T} {cin} {cout} 2 -> "
                              f"{lib.dwn_cortex_workspace_bytes(C.byref(c), 0)} {lib.dwn_cortex_workspace_bytes(C.byref(c), 1)}")
                        n += 1
                for n_out in readouts:
                    for drop, wt, beta in ((0, 0, 0), (256, 0, 0), (0, 256, 0), (256, 256, 256)):      # the pointers that choose slices
                        r = L.ReadoutArgs(); r.dtype = dtype; r.B = B; r.T = T; r.Cin = widths[-1]; r.groups = 2; r.n_out = n_out
                        r.drop_mask = drop or None; r.wt = wt or None; r.beta_dev = beta or None
                        print(f"size readout {dtype} {B} {T} {widths[-1]} 2 {n_out} {drop} {wt} {beta} -> "
                              f"{lib.dwn_readout_workspace_bytes(C.byref(r), 0)} {lib.dwn_readout_workspace_bytes(C.byref(r), 1)} "
                              f"{lib.dwn_readout_wt_bytes(C.byref(r))}")
                        n += 1
    return n


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
    n += sizes()
    print(f"tuples {n}")


if __name__ == "__main__":
    main()

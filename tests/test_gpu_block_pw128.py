"""dwn_block_backward at 128 input channels (C_mid = 896) with M_in % 128 == 0: conv_pw's backward runs through the one-pass
kernel of csrc/dwn_pw_bwd.hip and its output is dx (BlockPlan::dx_folded) — identity shortcut with C_out = C_in and 2 C_in, and
the gathered shortcut of a strided block.  Against the oracle with the body, assertions and bounds of
tests/test_gpu_block.py::test_block_train_forward_backward (dx and dw_pw are the last two gradients it checks).

test_plan_folds_dx_at_128_channels needs no device: it runs with the non-GPU tests.
"""
import ctypes as C

import pytest
import torch

from tests.test_gpu_block import _train_forward_backward
from tests.test_host_block_plan import bench_cases, block_args

# cin, cout, stride, exp, se_ratio, B, T, H, W: M_in = 2 * 4 * 8 * 16 = 1024
CASES128 = [(128, 128, 1, 7, 32, 2, 4, 8, 16), (128, 256, 1, 7, 32, 2, 4, 8, 16), (128, 128, 2, 7, 32, 2, 4, 8, 16)]


def with_maps(a, keep):
    """the plan asks only whether the inverse nearest maps are given"""
    hinv, winv = (C.c_int * a.Hin)(), (C.c_int * a.Win)()
    keep += [hinv, winv]
    a.hinv, a.winv = C.cast(hinv, C.c_void_p), C.cast(winv, C.c_void_p)
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES128, ids=lambda c: "-".join(map(str, c)))
def test_block_backward_through_the_one_pass_kernel(case):
    import sensorium_amd._lib as L
    keep = []
    a = with_maps(block_args(L, case, L.DWN_BF16, L.BN_TRAIN), keep)
    assert L.lib.dwn_pw_bwd_fused_supported(L.DWN_BF16, a.B * a.T * a.Hin * a.Win, a.Cmid, a.Cin) == 1
    assert L.lib.dwn_block_backward_route(C.byref(a)) == (1 if case[2] == 1 else 3)
    # (the block allocates exactly dwn_block_workspace_bytes: a backward that carved more would answer -6)
    _train_forward_backward(case, torch.bfloat16, False, "auto")


def test_plan_folds_dx_at_128_channels():
    """Blocks 4-6 of the metric geometry (stride 2 / 1 / 1 with C_out = 2 C_in on the last) and the three cases above: the plan
    reports dx_folded (gathered on the strided block, where the maps are given), for both training modes; fp32, a row count that
    is no multiple of 128 and a strided block without maps keep the separate dx pass.  The backward workspace does not depend on the
    route: the carver takes the same slices either way."""
    import sensorium_amd._lib as L
    keep = []
    metric = bench_cases()[4:7]
    assert [c[0] for c in metric] == [128, 128, 128] and [c[2] for c in metric] == [2, 1, 1] and metric[2][1] == 256
    for case in metric + CASES128:
        for mode in (L.BN_TRAIN, L.BN_FROZEN):
            a = with_maps(block_args(L, case, L.DWN_BF16, mode), keep)
            assert (a.B * a.T * a.Hin * a.Win) % 128 == 0
            assert L.lib.dwn_block_backward_route(C.byref(a)) == (1 if case[2] == 1 else 3), case
            ws = L.lib.dwn_block_workspace_bytes(C.byref(a), 1)
            # ... and they hold what conv_pw's backward carves for itself (Bp, the G / r3 accumulators, tacc; two alignment gaps at most)
            assert ws >= L.lib.dwn_pw_backward_workspace_bytes(a.Cmid, a.Cin, L.DWN_BF16) - 512, case
            bare = block_args(L, case, L.DWN_BF16, mode)                      # no maps: a strided block cannot gather
            assert L.lib.dwn_block_backward_route(C.byref(bare)) == (1 if case[2] == 1 else 0), case
            assert L.lib.dwn_block_workspace_bytes(C.byref(bare), 1) == ws, case
            f32 = with_maps(block_args(L, case, L.DWN_F32, mode), keep)
            assert L.lib.dwn_block_backward_route(C.byref(f32)) == 0, case
        ragged = with_maps(block_args(L, case[:5] + (1, 1, 9, 16), L.DWN_BF16, L.BN_TRAIN), keep)     # M_in = 144
        assert L.lib.dwn_block_backward_route(C.byref(ragged)) == 0, case
    # the 64-channel blocks answer as before, the 256-channel blocks keep the two-GEMM route
    for i, case in enumerate(bench_cases()):
        a = with_maps(block_args(L, case, L.DWN_BF16, L.BN_TRAIN), keep)
        want = 0 if case[0] == 256 else (1 if case[2] == 1 else 3)
        assert L.lib.dwn_block_backward_route(C.byref(a)) == want, (i, case)

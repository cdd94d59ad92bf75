"""CPU test of the block composite's route plan (csrc/dwn_api.hip plan_block): the three host entries that answer from it —
dwn_block_forward_writes and dwn_block_workspace_bytes forward / backward — agree with each other and with the support predicates
of the stencils over every block shape the GPU tests and the benchmark run, both dtypes, the three BatchNorm modes, y1_mode 0/1/2
and pwl_bwd 0/1/2.  No device, and no absolute byte count: a later layout change need not regenerate a table."""
import ctypes as C
import itertools

import torch

import bench
from tests.test_gpu_block import CASES, y1_free_case

Y1_MODES = {0: "auto", 1: "materialise", 2: "all"}


def bench_cases(batch=32, frames=32, height=36, width=64, expansion=7):
    """the nine blocks of the benchmarked model in the layout of test_gpu_block.CASES, checked against bench.block_shapes"""
    out, h, w = [], height, width
    for i, (cin, st) in enumerate(zip(bench.CORE_FEATURES, bench.STRIDES)):
        cout = bench.CORE_FEATURES[min(i + 1, len(bench.CORE_FEATURES) - 1)]
        out.append((cin, cout, st, expansion, 32, batch, frames, h, w))
        h, w = (h - 1) // st + 1, (w - 1) // st + 1
    assert [(c[5] * c[6] * c[7] * c[8], c[5] * c[6] * ((c[7] - 1) // c[2] + 1) * ((c[8] - 1) // c[2] + 1), c[0] * c[3])
            for c in out] == bench.block_shapes(batch, frames, height, width, expansion)
    return out


def block_args(L, case, dtype, training, y1_mode=0, pwl_bwd=0, B=None):
    cin, cout, stride, exp, ser, b, T, H, W = case
    a = L.BlockArgs()
    a.dtype = dtype; a.training = training; a.B = B or b; a.T = T; a.Hin = H; a.Win = W
    a.Hout = (H - 1) // stride + 1; a.Wout = (W - 1) // stride + 1
    a.Cin = cin; a.Cmid = cin * exp; a.Cout = cout; a.stride = stride; a.ks = 3; a.kt = 5; a.se_r = max(1, cin * exp // ser)
    a.y1_mode = y1_mode; a.pwl_bwd = pwl_bwd
    return a


def answers(L, a):
    """(forward_writes, forward workspace bytes, backward workspace bytes)"""
    return (L.lib.dwn_block_forward_writes(C.byref(a)), L.lib.dwn_block_workspace_bytes(C.byref(a), 0),
            L.lib.dwn_block_workspace_bytes(C.byref(a), 1))


def stencils_rebuild(L, case, dtype):
    """does either y1-rebuilding eval stencil take this geometry: the tile-resident one, the chained row-walk one?"""
    a = block_args(L, case, dtype, L.BN_EVAL)
    f = L.DwSpatialFwdArgs()
    f.planes = a.B * a.T; f.Hin = a.Hin; f.Win = a.Win; f.Hout = a.Hout; f.Wout = a.Wout; f.C = a.Cmid; f.stride = a.stride; f.ks = a.ks
    f.inp.ld = a.Cmid; f.a0_ld = a.Cin; f.Cin = a.Cin
    return (L.lib.dwn_dw_spatial_rc_supported(dtype, a.Cin, a.Cmid, a.ks, a.stride, a.Hin, a.Win) == 1,
            L.lib.dwn_dw_spatial_fwd_rc_supported(C.byref(f), dtype) == 1)


def grid():
    return itertools.product(CASES + bench_cases(), (0, 1), (0, 1, 2), (0, 1, 2), (0, 1, 2))     # case, dtype, BN mode, y1_mode, pwl_bwd


def test_the_three_entries_agree_over_the_grid():
    import sensorium_amd._lib as L
    assert (L.DWN_F32, L.DWN_BF16) == (0, 1) and (L.BN_EVAL, L.BN_TRAIN, L.BN_FROZEN) == (0, 1, 2)
    n = 0
    for case, dtype, mode, y1_mode, pwl_bwd in grid():
        what = f"{case} dtype {dtype} mode {mode} y1_mode {y1_mode} pwl_bwd {pwl_bwd}"
        a = block_args(L, case, dtype, mode, y1_mode, pwl_bwd)
        writes, ws_f, ws_b = answers(L, a)
        if mode == L.BN_EVAL:
            # eval never writes y3, and y1 exactly where neither stencil rebuilds it; fp32 has no such stencil
            assert writes == (0 if any(stencils_rebuild(L, case, dtype)) else 1), what
            assert dtype == L.DWN_BF16 or writes == 1, what
        else:
            # training and frozen write y3, and y1 unless the stencils rebuild it (test_gpu_block.y1_free_case mirrors that rule)
            tdtype = torch.bfloat16 if dtype == L.DWN_BF16 else torch.float32
            assert writes == (2 if y1_free_case(case, tdtype, Y1_MODES[y1_mode]) else 3), what
            other = block_args(L, case, dtype, L.BN_TRAIN + L.BN_FROZEN - mode, y1_mode, pwl_bwd)
            assert answers(L, other) == (writes, ws_f, ws_b), what
        # conv_pwl's backward route is a matter of the backward workspace alone: B x [Cout][Cmid] fp32 per-sample products, taken as
        # the carver's last slice (so at most one 256-byte alignment gap in front of them)
        per_sample = answers(L, block_args(L, case, dtype, mode, y1_mode, 1))
        materialised = answers(L, block_args(L, case, dtype, mode, y1_mode, 2))
        assert per_sample[:2] == materialised[:2] == (writes, ws_f), what
        pb = a.B * a.Cout * a.Cmid * 4
        if L.DETERMINISTIC:                    # the ordered-reduction build takes the per-sample products whatever pwl_bwd says
            assert per_sample[2] == materialised[2], what
        else:
            assert pb <= per_sample[2] - materialised[2] < pb + 256, what
        assert ws_b in (per_sample[2], materialised[2]), what
        # positive, and monotone in the batch size
        more = answers(L, block_args(L, case, dtype, mode, y1_mode, pwl_bwd, B=2 * a.B))
        assert 0 < ws_f <= more[1] and 0 < ws_b <= more[2] and more[0] == writes, what
        n += 1
    assert n == (len(CASES) + 9) * 2 * 3 * 3 * 3


def test_every_eval_route_has_a_block_case():
    """the tile-resident stencil, the chained stencil and the conv_pw fall-back each have a bf16 case in test_gpu_block.CASES"""
    import sensorium_amd._lib as L
    routes = {stencils_rebuild(L, case, L.DWN_BF16) for case in CASES if case[0] in (64, 128)}
    assert (True, False) in routes and (False, False) in routes and any(r[1] for r in routes)

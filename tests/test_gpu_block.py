"""GPU parity of one PositionalEncoding3d + InvertedResidual3d block (forward intermediates, output, input
gradient, every parameter gradient, BN running statistics) against the CPU oracle — which itself is pinned to
the reference (src/models/dwiseneuro.py:136-144, 184-192) by tests/golden.

fp32 path: <= 1e-3 relative (north-star tolerance; gradients norm-relative).
bf16 path: 4e-2 forward / 8e-2 gradients relative L2 (bf16 storage of every activation; stated separately).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests.gpu_helpers import dev, rel  # noqa: E402


def make_block(cin, cout, stride, expansion, se_ratio, seed, temporal_kernel=5):
    from sensorium_amd.dwiseneuro import InvertedResidual3d, PositionalEncoding3d
    torch.manual_seed(seed)
    blk = InvertedResidual3d(cin, cout, spatial_kernel=3, temporal_kernel=temporal_kernel, spatial_stride=stride,
                             expansion_ratio=expansion, se_reduce_ratio=se_ratio)
    pe = PositionalEncoding3d(cin)
    g = torch.Generator().manual_seed(seed)
    for name, p in blk.named_parameters():
        if p.dim() > 1:
            fan = p[0].numel()
            p.data = torch.randn(p.shape, generator=g) * (1.5 / math.sqrt(fan))
        elif "bn" in name and name.endswith("weight"):
            p.data = torch.rand(p.shape, generator=g) + 0.5
        else:
            p.data = torch.randn(p.shape, generator=g) * 0.2
    for name, b in blk.named_buffers():
        if name.endswith("running_mean"):
            b.data = torch.randn(b.shape, generator=g) * 0.1
        elif name.endswith("running_var"):
            b.data = torch.rand(b.shape, generator=g) + 0.5
    return blk, pe


CASES = [
    # cin, cout, stride, exp, se_ratio, B, T, H, W
    (8, 8, 1, 3, 4, 2, 6, 5, 6),
    (8, 16, 2, 3, 4, 3, 6, 9, 11),
    (16, 16, 1, 3, 4, 2, 5, 3, 3),
    (64, 64, 2, 7, 32, 2, 4, 12, 16),
    (64, 128, 1, 7, 32, 1, 8, 9, 16),
    # degenerate geometry: fewer frames than the temporal kernel, single-row / single-column planes, ragged slices
    (8, 8, 1, 3, 4, 1, 2, 2, 3),
    (8, 16, 2, 3, 4, 2, 3, 1, 5),
    (24, 40, 2, 7, 4, 2, 4, 7, 9),
    (16, 16, 1, 5, 4, 2, 1, 4, 1),
    # the plane widths the chained / row-walk bf16 stencils are built for (32 / 16 / 8 output columns, both strides, the 5x8
    # planes of the last block), straight against the oracle
    (64, 64, 1, 7, 32, 1, 4, 18, 32),
    (64, 64, 2, 7, 32, 1, 3, 36, 64),
    (64, 128, 2, 7, 32, 1, 4, 18, 32),
    (128, 128, 1, 7, 32, 2, 4, 5, 8),
    (64, 64, 2, 7, 32, 2, 3, 9, 16),
    # a plane too wide for either register geometry of the y1-rebuilding eval stencil (LDS fits): eval must fall back
    (64, 64, 1, 7, 32, 1, 2, 4, 130),
    # the 256-channel blocks (7 and 8 of the benchmarked model: Cin = 256, E = 1792).  The small pair checks the arithmetic at that
    # width; the large pair has the row counts / rows-per-sample at which the library takes the paths only those blocks run
    # (T*Hout*Wout = 1280 < 2048: bf16 conv_pwl backward through the materialised du + bn3_bwd_reduce; M_in >= 8192:
    # gemm_nn_xl for conv_pw; the K-concatenated conv_pw data gradient at K = 1792 + 256)
    (256, 256, 2, 7, 32, 1, 2, 9, 16),
    (256, 256, 1, 7, 32, 2, 2, 5, 8),
    (256, 256, 2, 7, 32, 2, 32, 9, 16),
    (256, 256, 1, 7, 32, 7, 32, 5, 8),
    # expansion 6 (the distillation student, configs/distillation_001.py:32: Cmid = 384 / 768 / 1536 — slices of 64 channels do
    # not divide 384 evenly into the 448-wide tilings the expansion-7 shapes were tuned on) at the three widths, both strides
    (64, 64, 2, 6, 32, 2, 4, 12, 16),
    (128, 256, 1, 6, 32, 2, 4, 9, 16),
    (256, 256, 2, 6, 32, 1, 4, 9, 16),
    # a plane the tile-resident y1-rebuilding eval stencil (dwn_dwrc.hip) is built for and the chained row-walk stencil is not (12
    # output columns): the one eval case that takes it through the block composite (test_block_eval_forward asserts that it does)
    (64, 64, 1, 7, 32, 1, 2, 4, 12),
]
RC_EVAL_CASE = 22


def y1_free_case(case, dtype, mode="auto"):
    """bf16 training leaves y1 (conv_pw's output) unmaterialised where both stencils rebuild it from the block input — whole
    64-channel slices, the plane widths of the row-walk kernels — by default on 64-channel inputs (where that is also faster), with
    y1_mode 2 ("all") on 128-channel inputs too (dwn_block_args.y1_mode, csrc/dwn_api.hip)."""
    cin, cout, stride, exp, ser, B, T, H, W = case
    cins = (64,) if mode == "auto" else (64, 128)
    return dtype == torch.bfloat16 and mode != "materialise" and cin in cins and (W in (32, 16, 8) if stride == 1 else W in (64, 32, 16))


def _train_params():
    """(case, dtype, drop, y1) combinations that run a distinct path — the drop-path variant only on the small cases, "materialise"
    only where the default leaves y1 unmaterialised, "all" only where it differs from the default: filtered HERE, so that the run
    shows no skips but the ones that matter (the two-GPU nccl tests on a one-GPU box)."""
    out = []
    for y1 in ("auto", "all", "materialise"):
        for drop in (False, True):
            for case in CASES:
                for dtype in (torch.float32, torch.bfloat16):
                    if drop and case[0] != 8:
                        continue
                    if y1 == "materialise" and not y1_free_case(case, dtype, "all"):
                        continue
                    if y1 == "all" and y1_free_case(case, dtype, "all") == y1_free_case(case, dtype, "auto"):
                        continue
                    out.append(pytest.param(case, dtype, drop, y1, id=f"{'-'.join(map(str, case))}-{str(dtype)[6:]}-{'drop' if drop else 'nodrop'}-{y1}"))
    return out


@pytest.mark.parametrize("case,dtype,drop,y1", _train_params())
def test_block_train_forward_backward(case, dtype, drop, y1):
    _train_forward_backward(case, dtype, drop, y1)


def _train_forward_backward(case, dtype, drop, y1, temporal_kernel=5):
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=cin + stride, temporal_kernel=temporal_kernel)
    assert blk.state_dict()["temp_covn_dw.0.weight"].shape[2] == temporal_kernel
    sd = {"blk." + k: v.clone() for k, v in blk.state_dict().items()}
    torch.manual_seed(1)
    x = torch.randn(B, T, H, W, cin) * 1.5 + 0.3
    drop_scale = torch.tensor([0.0, 1.25, 1.25][:B]) if drop else None

    # ---- oracle (float64 ground truth on CPU)
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v)
            for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    taps, new_stats = {}, {}
    a0 = x64 + orc.pe_table(cin, T, H, W, pe.inv_freq, torch.float64)
    ref = orc.inverted_residual(a0, "blk", sd64, stride, True, drop_scale, new_stats, taps)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7)).double()
    (ref * gout).sum().backward()

    # ---- HIP
    blk = blk.to(dev()).train()
    pe = pe.to(dev())
    blk._capture = True
    blk._dwn_y1_mode = {"auto": 0, "materialise": 1, "all": 2}[y1]
    xd = x.to(dev()).to(dtype).requires_grad_(True)
    if drop:
        blk.drop_path.sample = lambda b, d: drop_scale.to(d)
    out = blk(xd, pe, dtype)
    out.backward(gout.to(dev()).to(dtype))
    torch.cuda.synchronize()

    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (4e-2, 8e-2)
    cap = blk._captured
    # the y1-free path is the one that ran where it is built (and only there)
    assert (cap["y1"] is None) == y1_free_case(case, dtype, y1), "y1 materialisation is not what the case expects"
    for name in ("y1", "y2", "y3", "y4"):
        if cap[name] is None:
            continue
        e = rel(cap[name].float(), taps[name])
        assert e < ft, f"forward intermediate {name}: rel err {e:.3e}"
    e = rel(out.float(), ref)
    assert e < ft, f"block output rel err {e:.3e}"
    # running statistics (momentum 0.1, unbiased variance)
    for k, v in new_stats.items():
        mine = blk.state_dict()[k[4:]]
        if v.is_floating_point():
            assert rel(mine, v) < (1e-4 if dtype == torch.float32 else 2e-2), k
        else:
            assert int(mine) == int(v), k
    # gradients, in backward-chain order so the first failure localises the bug
    order = ["conv_pwl.1.bn", "bn_sc.bn", "conv_pwl.0", "se.conv_expand", "se.conv_reduce", "temp_covn_dw.1.bn",
             "temp_covn_dw.0", "spat_covn_dw.1.bn", "spat_covn_dw.0", "conv_pw.1.bn", "conv_pw.0"]
    named = dict(blk.named_parameters())
    gnorm = math.sqrt(sum(float(v.grad.norm()) ** 2 for k, v in sd64.items() if getattr(v, "grad", None) is not None))
    for prefix in order:
        for suffix in ("weight", "bias"):
            key = f"{prefix}.{suffix}"
            if key not in named:
                continue
            g_ref = sd64["blk." + key].grad
            g_mine = named[key].grad
            assert g_mine is not None, key
            err = float((g_mine.double().cpu() - g_ref).norm()) / (float(g_ref.norm()) + 1e-4 * gnorm)
            assert err < gt, f"grad {key}: rel err {err:.3e}"
    e = rel(xd.grad.float(), x64.grad)
    assert e < gt, f"input grad rel err {e:.3e}"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case_id", [1, 3, 4, 9, 10, 12, 14, 15, 16, 17, 18, 19, 20, 21, RC_EVAL_CASE])
def test_block_eval_forward(dtype, case_id):
    """Eval-mode forward.  In bf16, the cases with 64 / 128 input channels and a row-walk plane width (3, 4, 9, 10, 12, 19, 20) take
    the chained stencil's rebuilt-input form and RC_EVAL_CASE, whose 12-pixel rows that stencil is not built for, the tile-resident
    y1-recomputing stencil (dwn_dw_spatial_fwd_rc): conv_pw never runs as its own pass.  Case 14, whose 130-pixel rows fit neither,
    falls back to conv_pw + stencil, as do case 1, the 256-channel cases and every fp32 run."""
    if case_id == RC_EVAL_CASE and dtype == torch.bfloat16:      # the case must not drift onto another route
        import ctypes as C
        import sensorium_amd._lib as L
        cin, cout, stride, exp, ser, B, T, H, W = CASES[case_id]
        assert L.lib.dwn_dw_spatial_rc_supported(L.DWN_BF16, cin, cin * exp, 3, stride, H, W) == 1
        f = L.DwSpatialFwdArgs()
        f.planes = B * T; f.Hin = H; f.Win = W; f.Hout = (H - 1) // stride + 1; f.Wout = (W - 1) // stride + 1; f.C = cin * exp
        f.stride = stride; f.ks = 3; f.inp.ld = cin * exp; f.a0_ld = cin; f.Cin = cin
        assert L.lib.dwn_dw_spatial_fwd_rc_supported(C.byref(f), L.DWN_BF16) == 0
    _eval_forward(CASES[case_id], dtype)


def _eval_forward(case, dtype, temporal_kernel=5):
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=3, temporal_kernel=temporal_kernel)
    sd = {"blk." + k: v.clone().double() if v.is_floating_point() else v.clone() for k, v in blk.state_dict().items()}
    x = torch.randn(B, T, H, W, cin, generator=torch.Generator().manual_seed(2))
    a0 = x.double() + orc.pe_table(cin, T, H, W, pe.inv_freq, torch.float64)
    ref = orc.inverted_residual(a0, "blk", sd, stride, False, None, None)
    blk = blk.to(dev()).eval()
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    with torch.no_grad():
        out = blk(x.to(dev()).to(dtype), pe.to(dev()), dtype)
    assert rel(out.float(), ref) < (1e-3 if dtype == torch.float32 else 4e-2)
    for k, v in blk.state_dict().items():      # eval must not touch the BN buffers
        assert torch.equal(v, before[k]), k


# temporal_kernel = 3: the second kernel size dwn_block_forward accepts (fwd<T,3>, bwd_rc<T,3> and the eval epilogue), through a whole
# block against the oracle, with the bodies — assertions and bounds — of the tests above.  T = 1 .. 8: fewer frames than the kernel,
# exactly one unrolled batch, several; ragged and whole channel slices; the y1-free bf16 path (cases 3, 4) and the 256-channel blocks
KT3_CASES = [CASES[1], CASES[8], CASES[3], CASES[4], CASES[16], CASES[5], CASES[7]]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("case", KT3_CASES, ids=lambda c: "-".join(map(str, c)))
def test_block_temporal_kernel_3_train_forward_backward(case, dtype):
    _train_forward_backward(case, dtype, False, "auto", temporal_kernel=3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["float32", "bfloat16"])
@pytest.mark.parametrize("case", KT3_CASES, ids=lambda c: "-".join(map(str, c)))
def test_block_temporal_kernel_3_eval_forward(case, dtype):
    _eval_forward(case, dtype, temporal_kernel=3)


@pytest.mark.parametrize("path", ["old", "new"])
def test_block_backward_both_project_conv_paths(path):
    """The conv_pwl backward has two implementations (per-sample products + recompute epilogue, or the materialised du),
    chosen per shape; DWN_PWL_BWD forces one (read once per process), so the block and model parity tests are re-run in a
    child process under each."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, DWN_PWL_BWD=path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "tests/test_gpu_block.py",
                          "tests/test_gpu_model.py", "-k", "not both_project_conv_paths"],
                         cwd=root, env=env, capture_output=True, text=True, timeout=1500)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]

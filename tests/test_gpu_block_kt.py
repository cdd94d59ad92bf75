"""GPU parity of one PositionalEncoding3d + InvertedResidual3d block built with temporal_kernel 7 and 9 (reference:
src/models/dwiseneuro.py:74-144) against the CPU oracle, by the method of tests/test_gpu_block_ks.py (its make_block, which takes
both kernel sizes): forward intermediates and output, the input gradient, every parameter gradient and the running statistics in
training mode; the eval forward (z3 and the pooling sums from the temporal pass); and the eval-mode backward through frozen
BatchNorm statistics.  T = 3 is shorter than the padding of either size, T = 11 runs over more than one unrolled batch.

Bounds are those tests/test_gpu_block_ks.py states for the same quantities: fp32 1e-3; bf16 4e-2 forward / 8e-2 gradients (relative
L2); running statistics 1e-4 / 2e-2."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests.gpu_helpers import dev, rel  # noqa: E402
from tests.test_gpu_block_ks import make_block  # noqa: E402

CASES = [
    # cin, cout, stride, exp, se_ratio, B, T, H, W
    (8, 8, 1, 3, 4, 2, 3, 9, 11),
    (8, 16, 2, 3, 4, 2, 3, 9, 11),
    (16, 16, 1, 3, 4, 2, 11, 9, 11),
    (16, 24, 2, 3, 4, 2, 11, 9, 11),
]
PARAMS = [pytest.param(case, kt, dtype, id=f"{'-'.join(map(str, case))}-kt{kt}-{str(dtype)[6:]}")
          for case in CASES for kt in (7, 9) for dtype in (torch.float32, torch.bfloat16)]


def _bounds(dtype):
    return (1e-3, 1e-3) if dtype == torch.float32 else (4e-2, 8e-2)


@pytest.mark.parametrize("case,kt,dtype", PARAMS)
def test_block_train_forward_backward(case, kt, dtype):
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=cin + stride, spatial_kernel=3, temporal_kernel=kt)
    assert tuple(blk.state_dict()["temp_covn_dw.0.weight"].shape[2:]) == (kt, 1, 1)
    sd = {"blk." + k: v.clone() for k, v in blk.state_dict().items()}
    torch.manual_seed(1)
    x = torch.randn(B, T, H, W, cin) * 1.5 + 0.3

    # ---- oracle (float64 ground truth on CPU)
    sd64 = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    taps, new_stats = {}, {}
    a0 = x64 + orc.pe_table(cin, T, H, W, pe.inv_freq, torch.float64)
    ref = orc.inverted_residual(a0, "blk", sd64, stride, True, None, new_stats, taps)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7)).double()
    (ref * gout).sum().backward()

    # ---- HIP
    blk = blk.to(dev()).train()
    pe = pe.to(dev())
    blk._capture = True
    xd = x.to(dev()).to(dtype).requires_grad_(True)
    out = blk(xd, pe, dtype)
    out.backward(gout.to(dev()).to(dtype))
    torch.cuda.synchronize()

    ft, gt = _bounds(dtype)
    cap = blk._captured
    for name in ("y1", "y2", "y3", "y4"):
        if cap[name] is None:                   # (an intermediate the library did not materialise at this geometry)
            continue
        e = rel(cap[name].float(), taps[name])
        assert e < ft, f"forward intermediate {name}: rel err {e:.3e}"
    e = rel(out.float(), ref)
    assert e < ft, f"block output rel err {e:.3e}"
    for k, v in new_stats.items():          # running statistics (momentum 0.1, unbiased variance)
        mine = blk.state_dict()[k[4:]]
        if v.is_floating_point():
            assert rel(mine, v) < (1e-4 if dtype == torch.float32 else 2e-2), k
        else:
            assert int(mine) == int(v), k
    order = ["conv_pwl.1.bn", "bn_sc.bn", "conv_pwl.0", "se.conv_expand", "se.conv_reduce", "temp_covn_dw.1.bn",
             "temp_covn_dw.0", "spat_covn_dw.1.bn", "spat_covn_dw.0", "conv_pw.1.bn", "conv_pw.0"]
    named = dict(blk.named_parameters())
    gnorm = math.sqrt(sum(float(v.grad.norm()) ** 2 for k, v in sd64.items() if getattr(v, "grad", None) is not None))
    seen = 0
    for prefix in order:
        for suffix in ("weight", "bias"):
            key = f"{prefix}.{suffix}"
            if key not in named:
                continue
            seen += 1
            g_ref = sd64["blk." + key].grad
            g_mine = named[key].grad
            assert g_mine is not None, key
            err = float((g_mine.double().cpu() - g_ref).norm()) / (float(g_ref.norm()) + 1e-4 * gnorm)
            assert err < gt, f"grad {key}: rel err {err:.3e}"
    assert seen == len(named), "a parameter gradient was not compared"
    e = rel(xd.grad.float(), x64.grad)
    assert e < gt, f"input grad rel err {e:.3e}"


@pytest.mark.parametrize("case,kt,dtype", PARAMS)
def test_block_eval_forward(case, kt, dtype):
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=3, spatial_kernel=3, temporal_kernel=kt)
    sd = {"blk." + k: v.clone().double() if v.is_floating_point() else v.clone() for k, v in blk.state_dict().items()}
    x = torch.randn(B, T, H, W, cin, generator=torch.Generator().manual_seed(2))
    a0 = x.double() + orc.pe_table(cin, T, H, W, pe.inv_freq, torch.float64)
    ref = orc.inverted_residual(a0, "blk", sd, stride, False, None, None)
    blk = blk.to(dev()).eval()
    before = {k: v.clone() for k, v in blk.state_dict().items()}
    with torch.no_grad():
        out = blk(x.to(dev()).to(dtype), pe.to(dev()), dtype)
    assert rel(out.float(), ref) < _bounds(dtype)[0]
    for k, v in blk.state_dict().items():      # eval must not touch the BN buffers
        assert torch.equal(v, before[k]), k


@pytest.mark.parametrize("case,kt,dtype", PARAMS)
def test_block_frozen_forward_backward(case, kt, dtype):
    """Eval mode and an input that requires a gradient: frozen BatchNorm statistics, the training kernels, a backward."""
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=cin + stride, spatial_kernel=3, temporal_kernel=kt)
    sd = {"blk." + k: v.clone() for k, v in blk.state_dict().items()}
    torch.manual_seed(1)
    x = torch.randn(B, T, H, W, cin) * 1.5 + 0.3
    ref_sd = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k
                  else (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    a0 = x64 + orc.pe_table(cin, T, H, W, pe.inv_freq, torch.float64)
    ref = orc.inverted_residual(a0, "blk", ref_sd, stride, False, None, None)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7)).double()
    (ref * gout).sum().backward()

    blk = blk.to(dev()).eval()
    pe = pe.to(dev())
    blk._capture = True
    before = {k: v.clone() for k, v in blk.state_dict().items() if "running" in k or "num_batches" in k}
    xd = x.to(dev()).to(dtype).requires_grad_(True)
    out = blk(xd, pe, dtype)
    out.backward(gout.to(dev()).to(dtype))
    torch.cuda.synchronize()

    ft, gt = _bounds(dtype)
    assert before
    for k, v in before.items():
        assert torch.equal(blk.state_dict()[k], v), f"{k} changed in frozen mode"
    e = rel(out.float(), ref)
    assert e < ft, f"block output rel err {e:.3e}"
    named = dict(blk.named_parameters())
    gnorm = math.sqrt(sum(float(v.grad.norm()) ** 2 for v in ref_sd.values() if getattr(v, "grad", None) is not None))
    for key, p in named.items():
        g_ref = ref_sd["blk." + key].grad
        assert p.grad is not None, key
        err = float((p.grad.double().cpu() - g_ref).norm()) / (float(g_ref.norm()) + 1e-4 * gnorm)
        assert err < gt, f"grad {key}: rel err {err:.3e}"
    e = rel(xd.grad.float(), x64.grad)
    assert e < gt, f"input grad rel err {e:.3e}"

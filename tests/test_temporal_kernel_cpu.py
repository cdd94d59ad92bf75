"""CPU: the yardsticks of temporal_kernel 7 and 9.

The oracle against tests/golden/temporal_kernel_7_9.npz, which tools/make_golden_temporal_kernel.py wrote from the real reference
module in float64 (a tiny DwiseNeuro: weights, inputs of 3 and 11 frames, eval and training-mode predictions, the input gradient
of each); the GPU tests of these sizes (tests/test_gpu_block_kt.py, test_gpu_model_kt.py) compare with the oracle.  Tolerance: the
2e-5 tests/test_oracle_golden.py holds the tiny-model fixtures to.

tests/dw_reference.py, the float64 checker of the kernel-level tests (tests/test_gpu_dwt_wide.py), at these sizes against torch's
conv3d and autograd in float64 — the op src/models/dwiseneuro.py:105-109 itself calls.  Float64 arithmetic of the same sums in
another order: the 1e-12 of tests/test_dw_reference_cpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dwiseneuro_oracle as orc
from tests import dw_reference as R

KW = dict(strides=(2, 1), readout_outputs=(9,), groups=2, softplus_beta=0.07)
TOL = 1e-12


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("T", [3, 11])
@pytest.mark.parametrize("kt", [7, 9])
def test_oracle_matches_reference_module(golden_dir, kt, T, training):
    z = np.load(golden_dir / "temporal_kernel_7_9.npz")
    pre = f"k{kt}:sd:"
    sd = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    assert sd["core.blocks.1.temp_covn_dw.0.weight"].shape[2:] == (kt, 1, 1)
    assert sd["core.blocks.3.temp_covn_dw.0.weight"].shape[2:] == (kt, 1, 1)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = torch.from_numpy(z[f"x{T}"]).double().requires_grad_(True)
    assert x.shape == (2, 5, T, 9, 11)
    mode = "train" if training else "eval"
    pred = orc.forward(sd, x, index=0, training=training, **KW)
    pred.sum().backward()
    assert pred.shape == z[f"k{kt}:T{T}:{mode}:pred"].shape
    assert rel(pred.detach().numpy(), z[f"k{kt}:T{T}:{mode}:pred"]) < 2e-5
    assert float(np.abs(z[f"k{kt}:T{T}:{mode}:dx"]).max()) > 0
    assert rel(x.grad.numpy(), z[f"k{kt}:T{T}:{mode}:dx"]) < 2e-5


def _rand(*shape, seed):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("T", [1, 3, 4, 8, 11])
@pytest.mark.parametrize("kt", [7, 9])
def test_temporal_reference_equals_conv3d(kt, T):
    """BatchNorm-2 + SiLU -> (k,1,1) convolution: forward, dy3 with y3 recomputed, dh2 / dW / the two BatchNorm-2 backward sums."""
    B, HW, Cc = 2, 3, 5
    M = B * T * HW
    y2 = _rand(M, Cc, seed=11)
    scale, shift = torch.rand(Cc, dtype=torch.float64, generator=torch.Generator().manual_seed(12)) + 0.5, _rand(Cc, seed=13) * 0.3
    mean, invstd = _rand(Cc, seed=14) * 0.2, torch.rand(Cc, dtype=torch.float64, generator=torch.Generator().manual_seed(15)) + 0.5
    w = _rand(kt, Cc, seed=16) / kt                                    # [k][C] tap-major
    dh3 = _rand(M, Cc, seed=17)
    v = [_rand(Cc, seed=20 + i) * 0.5 for i in range(3)]

    # conv3d on [B, C, T, HW, 1], groups = C, pad (k/2, 0, 0); L = sum(y3 * dy3) with dy3 = v0 dh3 + v1 y3 + v2 held constant
    h = (y2.view(B, T, HW, Cc) * scale + shift).requires_grad_(True)
    wc = w.t().reshape(Cc, 1, kt, 1, 1).clone().requires_grad_(True)
    z2 = (h * torch.sigmoid(h)).permute(0, 3, 1, 2).unsqueeze(-1)
    y3c = F.conv3d(z2, wc, padding=(kt // 2, 0, 0), groups=Cc).squeeze(-1).permute(0, 2, 3, 1)
    y3o = y3c.detach().reshape(M, Cc)
    dy3o = v[0] * dh3 + v[1] * y3o + v[2]
    y3c.backward(dy3o.view(B, T, HW, Cc))
    dh2o, dwo = h.grad.reshape(M, Cc), wc.grad.reshape(Cc, kt)

    y3 = R.dw_temporal_fwd_f64(y2, scale, shift, w, B, T, HW)
    assert y3.shape == (M, Cc) and R.rel_l2(y3, y3o) < TOL
    dy_p = R.dy3_plain_f64(dh3, y2, scale, shift, w, v[0], v[1], v[2], B, T, HW)
    assert R.rel_l2(dy_p, dy3o) < TOL
    dh2, dw, s0, s1 = R.dw_temporal_bwd_f64(y2, scale, shift, mean, invstd, dy_p, w, B, T, HW)
    assert R.rel_l2(dh2, dh2o) < TOL
    assert dw.shape == (Cc, kt) and R.rel_l2(dw, dwo) < TOL
    assert R.rel_l2(s0, dh2o.sum(0)) < TOL
    assert R.rel_l2(s1, (dh2o * ((y2 - mean) * invstd)).sum(0)) < TOL

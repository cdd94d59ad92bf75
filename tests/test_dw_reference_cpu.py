"""tests/dw_reference.py — the float64 checker the kernel-level depth-wise tests lean on — against the oracle
(oracle/dwiseneuro_oracle.py, itself pinned to the reference by tests/golden), forward and backward through autograd, on the CPU in
float64; and the oracle's two depth-wise convolutions at kernel size 3 against their DW_IMPL = "library" form (torch's conv3d, the
op src/models/dwiseneuro.py:96-109 itself calls), which the goldens only exercise at 5.

Everything here is float64 arithmetic of the same sums in a different order: the bound is 1e-12 relative L2."""
import pytest
import torch

from oracle import dwiseneuro_oracle as orc
from tests import dw_reference as R

TOL = 1e-12


def _rand(*shape, seed):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("planes,H,W,cin,E", [(3, 5, 7, 6, 10), (2, 1, 4, 3, 5), (1, 6, 1, 4, 7), (2, 7, 9, 5, 3)])
def test_spatial_reference_equals_oracle(planes, H, W, cin, E, stride):
    """conv_pw -> BatchNorm-1 + SiLU -> 3x3 stencil: forward, and dh1 / dW / the two BatchNorm-backward sums."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    a0, w1 = _rand(planes * H * W, cin, seed=1), _rand(E, cin, seed=2) / cin ** 0.5
    scale, shift = torch.rand(E, dtype=torch.float64, generator=torch.Generator().manual_seed(3)) + 0.5, _rand(E, seed=4) * 0.3
    mean, invstd = _rand(E, seed=5) * 0.2, torch.rand(E, dtype=torch.float64, generator=torch.Generator().manual_seed(6)) + 0.5
    w = _rand(9, E, seed=7) / 3.0                                       # [9][E] tap-major, dy * 3 + dx
    g = _rand(planes * Ho * Wo, E, seed=8)

    # oracle: x [B=1, T=planes, H, W, C]; the affine in between is the BatchNorm's scale * y + shift
    x = a0.view(1, planes, H, W, cin)
    y1o = orc.pointwise(x, w1.view(E, cin, 1, 1, 1))
    h = (y1o * scale + shift).requires_grad_(True)
    wo = w.t().reshape(E, 1, 1, 3, 3).clone().requires_grad_(True)
    y2o = orc.dw_spatial(orc.silu(h), wo, stride)
    y2o.backward(g.view(1, planes, Ho, Wo, E))

    y1 = R.conv_pw_f64(a0, w1)
    assert R.rel_l2(y1, y1o.reshape(-1, E)) < TOL
    y2 = R.dw_spatial_fwd_f64(y1, scale, shift, w, planes, H, W, stride)
    assert y2.shape == (planes * Ho * Wo, E)
    assert R.rel_l2(y2, y2o.detach().reshape(-1, E)) < TOL
    dh1, dw, s0, s1 = R.dw_spatial_bwd_f64(y1, scale, shift, mean, invstd, g, w, planes, H, W, stride)
    dh1o = h.grad.reshape(-1, E)
    assert R.rel_l2(dh1, dh1o) < TOL
    assert dw.shape == (E, 9) and R.rel_l2(dw, wo.grad.reshape(E, 9)) < TOL
    assert R.rel_l2(s0, dh1o.sum(0)) < TOL
    assert R.rel_l2(s1, (dh1o * ((y1o.reshape(-1, E) - mean) * invstd)).sum(0)) < TOL


@pytest.mark.parametrize("kt", [3, 5])
@pytest.mark.parametrize("T", [1, 2, 3, 7])
@pytest.mark.parametrize("B,HW,Cc", [(2, 3, 5), (1, 1, 3), (3, 5, 7)])
def test_temporal_reference_equals_oracle(B, T, HW, Cc, kt):
    """BatchNorm-2 + SiLU -> (k,1,1) convolution: forward, dh2 / dW / the two sums, and the three spellings of dy3."""
    M = B * T * HW
    y2 = _rand(M, Cc, seed=11)
    scale, shift = torch.rand(Cc, dtype=torch.float64, generator=torch.Generator().manual_seed(12)) + 0.5, _rand(Cc, seed=13) * 0.3
    mean, invstd = _rand(Cc, seed=14) * 0.2, torch.rand(Cc, dtype=torch.float64, generator=torch.Generator().manual_seed(15)) + 0.5
    w = _rand(kt, Cc, seed=16) / kt                                    # [k][C] tap-major
    dh3 = _rand(M, Cc, seed=17)
    v = [_rand(Cc, seed=20 + i) * 0.5 for i in range(5)]
    gate, gate2 = _rand(B, Cc, seed=30), _rand(B, Cc, seed=31)

    def oracle(dy3_of_y3):
        """dL/dh, dL/dw of L = sum(y3 * dy3) with dy3 = dy3_of_y3(y3) held constant, as the kernels take it."""
        h = (y2.view(B, T, HW, 1, Cc) * scale + shift).requires_grad_(True)
        wo = w.t().reshape(Cc, 1, kt, 1, 1).clone().requires_grad_(True)
        y3 = orc.dw_temporal(orc.silu(h), wo)
        dy3 = dy3_of_y3(y3.detach().reshape(M, Cc))
        y3.backward(dy3.view(B, T, HW, 1, Cc))
        return y3.detach().reshape(M, Cc), dy3, h.grad.reshape(M, Cc), wo.grad.reshape(Cc, kt)

    y3 = R.dw_temporal_fwd_f64(y2, scale, shift, w, B, T, HW)
    y3o, dy3o, dh2o, dwo = oracle(lambda y: v[0] * dh3 + v[1] * y + v[2])
    assert y3.shape == (M, Cc) and R.rel_l2(y3, y3o) < TOL
    # DWN_LD_AFFINE2 (y3 given) and DWN_LD_PLAIN (y3 recomputed, unrounded) are the same numbers
    dy_a = R.dy3_affine2_f64(dh3, y3, v[0], v[1], v[2])
    dy_p = R.dy3_plain_f64(dh3, y2, scale, shift, w, v[0], v[1], v[2], B, T, HW)
    assert R.rel_l2(dy_a, dy3o) < TOL and R.rel_l2(dy_p, dy3o) < TOL
    # rounding the recomputed y3 to a storage type moves dy3 by at most v2 * half an ulp of y3, and not at all in float64
    assert torch.equal(R.dy3_plain_f64(dh3, y2, scale, shift, w, v[0], v[1], v[2], B, T, HW, round_to=torch.float64), dy_p)
    dy_r = R.dy3_plain_f64(dh3, y2, scale, shift, w, v[0], v[1], v[2], B, T, HW, round_to=torch.bfloat16)
    assert bool(((dy_r - dy_p).abs() <= v[1].abs() * y3.abs() * 2.0 ** -8 + 1e-300).all()) and not torch.equal(dy_r, dy_p)
    dh2, dw, s0, s1 = R.dw_temporal_bwd_f64(y2, scale, shift, mean, invstd, dy_p, w, B, T, HW)
    assert R.rel_l2(dh2, dh2o) < TOL
    assert dw.shape == (Cc, kt) and R.rel_l2(dw, dwo) < TOL
    assert R.rel_l2(s0, dh2o.sum(0)) < TOL
    assert R.rel_l2(s1, (dh2o * ((y2 - mean) * invstd)).sum(0)) < TOL

    # DWN_LD_DY3: SqueezeExcite gate and gradient, SiLU' of BatchNorm-3 (through autograd of orc.silu), BatchNorm-3 backward affine
    def se(y):
        h3 = (v[3] * y + v[4]).requires_grad_(True)
        orc.silu(h3).backward((dh3.view(B, -1, Cc) * gate[:, None] + gate2[:, None]).reshape(M, Cc))
        return v[0] * h3.grad + v[1] * y + v[2]

    _, dy3o, dh2o, dwo = oracle(se)
    dy_s = R.dy3_se_f64(dh3, y3, gate, gate2, *v, B)
    assert R.rel_l2(dy_s, dy3o) < TOL
    dh2, dw, _, _ = R.dw_temporal_bwd_f64(y2, scale, shift, mean, invstd, dy_s, w, B, T, HW)
    assert R.rel_l2(dh2, dh2o) < TOL and R.rel_l2(dw, dwo) < TOL


@pytest.mark.parametrize("B,T,H,W,Cc", [(2, 1, 3, 5, 4), (1, 2, 1, 4, 3), (2, 3, 5, 1, 5), (1, 7, 4, 3, 6)])
def test_oracle_stencils_equal_conv3d_at_kernel_3(B, T, H, W, Cc):
    """orc.dw_temporal and orc.dw_spatial at kernel size 3 against torch's conv3d, values and both gradients."""
    for op, wshape, args in ((orc.dw_temporal, (Cc, 1, 3, 1, 1), ()), (orc.dw_spatial, (Cc, 1, 1, 3, 3), (1,)),
                             (orc.dw_spatial, (Cc, 1, 1, 3, 3), (2,))):
        res = {}
        for impl in ("stencil", "library"):
            x = _rand(B, T, H, W, Cc, seed=41).requires_grad_(True)
            w = _rand(*wshape, seed=42).requires_grad_(True)
            try:
                orc.DW_IMPL = impl
                y = op(x, w, *args)
            finally:
                orc.DW_IMPL = "stencil"
            y.backward(_rand(*y.shape, seed=43))
            res[impl] = (y.detach(), x.grad, w.grad)
        for a, b in zip(res["stencil"], res["library"]):
            assert a.shape == b.shape and R.rel_l2(a, b) < TOL

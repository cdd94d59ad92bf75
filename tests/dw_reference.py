"""float64 reference of conv_pw -> BatchNorm-1 + SiLU -> spat_covn_dw, of BatchNorm-2 + SiLU -> temp_covn_dw and of their backward
passes (reference ops: src/models/dwiseneuro.py:90-111), channels-last, on whatever device the operands live on, by padded-slice
arithmetic and torch autograd — the checker the kernel-level tests of the depth-wise kernels compare with (tests/test_gpu_dwfwd.py,
test_gpu_dwbwd.py, test_gpu_dwt.py).  Itself pinned to the oracle by tests/test_dw_reference_cpu.py.  Test infrastructure only."""
import torch


def conv_pw_f64(a0: torch.Tensor, w1: torch.Tensor) -> torch.Tensor:
    """y1 = a0 . W1^T in float64 from the (bf16) operands as given — the unrounded product."""
    return a0.double() @ w1.double().t()


def _dw3x3(z: torch.Tensor, w: torch.Tensor, stride: int) -> torch.Tensor:
    """z [P, H, W, C] float64, w [9, C] tap-major (dy * 3 + dx) -> [P, Hout, Wout, C]; zero padding 1."""
    P, H, W, Cc = z.shape
    Hout, Wout = (H - 1) // stride + 1, (W - 1) // stride + 1
    zp = torch.nn.functional.pad(z, (0, 0, 1, 1, 1, 1))
    out = None
    for dy in range(3):
        for dx in range(3):
            t = zp[:, dy:dy + stride * (Hout - 1) + 1:stride, dx:dx + stride * (Wout - 1) + 1:stride, :] * w[dy * 3 + dx]
            out = t if out is None else out + t
    return out


def dw_spatial_fwd_f64(y1, scale, shift, w, planes, Hin, Win, stride):
    """y1 [planes*Hin*Win, C] -> y2 [planes*Hout*Wout, C] (float64): dwS * SiLU(scale * y1 + shift)."""
    Cc = y1.shape[1]
    h = y1.double().view(planes, Hin, Win, Cc) * scale.double() + shift.double()
    y2 = _dw3x3(h * torch.sigmoid(h), w.double(), stride)
    return y2.reshape(-1, Cc)


def dw_spatial_bwd_f64(y1, scale, shift, mean, invstd, g, w, planes, Hin, Win, stride):
    """Backward of the above for the output gradient g [planes*Hout*Wout, C]: returns (dh1 = dL/d(BN1 output) [rows, C],
    dW [C, 9], sum dh1 [C], sum dh1 * yhat1 [C]) in float64, yhat1 = (y1 - mean) * invstd."""
    Cc = y1.shape[1]
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    y1 = y1.double()
    h = (y1.view(planes, Hin, Win, Cc) * scale.double() + shift.double()).requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    y2 = _dw3x3(h * torch.sigmoid(h), wd, stride)
    y2.backward(g.double().view(planes, Hout, Wout, Cc))
    dh1 = h.grad.reshape(-1, Cc)
    yhat = (y1 - mean.double()) * invstd.double()
    return dh1, wd.grad.t().contiguous(), dh1.sum(0), (dh1 * yhat).sum(0)


# ---- temp_covn_dw: the depth-wise (k,1,1) convolution along T, rows ordered (b, t, hw) -----------------------------------------------
def _dwt(z: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """z [B, T, HW, C] float64, w [k, C] tap-major -> [B, T, HW, C]: out[t] = sum_j w[j] z[t + j - P], zero frames outside [0, T)."""
    k, T = w.shape[0], z.shape[1]
    zp = torch.nn.functional.pad(z, (0, 0, 0, 0, k // 2, k // 2))
    out = None
    for j in range(k):
        t = zp[:, j:j + T] * w[j]
        out = t if out is None else out + t
    return out


def dw_temporal_fwd_f64(y2, scale, shift, w, B, T, HW):
    """y2 [B*T*HW, C] -> y3 [B*T*HW, C] (float64): dwT * SiLU(scale * y2 + shift); w [k][C] as dwn_dw_temporal_fwd_args.w."""
    Cc = y2.shape[1]
    h = y2.double().view(B, T, HW, Cc) * scale.double() + shift.double()
    return _dwt(h * torch.sigmoid(h), w.double()).reshape(-1, Cc)


def dw_temporal_bwd_f64(y2, scale, shift, mean, invstd, dy3, w, B, T, HW):
    """Backward of the above for the output gradient dy3 [B*T*HW, C]: returns (dh2 = dL/d(BN2 output) [rows, C], dW [C, k] as
    dwn_dw_temporal_bwd_args.dw, sum dh2 [C], sum dh2 * yhat2 [C]) in float64, yhat2 = (y2 - mean) * invstd."""
    Cc = y2.shape[1]
    y2 = y2.double()
    h = (y2.view(B, T, HW, Cc) * scale.double() + shift.double()).requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    _dwt(h * torch.sigmoid(h), wd).backward(dy3.double().view(B, T, HW, Cc))
    dh2 = h.grad.reshape(-1, Cc)
    yhat = (y2 - mean.double()) * invstd.double()
    return dh2, wd.grad.t().contiguous(), dh2.sum(0), (dh2 * yhat).sum(0)


# the three ways dwn_dw_temporal_bwd obtains dy3 (include/dwn.h: dwn_dw_temporal_bwd_args.dy_kind, the DWN_LD_* loaders)
def dy3_affine2_f64(dh3, y3, v1, v2, v3):
    """DWN_LD_AFFINE2: v1 * dh3 + v2 * y3 + v3, y3 given (the stored tensor)."""
    return v1.double() * dh3.double() + v2.double() * y3.double() + v3.double()


def dy3_plain_f64(dh3, y2, scale, shift, w, v1, v2, v3, B, T, HW, round_to=None):
    """DWN_LD_PLAIN: the same with y3 recomputed from y2.  round_to (a torch dtype) rounds the recomputed y3 to the storage type
    first, "as a stored y3 would read back" — what the kernel states it does; None is the reference operation proper."""
    y3 = dw_temporal_fwd_f64(y2, scale, shift, w, B, T, HW)
    if round_to is not None:
        y3 = y3.to(round_to).double()
    return dy3_affine2_f64(dh3, y3, v1, v2, v3)


def dy3_se_f64(du, y3, gate, gate2, v1, v2, v3, v4, v5, B):
    """DWN_LD_DY3: v1 * ((du * gate[b] + gate2[b]) * SiLU'(v4 * y3 + v5)) + v2 * y3 + v3; gate, gate2 [B, C] per sample."""
    Cc = y3.shape[1]
    y3 = y3.double().view(B, -1, Cc)
    h = v4.double() * y3 + v5.double()
    sg = torch.sigmoid(h)
    dh = (du.double().view(B, -1, Cc) * gate.double()[:, None] + gate2.double()[:, None]) * (sg * (1.0 + h * (1.0 - sg)))
    return (v1.double() * dh + v2.double() * y3 + v3.double()).reshape(-1, Cc)


def rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-300))

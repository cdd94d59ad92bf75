"""Float64 checker of the gaze shift (include/dwn.h dwn_gaze_args): forward, input gradient and shift gradient of a
per-frame bilinear translation, written with explicit slicing — own arithmetic, no grid_sample, nothing from the code under test.

Semantics: the plane v [H][W] is extended by the constant ``fill`` outside the frame; with iy = floor(dy), fy = dy - iy (ix, fx alike)

    out[y][x] = (1-fy)(1-fx) v(y+iy, x+ix) + (1-fy) fx v(y+iy, x+ix+1) + fy (1-fx) v(y+iy+1, x+ix) + fy fx v(y+iy+1, x+ix+1)

A shift given as a float32 tensor is taken as the kernels take it: floor and the subtraction dy - iy are done in float32 (the
subtraction is exact whenever dy has a fraction it can hold, and rounds to 1 for a tiny negative dy such as -1e-9), then everything
is float64.  A float64 shift (the model tests put a float64 MLP in front) is used as it is and may require grad: ``resample`` is
differentiable with iy, ix held constant, i.e. the right derivative at integer shifts.  A NaN / Inf shift gives a frame of NaN.
"""
from __future__ import annotations

import math

import torch

U = 2.0 ** -24


def _split(shift: torch.Tensor):
    """floor and fraction of a [..., 2] shift: (floor as float64, fraction as float64)."""
    if shift.dtype == torch.float32:
        fl = shift.floor()
        return fl.double(), (shift - fl).double()            # the float32 subtraction, as on the device
    fl = shift.detach().floor()
    return fl, shift - fl


def _int_shift(fl: float, size: int) -> int:
    """floor(shift) as a Python int, clamped to +-(size + 2): beyond that every tap is outside the frame anyway."""
    return int(min(max(fl, -(size + 2.0)), size + 2.0))


def extended(v: torch.Tensor, oy: int, ox: int, fill: float) -> torch.Tensor:
    """E[y][x] = v(y + oy, x + ox) of the plane extended by ``fill``; v [H][W]."""
    H, W = v.shape
    out = torch.full((H, W), float(fill), dtype=v.dtype)
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = v[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def _frame_taps(v, fl, H, W, fill):
    iy, ix = _int_shift(float(fl[0]), H), _int_shift(float(fl[1]), W)
    return (extended(v, iy, ix, fill), extended(v, iy, ix + 1, fill), extended(v, iy + 1, ix, fill),
            extended(v, iy + 1, ix + 1, fill)), iy, ix


def resample(x: torch.Tensor, shift: torch.Tensor, video_channel: int = 0, fill: float = 0.0, magnitudes: bool = False):
    """x [B][C][T][H][W] (any float type, used as float64), shift [B][T][2] -> out float64 (and, with ``magnitudes``, the per-element
    sum of |w v| over the four taps of the resampled channel, zero elsewhere).  Differentiable w.r.t. a float64 x / shift."""
    x = x.double()
    B, C, T, H, W = x.shape
    fl, fr = _split(shift)
    planes, mags = [], []
    for b in range(B):
        for t in range(T):
            if not bool(torch.isfinite(shift[b, t]).all()):
                planes.append(torch.full((H, W), math.nan, dtype=torch.float64))
                mags.append(torch.zeros(H, W, dtype=torch.float64))
                continue
            (s00, s01, s10, s11), _, _ = _frame_taps(x[b, video_channel, t], fl[b, t], H, W, fill)
            fy, fx = fr[b, t, 0], fr[b, t, 1]
            w00, w01, w10, w11 = (1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx
            planes.append(w00 * s00 + w01 * s01 + w10 * s10 + w11 * s11)
            if magnitudes:
                mags.append((w00 * s00.abs() + w01 * s01.abs() + w10 * s10.abs() + w11 * s11.abs()).detach())
    video = torch.stack(planes).view(B, T, H, W)
    out = torch.cat([x[:, :video_channel], video[:, None], x[:, video_channel + 1:]], dim=1)
    if not magnitudes:
        return out
    mag = torch.zeros_like(out)
    mag[:, video_channel] = torch.stack(mags).view(B, T, H, W)
    return out, mag


def backward(x: torch.Tensor, shift: torch.Tensor, dout: torch.Tensor, video_channel: int = 0, fill: float = 0.0):
    """The two gradients by their formulas (not autograd):
      dx      the adjoint gather sum_{a,b} w_a w_b dout[y-iy-a][x-ix-b] on the resampled channel (out-of-frame terms dropped),
              dout itself on the copied channels;
      dshift  [B][T][2] = sum_{y,x} dout * d out / d (dy, dx), iy and ix held constant.
    Returns dx, dx_mag (sum of |w dout| per element), dshift, dshift_mag (sum of |dout| |w| |v| over the terms), all float64.
    A NaN / Inf shift: dx = 0 and dshift = NaN for that frame."""
    x, dout = x.double(), dout.double()
    B, C, T, H, W = x.shape
    fl, fr = _split(shift.detach())
    dx, dx_mag = dout.clone(), torch.zeros_like(dout)
    dshift = torch.zeros(B, T, 2, dtype=torch.float64)
    dshift_mag = torch.zeros(B, T, 2, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            d = dout[b, video_channel, t]
            if not bool(torch.isfinite(shift[b, t]).all()):
                dx[b, video_channel, t] = 0.0
                dshift[b, t] = math.nan
                continue
            (s00, s01, s10, s11), iy, ix = _frame_taps(x[b, video_channel, t], fl[b, t], H, W, fill)
            fy, fx = float(fr[b, t, 0]), float(fr[b, t, 1])
            w = ((1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx)
            taps = [extended(d, -(iy + a), -(ix + c), 0.0) for a in (0, 1) for c in (0, 1)]
            dx[b, video_channel, t] = sum(wk * tk for wk, tk in zip(w, taps))
            dx_mag[b, video_channel, t] = sum(wk * tk.abs() for wk, tk in zip(w, taps))
            gy = (1 - fx) * (s10 - s00) + fx * (s11 - s01)
            gx = (1 - fy) * (s01 - s00) + fy * (s11 - s10)
            dshift[b, t, 0], dshift[b, t, 1] = (d * gy).sum(), (d * gx).sum()
            dshift_mag[b, t, 0] = (d.abs() * ((1 - fx) * (s10.abs() + s00.abs()) + fx * (s11.abs() + s01.abs()))).sum()
            dshift_mag[b, t, 1] = (d.abs() * ((1 - fy) * (s01.abs() + s00.abs()) + fy * (s11.abs() + s10.abs()))).sum()
    return dx, dx_mag, dshift, dshift_mag


def shift_jacobian(x: torch.Tensor, shift: torch.Tensor, video_channel: int = 0, fill: float = 0.0) -> torch.Tensor:
    """d out[b][vc][t][y][x] / d shift[b][t][k], iy and ix held constant: [B][T][2][H][W] float64 (a frame depends on its own shift
    only).  dshift is its contraction with dout; the model tests take sum |dout * jacobian| from it."""
    x = x.double()
    B, C, T, H, W = x.shape
    fl, fr = _split(shift.detach())
    jac = torch.zeros(B, T, 2, H, W, dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            (s00, s01, s10, s11), _, _ = _frame_taps(x[b, video_channel, t].detach(), fl[b, t], H, W, fill)
            fy, fx = float(fr[b, t, 0]), float(fr[b, t, 1])
            jac[b, t, 0] = (1 - fx) * (s10 - s00) + fx * (s11 - s01)
            jac[b, t, 1] = (1 - fy) * (s01 - s00) + fy * (s11 - s10)
    return jac


def plane_mean(x: torch.Tensor, channels) -> torch.Tensor:
    """[B][T][len(channels)] float64 mean over H x W."""
    return torch.stack([x[:, c].double().mean(dim=(2, 3)) for c in channels], dim=2)

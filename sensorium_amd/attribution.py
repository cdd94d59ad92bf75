"""Gradient-based attribution on a trained DwiseNeuro: what in the video drives a set of neurons.

Both functions differentiate the eval-mode model w.r.t. its input: BatchNorm normalises with its running statistics and leaves
them alone (the library's frozen-statistics mode, include/dwn.h DWN_BN_FROZEN), DropPath / Dropout are the identity, and the
forward / backward run in the HIP kernels; the few element-wise updates of the ascent are plain torch ops on the device.

Model input (src/inputs.py of the reference): (batch, 5, frames, height, width) — channel 0 the grey-level video in 0..255,
channels 1-4 the two behaviour and the two pupil-centre traces, each constant over a frame.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import torch

Index = Optional[Union[Sequence[int], torch.Tensor, slice]]


def _as_index(idx: Index, device) -> Union[torch.Tensor, slice]:
    if idx is None:
        return slice(None)
    if isinstance(idx, slice):
        return idx
    return torch.as_tensor(idx, dtype=torch.long, device=device)


def _response(model, x: torch.Tensor, mouse_index: int, neurons, frames, reduce: str) -> torch.Tensor:
    """Scalar objective: the chosen neurons' predicted responses [B, N, T], summed or averaged."""
    out = model(x, index=mouse_index)
    sel = out[:, neurons][:, :, frames]
    return sel.sum() if reduce == "sum" else sel.mean()


def _eval_mode(model):
    class _Scope:
        def __enter__(self):
            self.was_training = model.training
            model.eval()

        def __exit__(self, *exc):
            model.train(self.was_training)
            return False
    return _Scope()


def input_gradient(model, inputs: torch.Tensor, mouse_index: int, neurons: Index = None, frames: Index = None,
                   reduce: str = "sum") -> torch.Tensor:
    """d(response) / d(inputs): a tensor shaped like ``inputs`` (saliency / gradient receptive field).

    ``response`` is the sum (``reduce="sum"``) or mean (``"mean"``) over the batch, the chosen ``neurons`` (indices into the
    mouse's readout; default all) and ``frames`` (default all) of ``model(inputs, index=mouse_index)``.  The model is evaluated
    in eval mode (restored afterwards); parameter ``.grad`` fields are not touched."""
    if reduce not in ("sum", "mean"):
        raise ValueError("reduce: 'sum' or 'mean'")
    x = inputs.detach().clone().requires_grad_(True)
    with _eval_mode(model), torch.enable_grad():
        r = _response(model, x, mouse_index, _as_index(neurons, x.device), _as_index(frames, x.device), reduce)
        (grad,) = torch.autograd.grad(r, x)
    return grad


def most_exciting_input(model, mouse_index: int, neurons: Index, *, shape: Tuple[int, int, int] = (16, 64, 64), steps: int,
                        lr: float, init: Optional[torch.Tensor] = None, video_range: Tuple[float, float] = (0.0, 255.0),
                        norm_budget: Optional[float] = None, behavior: Optional[Sequence[float]] = None,
                        pupil_center: Optional[Sequence[float]] = None, frames: Index = None,
                        device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Most-exciting-input synthesis by projected gradient ascent on the video channel.

    Starts from ``init`` (a full model input [B, 5, T, H, W] or [5, T, H, W]; its channels 1-4 are kept as they are) or, without
    it, from a mid-grey clip of ``shape`` = (frames, height, width) with the behaviour / pupil-centre planes set to the constants
    ``behavior`` / ``pupil_center`` (two values each, default 0).  Each of the ``steps`` iterations takes the gradient of the
    summed response of ``neurons`` (over ``frames``, default all) w.r.t. the input, normalises its video part to unit RMS per
    clip, moves the video by ``lr`` grey levels along it, and projects: onto the ball of radius ``norm_budget`` (L2 norm of the
    deviation from mid-grey, per clip) if given, then onto ``video_range``.  Channels 1-4 never change.

    Everything stays on the device and nothing synchronises with the host inside the loop.  Returns ``(inputs, trace)``: the
    final model input (same shape as the start) and the response before each step plus the final one, ``steps + 1`` values on
    the device."""
    lo, hi = float(video_range[0]), float(video_range[1])
    mid = 0.5 * (lo + hi)
    if device is None:
        device = next(model.parameters()).device
    if init is not None:
        x = init.detach().to(device=device, dtype=torch.float32).clone()
        squeeze = x.dim() == 4
        if squeeze:
            x = x[None]
        if x.dim() != 5 or x.shape[1] < 1:
            raise ValueError("init: (batch, channels, frames, height, width) or (channels, frames, height, width)")
    else:
        squeeze = False
        t, h, w = shape
        x = torch.zeros(1, 5, t, h, w, dtype=torch.float32, device=device)
        x[:, 0] = mid
        for base, vals in ((1, behavior), (3, pupil_center)):
            if vals is not None:
                if len(vals) != 2:
                    raise ValueError("behavior / pupil_center: two values each")
                x[:, base] = float(vals[0])
                x[:, base + 1] = float(vals[1])
    x = x.contiguous()
    nsel = _as_index(neurons, device)
    fsel = _as_index(frames, device)
    trace = torch.zeros(steps + 1, dtype=torch.float32, device=device)
    per_clip = x[0, 0].numel()
    with _eval_mode(model):
        for i in range(steps):
            xg = x.detach().requires_grad_(True)
            with torch.enable_grad():
                r = _response(model, xg, mouse_index, nsel, fsel, "sum")
                (g,) = torch.autograd.grad(r, xg)
            trace[i] = r.detach()
            gv = g[:, 0]
            rms = gv.flatten(1).norm(dim=1).div_(per_clip ** 0.5).clamp_min_(1e-20)
            video = x[:, 0] + lr * gv / rms.view(-1, 1, 1, 1)
            if norm_budget is not None:
                dev_ = video - mid
                n = dev_.flatten(1).norm(dim=1).clamp_min_(1e-20)
                video = mid + dev_ * (float(norm_budget) / n).clamp_max_(1.0).view(-1, 1, 1, 1)
            x[:, 0] = video.clamp_(lo, hi)          # channels 1-4 are never written
        with torch.enable_grad():       # (input requiring grad: the last entry comes from the same kernels as the others)
            trace[steps] = _response(model, x.detach().requires_grad_(True), mouse_index, nsel, fsel, "sum").detach()
    return (x[0] if squeeze else x), trace

"""Parametric stimuli for in-silico experiments on a trained DwiseNeuro.

``DriftingGabor`` holds one row of eight parameters per clip and renders the whole model input — the Gabor in the video channel,
the behaviour and pupil-centre planes as constants — in one HIP pass (``ops.GaborFn``, include/dwn.h dwn_gabor_args).  Its
backward reduces the gradient of the model input to the eight parameters in float64 and a fixed order, so gradient ascent in
parameter space (``attribution.optimal_gabor``) needs neither autograd through a renderer nor a ``cat`` of the input channels.

Parameter order (``PARAM_NAMES``): cy, cx, sigma (pixels of the plane), theta (radians), sf (cycles / pixel), tf (cycles /
frame), phase (radians), amplitude (grey levels).
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch
from torch import nn

from . import ops

PARAM_NAMES = ("cy", "cx", "sigma", "theta", "sf", "tf", "phase", "amplitude")
ENVELOPES = tuple(ops.GABOR_ENVELOPES)


def check_window(window, size) -> Optional[Tuple[int, int, int, int]]:
    """(y0, x0, height, width) inside the (H, W) plane, or None for the whole plane."""
    if window is None:
        return None
    if len(window) != 4 or any(int(n) != n for n in window):
        raise ValueError("window: four integers (y0, x0, height, width)")
    y0, x0, wh, ww = (int(n) for n in window)
    H, W = size
    if y0 < 0 or x0 < 0 or wh <= 0 or ww <= 0 or y0 + wh > H or x0 + ww > W:
        raise ValueError(f"window {tuple(window)} is not inside the {H} x {W} plane")
    return y0, x0, wh, ww


def default_params(size, window=None, video_range=(0.0, 255.0)) -> Dict[str, float]:
    """A Gabor of moderate size in the centre of the window: sigma a sixth of its short side, ten pixels and ten frames per cycle,
    40 % of the video range (amplitude 1 without one)."""
    y0, x0, wh, ww = window if window is not None else (0, 0, size[0], size[1])
    amp = 0.4 * (float(video_range[1]) - float(video_range[0])) if video_range is not None else 1.0
    return dict(cy=y0 + 0.5 * (wh - 1), cx=x0 + 0.5 * (ww - 1), sigma=max(min(wh, ww) / 6.0, 1.0), theta=0.0, sf=0.1, tf=0.1,
                phase=0.0, amplitude=amp)


def param_table(batch: int, values: Dict[str, object], defaults: Dict[str, float]) -> torch.Tensor:
    """[batch, 8] fp32 on the CPU from a dict of name -> scalar or [batch]; names left out take ``defaults``."""
    unknown = [k for k in values if k not in PARAM_NAMES]
    if unknown:
        raise ValueError(f"unknown Gabor parameter(s) {unknown}: the names are {PARAM_NAMES}")
    table = torch.empty(batch, len(PARAM_NAMES), dtype=torch.float32)
    for k, name in enumerate(PARAM_NAMES):
        v = torch.as_tensor(values.get(name, defaults[name]), dtype=torch.float32).detach().cpu()
        if v.dim() > 1 or (v.dim() == 1 and v.numel() != batch):
            raise ValueError(f"init[{name!r}]: a scalar or {batch} values (got shape {tuple(v.shape)})")
        table[:, k] = v
    return table


def make_template(batch, in_channels, frames, size, video_channel, behavior, pupil_center) -> torch.Tensor:
    """[batch, in_channels, frames, H, W] fp32 zeros with the non-video channels set, in channel order, to the two ``behavior`` and
    the two ``pupil_center`` constants (further channels stay zero)."""
    template = torch.zeros(batch, in_channels, frames, *size, dtype=torch.float32)
    others = [c for c in range(in_channels) if c != video_channel]
    for c, v in zip(others, (*behavior, *pupil_center)):
        template[:, c] = float(v)
    return template


class DriftingGabor(nn.Module):
    """``batch`` drifting Gabors as one ``nn.Parameter`` ``params`` [batch, 8]; ``forward()`` returns the model input
    [batch, in_channels, frames, H, W].

    ``envelope``: "gaussian" or "none" (a full-field grating).  ``video_range``: (lo, hi) to clamp to, or None.  ``window``:
    (y0, x0, height, width) of the screen inside the plane (the reference pads a 36 x 64 screen into a 64 x 64 input); outside it
    the video holds ``pad``.  ``behavior`` / ``pupil_center``: the two constants each of the non-video channels, in channel order
    (further channels are zero).  ``learn``: the names whose gradient columns are kept; the others receive exactly zero.
    ``init``: name -> scalar or [batch]; the default is ``default_params``.  Every name of ``PARAM_NAMES`` is also a read-only
    view of its column, e.g. ``g.theta``."""

    def __init__(self, batch: int, frames: int, size: Tuple[int, int] = (64, 64), *, envelope: str = "gaussian",
                 background: float = 127.5, video_range: Optional[Tuple[float, float]] = (0.0, 255.0),
                 window: Optional[Sequence[int]] = None, pad: float = 0.0, behavior: Sequence[float] = (0.0, 0.0),
                 pupil_center: Sequence[float] = (0.0, 0.0), in_channels: int = 5, video_channel: int = 0,
                 learn: Sequence[str] = PARAM_NAMES, init: Optional[Dict[str, object]] = None):
        super().__init__()
        if int(batch) < 1 or int(frames) < 1:
            raise ValueError("batch and frames must be positive")
        if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError("size: (height, width), both positive")
        if envelope not in ENVELOPES:
            raise ValueError(f"envelope: one of {ENVELOPES} (got {envelope!r})")
        if int(in_channels) < 1 or not 0 <= int(video_channel) < int(in_channels):
            raise ValueError("video_channel must lie in [0, in_channels)")
        if video_range is not None and (len(video_range) != 2 or not float(video_range[0]) <= float(video_range[1])):
            raise ValueError("video_range: (lo, hi) with lo <= hi, or None")
        if len(behavior) != 2 or len(pupil_center) != 2:
            raise ValueError("behavior / pupil_center: two values each")
        learn = tuple(learn)
        unknown = [k for k in learn if k not in PARAM_NAMES]
        if unknown:
            raise ValueError(f"learn: unknown Gabor parameter(s) {unknown}: the names are {PARAM_NAMES}")
        self.batch, self.frames, self.size = int(batch), int(frames), (int(size[0]), int(size[1]))
        self.envelope, self.background, self.pad = envelope, float(background), float(pad)
        self.video_range = None if video_range is None else (float(video_range[0]), float(video_range[1]))
        self.window = check_window(window, self.size)
        self.in_channels, self.video_channel, self.learn = int(in_channels), int(video_channel), learn
        table = param_table(self.batch, dict(init or {}), default_params(self.size, self.window, self.video_range))
        self.params = nn.Parameter(table)
        self.register_buffer("learn_mask", torch.tensor([n in learn for n in PARAM_NAMES]), persistent=False)
        self.register_buffer("template", make_template(self.batch, self.in_channels, self.frames, self.size, self.video_channel,
                                                       behavior, pupil_center), persistent=False)

    def render(self, params: torch.Tensor) -> torch.Tensor:
        """The model input for explicit ``params`` [batch, 8] (differentiable in all eight columns)."""
        return ops.GaborFn.apply(params, self.template, self.video_channel, self.envelope, self.background, self.video_range,
                                 self.window, self.pad)

    def forward(self) -> torch.Tensor:
        p = self.params
        if not all(n in self.learn for n in PARAM_NAMES):
            p = torch.where(self.learn_mask, p, p.detach())
        return self.render(p)

    def extra_repr(self) -> str:
        return (f"batch={self.batch}, frames={self.frames}, size={self.size}, envelope={self.envelope!r}, "
                f"window={self.window}, video_range={self.video_range}, learn={self.learn}")


NOISE_KINDS = tuple(ops.NOISE_KINDS)


class NoiseStimulus(nn.Module):
    """Counter-based noise for receptive-field mapping: ``stim(first_clip=0)`` returns the model input
    [batch, in_channels, frames, H, W] of clips ``first_clip .. first_clip + batch - 1``.  A clip is a function of ``(seed, clip
    number)`` alone, so a long experiment is rendered batch by batch on the device and can be reproduced in any chunking.

    The window is tiled by ``cell`` x ``cell`` squares; each keeps its value for ``hold`` frames.  ``kind="binary"``: every cell is
    ``background + contrast`` or ``background - contrast`` with equal probability.  ``kind="sparse"``: a cell is dark with
    probability ``density / 2``, bright with the same probability and ``background`` otherwise.  Nothing is clamped, so
    ``background +- contrast`` must lie inside ``video_range``.  Geometry arguments are those of ``DriftingGabor``.  The module
    has no parameters and no gradient."""

    def __init__(self, batch: int, frames: int, size: Tuple[int, int] = (64, 64), *, kind: str = "binary", cell: int = 1,
                 hold: int = 1, contrast: float = 64.0, density: float = 0.1, background: float = 127.5,
                 video_range: Optional[Tuple[float, float]] = (0.0, 255.0), window: Optional[Sequence[int]] = None,
                 pad: float = 0.0, behavior: Sequence[float] = (0.0, 0.0), pupil_center: Sequence[float] = (0.0, 0.0),
                 in_channels: int = 5, video_channel: int = 0, seed: int = 0):
        super().__init__()
        if int(batch) < 1 or int(frames) < 1:
            raise ValueError("batch and frames must be positive")
        if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError("size: (height, width), both positive")
        if kind not in NOISE_KINDS:
            raise ValueError(f"kind: one of {NOISE_KINDS} (got {kind!r})")
        if int(in_channels) < 1 or not 0 <= int(video_channel) < int(in_channels):
            raise ValueError("video_channel must lie in [0, in_channels)")
        if video_range is not None and (len(video_range) != 2 or not float(video_range[0]) <= float(video_range[1])):
            raise ValueError("video_range: (lo, hi) with lo <= hi, or None")
        if len(behavior) != 2 or len(pupil_center) != 2:
            raise ValueError("behavior / pupil_center: two values each")
        if int(cell) != cell or int(hold) != hold or int(cell) < 1 or int(hold) < 1:
            raise ValueError("cell and hold: positive integers")
        if not float(contrast) >= 0.0 or not 0.0 <= float(density) <= 1.0:
            raise ValueError("contrast must not be negative and density must lie in [0, 1]")
        if int(seed) != seed or not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed: an integer in [0, 2^64)")
        self.batch, self.frames, self.size = int(batch), int(frames), (int(size[0]), int(size[1]))
        self.kind, self.cell, self.hold, self.seed = kind, int(cell), int(hold), int(seed)
        self.contrast, self.density, self.background, self.pad = float(contrast), float(density), float(background), float(pad)
        self.video_range = None if video_range is None else (float(video_range[0]), float(video_range[1]))
        self.window = check_window(window, self.size)
        wh, ww = self.window[2:] if self.window is not None else self.size
        if wh % self.cell or ww % self.cell:
            raise ValueError(f"cell = {self.cell} does not divide the {wh} x {ww} window")
        if self.video_range is not None and not (self.video_range[0] <= self.background - self.contrast
                                                 and self.background + self.contrast <= self.video_range[1]):
            raise ValueError(f"background +- contrast = {self.background} +- {self.contrast} leaves video_range {self.video_range}: "
                             "the noise is never clamped")
        self.grid = (wh // self.cell, ww // self.cell)
        self.in_channels, self.video_channel = int(in_channels), int(video_channel)
        self.register_buffer("template", make_template(self.batch, self.in_channels, self.frames, self.size, self.video_channel,
                                                       behavior, pupil_center), persistent=False)

    @torch.no_grad()
    def forward(self, first_clip: int = 0, batch: Optional[int] = None) -> torch.Tensor:
        """Clips ``first_clip .. first_clip + batch - 1`` (``batch``: at most the module's own, default all of it)."""
        n = self.batch if batch is None else int(batch)
        if not 1 <= n <= self.batch:
            raise ValueError(f"batch must lie in [1, {self.batch}]")
        return ops.noise_stimulus(self.template[:n], kind=self.kind, cell=self.cell, hold=self.hold, contrast=self.contrast,
                                  density=self.density, background=self.background, window=self.window, pad=self.pad,
                                  video_channel=self.video_channel, seed=self.seed, first_clip=first_clip)

    def extra_repr(self) -> str:
        return (f"batch={self.batch}, frames={self.frames}, size={self.size}, kind={self.kind!r}, cell={self.cell}, "
                f"hold={self.hold}, window={self.window}, seed={self.seed}")


def _column(k):
    return property(lambda self: self.params.detach()[:, k])


for _k, _name in enumerate(PARAM_NAMES):
    setattr(DriftingGabor, _name, _column(_k))

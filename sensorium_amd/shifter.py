"""Learned gaze shifter: the pupil centre, which the reference model sees only as two constant planes of its input,
mapped by a small network to a per-frame translation of the video channel, resampled bilinearly.

The resample, its two gradients and the per-plane mean of the pupil channels are HIP kernels (csrc/dwn_gaze.hip through
``ops.GazeShiftFn`` / ``ops.PlaneMeanFn``).  The MLP between them is plain torch on ``B*T`` rows of two numbers: plumbing, a dozen
tiny launches, in fp32 whatever the autocast state.  The reference has no shifter: a ``DwiseNeuroGaze`` whose last layer is still
zero (its initial state) computes exactly what the ``DwiseNeuro`` inside it computes.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from . import ops
from .dwiseneuro import DwiseNeuro


class GazeShifter(nn.Module):
    """``forward(x)``: x [B][C][T][H][W] with channel ``video_channel`` translated per frame by
    ``max_shift * tanh(MLP((mean(pupil planes) - pupil_mean) / pupil_std))`` pixels (dy, dx), every other channel unchanged.

    The gaze of a frame is the MEAN over the frame of each pupil plane: the planes are constant for a plain sample, but CutMix
    pastes all five channels inside its box, so a mixed sample's planes are not — the area-weighted mean is the one gaze a single
    translation can use.  ``pupil_mean`` / ``pupil_std`` are buffers (in the state_dict): the statistics of the data set's pupil
    centre, so that the MLP sees inputs of order one.  The last ``Linear`` starts at zero: the initial shift is exactly 0 and the
    resample is then a bit-exact copy."""

    def __init__(self, hidden_features: int = 16, hidden_layers: int = 1, max_shift: float = 8.0,
                 pupil_channels: Sequence[int] = (3, 4), video_channel: int = 0, fill: float = 0.0,
                 pupil_mean: Sequence[float] = (0., 0.), pupil_std: Sequence[float] = (1., 1.)):
        super().__init__()
        self.pupil_channels = tuple(int(c) for c in pupil_channels)
        if len(self.pupil_channels) < 1 or len(pupil_mean) != len(self.pupil_channels) or len(pupil_std) != len(self.pupil_channels):
            raise ValueError("GazeShifter: pupil_mean and pupil_std need one entry per pupil channel")
        if hidden_layers < 0 or hidden_features < 1:
            raise ValueError("GazeShifter: hidden_layers >= 0 and hidden_features >= 1")
        self.max_shift = float(max_shift)
        self.video_channel = int(video_channel)
        self.fill = float(fill)
        layers, width = [], len(self.pupil_channels)
        for _ in range(int(hidden_layers)):
            layers += [nn.Linear(width, hidden_features), nn.Tanh()]
            width = hidden_features
        last = nn.Linear(width, 2)
        nn.init.zeros_(last.weight)
        nn.init.zeros_(last.bias)
        self.mlp = nn.Sequential(*layers, last, nn.Tanh())
        self.register_buffer("pupil_mean", torch.tensor([float(v) for v in pupil_mean], dtype=torch.float32))
        self.register_buffer("pupil_std", torch.tensor([float(v) for v in pupil_std], dtype=torch.float32))

    def gaze(self, x: torch.Tensor) -> torch.Tensor:
        """Per-frame mean of the pupil planes, [B][T][len(pupil_channels)] fp32."""
        ch = self.pupil_channels
        if all(b - a == 1 for a, b in zip(ch, ch[1:])):
            return ops.PlaneMeanFn.apply(x, ch[0], len(ch))
        return torch.cat([ops.PlaneMeanFn.apply(x, c, 1) for c in ch], dim=2)

    def shifts(self, x: torch.Tensor) -> torch.Tensor:
        """The (dy, dx) shifts in pixels, [B][T][2] fp32, without resampling."""
        g = self.gaze(x)
        with torch.autocast(g.device.type, enabled=False):
            z = (g - self.pupil_mean) / self.pupil_std
            return self.mlp(z) * self.max_shift

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return ops.GazeShiftFn.apply(x, self.shifts(x), self.video_channel, self.fill)

    def extra_repr(self) -> str:
        return (f"max_shift={self.max_shift}, pupil_channels={self.pupil_channels}, video_channel={self.video_channel}, "
                f"fill={self.fill}")


class DwiseNeuroGaze(DwiseNeuro):
    """``DwiseNeuro`` behind a ``GazeShifter``: ``gaze_shifter`` holds the shifter's keyword arguments, everything else is the base
    class's.  The state_dict is the base's keys in the base's order, then ``shifter.*``; the shifter's parameters are registered
    last, so under data parallelism they form the last-completing, mandatory gradient bucket of their own behind the readouts'.

    BatchNorm mode in eval: decided from the CALLER's input and ``freeze_batchnorm()``, as in the base class — the shifted tensor
    requires grad whenever a shifter parameter does, which says nothing about what the caller wants.  To fit only the shifter on a
    trained model: ``model.eval(); model.freeze_batchnorm(True)``."""

    def __init__(self, *args, gaze_shifter: Optional[dict] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.shifter = GazeShifter(**(gaze_shifter or {}))

    def forward(self, x: torch.Tensor, index: Optional[int] = None):
        if x.dim() != 5:
            raise RuntimeError("DwiseNeuro expects (batch, channel, time, height, width)")
        feats = self.trunk(self.shifter(x), mode_from=x)
        if index is None:
            return [readout(feats) for readout in self.readouts]
        return self.readouts[index](feats)

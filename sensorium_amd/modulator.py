"""Behaviour modulator: pupil dilation and running speed, which the reference model sees only as two constant
planes of its input, mapped to a multiplicative gain of every neuron's response.

The gain, ``exp(max_log_gain * tanh(c[n] + h[b,t,:] . u[n,:]))`` on the readout's output, and its four gradients are HIP kernels
(csrc/dwn_modulator.hip through ``ops.ModulatorFn``); the per-frame behaviour traces come from ``ops.PlaneMeanFn``.  The small
network between them that turns two traces into ``K`` features per frame is plain torch on ``B*T`` rows: plumbing, in fp32
whatever the autocast state.  The reference has no modulator: a ``DwiseNeuroBehavior`` whose heads are still zero (their initial
state) computes exactly what the ``DwiseNeuro`` inside it computes.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from . import ops
from .dwiseneuro import DwiseNeuro
from .shifter import GazeShifter


class ModulatorHead(nn.Module):
    """One mouse's gain parameters: ``weight`` [N][K] and ``bias`` [N], both zero at construction (gain exactly 1)."""

    def __init__(self, out_features: int, in_features: int):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(int(out_features), int(in_features), dtype=torch.float32))
        self.bias = nn.Parameter(torch.zeros(int(out_features), dtype=torch.float32))

    def extra_repr(self) -> str:
        return f"in_features={self.weight.shape[1]}, out_features={self.weight.shape[0]}"


class BehaviorModulator(nn.Module):
    """``features(x)``: x [B][C][T][H][W] -> h [B][T][K]; ``forward(y, h, index)``: the readout output y [B][N][T] of mouse
    ``index`` times ``exp(max_log_gain * tanh(bias[n] + h[b,t,:] . weight[n,:]))``.

    The behaviour of a frame is the MEAN over the frame of each behaviour plane, for the reason given in ``GazeShifter``: the
    planes are constant for a plain sample, but CutMix pastes all channels inside its box.  ``behavior_mean`` / ``behavior_std``
    are buffers (in the state_dict): the statistics of the data set's traces, so that the network sees inputs of order one.
    ``derivative=True`` appends the frame-to-frame difference of each normalised trace (0 at the first frame).  A tanh MLP
    (``hidden_layers`` x ``Linear(., hidden_features)`` + ``Tanh``, then ``Linear(., features)`` + ``Tanh``) maps the traces to
    ``K = features`` numbers per frame; with ``hidden_layers=0`` and ``features=None`` there is no network and the normalised
    traces themselves are ``h``: the pure per-neuron linear gain model."""

    def __init__(self, readout_outputs: Sequence[int], features: Optional[int] = 8, hidden_features: int = 16,
                 hidden_layers: int = 1, max_log_gain: float = 2.0, behavior_channels: Sequence[int] = (1, 2),
                 derivative: bool = False, behavior_mean: Sequence[float] = (0., 0.), behavior_std: Sequence[float] = (1., 1.)):
        super().__init__()
        self.behavior_channels = tuple(int(c) for c in behavior_channels)
        nch = len(self.behavior_channels)
        if nch < 1 or len(behavior_mean) != nch or len(behavior_std) != nch:
            raise ValueError("BehaviorModulator: behavior_mean and behavior_std need one entry per behaviour channel")
        if any(c < 0 for c in self.behavior_channels):
            raise ValueError("BehaviorModulator: behaviour channels must be non-negative")
        if hidden_layers < 0 or hidden_features < 1:
            raise ValueError("BehaviorModulator: hidden_layers >= 0 and hidden_features >= 1")
        if features is None and hidden_layers != 0:
            raise ValueError("BehaviorModulator: features=None (the traces themselves) needs hidden_layers=0")
        if not (float(max_log_gain) > 0.0 and float(max_log_gain) < float("inf")):
            raise ValueError("BehaviorModulator: max_log_gain must be finite and positive")
        if len(readout_outputs) < 1 or any(int(n) < 1 for n in readout_outputs):
            raise ValueError("BehaviorModulator: readout_outputs must hold positive neuron counts")
        if features is not None and not 1 <= int(features) <= 32:
            raise ValueError("BehaviorModulator: between 1 and 32 features per frame")
        self.derivative = bool(derivative)
        self.max_log_gain = float(max_log_gain)
        width = nch * (2 if self.derivative else 1)
        if features is None:
            self.mlp = None
            self.features_out = width
        else:
            layers = []
            for _ in range(int(hidden_layers)):
                layers += [nn.Linear(width, hidden_features), nn.Tanh()]
                width = hidden_features
            self.mlp = nn.Sequential(*layers, nn.Linear(width, int(features)), nn.Tanh())
            self.features_out = int(features)
        if not 1 <= self.features_out <= 32:
            raise ValueError("BehaviorModulator: between 1 and 32 features per frame")
        self.register_buffer("behavior_mean", torch.tensor([float(v) for v in behavior_mean], dtype=torch.float32))
        self.register_buffer("behavior_std", torch.tensor([float(v) for v in behavior_std], dtype=torch.float32))
        self.heads = nn.ModuleList([ModulatorHead(int(n), self.features_out) for n in readout_outputs])

    def traces(self, x: torch.Tensor) -> torch.Tensor:
        """Per-frame mean of the behaviour planes, [B][T][len(behavior_channels)] fp32."""
        ch = self.behavior_channels
        if all(b - a == 1 for a, b in zip(ch, ch[1:])):
            return ops.PlaneMeanFn.apply(x, ch[0], len(ch))
        return torch.cat([ops.PlaneMeanFn.apply(x, c, 1) for c in ch], dim=2)

    def features(self, x: torch.Tensor) -> torch.Tensor:
        """The behaviour features h [B][T][K] fp32 of the model input x."""
        g = self.traces(x)
        with torch.autocast(g.device.type, enabled=False):
            z = (g - self.behavior_mean) / self.behavior_std
            if self.derivative:
                dz = torch.zeros_like(z)
                dz[:, 1:] = z[:, 1:] - z[:, :-1]
                z = torch.cat([z, dz], dim=2)
            return z if self.mlp is None else self.mlp(z)

    def forward(self, y: torch.Tensor, h: torch.Tensor, index: int) -> torch.Tensor:
        head = self.heads[index]
        return ops.ModulatorFn.apply(y, h, head.weight, head.bias, self.max_log_gain)

    def extra_repr(self) -> str:
        return (f"max_log_gain={self.max_log_gain}, behavior_channels={self.behavior_channels}, derivative={self.derivative}, "
                f"features={self.features_out}")


class DwiseNeuroBehavior(DwiseNeuro):
    """``DwiseNeuro`` with a ``BehaviorModulator`` behind its readouts and, when ``gaze_shifter`` is given, a ``GazeShifter`` in
    front of its core.  ``modulator`` / ``gaze_shifter`` hold the two modules' keyword arguments (``readout_outputs`` is passed
    on), everything else is the base class's.  The state_dict is the base's keys in the base's order, then ``shifter.*`` if
    present, then ``modulator.*``; the parameters are registered in that order.

    The behaviour features are taken ONCE from the caller's input (not from the shifted one: the shifter moves the video channel
    only) and shared by all readouts.  BatchNorm mode in eval: decided from the caller's input, as in ``DwiseNeuroGaze``."""

    def __init__(self, *args, gaze_shifter: Optional[dict] = None, modulator: Optional[dict] = None, **kwargs):
        super().__init__(*args, **kwargs)
        if gaze_shifter is not None:
            self.shifter = GazeShifter(**gaze_shifter)
        self.modulator = BehaviorModulator([r.out_features for r in self.readouts], **(modulator or {}))

    def forward(self, x: torch.Tensor, index: Optional[int] = None):
        if x.dim() != 5:
            raise RuntimeError("DwiseNeuro expects (batch, channel, time, height, width)")
        h = self.modulator.features(x)
        shifter = getattr(self, "shifter", None)
        feats = self.trunk(x) if shifter is None else self.trunk(shifter(x), mode_from=x)
        if index is None:
            return [self.modulator(readout(feats), h, k) for k, readout in enumerate(self.readouts)]
        return self.modulator(self.readouts[index](feats), h, index)

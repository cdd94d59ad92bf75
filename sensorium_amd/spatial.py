"""Retinotopic readout gain: every neuron gets a learned position on the core's feature map.

The reference pools the core map over its spatial axes before any per-neuron quantity exists, so where on the screen a neuron's
drive sits is not a parameter of that model.  Here each neuron samples the map bilinearly at its own position ``pos[n]`` and turns
what it finds there into a bounded multiplicative gain on the readout's output, ``exp(max_log_gain * tanh(bias[n] + weight[n,:] .
sample))``: the Poisson model's log link makes a multiplicative term the natural form, and the cortex never has to run per cell.

The gather, the gain and the five gradients (into the readout's output, the map, the positions, the weights and the offsets) are HIP
kernels (csrc/dwn_spatial.hip through ``ops.SpatialGainFn``).  The one projection in front of them, shared by all mice, that takes
the core's channels to ``features`` channels is plain torch in the map's dtype: plumbing.  A ``DwiseNeuroSpatial`` whose heads are
still zero (their initial state) computes exactly what the ``DwiseNeuro`` inside it computes.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import torch
from torch import nn

from . import ops
from .dwiseneuro import DwiseNeuro
from .modulator import BehaviorModulator
from .shifter import GazeShifter


class SpatialHead(nn.Module):
    """One mouse's parameters: ``pos`` [N][2] = (x, y) in normalised coordinates (-1 / +1: the centres of the first / last cell),
    ``weight`` [N][K] and ``bias`` [N]; the last two are zero at construction (gain exactly 1)."""

    def __init__(self, out_features: int, in_features: int, init_range: float, generator: torch.Generator):
        super().__init__()
        pos = (torch.rand(int(out_features), 2, generator=generator, dtype=torch.float32) * 2.0 - 1.0) * float(init_range)
        self.pos = nn.Parameter(pos)
        self.weight = nn.Parameter(torch.zeros(int(out_features), int(in_features), dtype=torch.float32))
        self.bias = nn.Parameter(torch.zeros(int(out_features), dtype=torch.float32))

    def extra_repr(self) -> str:
        return f"in_features={self.weight.shape[1]}, out_features={self.weight.shape[0]}"


class SpatialGain(nn.Module):
    """``project_map(core_map)``: [B][T][h][w][C] -> [B][T][h][w][K]; ``forward(y, g, index)``: the readout output y [B][N][T] of mouse
    ``index`` times ``exp(max_log_gain * tanh(bias[n] + weight[n,:] . sample(g[b,t], pos[n])))``.

    ``features=None`` samples the core's channels directly (no projection).  ``pos`` is drawn uniformly in
    ``[-init_range, init_range]^2`` from a generator seeded with ``seed`` (one stream, mouse after mouse).  ``detach_core=True``
    detaches the map: the branch then trains only its own parameters and asks the kernels for no map gradient.
    ``stride`` is the number of input pixels between two cells of the map (``DwiseNeuroSpatial`` sets it), used by ``positions``."""

    def __init__(self, readout_outputs: Sequence[int], in_features: int, features: Optional[int] = 16, max_log_gain: float = 1.0,
                 init_range: float = 0.5, seed: int = 0, detach_core: bool = False, stride: int = 1):
        super().__init__()
        if len(readout_outputs) < 1 or any(int(n) < 1 for n in readout_outputs):
            raise ValueError("SpatialGain: readout_outputs must hold positive neuron counts")
        if not (float(max_log_gain) > 0.0 and float(max_log_gain) < float("inf")):
            raise ValueError("SpatialGain: max_log_gain must be finite and positive")
        if not 0.0 <= float(init_range) <= 1.0:
            raise ValueError("SpatialGain: init_range must lie in [0, 1]")
        width = int(in_features) if features is None else int(features)
        if int(in_features) < 1 or not 1 <= width <= 64:
            raise ValueError("SpatialGain: between 1 and 64 sampled features")
        self.max_log_gain = float(max_log_gain)
        self.detach_core = bool(detach_core)
        self.features_out = width
        self.stride = int(stride)
        self.project = None if features is None else nn.Linear(int(in_features), width, bias=False)
        gen = torch.Generator().manual_seed(int(seed))
        self.heads = nn.ModuleList([SpatialHead(int(n), width, init_range, gen) for n in readout_outputs])
        self._map_size: Optional[Tuple[int, int]] = None

    def project_map(self, core_map: torch.Tensor) -> torch.Tensor:
        """The sampled map g [B][T][h][w][K] (channels-last, the core map's dtype) of the core's output."""
        if core_map.dim() != 5:
            raise RuntimeError("SpatialGain: the core map must be [B][T][h][w][C]")
        if self.detach_core:
            core_map = core_map.detach()
        self._map_size = (int(core_map.shape[2]), int(core_map.shape[3]))
        if self.project is None:
            return core_map
        with torch.autocast(core_map.device.type, enabled=False):
            return torch.nn.functional.linear(core_map, self.project.weight.to(core_map.dtype))

    def forward(self, y: torch.Tensor, g: torch.Tensor, index: int) -> torch.Tensor:
        head = self.heads[index]
        return ops.SpatialGainFn.apply(y, g, head.pos, head.weight, head.bias, self.max_log_gain)

    def position_parameters(self):
        return [head.pos for head in self.heads]

    @torch.no_grad()
    def positions(self, index: int, units: str = "normalised", map_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """The clamped receptive-field centres [N][2] = (x, y) of mouse ``index``.  ``"normalised"``: in [-1, 1]; ``"cells"``: in
        cells of the map (0 = the first cell's centre); ``"input"``: in input pixels.  Cell j sits at pixel ``j * stride``: the
        core's strided convolutions pad k // 2, so output j is centred on input pixel j * s and no half-pixel term appears
        (tests/test_host_spatial_gain.py checks it with a delta image through the oracle's depth-wise convolution).
        ``map_size`` = (h, w) of the map; by default the one of the last forward."""
        pos = self.heads[index].pos.detach().float().clamp(-1.0, 1.0)
        if units == "normalised":
            return pos
        if units not in ("cells", "input"):
            raise ValueError("SpatialGain.positions: units must be 'normalised', 'cells' or 'input'")
        size = map_size if map_size is not None else self._map_size
        if size is None:
            raise RuntimeError("SpatialGain.positions: the map's size is not known yet (pass map_size or run a forward)")
        scale = torch.tensor([size[1] - 1, size[0] - 1], dtype=torch.float32, device=pos.device)
        cells = (pos + 1.0) * 0.5 * scale
        return cells if units == "cells" else cells * float(self.stride)

    @torch.no_grad()
    def set_positions(self, index: int, xy: torch.Tensor, units: str = "normalised", neurons=None,
                      map_size: Optional[Tuple[int, int]] = None) -> None:
        """The inverse of ``positions``: writes ``xy`` [n][2] = (x, y) in ``units`` into the positions of mouse ``index``, in place
        (rows ``neurons``, an index tensor or sequence; default all).  Non-finite values are refused; the result is clamped to
        [-1, 1].  A map side of one cell has no extent: its coordinate is set to 0."""
        pos = self.heads[index].pos
        xy = torch.as_tensor(xy).detach().to(device=pos.device, dtype=torch.float64)
        rows = None if neurons is None else torch.as_tensor(neurons, device=pos.device).long().flatten()
        n = int(pos.shape[0]) if rows is None else int(rows.numel())
        if xy.shape != (n, 2):
            raise ValueError(f"SpatialGain.set_positions: xy must be [{n}][2] (got {tuple(xy.shape)})")
        if not bool(torch.isfinite(xy).all()):
            raise ValueError("SpatialGain.set_positions: non-finite position")
        if units != "normalised":
            if units not in ("cells", "input"):
                raise ValueError("SpatialGain.set_positions: units must be 'normalised', 'cells' or 'input'")
            size = map_size if map_size is not None else self._map_size
            if size is None:
                raise RuntimeError("SpatialGain.set_positions: the map's size is not known yet (pass map_size or run a forward)")
            cells = xy if units == "cells" else xy / float(self.stride)
            scale = torch.tensor([size[1] - 1, size[0] - 1], dtype=torch.float64, device=pos.device)
            xy = torch.where(scale > 0, 2.0 * cells / scale.clamp(min=1.0) - 1.0, torch.zeros_like(cells))
        new = xy.clamp(-1.0, 1.0).to(pos.dtype)
        if rows is None:
            pos.copy_(new)
        else:
            pos[rows] = new

    def extra_repr(self) -> str:
        return f"max_log_gain={self.max_log_gain}, features={self.features_out}, detach_core={self.detach_core}, stride={self.stride}"


class DwiseNeuroSpatial(DwiseNeuro):
    """``DwiseNeuro`` with a ``SpatialGain`` behind its readouts, optionally a ``BehaviorModulator`` behind that and a
    ``GazeShifter`` in front of its core.  ``spatial`` / ``gaze_shifter`` / ``modulator`` hold the modules' keyword arguments
    (``readout_outputs``, the core's width and its total stride are passed on), everything else is the base class's.  The state_dict
    is the base's keys in the base's order, then ``shifter.*``, then ``spatial.*``, then ``modulator.*``; the parameters are
    registered in that order.

    The core map has two consumers here, the pool and the sampled gain: autograd adds their two gradients before the last block's
    backward sees them.  The behaviour features are taken from the caller's input, as in ``DwiseNeuroBehavior``."""

    def __init__(self, *args, spatial: Optional[dict] = None, gaze_shifter: Optional[dict] = None,
                 modulator: Optional[dict] = None, **kwargs):
        super().__init__(*args, **kwargs)
        if gaze_shifter is not None:
            self.shifter = GazeShifter(**gaze_shifter)
        blocks = list(self.core.blocks)[1::2]
        self.total_stride = int(math.prod(int(b.spatial_stride) for b in blocks))
        self.spatial = SpatialGain([r.out_features for r in self.readouts], int(blocks[-1].out_features),
                                   **{"stride": self.total_stride, **(spatial or {})})
        if modulator is not None:
            self.modulator = BehaviorModulator([r.out_features for r in self.readouts], **modulator)

    def position_parameters(self):
        """The per-neuron positions: they take no weight decay (MouseModel puts them with the Softplus gate parameters)."""
        return self.spatial.position_parameters()

    def map_size(self, height: int, width: int) -> Tuple[int, int]:
        """(h, w) of the core map for an input of ``height`` x ``width`` pixels."""
        for b in list(self.core.blocks)[1::2]:
            s = int(b.spatial_stride)
            height, width = (height - 1) // s + 1, (width - 1) // s + 1
        return height, width

    def positions(self, index: int, units: str = "normalised", input_size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """``SpatialGain.positions`` with the map's size derived from ``input_size`` = (H, W) of the video."""
        return self.spatial.positions(index, units, None if input_size is None else self.map_size(*input_size))

    def set_positions_from(self, fits, index: int, *, input_size: Tuple[int, int], min_r2: float = 0.5, neurons=None) -> torch.Tensor:
        """Writes the fitted receptive-field centres (``GaussianFits``) into the positions of mouse ``index``,
        in input pixels, for the fits that pass ``fits.good(min_r2)``; every other neuron is left alone.  ``neurons``: the model's
        neuron of every row of ``fits`` (default row k is neuron k).  Returns the index tensor of the neurons written."""
        rows = fits.good(min_r2)
        xy = fits.centres("input")[rows].flip(1)
        dev = self.spatial.heads[index].pos.device
        target = rows if neurons is None else torch.as_tensor(neurons, device=rows.device).long().flatten()[rows]
        target = target.to(dev)
        if target.numel():
            self.spatial.set_positions(index, xy.to(dev), "input", neurons=target, map_size=self.map_size(*input_size))
        return target

    @torch.no_grad()
    def position_error(self, fits, index: int, input_size: Tuple[int, int]) -> torch.Tensor:
        """[N] distance in input pixels between the learned position and the fitted centre of every neuron of mouse ``index`` (row k
        of ``fits`` is neuron k); NaN where a map has no fit."""
        learned = self.positions(index, "input", input_size).double()
        fitted = fits.centres("input").flip(1).to(learned.device)
        if fitted.shape != learned.shape:
            raise ValueError(f"position_error: {tuple(fitted.shape)} fitted centres for {tuple(learned.shape)} positions")
        return (learned - fitted).norm(dim=1)

    def forward(self, x: torch.Tensor, index: Optional[int] = None):
        if x.dim() != 5:
            raise RuntimeError("DwiseNeuro expects (batch, channel, time, height, width)")
        modulator = getattr(self, "modulator", None)
        shifter = getattr(self, "shifter", None)
        h = None if modulator is None else modulator.features(x)
        if shifter is None:
            feats, core_map = self.trunk_with_map(x)
        else:
            feats, core_map = self.trunk_with_map(shifter(x), mode_from=x)
        g = self.spatial.project_map(core_map)

        def head(k):
            y = self.spatial(self.readouts[k](feats), g, k)
            return y if modulator is None else modulator(y, h, k)

        if index is None:
            return [head(k) for k in range(len(self.readouts))]
        return head(index)

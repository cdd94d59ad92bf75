"""Receptive-field mapping by reverse correlation: the spatio-temporal receptive field of every neuron at
once from the model's responses to a stimulus, at the price of eval forwards plus one lagged cross-correlation per batch.

``StaAccumulator`` keeps the float64 state on the device: the lagged cross-sums of the responses with the cell means of the
stimulus and the four moment vectors, all as sums of deviations from a stimulus centre ``s0`` and per-neuron response centres
``r0`` (the covariance does not depend on them; with centres near the means nothing cancels).  ``compute()`` turns the state into
``ReceptiveFields``: the covariance map (the spike-triggered average up to a factor), its z-score against the null of no
coupling, and per neuron the peak lag, the polarity, and the centre and size of the field.  ``attribution.receptive_fields`` is
the whole experiment on a model: noise -> eval forward -> ``add``.

``fit_gaussian2d`` / ``ReceptiveFields.fit`` (section 12r) put an elliptical Gaussian through every map on the device —
``GaussianFits``: centre, sigmas, orientation, R2, standard errors, the temporal kernel on the fitted shape and a space-time
separability index.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import ops
from .stimuli import check_window

SUMMARY_COLUMNS = ("peak_lag", "peak_z", "cy", "cx", "sy", "sx", "lag_share", "cells")


class ReceptiveFields:
    """The result of ``StaAccumulator.compute``; every tensor lives on the accumulator's device.

    ``sta`` fp32 [N, L, gh, gw]: cov(response_t, stimulus cell at t - l).  ``z`` (or None): the same as a z-score,
    ``corr * sqrt(samples)``.  ``summary`` float64 [N, 8] in the order of ``SUMMARY_COLUMNS`` (include/dwn.h dwn_sta_args)."""

    def __init__(self, sta, z, summary, samples: int, window: Tuple[int, int, int, int], cell: int, size: Tuple[int, int]):
        self.sta, self.z, self.summary, self.samples = sta, z, summary, int(samples)
        self.window, self.cell, self.size = tuple(window), int(cell), tuple(size)
        self.accumulator = None                     # set by attribution.receptive_fields: the state to continue with
        self.fits = None                            # set by fit(): the parametric fits (GaussianFits)

    @property
    def peak_lag(self) -> torch.Tensor:
        return self.summary[:, 0].long()

    @property
    def polarity(self) -> torch.Tensor:
        """+1 (ON), -1 (OFF) or 0 (no field): the sign of the peak cell."""
        return torch.sign(self.summary[:, 1])

    def centres(self, units: str = "cells") -> torch.Tensor:
        """[N, 2] = (y, x) of the field centres; NaN where a neuron has no field.  ``"cells"``: cell indices of the grid.
        ``"input"``: pixel coordinates of the model input (the cell's centre times ``cell``, plus the window origin).
        ``"normalised"``: (x, y) with -1 / +1 the centres of the first / last pixel of the input plane, the convention (and the
        column order) of ``DwiseNeuroSpatial.positions``."""
        c = self.summary[:, 2:4]
        if units == "cells":
            return c.clone()
        if units not in ("input", "normalised"):
            raise ValueError("units: 'cells', 'input' or 'normalised'")
        origin = torch.tensor([self.window[0], self.window[1]], dtype=c.dtype, device=c.device)
        pix = (c + 0.5) * self.cell - 0.5 + origin
        if units == "input":
            return pix
        H, W = self.size
        span = torch.tensor([max(H - 1, 1), max(W - 1, 1)], dtype=c.dtype, device=c.device)
        return (2.0 * pix / span - 1.0).flip(1)

    def significant(self, min_z: float) -> torch.Tensor:
        """Indices (a device LongTensor) of the neurons whose peak cell reaches ``|z| >= min_z``."""
        return torch.nonzero(self.summary[:, 1].abs() >= float(min_z)).flatten()

    def fit(self, lag="peak", profile: bool = True, **options) -> "GaussianFits":
        """The elliptical-Gaussian fit of one lag of every neuron's map, kept as ``.fits`` and returned.
        ``lag``: ``"peak"`` (each neuron's peak lag), one int for all, or a LongTensor [N].  The slices are chosen through the
        kernel's row table: no copy of the map is made and nothing is read back.  ``profile``: also the temporal kernel of the whole
        map on the fitted shape and the separability index.  ``options``: those of ``fit_gaussian2d``."""
        N, lags, gh, gw = (int(n) for n in self.sta.shape)
        dev = self.sta.device
        if isinstance(lag, str):
            if lag != "peak":
                raise ValueError("lag: 'peak', an int or a LongTensor [N]")
            lag_n = self.summary[:, 0].to(torch.int32)
        elif torch.is_tensor(lag):
            if lag.shape != (N,) or lag.dtype not in (torch.int64, torch.int32):
                raise ValueError(f"lag: an integer tensor [{N}] (got {tuple(lag.shape)}, {lag.dtype})")
            lag_n = lag.to(device=dev, dtype=torch.int32).clamp(0, lags - 1)
        else:
            if not 0 <= int(lag) < lags:
                raise ValueError(f"lag = {lag} outside [0, {lags})")
            lag_n = torch.full((N,), int(lag), dtype=torch.int32, device=dev)
        sel = (torch.arange(N, dtype=torch.int32, device=dev) * lags + lag_n).contiguous()
        fits = fit_gaussian2d(self.sta.view(N * lags, gh, gw), sel=sel, window=self.window, cell=self.cell, size=self.size, **options)
        fits.lag = lag_n.long()
        if profile:
            fits.profile, fits.separability = ops.gauss2d_profile(fits.params, self.sta, fit_baseline=fits.fit_baseline)
        self.fits = fits
        return fits


GAUSS_FIT_COLUMNS = ("status", "iterations", "baseline", "amplitude", "cy", "cx", "sigma_major", "sigma_minor", "theta", "sse", "r2",
                     "se_cy", "se_cx", "se_amplitude", "lambda", "row")


class GaussianFits:
    """The result of ``fit_gaussian2d`` / ``ReceptiveFields.fit``; every tensor lives on the maps' device.

    ``table`` float64 [M, 16] in the order of ``GAUSS_FIT_COLUMNS`` and ``params`` float64 [M, 7] =
    (b, a, cy, cx, log l11, l21, log l22) (include/dwn.h dwn_gauss2d_args); ``profile`` float64 [M, L] and ``separability`` [M]
    where the fit was asked for them (else None); ``start`` float64 [M, 8]: the start vector and its S."""

    def __init__(self, table, params, start, grid: Tuple[int, int], window: Tuple[int, int, int, int], cell: int, size: Tuple[int, int],
                 fit_baseline: bool):
        self.table, self.params, self.start = table, params, start
        self.grid, self.window, self.cell, self.size = tuple(grid), tuple(window), int(cell), tuple(size)
        self.fit_baseline = bool(fit_baseline)
        self.profile = self.separability = self.lag = None

    def column(self, name: str) -> torch.Tensor:
        return self.table[:, GAUSS_FIT_COLUMNS.index(name)]

    @property
    def theta(self) -> torch.Tensor:
        """The angle of the major axis from the x axis, in (-pi/2, pi/2]."""
        return self.table[:, 8]

    @property
    def r2(self) -> torch.Tensor:
        return self.table[:, 10]

    @property
    def converged(self) -> torch.Tensor:
        return self.table[:, 0] == 0

    def centres(self, units: str = "cells") -> torch.Tensor:
        """[M, 2] fitted centres, NaN where a map has no fit; the units (and, for ``"normalised"``, the (x, y) column order) of
        ``ReceptiveFields.centres``."""
        c = self.table[:, 4:6]
        if units == "cells":
            return c.clone()
        if units not in ("input", "normalised"):
            raise ValueError("units: 'cells', 'input' or 'normalised'")
        origin = torch.tensor([self.window[0], self.window[1]], dtype=c.dtype, device=c.device)
        pix = (c + 0.5) * self.cell - 0.5 + origin
        if units == "input":
            return pix
        H, W = self.size
        span = torch.tensor([max(H - 1, 1), max(W - 1, 1)], dtype=c.dtype, device=c.device)
        return (2.0 * pix / span - 1.0).flip(1)

    def sigmas(self, units: str = "cells") -> torch.Tensor:
        """[M, 2] = (sigma_major, sigma_minor) in cells or in input pixels."""
        if units not in ("cells", "input"):
            raise ValueError("units: 'cells' or 'input'")
        s = self.table[:, 6:8]
        return s.clone() if units == "cells" else s * float(self.cell)

    def good(self, min_r2: float, max_se: Optional[float] = None) -> torch.Tensor:
        """Indices (a device LongTensor) of the converged fits with ``r2 >= min_r2`` and, with ``max_se``, both centre standard
        errors (in cells) at most ``max_se``."""
        ok = self.converged & (self.r2 >= float(min_r2))
        if max_se is not None:
            ok = ok & (self.table[:, 11] <= float(max_se)) & (self.table[:, 12] <= float(max_se))
        return torch.nonzero(ok).flatten()

    def render(self) -> torch.Tensor:
        """The model maps float64 [M, gh, gw] (NaN where a map has no fit), by plain torch: for plots."""
        gh, gw = self.grid
        p = self.params
        y = torch.arange(gh, dtype=torch.float64, device=p.device).view(1, gh, 1)
        x = torch.arange(gw, dtype=torch.float64, device=p.device).view(1, 1, gw)
        b, a, cy, cx, u1, l21, u2 = (p[:, k].view(-1, 1, 1) for k in range(7))
        dx, dy = x - cx, y - cy
        u, v = torch.exp(u1) * dx, l21 * dx + torch.exp(u2) * dy
        return b + a * torch.exp(-0.5 * (u * u + v * v))


def fit_gaussian2d(maps: torch.Tensor, *, sel: Optional[torch.Tensor] = None, baseline: str = "fit", rel_threshold: float = 0.5,
                   max_iter: int = 100, xtol: float = 1e-8, ftol: float = 1e-12, window: Optional[Sequence[int]] = None, cell: int = 1,
                   size: Optional[Tuple[int, int]] = None) -> GaussianFits:
    """An elliptical Gaussian ``b + a exp(-q / 2)`` fitted to every map of ``maps`` fp32 [R, gh, gw] on the device (a receptive-field
    slice, a saliency frame, an MEI frame) by Levenberg-Marquardt, one wave per map in one launch.
    ``sel``: an integer device tensor of the rows to fit, in the order of the result (default all).  ``baseline``: ``"fit"`` or
    ``"zero"`` (b held at 0).  ``window`` / ``cell`` / ``size``: where the grid lies in an input plane, for the unit conversions of
    the result (default: the grid is the plane)."""
    if not maps.is_cuda:
        raise RuntimeError(f"sensorium_amd.fit_gaussian2d: tensors must be on a GPU (got {maps.device}); the HIP path has no CPU fallback")
    if maps.dim() != 3 or maps.dtype != torch.float32:
        raise ValueError(f"maps: fp32 [R, gh, gw] (got {tuple(maps.shape)}, {maps.dtype})")
    if baseline not in ("fit", "zero"):
        raise ValueError("baseline: 'fit' or 'zero'")
    if not 0.0 <= float(rel_threshold) <= 1.0:
        raise ValueError("rel_threshold must lie in [0, 1]")
    if int(max_iter) < 0 or not float(xtol) >= 0.0 or not float(ftol) >= 0.0:
        raise ValueError("max_iter, xtol and ftol must not be negative")
    gh, gw = int(maps.shape[1]), int(maps.shape[2])
    if sel is not None:
        if not torch.is_tensor(sel) or sel.dim() != 1 or sel.dtype not in (torch.int32, torch.int64) or sel.numel() < 1:
            raise ValueError("sel: a non-empty integer tensor [M]")
        sel = sel.to(device=maps.device, dtype=torch.int32).contiguous()
    window = tuple(int(n) for n in window) if window is not None else (0, 0, gh * int(cell), gw * int(cell))
    if window[2] != gh * int(cell) or window[3] != gw * int(cell):
        raise ValueError(f"window {window} does not hold {gh} x {gw} cells of {cell} pixels")
    size = (int(size[0]), int(size[1])) if size is not None else (window[0] + window[2], window[1] + window[3])
    params, table, start = ops.gauss2d_fit(maps.contiguous(), sel, fit_baseline=baseline == "fit", rel_threshold=rel_threshold,
                                           max_iter=max_iter, xtol=xtol, ftol=ftol)
    return GaussianFits(table, params, start, (gh, gw), window, cell, size, baseline == "fit")


class StaAccumulator:
    """Lagged spike-triggered average of ``num_neurons`` responses against any stimulus of plane ``size`` = (H, W).

    ``lags``: the map covers frames t, t - 1, ..., t - lags + 1.  ``window`` = (y0, x0, height, width) of the stimulus inside the
    plane (default all of it), tiled by ``cell`` x ``cell`` squares whose means are correlated; ``channel``: the stimulus channel.
    Frames below ``max(skip, lags - 1)`` of every clip are left out (the model's warm-up).  ``stimulus_centre`` and
    ``response_centre`` ([N] or None = zeros) are the shifts of the sums."""

    def __init__(self, num_neurons: int, lags: int, size: Tuple[int, int], *, window: Optional[Sequence[int]] = None, cell: int = 1,
                 channel: int = 0, skip: int = 0, stimulus_centre: float = 127.5, response_centre: Optional[torch.Tensor] = None,
                 device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"sensorium_amd.StaAccumulator: the state lives on a GPU (got {device}); the HIP path has no CPU fallback")
        if int(num_neurons) < 1 or int(lags) < 1 or int(skip) < 0 or int(channel) < 0 or int(cell) < 1:
            raise ValueError("num_neurons, lags and cell must be positive, skip and channel not negative")
        if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
            raise ValueError("size: (height, width), both positive")
        self.N, self.lags, self.size = int(num_neurons), int(lags), (int(size[0]), int(size[1]))
        self.window = check_window(window, self.size) or (0, 0, *self.size)
        self.cell, self.channel, self.skip, self.s0 = int(cell), int(channel), int(skip), float(stimulus_centre)
        if self.window[2] % self.cell or self.window[3] % self.cell:
            raise ValueError(f"cell = {self.cell} does not divide the {self.window[2]} x {self.window[3]} window")
        self.grid = (self.window[2] // self.cell, self.window[3] // self.cell)
        self.device = device
        self.r0 = None
        if response_centre is not None:
            if not response_centre.is_cuda:
                raise RuntimeError(f"sensorium_amd.StaAccumulator: tensors must be on a GPU (got {response_centre.device}); "
                                   "the HIP path has no CPU fallback")
            if response_centre.shape != (self.N,):
                raise ValueError(f"response_centre: [{self.N}] (got {tuple(response_centre.shape)})")
            self.r0 = response_centre.detach().to(device=device, dtype=torch.float32).contiguous().clone()
        self.state = torch.zeros(ops.sta_state_numel(self.N, self.lags, self.window, self.cell), dtype=torch.float64, device=device)
        self.samples = 0

    def add(self, x: torch.Tensor, responses: torch.Tensor) -> "StaAccumulator":
        """One batch: ``x`` [B, C, T, H, W] fp32 (the model input) and ``responses`` [B, N, T] (fp32 or bf16).  Never synchronises."""
        if not x.is_cuda or not responses.is_cuda:
            raise RuntimeError(f"sensorium_amd.StaAccumulator: tensors must be on a GPU (got {x.device}, {responses.device}); "
                               "the HIP path has no CPU fallback")
        if x.dim() != 5 or tuple(x.shape[3:]) != self.size or not self.channel < x.shape[1]:
            raise ValueError(f"x: [B, C > {self.channel}, T, {self.size[0]}, {self.size[1]}] (got {tuple(x.shape)})")
        if responses.dim() != 3 or responses.shape[0] != x.shape[0] or responses.shape[1] != self.N or responses.shape[2] != x.shape[2]:
            raise ValueError(f"responses: [{x.shape[0]}, {self.N}, {x.shape[2]}] (got {tuple(responses.shape)})")
        if max(self.skip, self.lags - 1) >= x.shape[2]:
            raise ValueError(f"clips of {x.shape[2]} frames hold no valid frame for lags = {self.lags}, skip = {self.skip}")
        self.samples += ops.sta_accumulate(self.state, x.detach().float(), responses.detach().float(), lags=self.lags, window=self.window,
                                           cell=self.cell, channel=self.channel, skip=self.skip, s0=self.s0, r0=self.r0)
        return self

    def compute(self, rel_threshold: float = 0.5, z: bool = True) -> ReceptiveFields:
        if self.samples < 1:
            raise RuntimeError("sensorium_amd.StaAccumulator: compute() before the first add()")
        if not 0.0 <= float(rel_threshold) <= 1.0:
            raise ValueError("rel_threshold must lie in [0, 1]")
        cov, zz, summary = ops.sta_finalize(self.state, self.samples, N=self.N, lags=self.lags, window=self.window, cell=self.cell,
                                            rel_threshold=rel_threshold, z=z)
        return ReceptiveFields(cov, zz, summary, self.samples, self.window, self.cell, self.size)

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


def _set_response(model, x: torch.Tensor, mouse_index: int, idx: torch.Tensor, maskf: torch.Tensor, frames) -> torch.Tensor:
    """[B] objectives: clip b's predicted responses summed over its own neurons ``idx[b]`` (padded; ``maskf`` marks the real
    entries) and the chosen frames.  A padded gather and a mask: plain torch, nothing synchronises with the host."""
    out = model(x, index=mouse_index)                            # [B, N, T]
    sel = out.gather(1, idx[:, :, None].expand(-1, -1, out.shape[2]))[:, :, frames].float()
    return (sel * maskf[:, :, None]).sum(dim=(1, 2))


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
    in eval mode (restored afterwards); parameter ``.grad`` fields are not touched.  ``neurons`` may also be one index list per
    clip (a sequence of ``B`` sequences, possibly ragged, or a 2-D LongTensor; ``reduce="sum"``): the eval-mode clips are
    independent, so clip ``b`` then holds the gradient of the summed response of its own set."""
    if reduce not in ("sum", "mean"):
        raise ValueError("reduce: 'sum' or 'mean'")
    x = inputs.detach().clone().requires_grad_(True)
    if _per_clip_sets(neurons):         # one index list per clip: clip b gets the gradient of the response of its own set
        if reduce != "sum":
            raise ValueError("per-clip neuron sets: reduce must be 'sum'")
        idx, maskf = _padded_sets(neurons, x.device)
        if idx.shape[0] != x.shape[0]:
            raise ValueError(f"neurons: {idx.shape[0]} index lists for {x.shape[0]} clips")
        with _eval_mode(model), torch.enable_grad():
            (grad,) = torch.autograd.grad(_set_response(model, x, mouse_index, idx, maskf, _as_index(frames, x.device)).sum(), x)
        return grad
    with _eval_mode(model), torch.enable_grad():
        r = _response(model, x, mouse_index, _as_index(neurons, x.device), _as_index(frames, x.device), reduce)
        (grad,) = torch.autograd.grad(r, x)
    return grad


def most_exciting_input(model, mouse_index: int, neurons: Index, *, shape: Tuple[int, int, int] = (16, 64, 64), steps: int,
                        lr: float, init: Optional[torch.Tensor] = None, video_range: Tuple[float, float] = (0.0, 255.0),
                        norm_budget: Optional[float] = None, behavior: Optional[Sequence[float]] = None,
                        pupil_center: Optional[Sequence[float]] = None, frames: Index = None,
                        device=None, blur_sigma=None, mean: Optional[float] = None, contrast: Optional[float] = None,
                        contrast_mode: str = "max", window: Optional[Sequence[int]] = None,
                        use_graph: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Most-exciting-input synthesis by projected gradient ascent on the video channel.

    Starts from ``init`` (a full model input [B, 5, T, H, W] or [5, T, H, W]; its channels 1-4 are kept as they are) or, without
    it, from a mid-grey clip of ``shape`` = (frames, height, width) with the behaviour / pupil-centre planes set to the constants
    ``behavior`` / ``pupil_center`` (two values each, default 0).  Each of the ``steps`` iterations takes the gradient of the
    summed response of ``neurons`` (over ``frames``, default all) w.r.t. the input, normalises its video part to unit RMS per
    clip, moves the video by ``lr`` grey levels along it, and projects: onto the ball of radius ``norm_budget`` (L2 norm of the
    deviation from mid-grey, per clip) if given, then onto ``video_range``.  Channels 1-4 never change.

    Everything stays on the device and nothing synchronises with the host inside the loop.  Returns ``(inputs, trace)``: the
    final model input (same shape as the start) and the response before each step plus the final one, ``steps + 1`` values on
    the device.

    The regularised ascent runs when any of the following is given; without them the plain loop above runs.
    ``blur_sigma``: the gradient's video part is blurred by a separable Gaussian before the step: three sigmas (frames, pixels,
    pixels) or a ``[steps][3]`` schedule (the radii come from the largest sigma of each axis).  ``lr`` may be a length-``steps``
    schedule.  ``mean``: every clip is shifted to this mean luminance after each step.  ``contrast``: the RMS deviation from the
    clip's mean in grey levels, an upper bound (``contrast_mode="max"``) or an equality (``"fixed"``); not together with
    ``norm_budget``.  ``window`` = (y0, x0, height, width): blur, statistics and updates see that rectangle of every frame only,
    pixels outside it never change.  ``neurons`` may be one index list per clip (a sequence of ``B`` sequences, possibly ragged,
    or a 2-D LongTensor): clip ``b`` then ascends the summed response of its own set and ``trace`` is ``[steps + 1, B]`` (a start
    of one clip is repeated ``B`` times).  ``use_graph``: one step is captured into a graph and replayed ``steps`` times; between
    replays only device-to-device copies run (the step's taps, its ``lr``, its response).  Eager and replayed steps make the same
    calls on the same buffers: the same bits wherever the model's own kernels are reproducible (the ordered-reduction build)."""
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
    if (blur_sigma is not None or mean is not None or contrast is not None or contrast_mode != "max" or window is not None
            or use_graph or not isinstance(lr, (int, float)) or _per_clip_sets(neurons)):
        x, trace = _mei_regularised(model, mouse_index, neurons, x, steps=steps, lr=lr, video_range=(lo, hi),
                                    norm_budget=norm_budget, frames=frames, blur_sigma=blur_sigma, mean=mean, contrast=contrast,
                                    contrast_mode=contrast_mode, window=window, use_graph=use_graph)
        return (x[0] if squeeze and x.shape[0] == 1 else x), trace
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


# ------------------------------------------------------------------------------------------------------------------------------
# regularised pixel-space ascent
# ------------------------------------------------------------------------------------------------------------------------------
def _per_clip_sets(neurons) -> bool:
    """True for one index list per clip: a 2-D tensor or a sequence of sequences."""
    if isinstance(neurons, torch.Tensor):
        return neurons.dim() == 2
    if neurons is None or isinstance(neurons, slice):
        return False
    return len(neurons) > 0 and all(isinstance(n, (list, tuple)) or (isinstance(n, torch.Tensor) and n.dim() >= 1) for n in neurons)


def _padded_sets(neurons, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """Per-clip index lists -> (indices [B, K] padded with 0, mask [B, K] fp32)."""
    if isinstance(neurons, torch.Tensor):
        idx = neurons.to(device=device, dtype=torch.long)
        return idx.contiguous(), torch.ones(idx.shape, dtype=torch.float32, device=device)
    sets = [torch.as_tensor(n, dtype=torch.long).flatten() for n in neurons]
    K = max(int(n.numel()) for n in sets)
    if K < 1 or any(n.numel() < 1 for n in sets):
        raise ValueError("neurons: every clip needs at least one neuron")
    idx = torch.zeros(len(sets), K, dtype=torch.long)
    mask = torch.zeros(len(sets), K, dtype=torch.float32)
    for b, n in enumerate(sets):
        idx[b, :n.numel()] = n
        mask[b, :n.numel()] = 1.0
    return idx.to(device), mask.to(device)


def mei_schedules(steps: int, lr, blur_sigma):
    """Host side of the schedules of the regularised ascent: ``(lr [steps] fp32, tables [steps][3][DWN_BLUR_TAPS_STRIDE] fp32 or
    None, radii or None)`` on the CPU.  The radius of an axis is ``ceil(3 sigma)`` of its largest sigma (capped at
    ``DWN_BLUR_MAX_RADIUS``), so the geometry of the blur does not change along a schedule."""
    import math
    from . import ops
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must not be negative")
    lr_t = torch.as_tensor(lr, dtype=torch.float32).detach().cpu().flatten()
    if lr_t.numel() == 1 and not isinstance(lr, (list, tuple, torch.Tensor)):
        lr_t = lr_t.expand(steps).clone()
    if lr_t.numel() != steps or not bool(torch.isfinite(lr_t).all()):
        raise ValueError("lr: a finite float or a schedule of length `steps`")
    if blur_sigma is None:
        return lr_t, None, None
    sig = torch.as_tensor(blur_sigma, dtype=torch.float64).detach().cpu()
    if sig.dim() == 1 and sig.numel() == 3:
        sig = sig[None].expand(max(steps, 1), 3)
    if sig.dim() != 2 or sig.shape != (max(steps, 1), 3) and sig.shape != (steps, 3):
        raise ValueError("blur_sigma: three floats (frames, pixels, pixels) or a [steps][3] schedule")
    if not bool((torch.isfinite(sig) & (sig >= 0)).all()):
        raise ValueError("blur_sigma: finite and not negative")
    radii = tuple(min(int(math.ceil(3.0 * float(sig[:, a].max()))), ops.L.BLUR_MAX_RADIUS) if sig.shape[0] else 0 for a in range(3))
    tables = torch.stack([ops.blur_taps_table([ops.gaussian_taps(float(row[a]), radii[a]) for a in range(3)])[0] for row in sig]) \
        if sig.shape[0] else torch.zeros(0, 3, ops.L.BLUR_TAPS_STRIDE)
    return lr_t, tables, radii


def _mei_regularised(model, mouse_index: int, neurons, x: torch.Tensor, *, steps: int, lr, video_range, norm_budget, frames,
                     blur_sigma, mean, contrast, contrast_mode, window, use_graph) -> Tuple[torch.Tensor, torch.Tensor]:
    """The regularised ascent of ``most_exciting_input`` on the start ``x`` [B, C, T, H, W] (changed in place)."""
    from . import ops
    device = x.device
    lo, hi = video_range
    mid = 0.5 * (lo + hi)
    if contrast is not None and norm_budget is not None:
        raise ValueError("contrast and norm_budget are two different budgets: give one")
    if contrast_mode not in ops.MEI_CONTRAST_MODES:
        raise ValueError(f"contrast_mode: one of {tuple(ops.MEI_CONTRAST_MODES)} (got {contrast_mode!r})")
    if contrast is not None and not float(contrast) >= 0.0:
        raise ValueError("contrast must not be negative")
    if not lo <= hi:
        raise ValueError("video_range: lo <= hi")
    H, W = int(x.shape[3]), int(x.shape[4])
    if window is not None:
        if len(window) != 4:
            raise ValueError("window: (y0, x0, height, width)")
        y0, x0, wh, ww = (int(n) for n in window)
        if y0 < 0 or x0 < 0 or wh < 1 or ww < 1 or y0 + wh > H or x0 + ww > W:
            raise ValueError(f"window {tuple(window)} is not inside the {H} x {W} plane")
        window = (y0, x0, wh, ww)
    lr_sched, tables, radii = mei_schedules(steps, lr, blur_sigma)
    steps = int(steps)
    sets = _per_clip_sets(neurons)
    fsel = _as_index(frames, device)
    if sets:
        idx, maskf = _padded_sets(neurons, device)
        if x.shape[0] == 1 and idx.shape[0] > 1:
            x = x.expand(idx.shape[0], *x.shape[1:]).contiguous()
        if idx.shape[0] != x.shape[0]:
            raise ValueError(f"neurons: {idx.shape[0]} index lists for {x.shape[0]} clips")
    else:
        nsel = _as_index(neurons, device)
    B = int(x.shape[0])

    def objective(xg):
        if not sets:
            return _response(model, xg, mouse_index, nsel, fsel, "sum")
        return _set_response(model, xg, mouse_index, idx, maskf, fsel)

    # everything a step reads or writes besides x lives in buffers that exist before the first step: the eager loop and the
    # captured graph run the same calls on the same memory
    lr_sched = lr_sched.to(device)
    lr_cur = torch.zeros(1, dtype=torch.float32, device=device)
    if tables is not None:
        tables = tables.to(device)
        table_cur = torch.zeros(3, ops.L.BLUR_TAPS_STRIDE, dtype=torch.float32, device=device)
        gb = torch.zeros(B, 1, *x.shape[2:], dtype=torch.float32, device=device)
        blur_ws = torch.empty(gb.numel(), dtype=torch.float32, device=device)
    stat_g = torch.zeros(B, 4, dtype=torch.float64, device=device)
    stat_x = torch.zeros(B, 4, dtype=torch.float64, device=device)
    mom_ws = torch.empty(ops.clip_moments_ws(x.shape, window), dtype=torch.float64, device=device)
    r_cur = torch.zeros(B if sets else 1, dtype=torch.float32, device=device)
    trace = torch.zeros((steps + 1, B) if sets else (steps + 1,), dtype=torch.float32, device=device)
    wy, wx = (slice(window[0], window[0] + window[2]), slice(window[1], window[1] + window[3])) if window else (slice(None),) * 2

    def step():
        xg = x.detach().requires_grad_(True)
        with torch.enable_grad():
            r = objective(xg)
            (g,) = torch.autograd.grad(r.sum() if sets else r, xg)
        r_cur.copy_(r.detach().reshape(-1))
        g = g.contiguous()
        if tables is not None:
            ops.blur3d(g, table_cur, radii, c_src=0, out=gb, window=window, ws=blur_ws)
            g = gb
        ops.clip_moments(g, c=0, window=window, out=stat_g, ws=mom_ws)
        ops.mei_update(x, stat_g, "step", g=g, lr=lr_cur, window=window)
        if norm_budget is not None:
            v = x[:, 0, :, wy, wx]
            dev_ = v - mid
            n = dev_.flatten(1).norm(dim=1).clamp_min_(1e-20)
            v.copy_(mid + dev_ * (float(norm_budget) / n).clamp_max_(1.0).view(-1, 1, 1, 1))
        ops.clip_moments(x, c=0, window=window, out=stat_x, ws=mom_ws)
        ops.mei_update(x, stat_x, "project", window=window, mean=mean, contrast=contrast, contrast_mode=contrast_mode,
                       video_range=(lo, hi))

    def load(i):
        lr_cur.copy_(lr_sched[i:i + 1])
        if tables is not None:
            table_cur.copy_(tables[i])

    with _eval_mode(model):
        graph = None
        if use_graph and steps > 0:
            start = x.clone()
            load(0)
            side = torch.cuda.Stream(device)
            side.wait_stream(torch.cuda.current_stream(device))
            with torch.cuda.stream(side):                          # warm-up outside the capture (allocator, lazy loads)
                step()
            torch.cuda.current_stream(device).wait_stream(side)
            x.copy_(start)                                         # the warm-up stepped x: put the start back
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
        for i in range(steps):
            load(i)
            if graph is not None:
                graph.replay()
            else:
                step()
            trace[i].copy_(r_cur if sets else r_cur[0])
        with torch.enable_grad():       # (input requiring grad: the last entry comes from the same kernels as the others)
            trace[steps] = objective(x.detach().requires_grad_(True)).detach()
    return x, trace


# ------------------------------------------------------------------------------------------------------------------------------
# parametric stimuli (sensorium_amd/stimuli.py)
# ------------------------------------------------------------------------------------------------------------------------------
def _split_base(base: dict):
    """A ``base`` dict -> (Gabor parameters, DriftingGabor geometry)."""
    from .stimuli import PARAM_NAMES
    base = dict(base)
    values = {k: base.pop(k) for k in list(base) if k in PARAM_NAMES}
    for k in ("batch", "learn", "init"):
        if k in base:
            raise ValueError(f"base: {k!r} is set by the experiment, not by the caller")
    if "frames" not in base:
        raise ValueError("base: 'frames' (the length of the clips) is required")
    return values, base


def tuning_curve(model, mouse_index: int, base: dict, sweep: dict, *, neurons: Index = None, frames: Index = None,
                 chunk: Optional[int] = None) -> torch.Tensor:
    """Responses to ``K`` drifting Gabors that differ in one parameter: a tuning curve per neuron.

    ``base`` holds the fixed Gabor parameters by name (``stimuli.PARAM_NAMES``; names left out take the defaults of
    ``DriftingGabor``) together with the geometry of ``DriftingGabor``: ``frames`` (required), ``size``, ``envelope``,
    ``background``, ``video_range``, ``window``, ``pad``, ``behavior``, ``pupil_center``, ``in_channels``, ``video_channel``.
    ``sweep`` is ``{name: K values}``.  The clips are rendered on the model's device ``chunk`` at a time (default: all ``K`` in
    one batch) and run through the eval-mode model without grad (restored afterwards).  Returns [K, N_sel] on the device: the
    mean predicted response of the chosen ``neurons`` over the chosen ``frames`` (indices into the clip; default all)."""
    from .stimuli import PARAM_NAMES, DriftingGabor
    if len(sweep) != 1:
        raise ValueError("sweep: exactly one parameter name")
    (name, values), = sweep.items()
    if name not in PARAM_NAMES:
        raise ValueError(f"sweep: unknown Gabor parameter {name!r}: the names are {PARAM_NAMES}")
    values = torch.as_tensor(values, dtype=torch.float32).flatten()
    K = int(values.numel())
    if K < 1:
        raise ValueError("sweep: at least one value")
    fixed, geometry = _split_base(base)
    for k, v in fixed.items():
        if torch.as_tensor(v).dim() != 0:
            raise ValueError(f"base[{k!r}]: a scalar")
    chunk = K if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    device = next(model.parameters()).device
    nsel, fsel = _as_index(neurons, device), _as_index(frames, device)
    rows = []
    with _eval_mode(model), torch.no_grad():
        for k0 in range(0, K, chunk):
            vals = values[k0:k0 + chunk]
            clips = DriftingGabor(int(vals.numel()), init={**fixed, name: vals}, **geometry).to(device)
            out = model(clips(), index=mouse_index)
            rows.append(out[:, nsel][:, :, fsel].float().mean(dim=2))
    return torch.cat(rows, dim=0)


DEFAULT_GABOR_SCALES = dict(cy=2.0, cx=2.0, sigma=1.0, theta=0.2, sf=0.01, tf=0.01, phase=0.3, amplitude=10.0)


def gabor_bounds(gabor, bounds: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lower, upper) [8] of the projection of ``optimal_gabor`` for the geometry of ``gabor``: the centre inside the window,
    sigma >= ``sigma_min`` (1), 0 <= sf <= ``sf_max`` (0.5, Nyquist), 0 <= amplitude <= ``amplitude_max`` (half the video range;
    unbounded without one); theta, tf and phase are free."""
    from .stimuli import PARAM_NAMES
    b = dict(sigma_min=1.0, sf_max=0.5, amplitude_max=None)
    unknown = [k for k in (bounds or {}) if k not in b]
    if unknown:
        raise ValueError(f"bounds: unknown key(s) {unknown}: the keys are {tuple(b)}")
    b.update(bounds or {})
    if b["amplitude_max"] is None:
        b["amplitude_max"] = 0.5 * (gabor.video_range[1] - gabor.video_range[0]) if gabor.video_range is not None else float("inf")
    y0, x0, wh, ww = gabor.window if gabor.window is not None else (0, 0, *gabor.size)
    inf = float("inf")
    lo = dict(cy=float(y0), cx=float(x0), sigma=float(b["sigma_min"]), theta=-inf, sf=0.0, tf=-inf, phase=-inf, amplitude=0.0)
    hi = dict(cy=float(y0 + wh - 1), cx=float(x0 + ww - 1), sigma=inf, theta=inf, sf=float(b["sf_max"]), tf=inf, phase=inf,
              amplitude=float(b["amplitude_max"]))
    return torch.tensor([lo[n] for n in PARAM_NAMES]), torch.tensor([hi[n] for n in PARAM_NAMES])


def optimal_gabor(model, mouse_index: int, neurons: Index, *, starts, steps: int, lr: float, scales: Optional[dict] = None,
                  bounds: Optional[dict] = None, frames: Index = None, shape: Tuple[int, int, int] = (16, 64, 64),
                  betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, learn: Optional[Sequence[str]] = None,
                  **geometry) -> Tuple[torch.Tensor, torch.Tensor]:
    """The Gabor that drives ``neurons`` best: multi-start gradient ascent in Gabor-parameter space.

    ``starts`` is the start table — a dict of name -> scalar or [S] with at least one [S] entry, or a tensor [S, 8] in the order
    of ``stimuli.PARAM_NAMES``; all ``S`` clips are one batch (in eval mode the clips are independent: BatchNorm is frozen and
    squeeze-excitation is per sample).  The objective of a start is the summed predicted response of ``neurons`` over ``frames``
    (default all) to its clip of ``shape`` = (frames, height, width); ``geometry`` are further ``DriftingGabor`` arguments
    (``envelope``, ``background``, ``video_range``, ``window``, ``pad``, ``behavior``, ``pupil_center``, ...).

    The eight parameters differ in scale, so the ascent runs on ``z`` with ``params = start + scales * z`` (``scales``: name ->
    step scale, default ``DEFAULT_GABOR_SCALES``): ``steps`` Adam steps of size ``lr`` on ``z``, in plain torch on [S, 8].  After
    every step the parameters are projected onto ``gabor_bounds(bounds)``.  ``learn`` restricts the ascent to some names.
    Nothing synchronises with the host inside the loop; parameter ``.grad`` fields of the model are not touched.

    Returns ``(params [S, 8], trace [steps + 1, S])``: the final parameters and the objective of every start before each step
    plus the final one, on the device.  The best start is ``trace[-1].argmax()``."""
    from .stimuli import PARAM_NAMES, DriftingGabor, default_params, param_table
    device = next(model.parameters()).device
    t, h, w = (int(n) for n in shape)
    if isinstance(starts, dict):
        sizes = {int(torch.as_tensor(v).numel()) for v in starts.values() if torch.as_tensor(v).dim() == 1}
        if len(sizes) != 1:
            raise ValueError("starts: a dict needs at least one [S] entry, and all [S] entries of one length")
        S = sizes.pop()
        probe = DriftingGabor(1, 1, (h, w), **{k: v for k, v in geometry.items() if k in ("window", "video_range")})
        table = param_table(S, starts, default_params((h, w), probe.window, probe.video_range))
    else:
        table = torch.as_tensor(starts, dtype=torch.float32).detach().cpu()
        if table.dim() != 2 or table.shape[1] != len(PARAM_NAMES) or table.shape[0] < 1:
            raise ValueError("starts: a dict of name -> values or a tensor [S, 8]")
        S = int(table.shape[0])
    unknown = [k for k in (scales or {}) if k not in PARAM_NAMES]
    if unknown:
        raise ValueError(f"scales: unknown Gabor parameter(s) {unknown}")
    sc = {**DEFAULT_GABOR_SCALES, **(scales or {})}
    if int(steps) < 0 or any(not float(v) > 0 for v in sc.values()):
        raise ValueError("steps must not be negative and every scale must be positive")
    gabor = DriftingGabor(S, t, (h, w), **geometry).to(device)
    lo, hi = (b.to(device) for b in gabor_bounds(gabor, bounds))
    scale = torch.tensor([float(sc[n]) for n in PARAM_NAMES], device=device)
    mask = torch.tensor([learn is None or n in learn for n in PARAM_NAMES], device=device)
    start = table.to(device).clamp(lo, hi)
    z = torch.zeros(S, len(PARAM_NAMES), device=device)
    m, v = torch.zeros_like(z), torch.zeros_like(z)
    nsel, fsel = _as_index(neurons, device), _as_index(frames, device)
    trace = torch.zeros(steps + 1, S, dtype=torch.float32, device=device)

    def objective(zz):
        out = model(gabor.render(start + scale * zz), index=mouse_index)
        return out[:, nsel][:, :, fsel].float().sum(dim=(1, 2))

    b1, b2 = betas
    with _eval_mode(model):
        for i in range(steps):
            zg = z.detach().requires_grad_(True)
            with torch.enable_grad():
                r = objective(zg)
                (g,) = torch.autograd.grad(r.sum(), zg)
            trace[i] = r.detach()
            g = torch.where(mask, g, torch.zeros_like(g))
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            step = (m / (1 - b1 ** (i + 1))) / ((v / (1 - b2 ** (i + 1))).sqrt() + eps)
            p = (start + scale * (z + lr * step)).clamp(lo, hi)
            z = (p - start) / scale
        with torch.enable_grad():       # (an input requiring grad: the last entry comes from the same kernels as the others)
            trace[steps] = objective(z.detach().requires_grad_(True)).detach()
    return (start + scale * z).clamp(lo, hi), trace


# ------------------------------------------------------------------------------------------------------------------------------
# receptive-field mapping (sensorium_amd/receptive_fields.py)
# ------------------------------------------------------------------------------------------------------------------------------
def receptive_fields(model, mouse_index: int, *, clips: int, frames: int, lags: int, batch: int = 32, noise: Optional[dict] = None,
                     seed: int = 0, neurons: Index = None, skip: Optional[int] = None, size: Tuple[int, int] = (64, 64),
                     window: Optional[Sequence[int]] = None, behavior: Sequence[float] = (0.0, 0.0),
                     pupil_center: Sequence[float] = (0.0, 0.0), first_clip: int = 0, accumulator=None, fit: Optional[dict] = None):
    """The spatio-temporal receptive field of every neuron of mouse ``mouse_index`` by reverse correlation.

    ``clips`` noise clips of ``frames`` frames (numbered ``first_clip ..``; a clip is a function of ``(seed, number)`` alone) are
    rendered on the model's device ``batch`` at a time — the last batch may be smaller —, run through the eval-mode model without
    grad (restored afterwards) and correlated with its responses at ``lags`` lags.  ``noise``: further ``NoiseStimulus`` arguments
    (``kind``, ``cell``, ``hold``, ``contrast``, ``density``, ``background``, ``video_range``, ``pad``, ``in_channels``,
    ``video_channel``); ``size`` / ``window`` / ``behavior`` / ``pupil_center`` as for ``DriftingGabor``.  ``skip``: the frames
    of every clip left out as the model's warm-up (default ``lags - 1``, the least possible).  ``neurons`` selects rows before the
    accumulation: the state then has ``len(neurons)`` rows.  The response centre is the per-neuron mean of the first batch's
    responses, taken on the device; nothing is read back inside the loop.  ``accumulator``: continue an existing
    ``StaAccumulator`` (its geometry must be the call's) — the way to split an experiment over several calls.  ``fit``: a dict of
    ``ReceptiveFields.fit`` arguments (``{}`` for the defaults): the parametric fits are then run on the result and kept as its
    ``.fits``; ``None`` runs none.

    Returns ``ReceptiveFields`` (``.sta``, ``.z``, ``.summary``, ``.centres()``, ``.significant()``); its ``.accumulator`` is the
    ``StaAccumulator`` behind it, to continue with."""
    from .receptive_fields import StaAccumulator
    from .stimuli import NoiseStimulus
    clips, batch, lags = int(clips), int(batch), int(lags)
    if clips < 1 or batch < 1 or lags < 1:
        raise ValueError("clips, batch and lags must be positive")
    skip = lags - 1 if skip is None else int(skip)
    if skip < 0 or max(skip, lags - 1) >= int(frames):
        raise ValueError(f"clips of {frames} frames hold no valid frame for lags = {lags}, skip = {skip}")
    noise = dict(noise or {})
    for k in ("seed", "window", "behavior", "pupil_center", "batch", "frames", "size"):
        if k in noise:
            raise ValueError(f"noise: {k!r} is an argument of receptive_fields itself")
    device = next(model.parameters()).device
    stim = NoiseStimulus(min(batch, clips), int(frames), size, window=window, behavior=behavior, pupil_center=pupil_center, seed=seed,
                         **noise).to(device)
    nsel = _as_index(neurons, device)
    acc = accumulator
    with _eval_mode(model), torch.no_grad():
        for k0 in range(0, clips, batch):
            x = stim(first_clip=int(first_clip) + k0, batch=min(batch, clips - k0))
            full = model(x, index=mouse_index).float()
            out = full[:, nsel]
            if acc is None:
                # the centre of a neuron is taken from the whole output: a row's bits do not depend on which rows are selected
                centre = full.mean(dim=(0, 2))[nsel]
                acc = StaAccumulator(int(out.shape[1]), lags, stim.size, window=stim.window, cell=stim.cell, channel=stim.video_channel,
                                     skip=skip, stimulus_centre=stim.background, response_centre=centre, device=device)
            acc.add(x, out)
    fields = acc.compute()
    fields.accumulator = acc
    if fit is not None:
        fields.fit(**dict(fit))
    return fields

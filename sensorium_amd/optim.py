"""Fused multi-tensor AdamW (+ parameter EMA) on the HIP kernel ``dwn_adamw_ema_multi``.

Semantics: ``torch.optim.AdamW`` as named by the reference config (configs/true_batch_001.py:45-48) — decoupled
weight decay, bias-corrected moments, scalar arithmetic in double on the host exactly as torch does — and,
optionally in the same pass, ``ModelEma.update`` (src/ema.py:47-55) for the parameters.  One kernel launch per
parameter group instead of ~200 tensors x several ops.

Optionally guarded (``max_grad_norm`` / ``skip_nonfinite``): global gradient-norm clipping and the skip of a step
whose gradients hold an Inf or NaN — what ``GradScaler.step`` did for the reference under fp16 — both decided on the device:
a multi-tensor sum of squares, a one-workgroup finaliser and ``dwn_adamw_ema_multi_guarded``, without a host read-back.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional

import numpy as np
import torch

from . import _lib as L

_ENTRY_DTYPE = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"),
                         ("ema", "<u8"), ("numel", "<i8"), ("is_int64", "<i4"), ("pad", "<i4")])
assert _ENTRY_DTYPE.itemsize == C.sizeof(L.TensorEntry)
_GUARDED_DTYPE = np.dtype(_ENTRY_DTYPE.descr + [("step", "<u8")])
assert _GUARDED_DTYPE.itemsize == C.sizeof(L.GuardedEntry)


class _TableCache:
    """Device copy of a pointer table, re-uploaded only when its contents change.

    The table of a training step is almost always identical to the previous step's (parameters, optimizer state and
    EMA tensors never move; the caching allocator hands the gradients the same blocks every step).  A blocking
    host-to-device copy per step would also stall the host until the whole backward has drained, leaving the GPU idle
    while the next step's first kernels are being queued — so a changed table goes through pinned memory, asynchronously.
    """

    def __init__(self):
        self._bytes = None
        self._dev = None
        self._pinned = None          # kept alive until the next upload: the async copy reads it

    def get(self, entries: np.ndarray, device) -> torch.Tensor:
        raw = entries.view(np.uint8).tobytes()
        if self._dev is not None and self._bytes == raw and self._dev.device == device:
            return self._dev
        host = torch.frombuffer(bytearray(raw), dtype=torch.uint8).pin_memory()
        dev = torch.empty(len(raw), dtype=torch.uint8, device=device)
        dev.copy_(host, non_blocking=True)
        self._bytes, self._dev, self._pinned = raw, dev, host
        return dev


_lerp_cache = _TableCache()


class FusedAdamWEma(torch.optim.Optimizer):
    def __init__(self, params: Iterable, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, ema_params: Optional[List[torch.Tensor]] = None,
                 ema_decay: float = 0.999, max_blocks: int = 1024, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False):
        """``max_grad_norm``: clip the global L2 norm of all gradients (times ``grad_scale``) to it, as
        ``torch.nn.utils.clip_grad_norm_`` does.  ``skip_nonfinite``: a step whose gradients hold an Inf or NaN leaves the
        parameters, both moments and the step counts as they are; the EMA leg still runs.  With either set, ``state[p]["step"]``
        is a 0-dim int64 device tensor and ``guard_stats()`` reports what the last step did."""
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError("max_grad_norm must be positive (or None: no clipping)")
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.ema_decay = float(ema_decay)
        self.max_blocks = int(max_blocks)
        self.grad_scale = 1.0
        self._ema_of = {}
        self._ema_owner = None          # the ModelEma whose parameter copies ride in this optimizer's kernel (or None)
        self._tables = {}
        self._range_of = None
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._guard_group = None        # process group of the sharded buckets: their part of the norm is all-reduced over it
        self._guard_dev = None          # (guard struct, the two [sumsq, nonfinite] pairs, partials workspace) on the device
        if ema_params is not None:
            self.bind_ema(ema_params, ema_decay)

    def set_shard_map(self, range_of):
        """Sharded optimizer (ddp.GradBuckets(shard_optional=True)): ``range_of(p)`` returns ``None`` (update all of ``p``)
        or the flattened element range ``(lo, hi)`` of ``p`` this rank owns: only that range is updated (moments exist for it
        alone) and only that range of ``p.grad`` is read; the other ranks' slices arrive by all-gather."""
        self._range_of = range_of
        self._tables = {}

    def set_guard_group(self, group):
        """Sharded optimizer: the process group over which the owned slices' ``[sumsq, nonfinite]`` pair is summed before the
        guard is finalised (16 bytes per step) — a non-finite value in one rank's slice makes every rank skip."""
        self._guard_group = group

    @property
    def guarded(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _guard_buffers(self, dev, ws_bytes: int):
        """The guard struct (zeroed once: it carries the running totals), the two pairs and the partials workspace; only the
        workspace is replaced when a later step needs a larger one."""
        g = self._guard_dev
        if g is None or g[0].device != dev:
            g = (torch.zeros(C.sizeof(L.StepGuard), dtype=torch.uint8, device=dev), torch.zeros(4, dtype=torch.float64, device=dev),
                 torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=dev))
        elif g[2].numel() < ws_bytes:
            g = (g[0], g[1], torch.empty(ws_bytes, dtype=torch.uint8, device=dev))
        self._guard_dev = g
        return g

    def guard_stats(self) -> Optional[dict]:
        """What the guard of the last step decided, read from the device (the one place that synchronises); ``None`` when the
        guard is off."""
        if not self.guarded:
            return None
        if self._guard_dev is None:
            g = L.StepGuard()
            g.coef = 1.0
        else:
            g = L.StepGuard.from_buffer_copy(self._guard_dev[0].cpu().numpy().tobytes())
        return {"norm": float(g.norm), "coef": float(g.coef), "skipped": bool(g.skip), "nonfinite": int(g.nonfinite),
                "good_steps": int(g.good_steps), "skipped_steps": int(g.skipped_steps)}

    def _steps_as(self, on_device: bool):
        """``state[p]["step"]`` in the form this mode keeps: a Python int (unguarded: the host counts) or a 0-dim int64 device
        tensor (guarded: the device counts).  Converting device counters reads them back — at load / save time only."""
        states = [(p, st) for p, st in self.state.items() if "step" in st and torch.is_tensor(st["step"]) != on_device]
        if not states:
            return
        if on_device:
            for p, st in states:
                st["step"] = torch.tensor(int(st["step"]), dtype=torch.int64, device=p.device)
        else:
            host = torch.stack([st["step"].reshape(()).to(torch.int64) for _, st in states]).cpu().tolist()
            for (_, st), n in zip(states, host):
                st["step"] = int(n)

    def state_dict(self):
        """``step`` is written as a Python int in either mode, so a checkpoint of a guarded run loads into an unguarded optimizer
        and the other way round (one read-back of the device counters per call)."""
        sd = super().state_dict()
        dev_steps = [(k, st["step"]) for k, st in sd["state"].items() if torch.is_tensor(st.get("step"))]
        if dev_steps:
            host = torch.stack([t.reshape(()).to(torch.int64) for _, t in dev_steps]).cpu().tolist()
            state = {k: dict(st) for k, st in sd["state"].items()}
            for (k, _), n in zip(dev_steps, host):
                state[k]["step"] = int(n)
            sd = {"state": state, "param_groups": sd["param_groups"]}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._steps_as(on_device=self.guarded)
        self._tables = {}

    def bind_ema(self, ema_params: Optional[List[torch.Tensor]], ema_decay: float, owner=None):
        """(Re)attach the EMA copies of the optimised parameters without touching the Adam moments / step counts:
        the reference assigns ``model.model_ema`` at any time (scripts/train.py:53), also after the optimizer exists.
        ``ema_params=None`` detaches (ModelEma.update then lerps the parameters itself)."""
        flat = [p for g in self.param_groups for p in g["params"]]
        if ema_params is not None and len(ema_params) != len(flat):
            raise ValueError("ema_params must align one-to-one with the optimised parameters")
        self._ema_of = {id(p): e for p, e in zip(flat, ema_params)} if ema_params is not None else {}
        self._ema_owner = owner if ema_params is not None else None
        self.ema_decay = float(ema_decay)
        self._tables = {}

    def folds_ema_of(self, owner) -> bool:
        """True when this optimizer's step also updates the parameter EMA of ``owner`` (a ModelEma)."""
        return owner is not None and self._ema_owner is owner and bool(self._ema_of)

    def state_for(self, p):
        return self.state[p]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if self.guarded:
            self._step_guarded()
            return loss
        for gi, group in enumerate(self.param_groups):
            live = [p for p in group["params"] if p.grad is not None]
            if not live:
                continue
            dev = live[0].device
            if not live[0].is_cuda:
                raise RuntimeError("FusedAdamWEma: parameters must be on a GPU (no CPU fallback)")
            # one launch per distinct step count: parameters a step left without a gradient (the other mice's readouts under
            # forward(x, index), dwiseneuro.py:404-405) are skipped like torch.optim.AdamW skips them, so their bias
            # corrections lag; ordinarily every parameter shares one count and this is a single launch
            by_step = {}
            for p in live:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdamWEma: fp32 contiguous parameters only")
                st = self.state[p]
                if not st:
                    self._init_state(p, st, 0)
                elif torch.is_tensor(st["step"]):
                    st["step"] = int(st["step"])
                st["step"] += 1
                by_step.setdefault(int(st["step"]), []).append(p)
            b1, b2 = group["betas"]
            for step, params in sorted(by_step.items()):
                entries = np.zeros(len(params), dtype=_ENTRY_DTYPE)
                keep = []
                n_live = 0
                for p in params:
                    st = self.state[p]
                    g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                    keep.append(g)
                    ema = self._ema_of.get(id(p))
                    rng = self._range_of(p) if self._range_of is not None else None
                    lo, n = (0, p.numel()) if rng is None else (rng[0], rng[1] - rng[0])
                    if n == 0:
                        continue                      # another rank's slice
                    entries[n_live] = (p.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, st["exp_avg"].data_ptr(),
                                       st["exp_avg_sq"].data_ptr(), 0 if ema is None else ema.data_ptr() + 4 * lo, n, 0, 0)
                    n_live += 1
                if n_live == 0:
                    continue
                entries = entries[:n_live]
                # the table cache is keyed by the set of parameters taking part, so alternating sets do not thrash it
                key = (gi, tuple(id(p) for p in params)) if len(params) != len(group["params"]) else (gi, None)
                table = self._tables.setdefault(key, _TableCache()).get(entries, dev)
                L.check(L.lib.dwn_adamw_ema_multi(table.data_ptr(), n_live, self.max_blocks, float(group["lr"]),
                                                  float(b1), float(b2), float(group["eps"]),
                                                  float(group["weight_decay"]), int(step), self.ema_decay,
                                                  float(self.grad_scale), dev.index,
                                                  torch.cuda.current_stream(dev).cuda_stream),
                        "dwn_adamw_ema_multi")
                del keep
        return loss

    def _init_state(self, p, st, step):
        st["step"] = step
        rng = self._range_of(p) if self._range_of is not None else None
        if rng is None:
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        else:                             # moments for the owned slice only
            st["exp_avg"] = torch.zeros(rng[1] - rng[0], dtype=p.dtype, device=p.device)
            st["exp_avg_sq"] = torch.zeros(rng[1] - rng[0], dtype=p.dtype, device=p.device)

    def _step_guarded(self):
        """Sum of squares over the gradients of ALL groups -> (all-reduce of the sharded slices' part) -> guard -> one guarded
        AdamW/EMA launch per group.  One table: the entries updated whole, group by group, then the owned slices of sharded
        parameters, group by group; every launch takes a contiguous run of it.  Parameters of different step counts (the other
        mice's readouts under forward(x, index)) ride together: each reads its own device counter."""
        rep, shd = [], []                                  # per group: entry tuples
        dev, keep, live = None, [], []
        for group in self.param_groups:
            r, s = [], []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if not p.is_cuda:
                    raise RuntimeError("FusedAdamWEma: parameters must be on a GPU (no CPU fallback)")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("FusedAdamWEma: fp32 contiguous parameters only")
                dev = p.device if dev is None else dev
                st = self.state[p]
                if not st:
                    self._init_state(p, st, torch.zeros((), dtype=torch.int64, device=p.device))
                elif not torch.is_tensor(st["step"]):
                    st["step"] = torch.tensor(int(st["step"]), dtype=torch.int64, device=p.device)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(g)
                ema = self._ema_of.get(id(p))
                rng = self._range_of(p) if self._range_of is not None else None
                lo, n = (0, p.numel()) if rng is None else (rng[0], rng[1] - rng[0])
                # (n == 0: another rank's slice — an entry without elements, so that its step count advances like everybody's)
                live.append(id(p))
                (r if rng is None else s).append(
                    (p.data_ptr() + 4 * lo, g.data_ptr() + 4 * lo, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(),
                     0 if ema is None else ema.data_ptr() + 4 * lo, n, 0, 0, st["step"].data_ptr()))
            rep.append(r)
            shd.append(s)
        sharded = self._range_of is not None
        if dev is None:
            if not sharded:
                return
            # no gradient at all on this rank: the other ranks still wait in the collective below (a zero pair from here)
            dev = next(p.device for group in self.param_groups for p in group["params"])
        n_rep, n_shd = sum(map(len, rep)), sum(map(len, shd))
        flat = [e for r in rep for e in r] + [e for s in shd for e in s]
        entries = np.zeros(max(len(flat), 1), dtype=_GUARDED_DTYPE)
        for i, e in enumerate(flat):
            entries[i] = e
        # keyed by the set of parameters taking part, as the unguarded path does: alternating sets do not thrash the cache
        n_all = sum(len(group["params"]) for group in self.param_groups)
        key = ("guarded", None if len(live) == n_all else tuple(live))
        table = self._tables.setdefault(key, _TableCache()).get(entries, dev)
        size = _GUARDED_DTYPE.itemsize
        lib, stream = L.lib, torch.cuda.current_stream(dev).cuda_stream
        ws_bytes = int(lib.dwn_grad_guard_workspace_bytes(max(n_rep, n_shd), self.max_blocks))
        guard, pairs, ws = self._guard_buffers(dev, ws_bytes)
        pair_a, pair_b = pairs.data_ptr(), pairs.data_ptr() + 16
        L.check(lib.dwn_grad_sumsq_multi(table.data_ptr(), n_rep, self.max_blocks, float(self.grad_scale), ws.data_ptr(),
                                         ws.numel(), pair_a, dev.index, stream), "dwn_grad_sumsq_multi")
        if sharded:
            # every rank calls the collective, also one that owns no slice of anything used this step (its pair is zero)
            L.check(lib.dwn_grad_sumsq_multi(table.data_ptr() + size * n_rep, n_shd, self.max_blocks, float(self.grad_scale),
                                             ws.data_ptr(), ws.numel(), pair_b, dev.index, stream), "dwn_grad_sumsq_multi")
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                torch.distributed.all_reduce(pairs[2:4], op=torch.distributed.ReduceOp.SUM, group=self._guard_group)
        L.check(lib.dwn_step_guard_finalize(pair_a, pair_b if sharded else None, float(self.max_grad_norm or 0.0),
                                            int(self.skip_nonfinite), table.data_ptr(), n_rep + n_shd, guard.data_ptr(),
                                            dev.index, stream), "dwn_step_guard_finalize")
        off_r, off_s = 0, n_rep
        for group, r, s in zip(self.param_groups, rep, shd):
            b1, b2 = group["betas"]
            for off, n in ((off_r, len(r)), (off_s, len(s))):
                if n:
                    L.check(lib.dwn_adamw_ema_multi_guarded(table.data_ptr() + size * off, n, self.max_blocks, float(group["lr"]),
                                                            float(b1), float(b2), float(group["eps"]),
                                                            float(group["weight_decay"]), self.ema_decay, float(self.grad_scale),
                                                            guard.data_ptr(), dev.index, stream), "dwn_adamw_ema_multi_guarded")
            off_r += len(r)
            off_s += len(s)
        del keep


def ema_lerp_state(ema_tensors: List[torch.Tensor], model_tensors: List[torch.Tensor], decay: float,
                   max_blocks: int = 16):
    """e <- decay*e + (1-decay)*m over a list of state tensors in ONE launch (src/ema.py:47-55).
    float32 tensors are lerped; int64 tensors (``num_batches_tracked``) follow the reference's float-then-truncate."""
    if not ema_tensors:
        return
    dev = ema_tensors[0].device
    entries = np.zeros(len(ema_tensors), dtype=_ENTRY_DTYPE)
    for i, (e, m) in enumerate(zip(ema_tensors, model_tensors)):
        if e.dtype == torch.int64:
            is_int = 1
        elif e.dtype == torch.float32:
            is_int = 0
        else:
            raise RuntimeError(f"ema_lerp_state: unsupported dtype {e.dtype}")
        if not (e.is_contiguous() and m.is_contiguous() and e.is_cuda and m.is_cuda):
            raise RuntimeError("ema_lerp_state: contiguous GPU tensors only")
        entries[i] = (m.data_ptr(), 0, 0, 0, e.data_ptr(), e.numel(), is_int, 0)
    table = _lerp_cache.get(entries, dev)
    L.check(L.lib.dwn_ema_lerp_multi(table.data_ptr(), len(ema_tensors), max_blocks, float(decay), dev.index,
                                     torch.cuda.current_stream(dev).cuda_stream), "dwn_ema_lerp_multi")

"""Single-trial correlation (reference: src/metrics.py:11-31), the parity metric of the north star."""

import numpy as np
import torch

from .engine import Metric


def corr(y1: np.ndarray, y2: np.ndarray, axis=-1, eps: float = 1e-8, **kwargs) -> np.ndarray:
    y1 = (y1 - y1.mean(axis=axis, keepdims=True)) / (y1.std(axis=axis, keepdims=True, ddof=0) + eps)
    y2 = (y2 - y2.mean(axis=axis, keepdims=True)) / (y2.std(axis=axis, keepdims=True, ddof=0) + eps)
    return (y1 * y2).mean(axis=axis, **kwargs)


class CorrelationMetric(Metric):
    """``val_corr`` / ``val_corr_mouse_<i>`` of scripts/train.py:137-139 — what src/metrics.py:34-82 computes, as a STREAMING
    statistic on the device: per mouse and neuron the five running sums (n, sum p, sum t, sum p^2, sum t^2, sum p*t) over the
    (sample, frame) rows whose mouse weight is not zero, in float64, updated by a handful of reductions per batch.  The
    reference keeps every prediction and target of the epoch on the host (one device->host copy and one ``torch.any`` sync
    per mouse and batch, O(epoch) memory) and calls ``corr`` on the concatenation at the end; the Pearson coefficient with
    the reference's ``eps`` on each standard deviation is a function of those sums alone:
    ``(E[pt] - E[p]E[t]) / ((std p + eps)(std t + eps))`` — equal to ``corr(..., axis=0)`` up to rounding (checked at 1e-6).
    Mice without a weighted row in the epoch are left out, as in the reference.

    ``fused=True``: ``update`` is one ``dwn_corr_moments`` launch per mouse — the batch's CENTRED moments (means,
    M2p, M2t, C and n, float64) — merged into the running ones with the pairwise (Chan) formulas on N-vectors on the device; an
    empty batch or an empty running state is handled by a ``where``, not a read-back.  ``compute`` keeps its one read-back per mouse
    and epoch.  GPU tensors only.  The default computes exactly what it always did."""
    name = "corr"
    better = "max"
    eps = 1e-8

    def __init__(self, fused: bool = False):
        self.fused = bool(fused)
        self.reset()

    def reset(self):
        self.sums = {}                # mouse index -> [count (0-d), sum_p, sum_t, sum_pp, sum_tt, sum_pt] (float64, on the device)
        self.moments = {}             # fused: mouse index -> [n (0-d), mean_p, mean_t, M2p, M2t, C] (float64, on the device)

    @staticmethod
    def merge_moments(a, b):
        """Pairwise (Chan) merge of two sets [n, mean_p, mean_t, M2p, M2t, C]; either side may be empty (n = 0)."""
        na, nb = a[0], b[0]
        n = na + nb
        fb = torch.where(n > 0, nb / n.clamp_min(1), torch.zeros_like(n))      # nb / n, 0 for two empty sides
        dp, dt = b[1] - a[1], b[2] - a[2]
        cross = na * fb                                                        # na nb / n
        return [n, a[1] + dp * fb, a[2] + dt * fb, a[3] + b[3] + dp * dp * cross, a[4] + b[4] + dt * dt * cross,
                a[5] + b[5] + dp * dt * cross]

    @torch.no_grad()
    def _update_fused(self, predictions, targets, mice_weights):
        from . import ops
        weights = mice_weights.float()
        for k, (p, t) in enumerate(zip(predictions, targets)):
            N = p.shape[1]
            stat = ops.corr_moments(p, t, weights[..., k])
            new = [stat[8 * N]] + [stat[i * N:(i + 1) * N] for i in range(5)]
            old = self.moments.get(k)
            self.moments[k] = new if old is None else self.merge_moments(old, new)

    @torch.no_grad()
    def update(self, step_output: dict):
        predictions = step_output["prediction"]
        targets, mice_weights = step_output["target"]
        if self.fused:
            return self._update_fused(predictions, targets, mice_weights)
        for k, (p, t) in enumerate(zip(predictions, targets)):
            rows = (mice_weights[..., k] != 0).to(torch.float64)              # [B]: 1 for this mouse's samples
            p, t = p.to(torch.float64), t.to(torch.float64)
            if p.dim() == 2:                                                  # (B, N): one row per sample
                p, t = p.unsqueeze(-1), t.unsqueeze(-1)
            w = rows.view(-1, 1, 1)
            pw, tw = p * w, t * w
            new = [rows.sum() * p.shape[-1], pw.sum((0, 2)), tw.sum((0, 2)), (pw * p).sum((0, 2)), (tw * t).sum((0, 2)),
                   (pw * t).sum((0, 2))]
            old = self.sums.get(k)
            self.sums[k] = new if old is None else [a + b for a, b in zip(old, new)]

    def compute(self):
        out = {}
        for k, (n, mp, mt, m2p, m2t, c) in self.moments.items():
            n = float(n)                                                      # the epoch's one read-back per mouse
            if n == 0:
                continue
            r = (c / n) / (((m2p / n).sqrt() + self.eps) * ((m2t / n).sqrt() + self.eps))
            out[k] = float(r.mean())
        for k, (n, sp, st, spp, stt, spt) in self.sums.items():
            n = float(n)                                                      # the epoch's one read-back per mouse
            if n == 0:
                continue
            mp, mt = sp / n, st / n
            sd_p = (spp / n - mp * mp).clamp_min(0).sqrt()
            sd_t = (stt / n - mt * mt).clamp_min(0).sqrt()
            r = (spt / n - mp * mt) / ((sd_p + self.eps) * (sd_t + self.eps))
            out[k] = float(r.mean())
        return out

    def epoch_complete(self, state):
        per_mouse = self.compute()
        prefix = f"{state.phase}_" if state.phase else ""
        for k, value in per_mouse.items():
            state.metrics[f"{prefix}{self.name}_mouse_{k}"] = value
        state.metrics[prefix + self.name] = float(np.mean(list(per_mouse.values())))

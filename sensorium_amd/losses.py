"""MicePoissonLoss drop-in (reference: src/losses.py:5-21) on the HIP Poisson kernels."""
from __future__ import annotations

import torch
from torch import nn

from . import ops


class MicePoissonLoss(nn.Module):
    """sum over mice of the weight-normalised Poisson NLL (log_input=False, full=False).

    ``forward(inputs, targets)`` with ``inputs`` = list of (B, N_m, T) predictions and ``targets`` =
    (list of (B, N_m, T) targets, (B, n_mice) mice_weights), exactly as the reference.  The per-mouse
    ``torch.any(mask)`` host sync of the reference (losses.py:17) is not needed: samples with weight 0
    contribute exactly 0 in the kernel, so the value and gradients are identical.
    """

    def __init__(self, log_input: bool = False, full: bool = False, eps: float = 1e-8):
        super().__init__()
        if log_input or full:
            raise NotImplementedError("sensorium_amd.MicePoissonLoss: only log_input=False, full=False is built")
        self.eps = float(eps)

    def forward(self, inputs, targets):
        target_tensors, mice_weights = targets
        weights = (mice_weights / mice_weights.sum()).float()
        total = None
        for m, (pred, target) in enumerate(zip(inputs, target_tensors)):
            term = ops.PoissonLossFn.apply(pred, target, weights[..., m], self.eps)
            total = term if total is None else total + term
        return total


def _check_correlation_args(eps, reduction):
    if reduction not in ops.CORR_REDUCTIONS:
        raise ValueError(f"reduction must be one of {sorted(ops.CORR_REDUCTIONS)}, got {reduction!r}")
    if not float(eps) > 0:
        raise ValueError(f"eps must be positive, got {eps!r}")


class MiceCorrelationLoss(nn.Module):
    """1 - single-trial correlation, the quantity the models are scored on (reference: ``corr`` of src/metrics.py:11-31), as a
    loss on the HIP correlation kernels.

    ``forward(inputs, targets)`` has the contract of ``MicePoissonLoss``.  Per mouse m, over the rows R = {b : mice_weights[b, m]
    != 0} and the n = |R| * T values of each neuron j: ``r_j = cov(p, t) / ((std p + eps)(std t + eps))`` (population statistics,
    as ``metrics.corr`` on the selected rows) and ``loss_m = share_m * red_j (1 - r_j)`` with ``share_m = sum_b w[b, m] / sum w``
    and ``red`` the mean (default) or the sum over neurons; the loss is the sum over mice.  With one-hot weights and the mean it
    is exactly 1 - (weighted mean over mice of the batch's ``val_corr``).

    The weights' magnitudes enter through ``share_m`` alone: inside a mouse the correlation is unweighted, as in the metric.
    Under distillation every weight is non-zero, so every row counts for every mouse, with the teacher's predictions as the
    targets of the rows the mouse does not own; nothing is special-cased.  A mouse without a row in the batch contributes
    exactly 0 and gets a zero gradient (decided on the device: no ``torch.any``, no ``.item()``), rows of weight 0 get a zero
    gradient and are never read.  A constant target gives r = 0 and a zero gradient; at a constant prediction the term of the
    gradient that divides by std p is defined as 0.

    The statistic is PER CALL, as the batch statistic of a train-mode BatchNorm is: per ``iter_size`` chunk and per rank under
    data parallelism, not per global batch.  The mean of chunk-wise correlations is not the correlation of the whole batch.
    """

    def __init__(self, eps: float = 1e-8, reduction: str = "mean"):
        super().__init__()
        _check_correlation_args(eps, reduction)
        self.eps = float(eps)
        self.reduction = reduction

    def forward(self, inputs, targets):
        target_tensors, mice_weights = targets
        weights = mice_weights.float()
        shares = weights.sum(0) / weights.sum()
        total = None
        for m, (pred, target) in enumerate(zip(inputs, target_tensors)):
            term = ops.CorrelationLossFn.apply(pred, target, weights[..., m], shares[m], self.eps, self.reduction)
            total = term if total is None else total + term
        return total


class MicePoissonCorrelationLoss(nn.Module):
    """``poisson_weight * MicePoissonLoss + correlation_weight * MiceCorrelationLoss`` on the same predictions and targets.  The
    two backward passes are separate kernels; autograd adds the two ``dpred``.  ``eps`` is the correlation's (the Poisson term
    keeps its own ``poisson_eps``)."""

    def __init__(self, poisson_weight: float = 1.0, correlation_weight: float = 1.0, eps: float = 1e-8,
                 reduction: str = "mean", poisson_eps: float = 1e-8):
        super().__init__()
        for name, v in (("poisson_weight", poisson_weight), ("correlation_weight", correlation_weight)):
            if not (float(v) >= 0 and float(v) < float("inf")):
                raise ValueError(f"{name} must be a finite non-negative number, got {v!r}")
        if float(poisson_weight) == 0 and float(correlation_weight) == 0:
            raise ValueError("poisson_weight and correlation_weight are both 0")
        self.poisson_weight = float(poisson_weight)
        self.correlation_weight = float(correlation_weight)
        self.poisson = MicePoissonLoss(eps=poisson_eps)
        self.correlation = MiceCorrelationLoss(eps=eps, reduction=reduction)

    def forward(self, inputs, targets):
        return self.poisson_weight * self.poisson(inputs, targets) + self.correlation_weight * self.correlation(inputs, targets)

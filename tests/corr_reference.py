"""Float64 checker of the correlation objective (include/dwn.h dwn_corr_args): centred moments, Pearson coefficient,
loss and closed-form gradient of one mouse, and the pairwise merge of two sets of moments — own arithmetic in numpy, nothing from the
code under test.

Definition, for predictions p and targets t of shape (B, N, T) ((B, N): T = 1) and row weights w (B,):
    R = {b : w[b] != 0},  n = |R| T;  per neuron j over the n values of the rows in R
    mp, mt the means;  M2p = sum (p - mp)^2,  M2t = sum (t - mt)^2,  C = sum (p - mp)(t - mt)
    sd_p = sqrt(M2p / n), sd_t = sqrt(M2t / n), a = sd_p + eps, c = sd_t + eps,  r_j = (C / n) / (a c)
    loss = share * red_j (1 - r_j)          (red = mean or sum; 0 when n = 0)
    dpred[b] = -g share rho [ (t - mt) / (n a c) - r_j (p - mp) / (n sd_p a) ]  for b in R, rho = 1/N or 1; the second term is
    DEFINED as 0 where sd_p == 0 (the kink of sqrt at a constant prediction);  dpred[b] = 0 for b outside R.
Sums run in extended precision where the platform has it and are rounded to float64 once, so that the checker's own summation
error stays well below the float64 ordering slack the kernels are allowed.  ``raw=True`` builds the second moments from the raw
sums (sum p^2 - n mp^2, ...) in float64 instead: the formulation the kernels must NOT use, kept to show what a test would catch.
"""
from __future__ import annotations

import numpy as np

EPS = 1e-8
_LD = np.longdouble


def select_rows(p, t, w):
    """(n, N) float64 views of the counted rows: p[R], t[R] with (sample, frame) flattened sample-major."""
    p, t, w = np.asarray(p, np.float64), np.asarray(t, np.float64), np.asarray(w)
    if p.ndim == 2:
        p, t = p[:, :, None], t[:, :, None]
    rows = np.flatnonzero(w != 0)
    N = p.shape[1]
    return p[rows].transpose(0, 2, 1).reshape(-1, N), t[rows].transpose(0, 2, 1).reshape(-1, N)


def moments(p, t, w, raw: bool = False) -> dict:
    """n and the per-neuron mean_p, mean_t, M2p, M2t, C (float64 N-vectors; all 0 when no row counts)."""
    P, Tt = select_rows(p, t, w)
    n, N = P.shape
    z = np.zeros(N)
    if n == 0:
        return dict(n=0, mean_p=z, mean_t=z.copy(), M2p=z.copy(), M2t=z.copy(), C=z.copy())
    if raw:
        sp, st = P.sum(0), Tt.sum(0)
        mp, mt = sp / n, st / n
        return dict(n=n, mean_p=mp, mean_t=mt, M2p=(P * P).sum(0) - n * mp * mp, M2t=(Tt * Tt).sum(0) - n * mt * mt,
                    C=(P * Tt).sum(0) - n * mp * mt)
    Pl, Tl = P.astype(_LD), Tt.astype(_LD)
    mp, mt = Pl.sum(0) / n, Tl.sum(0) / n
    dp, dt = Pl - mp, Tl - mt
    f = lambda v: np.asarray(v, np.float64)
    return dict(n=n, mean_p=f(mp), mean_t=f(mt), M2p=f((dp * dp).sum(0)), M2t=f((dt * dt).sum(0)), C=f((dp * dt).sum(0)))


def coefficients(mom: dict, eps: float = EPS) -> dict:
    """r and the two gradient coefficients c1 = 1/(n a c), c2 = r/(n sd_p a) (0 where sd_p == 0); all 0 when n == 0."""
    n = mom["n"]
    N = mom["M2p"].shape[0]
    if n == 0:
        return dict(r=np.zeros(N), c1=np.zeros(N), c2=np.zeros(N), sd_p=np.zeros(N), sd_t=np.zeros(N))
    sd_p, sd_t = np.sqrt(mom["M2p"] / n), np.sqrt(mom["M2t"] / n)
    a, c = sd_p + eps, sd_t + eps
    r = (mom["C"] / n) / (a * c)
    c1 = 1.0 / (n * a * c)
    with np.errstate(divide="ignore", invalid="ignore"):
        c2 = np.where(sd_p > 0, r / (n * sd_p * a), 0.0)
    return dict(r=r, c1=c1, c2=c2, sd_p=sd_p, sd_t=sd_t)


def pearson(p, t, w, eps: float = EPS, raw: bool = False) -> np.ndarray:
    return coefficients(moments(p, t, w, raw=raw), eps)["r"]


def loss_term(p, t, w, share: float, eps: float = EPS, reduction: str = "mean", raw: bool = False) -> float:
    """share * red_j (1 - r_j) of one mouse, float64; exactly 0.0 when no row counts."""
    mom = moments(p, t, w, raw=raw)
    if mom["n"] == 0:
        return 0.0
    one_minus = 1.0 - coefficients(mom, eps)["r"]
    red = float(one_minus.astype(_LD).sum())
    return float(share) * (red / one_minus.shape[0] if reduction == "mean" else red)


def shares(weights) -> np.ndarray:
    """share_m = sum_b w[b, m] / sum w, formed in float32 as the caller of the kernels forms it, returned as float64."""
    w = np.asarray(weights, np.float32)
    return (w.sum(0, dtype=np.float32) / w.sum(dtype=np.float32)).astype(np.float64)


def loss(preds, targets, weights, eps: float = EPS, reduction: str = "mean") -> float:
    """The loss of MiceCorrelationLoss: the sum over mice of the terms, with the shares of ``shares``."""
    sh = shares(weights)
    return float(sum(loss_term(p, t, np.asarray(weights)[:, m], sh[m], eps, reduction) for m, (p, t) in enumerate(zip(preds, targets))))


def grad_term(p, t, w, share: float, g: float = 1.0, eps: float = EPS, reduction: str = "mean"):
    """Closed-form dpred of one mouse (float64, the shape of p) and, per neuron, the largest |(t - mt) c1| (the magnitude the
    cancellation slack of the GPU test is stated in)."""
    p64, t64, w = np.asarray(p, np.float64), np.asarray(t, np.float64), np.asarray(w)
    squeeze = p64.ndim == 2
    if squeeze:
        p64, t64 = p64[:, :, None], t64[:, :, None]
    N = p64.shape[1]
    mom = moments(p64, t64, w)
    co = coefficients(mom, eps)
    rho = 1.0 / N if reduction == "mean" else 1.0
    counted = (w != 0)[:, None, None]
    with np.errstate(invalid="ignore"):             # rows outside R may hold NaN: they are selected away below
        first = (t64 - mom["mean_t"][None, :, None]) * co["c1"][None, :, None]
        second = (p64 - mom["mean_p"][None, :, None]) * co["c2"][None, :, None]
        d = np.where(counted, -float(g) * float(share) * rho * (first - second), 0.0)
        mag = np.where(counted, np.abs(first), 0.0).max(axis=(0, 2)) if mom["n"] else np.zeros(N)
    return (d[:, :, 0] if squeeze else d), mag


def chan_merge(a: dict, b: dict) -> dict:
    """Moments of the union of two disjoint sets of rows from their moments (pairwise / Chan formulas); either may be empty."""
    n = a["n"] + b["n"]
    if n == 0:
        return dict(a)
    fb = b["n"] / n
    cross = a["n"] * fb
    dp, dt = b["mean_p"] - a["mean_p"], b["mean_t"] - a["mean_t"]
    return dict(n=n, mean_p=a["mean_p"] + dp * fb, mean_t=a["mean_t"] + dt * fb, M2p=a["M2p"] + b["M2p"] + dp * dp * cross,
                M2t=a["M2t"] + b["M2t"] + dt * dt * cross, C=a["C"] + b["C"] + dp * dt * cross)


def ulp32(x) -> np.ndarray:
    """One fp32 ulp at |x| (x taken as float64, rounded to fp32 first)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def centred_case(B=5, N=7, T=16, seed=21):
    """Predictions 1e6 + k/16 for small integers k (exact in fp32, spread about 1) against ordinary targets."""
    rng = np.random.default_rng(seed)
    k = rng.integers(-24, 25, size=(B, N, T))
    p = (1.0e6 + k / 16.0).astype(np.float32)
    assert np.array_equal(p.astype(np.float64), 1.0e6 + k / 16.0)
    t = np.maximum(rng.normal(size=(B, N, T)), 0).astype(np.float32) + (k / 16.0).astype(np.float32) * 0.5
    return p, t


CENTRED_BOUND = 1e-9         # relative, on M2p and on r: float64 ordering slack is ~1e-14 here, a raw-sum build misses by ~1e-3


def torch_loss(preds, targets, weights, eps: float = EPS, reduction: str = "mean"):
    """The loss of MiceCorrelationLoss as a differentiable float64 torch expression (the ``corr`` formula spelled out on the counted
    rows; shares formed in float32 as ``shares``): for autograd references.  ``weights`` is a host tensor or array; mice without a
    row are left out (their term is 0).  Not defined at a constant prediction (sqrt at 0), where the closed form above rules."""
    import torch
    w = np.asarray(weights, np.float32)
    sh = shares(w)
    total = 0.0
    for m, (p, t) in enumerate(zip(preds, targets)):
        rows = torch.from_numpy(np.flatnonzero(w[:, m] != 0))
        if rows.numel() == 0:
            continue
        p, t = p.double(), t.double()
        if p.dim() == 2:
            p, t = p[:, :, None], t[:, :, None]
        N = p.shape[1]
        P, Tt = p[rows].permute(0, 2, 1).reshape(-1, N), t[rows].permute(0, 2, 1).reshape(-1, N)
        std = lambda v: ((v - v.mean(0, keepdim=True)) ** 2).mean(0, keepdim=True).sqrt()
        y1 = (P - P.mean(0, keepdim=True)) / (std(P) + eps)
        y2 = (Tt - Tt.mean(0, keepdim=True)) / (std(Tt) + eps)
        one_minus = 1.0 - (y1 * y2).mean(0)
        total = total + float(sh[m]) * (one_minus.mean() if reduction == "mean" else one_minus.sum())
    return total

"""Inputs of the ten-step trajectory of tests/test_gpu_guarded_step.py, built here because tests/test_host_guarded_step.py checks on
the CPU that they are well conditioned for the bound they are held to (imported only by tests)."""
import math

import torch

from oracle import dwiseneuro_oracle as orc
from tests import gpu_helpers as H

TRAJ_SIZES = [257, 4097, 3, 1, 16 * 256 + 1]
BAD_STEPS = (3, 7)
TRAJ_STEP0 = (1, 1000, 100_000)
TRAJ_SEED = 41
# The table holds a 1-element and a 3-element tensor (kernel edge cases).  For those the norm of a tensor is one number or three, and a
# first moment that passes through zero on the last step turns float32's 6e-8 per operation into 1e-6 .. 1e-4 of the RESULT whatever
# computes it (seeds 41, 43, 54): rounding errors of m + (1-b1)(g - m) are relative to its operands, not to what is left after they
# cancel.  Tensors of at most TINY elements are therefore compared per element against the largest magnitude the element's state and
# its update's operands took along the trajectory (traj_reference's `scale`); every other tensor norm-relative, as the optimizer
# tests do.  The bound is gpu_helpers.ADAMW_BOUND for both.
TINY = 3
LR, WD, DECAY, GSCALE = 2.4e-3, 0.05, 0.999, 0.37


def ref_norm(grads, gscale=GSCALE):
    """sqrt(sum (grad_scale * g)^2) over the finite elements, float64 on the CPU, and the number of the others."""
    tot, bad = 0.0, 0
    for g in grads:
        g = g.double()
        fin = torch.isfinite(g)
        tot += float(((gscale * g[fin]) ** 2).sum())
        bad += int((~fin).sum())
    return math.sqrt(tot), bad


def traj_case(step0):
    return H.adamw_case(TRAJ_SEED + step0, TRAJ_SIZES, step0)


def traj_step(case, s, clip):
    """gradients of step s (a NaN in one element on the bad steps), their norm, the non-finite count, max_norm and the clip coefficient:
    norm / max_norm is 3 on even steps and 0.5 on odd ones."""
    grads = [c["grads"][s].clone() for c in case]
    if s in BAD_STEPS:
        grads[s % len(grads)][0] = float("nan")
    norm, bad = ref_norm(grads)
    max_norm = (norm / 3.0 if s % 2 == 0 else norm / 0.5) if clip else 0.0
    coef = min(1.0, max_norm / (norm + 1e-6)) if clip else 1.0
    return grads, norm, bad, max_norm, coef


def traj_reference(case, step0, clip, has_ema, dtype=torch.float64, with_scale=False):
    """Eight AdamW steps over the good gradients with counts step0 .. step0 + 7 and ten EMA lerps.  float64: the reference.
    float32: the same formulas as the kernel writes them (adamw_ema_kernel), every operation rounded to float32 by torch on the CPU —
    what float32 arithmetic costs by itself on these inputs, whatever runs it.  with_scale: also, per tensor and state, the largest
    magnitude per element of the state along the trajectory and of the operands of its update (|g| for m, g^2 for v, |p| for ema)."""
    st = [{k: c[k].to(dtype) for k in ("p", "m", "v", "ema")} for c in case]
    scale = [{k: r[k].abs().double() for k in r} for r in st]

    def grow(i):
        for k in scale[i]:
            scale[i][k] = torch.maximum(scale[i][k], st[i][k].abs().double())

    count = step0
    for s in range(10):
        grads, _, _, _, coef = traj_step(case, s, clip)
        for i, r in enumerate(st):
            if s not in BAD_STEPS:
                if dtype == torch.float64:
                    g = grads[i].double() * GSCALE * coef
                    r["p"], r["m"], r["v"] = orc.adamw_step(r["p"], g, r["m"], r["v"], count, LR, weight_decay=WD)
                else:
                    f = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
                    g = grads[i] * (f(GSCALE) * f(coef))
                    p = r["p"] * f(1.0 - LR * WD)
                    m = r["m"] + f(1.0 - 0.9) * (g - r["m"])
                    v = f(0.999) * r["v"] + f(1.0 - 0.999) * g * g
                    denom = v.sqrt() / f(math.sqrt(1.0 - 0.999 ** count)) + f(1e-8)
                    r["p"], r["m"], r["v"] = p - f(LR / (1.0 - 0.9 ** count)) * (m / denom), m, v
                scale[i]["m"] = torch.maximum(scale[i]["m"], g.abs().double())
                scale[i]["v"] = torch.maximum(scale[i]["v"], g.double() ** 2)
            if has_ema[i]:
                if dtype == torch.float64:
                    r["ema"] = orc.ema_update(r["ema"], r["p"], DECAY)
                else:
                    r["ema"] = torch.tensor(DECAY, dtype=torch.float32) * r["ema"] + torch.tensor(1.0 - DECAY, dtype=torch.float32) * r["p"]
                scale[i]["ema"] = torch.maximum(scale[i]["ema"], r["p"].abs().double())
            grow(i)
        count += int(s not in BAD_STEPS)
    return (st, scale) if with_scale else st


def traj_error(got, ref, scale):
    """The figure held to ADAMW_BOUND: norm-relative for a tensor of more than TINY elements, else the largest per-element error
    relative to that element's `scale`."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    if ref.numel() > TINY:
        return float((got - ref).norm() / (ref.norm() + 1e-30))
    return float(((got - ref).abs() / (scale.reshape(-1) + 1e-30)).max())

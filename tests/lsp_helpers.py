"""Learnable Softplus beta: what the tests of the feature share.

``term_f32`` restates, in numpy float32, the per-element term the dbeta variant of ``readout_dz_kernel`` evaluates from the stored
fp32 output (``readout_dbeta_term`` in csrc/dwn_elementwise.hip); ``term_f64`` is the same formula in float64 on the same stored
output — the reference of the element-by-element checks; ``term_recovered_f32`` / ``term_true_z_f32`` are the two cancelling
forms the kernel does NOT use.  All four return beta^2 * d out / d beta; ``dgdbeta`` divides by beta^2 in float64, as the
kernel's finaliser does.

With g = softplus(beta z) / beta, u = beta g, e = exp(-u), sigma = sigmoid(beta z) = 1 - e and beta z = u + log(sigma):
    beta^2 dg/dbeta = beta z sigma - u = sigma log(sigma) - u e
"""
import numpy as np
import torch

from oracle import dwiseneuro_oracle as orc

LN2 = 0.69314718
BETAS = (0.07, 1.0, 5.0)
# the bound on |term_f32 - term_f64| / |term_f64| over beta in BETAS and beta z = -69 ... 25 (step 0.25).  Measured maximum with this
# file's numpy restatement: 1.8e-7 (beta 0.07, beta z 7.25); 1.03e-6 at beta z 22.75 before the kernel put the rounding of
# u = beta * out back into exp(-u).  tests/test_learnable_softplus_cpu.py re-measures and prints it.
TERM_BOUND = 1.0e-6


def sweep_bz(lo=-69.0, hi=25.0, step=0.25):
    return torch.arange(lo, hi + step / 2, step, dtype=torch.float64)


def stored_out(bz, beta):
    """The fp32 output a readout stores for pre-activations z = bz / beta: oracle.softplus in float64, rounded once."""
    b32 = float(np.float32(beta))
    return orc.softplus(bz / b32, b32).float().numpy()


def term_f32(out, beta):
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (f(beta) * out.astype(f)).astype(f)
        # the kernel's fma(beta, out, -u): the fp32 product's exact residual (a 24 x 24 bit product is exact in float64)
        du = (np.float64(f(beta)) * out.astype(np.float64) - u.astype(np.float64)).astype(f)
        e0 = np.exp(-u).astype(f)
        e = (e0.astype(np.float64) - e0.astype(np.float64) * du.astype(np.float64)).astype(f)
        sg = (-np.expm1(-u)).astype(f)
        lg = np.where(u <= f(LN2), np.log(sg), np.log1p(-e)).astype(f)
        t = ((sg * lg).astype(f) - (u * e).astype(f)).astype(f)
    return np.where(sg > 0, t, f(0)).astype(f)


def term_f64(out, beta):
    b = np.float64(np.float32(beta))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = b * out.astype(np.float64)
        e = np.exp(-u)
        sg = -np.expm1(-u)
        lg = np.where(u <= np.log(2.0), np.log(sg), np.log1p(-e))
        t = sg * lg - u * e
    return np.where(sg > 0, t, 0.0)


def term_recovered_f32(out, beta):
    """beta z recovered as log(expm1(u)), then beta z sigma - u: the two products cancel."""
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u = (f(beta) * out.astype(f)).astype(f)
        bz = np.log(np.expm1(u).astype(f)).astype(f)
        sg = (-np.expm1(-u)).astype(f)
        t = ((bz * sg).astype(f) - u).astype(f)
    return np.where(sg > 0, t, f(0)).astype(f)


def term_true_z_f32(out, beta, bz):
    """The same with the true pre-activation kept: beta z sigmoid(beta z) - u still cancels."""
    f = np.float32
    bz = bz.astype(f)
    with np.errstate(over="ignore"):
        sg = (f(1) / (f(1) + np.exp(-bz).astype(f))).astype(f)
    u = (f(beta) * out.astype(f)).astype(f)
    return ((bz * sg).astype(f) - u).astype(f)


def dgdbeta(term, beta):
    b = np.float64(np.float32(beta))
    return term.astype(np.float64) / (b * b)


def max_rel(term, ref):
    """max |term - ref| / |ref| over the elements with ref != 0, and the beta z index where it is reached"""
    ref = ref.astype(np.float64)
    ok = ref != 0
    err = np.zeros_like(ref)
    err[ok] = np.abs(term.astype(np.float64)[ok] - ref[ok]) / np.abs(ref[ok])
    i = int(err.argmax())
    return float(err[i]), i


def oracle_dbeta(z64, beta, dout64):
    """d/dbeta of sum(dout * oracle.softplus(z, beta)) by float64 autograd (0 in the thresholded branch)."""
    b = torch.tensor(float(np.float32(beta)), dtype=torch.float64, requires_grad=True)
    (orc.softplus(z64, b) * dout64).sum().backward()
    return float(b.grad)


def readout_reference_beta(d, groups, n_out, beta):
    """gpu_helpers.readout_reference with beta a float64 0-d leaf: the same float64 oracle and autograd, plus dbeta."""
    pre = "readouts.0"
    w = d["w"].double()[:, :, None].clone().requires_grad_()
    bias = d["bias"].double().clone().requires_grad_()
    x = d["x"].double().clone().requires_grad_()
    b = torch.tensor(float(np.float32(beta)), dtype=torch.float64, requires_grad=True)
    dm = None if d["drop_mask"] is None else d["drop_mask"].double()
    out = orc.readout(x, pre, {pre + ".layer.1.weight": w, pre + ".layer.1.bias": bias}, groups, n_out, b, dm)
    out.backward(d["dout"].double())
    return dict(out=out.detach(), dx=x.grad, dw=w.grad[:, :, 0], dbias=bias.grad, dbeta=float(b.grad))

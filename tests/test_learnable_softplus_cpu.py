"""Learnable Softplus beta, the arithmetic of d out / d beta on the CPU (no GPU, no kernels).

tests/lsp_helpers.term_f32 restates the kernel's per-element term in numpy float32.  It is held, element by element, to the same
formula in float64 on the same stored fp32 output, and its sum to float64 autograd through oracle.softplus; the two cancelling
forms the kernel does not use are shown to miss the same bound, which is why the form matters.
"""
import numpy as np
import pytest
import torch

from tests import lsp_helpers as S


@pytest.mark.parametrize("beta", S.BETAS)
def test_term_fp32_matches_float64_element_by_element(beta):
    bz = S.sweep_bz()
    out = S.stored_out(bz, beta)
    err, i = S.max_rel(S.term_f32(out, beta), S.term_f64(out, beta))
    print(f"LSPFIG term beta {beta} max rel {err:.3e} at beta*z {float(bz[i]):.2f}")
    assert err <= S.TERM_BOUND, f"beta {beta}: {err:.3e} at beta*z = {float(bz[i])}"


@pytest.mark.parametrize("beta", S.BETAS)
def test_term_finite_down_to_underflow(beta):
    """beta z down to -120: the stored output underflows to exactly 0 on the way; such an element contributes 0, not NaN."""
    bz = S.sweep_bz(-120.0, 25.0)
    out = S.stored_out(bz, beta)
    t = S.term_f32(out, beta)
    assert (out == 0).any() and np.isfinite(t).all()
    assert (t[out == 0] == 0).all() and (t <= 0).all()      # (a subnormal out may leave u * e = 0 as well)


@pytest.mark.parametrize("beta", S.BETAS)
def test_sum_matches_oracle_autograd(beta):
    """dout = 1: every term has the same sign, nothing averages out.  Against float64 autograd through oracle.softplus at the true
    z (0 in the thresholded branch, where the formula leaves at most 21 e^-20 / beta^2 per element): 1e-7 of the sum of |terms|."""
    bz = S.sweep_bz()
    z = bz / float(np.float32(beta))
    out = S.stored_out(bz, beta)
    ref = S.oracle_dbeta(z, beta, torch.ones_like(z))
    got = S.dgdbeta(S.term_f32(out, beta), beta).sum()
    sumabs = np.abs(S.dgdbeta(S.term_f64(out, beta), beta)).sum()
    err = abs(got - ref) / sumabs
    print(f"LSPFIG sum beta {beta} {err:.3e}")
    assert err <= 1e-7


@pytest.mark.parametrize("beta", S.BETAS)
def test_cancelling_forms_miss_the_bound(beta):
    """Recovering beta z = log(expm1(u)) and forming beta z sigma - u, or the same with the true z kept: both are percent-level
    wrong at beta z = 15 and exactly 0 from about 18 up."""
    bz = S.sweep_bz()
    out = S.stored_out(bz, beta)
    ref = S.term_f64(out, beta)
    for name, t in (("recovered", S.term_recovered_f32(out, beta)), ("true z", S.term_true_z_f32(out, beta, bz.numpy()))):
        err, i = S.max_rel(t, ref)
        at15 = abs(float(t[bz == 15.0][0]) - float(ref[bz == 15.0][0])) / abs(float(ref[bz == 15.0][0]))
        print(f"LSPFIG {name} beta {beta} max rel {err:.3e} at {float(bz[i]):.2f}; at 15: {at15:.3e}")
        assert err > 1e3 * S.TERM_BOUND and at15 > 1e2 * S.TERM_BOUND, name

"""The float64 checker of the drifting-Gabor stimulus (tests/gabor_reference.py) held to two independent witnesses: float64
autograd of a separately written form (the wave-vector form ky * y + kx * x instead of rotated coordinates), and central
differences.  Also the rules the GPU tests rely on: envelope "none" has dsigma == 0, window and pad, the clamp passes the gradient
at equality, the NaN rule, and the clamp case of tests/test_gpu_gabor.py has a useful share of clamped elements none of which sits
near an edge.  No GPU here."""
import math

import pytest
import torch

from tests import gabor_reference as gb

# the clamp case of the GPU tests: H, W, T and the eight parameters
CLAMP_SHAPE = (36, 64, 16)
CLAMP_PARAMS = (17.3, 30.6, 6.5, 0.7, 0.11, 0.13, 0.4, 160.0)
CLAMP_BACKGROUND, CLAMP_RANGE = 127.5, (0.0, 255.0)


def wave_vector_form(params, T, H, W, envelope, background):
    """raw [B][T][H][W] written independently: phase = 2 pi (ky (y - cy) + kx (x - cx) - tf t) + phase with the wave vector
    (ky, kx) = sf (sin theta, cos theta); differentiable in ``params``."""
    rows = []
    for p in params:
        cy, cx, sigma, theta, sf, tf, phase, amp = p
        ky, kx = sf * torch.sin(theta), sf * torch.cos(theta)
        t = torch.arange(T, dtype=torch.float64)[:, None, None]
        y = torch.arange(H, dtype=torch.float64)[None, :, None] - cy
        x = torch.arange(W, dtype=torch.float64)[None, None, :] - cx
        arg = 2.0 * math.pi * (ky * y + kx * x - tf * t) + phase
        env = torch.exp(-0.5 * (x * x + y * y) / (sigma * sigma)) if envelope == "gaussian" else 1.0
        rows.append(background + amp * env * torch.cos(arg) + 0.0 * t)
    return torch.stack(rows)


def some_params(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.rand(B, 8, generator=g, dtype=torch.float64)
    lo = torch.tensor([0.2 * H, 0.2 * W, 1.5, -3.0, 0.02, -0.3, -3.0, 20.0], dtype=torch.float64)
    hi = torch.tensor([0.8 * H, 0.8 * W, 6.0, 3.0, 0.3, 0.3, 3.0, 90.0], dtype=torch.float64)
    return lo + (hi - lo) * r


@pytest.mark.parametrize("envelope", ["gaussian", "none"])
def test_render_and_jacobian_against_autograd_of_the_wave_vector_form(envelope):
    B, T, H, W = 3, 4, 9, 11
    params = some_params(B, H, W, 1)
    p = params.clone().requires_grad_(True)
    raw = wave_vector_form(p, T, H, W, envelope, 100.0)
    ref = gb.raw_video(params, T, H, W, envelope, 100.0)
    e = float((raw.detach() - ref).abs().max())
    print(f"render vs wave-vector form ({envelope}): max abs diff {e:.3e}")
    assert e < 1e-11
    dout = torch.randn(B, T, H, W, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    (g,) = torch.autograd.grad((raw * dout).sum(), p)
    full = torch.zeros(B, 5, T, H, W, dtype=torch.float64)
    full[:, 0] = dout
    dp = gb.dparams(full, params, 0, envelope, 100.0, None, None)
    rel = float(((dp - g).abs() / (g.abs() + 1e-9 * g.abs().max())).max())
    print(f"analytic dparams vs autograd ({envelope}): max rel diff {rel:.3e}")
    assert rel < 1e-9
    if envelope == "none":
        assert bool((dp[:, 2] == 0).all()) and bool((gb.param_jacobian(params, T, H, W, "none")[:, 2] == 0).all())


@pytest.mark.parametrize("envelope", ["gaussian", "none"])
def test_jacobian_against_central_differences(envelope):
    B, T, H, W = 2, 3, 7, 8
    params = some_params(B, H, W, 3)
    J = gb.param_jacobian(params, T, H, W, envelope)
    for k in range(8):
        h = 1e-6 * max(1.0, float(params[:, k].abs().max()))
        up, dn = params.clone(), params.clone()
        up[:, k] += h
        dn[:, k] -= h
        fd = (gb.raw_video(up, T, H, W, envelope) - gb.raw_video(dn, T, H, W, envelope)) / (2 * h)
        e = float((fd - J[:, k]).abs().max()) / (float(J[:, k].abs().max()) + 1e-30 if float(J[:, k].abs().max()) > 0 else 1.0)
        print(f"central difference {gb.PARAM_NAMES[k]} ({envelope}): rel err {e:.3e}")
        assert e < 1e-6, gb.PARAM_NAMES[k]


def test_window_and_pad():
    B, T, H, W = 2, 2, 8, 12
    window = (2, 3, 4, 6)
    params = some_params(B, H, W, 4)
    tmpl = torch.randn(B, 5, T, H, W, dtype=torch.float64)
    out = gb.render(params, tmpl, 2, "gaussian", 127.5, (0.0, 255.0), window, 0.5)
    inside = gb.window_mask(H, W, window)
    assert int(inside.sum()) == 24
    whole = gb.render(params, tmpl, 2, "gaussian", 127.5, (0.0, 255.0), None, 0.5)
    assert bool((out[:, 2][..., ~inside] == 0.5).all())
    assert torch.equal(out[:, 2][..., inside], whole[:, 2][..., inside])          # plane coordinates, not window coordinates
    assert torch.equal(out[:, [0, 1, 3, 4]], tmpl[:, [0, 1, 3, 4]])
    dout = torch.randn(B, 5, T, H, W, dtype=torch.float64)
    only_inside = dout.clone()
    only_inside[:, 2][..., ~inside] = 1e6                                       # outside the window nothing contributes
    assert torch.equal(gb.dparams(dout, params, 2, window=window), gb.dparams(only_inside, params, 2, window=window))


def test_clamp_passes_the_gradient_at_equality():
    """A grating of amplitude 10 around 245 reaches hi = 255 exactly at its crests (q integer): those elements pass, as with
    torch.clamp, and the elements beyond an edge do not."""
    params = torch.tensor([[0.0, 0.0, 1.0, 0.0, 0.25, 0.0, 0.0, 10.0]], dtype=torch.float64)
    T, H, W = 1, 1, 8
    raw = gb.raw_video(params, T, H, W, "none", 245.0)
    assert raw[0, 0, 0, 0] == 255.0 and raw[0, 0, 0, 4] == 255.0
    m = gb.pass_mask(params, T, H, W, "none", 245.0, (0.0, 255.0), None)
    assert bool(m.all())
    m2 = gb.pass_mask(params, T, H, W, "none", 245.0 + 1e-9, (0.0, 255.0), None)
    assert not bool(m2[0, 0, 0, 0]) and bool(m2[0, 0, 0, 1])
    x = torch.tensor([255.0, 255.0 + 1e-9], dtype=torch.float64, requires_grad=True)
    x.clamp(0.0, 255.0).sum().backward()
    assert x.grad.tolist() == [1.0, 0.0]


@pytest.mark.parametrize("bad", [("theta", math.nan), ("sigma", 0.0), ("sigma", -1.0), ("sf", math.inf)])
def test_nan_rule(bad):
    B, T, H, W = 2, 2, 5, 6
    params = some_params(B, H, W, 5)
    params[1, gb.PARAM_NAMES.index(bad[0])] = bad[1]
    tmpl = torch.zeros(B, 5, T, H, W, dtype=torch.float64)
    window = (1, 1, 3, 4)
    out = gb.render(params, tmpl, 0, "gaussian", 127.5, (0.0, 255.0), window, 0.5)
    inside = gb.window_mask(H, W, window)
    assert bool(torch.isnan(out[1, 0][..., inside]).all()) and bool((out[1, 0][..., ~inside] == 0.5).all())
    assert not bool(torch.isnan(out[0]).any()) and not bool(torch.isnan(out[1, 1:]).any())
    dp = gb.dparams(torch.ones(B, 5, T, H, W, dtype=torch.float64), params, 0, window=window)
    assert bool(torch.isnan(dp[1]).all()) and bool(torch.isfinite(dp[0]).all())
    if bad[0] == "sigma":      # sigma is not used without the envelope
        dp = gb.dparams(torch.ones(B, 5, T, H, W, dtype=torch.float64), params, 0, "none", window=window)
        assert bool(torch.isfinite(dp).all())


def test_the_gpu_clamp_case_clamps_a_few_elements_and_none_near_an_edge():
    H, W, T = CLAMP_SHAPE
    params = torch.tensor([CLAMP_PARAMS], dtype=torch.float32)
    raw = gb.raw_video(params, T, H, W, "gaussian", CLAMP_BACKGROUND)
    lo, hi = CLAMP_RANGE
    share = float(((raw < lo) | (raw > hi)).double().mean())
    near = int((((raw - lo).abs() < 1e-3) | ((raw - hi).abs() < 1e-3)).sum())
    print(f"clamp case: {100 * share:.2f} % of the elements clamped, {near} within 1e-3 of an edge")
    assert 0.001 <= share <= 0.05 and near == 0

"""The float64 checker of the behaviour modulator (tests/modulator_reference.py) held to float64 torch autograd of
``y * exp(m * tanh(c + h @ u.T))``, to the exact identity at u = c = 0 and to closed forms of sech^2.  CPU only."""
import math

import numpy as np
import pytest
import torch

from tests.modulator_reference import EPS, c0_element, reference, sech2


def _case(B, N, T, K, seed):
    rng = np.random.default_rng(seed)
    y = rng.gamma(2.0, 1.0, size=(B, N, T))
    h = rng.normal(size=(B, T, K))
    u = rng.normal(size=(N, K)) * 0.7 / math.sqrt(K)
    c = rng.normal(size=(N,)) * 0.3
    dout = rng.normal(size=(B, N, T))
    return y, h, u, c, dout


@pytest.mark.parametrize("B,N,T,K,m", [(1, 1, 1, 1, 2.0), (3, 17, 5, 3, 2.0), (2, 67, 32, 8, 0.7), (1, 9, 7, 32, 3.0)])
def test_checker_matches_float64_autograd(B, N, T, K, m):
    y, h, u, c, dout = _case(B, N, T, K, seed=B * 1000 + N)
    r = reference(y, h, u, c, m, dout)
    ty, th, tu, tc = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (y, h, u, c))
    a = tc[None, :, None] + torch.einsum("btk,nk->bnt", th, tu)
    out = ty * torch.exp(m * torch.tanh(a))
    out.backward(torch.tensor(dout))
    assert np.allclose(r["out"], out.detach().numpy(), rtol=1e-12, atol=0)
    for name, t in (("dy", ty), ("dh", th), ("du", tu), ("dc", tc)):
        want = t.grad.numpy()
        tol = 1e-12 * np.maximum(np.abs(want), np.abs(r[name]))
        # a sum may cancel: its terms set the scale of what float64 can resolve
        scale = {"dy": 0.0, "dh": np.einsum("bnt,nk->btk", np.abs(r["s"]), np.abs(u)),
                 "du": np.einsum("bnt,btk->nk", np.abs(r["s"]), np.abs(h)), "dc": np.abs(r["s"]).sum(axis=(0, 2))}[name]
        assert np.all(np.abs(r[name] - want) <= tol + 1e-13 * scale), name
        assert r["floor"][name].shape == want.shape and np.all(r["floor"][name] >= 0)
    assert r["floor"]["out"].shape == r["out"].shape and r["floor"]["s"].shape == r["s"].shape


def test_gain_is_exactly_one_at_zero_weights():
    y, h, u, c, dout = _case(2, 5, 4, 3, seed=7)
    r = reference(y, h, np.zeros_like(u), np.zeros_like(c), 2.0, dout)
    assert np.all(r["gain"] == 1.0) and np.array_equal(r["out"], y) and np.array_equal(r["dy"], dout)
    assert np.all(r["sech2"] == 1.0)
    assert np.array_equal(r["dc"], (dout * y * 2.0).sum(axis=(0, 2)))
    assert not r["dh"].any()                               # u = 0: no path back to the behaviour


@pytest.mark.parametrize("a", [0.0, 0.5, 5.0, 12.0, 20.0, 40.0])
def test_sech2_does_not_cancel(a):
    for sign in (1.0, -1.0):
        got = float(sech2(np.float64(sign * a)))
        e = math.exp(-2.0 * a)
        want = 4.0 * e / (1.0 + e) ** 2
        assert got == pytest.approx(want, rel=1e-15)
        assert got == pytest.approx(1.0 / math.cosh(a) ** 2, rel=1e-13)          # the other closed form
        assert got > 0.0
    if a >= 20.0:                                          # the cancelling form is exactly 0 here, the true value is not
        assert 1.0 - math.tanh(a) ** 2 == 0.0 and float(sech2(np.float64(a))) > 1e-70
    if a >= 12.0:                                          # ... and in fp32 from 12 on
        assert float(np.float32(1.0) - np.tanh(np.float32(a)) ** 2) == 0.0


def test_floor_constants():
    assert EPS == 2.0 ** -24
    assert c0_element(2.0, "out") == c0_element(2.0, "dy") == 23.0 and c0_element(2.0, "s") == 31.0
    # the floor of an element grows with the error of a only where the gain still depends on a
    y, h, u, c, dout = _case(1, 3, 2, 4, seed=3)
    sat = reference(y, h, u * 0, c * 0 + 30.0, 2.0, dout)["floor"]["out"]
    out = reference(y, h, u * 0, c * 0 + 30.0, 2.0, dout)["out"]
    assert np.allclose(sat, EPS * np.abs(out) * 23.0, rtol=1e-12)

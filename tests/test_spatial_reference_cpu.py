"""The float64 checker of the retinotopic readout gain (tests/spatial_reference.py) held to float64 ``grid_sample(bilinear, border,
align_corners=True)`` followed by ``y * exp(m * tanh(.))`` and to its autograd, for positions inside the map, on +-1 and outside,
and for one-cell axes.  CPU only.

Random positions are drawn with the fractional pixel coordinate in [0.05, 0.95]: on a cell boundary the position gradient is
one-sided and grid_sample may take the other side.  Boundary positions have their own test, with the expected side written out and
checked against a one-sided difference quotient of the checker's own forward."""
import numpy as np
import pytest
import torch

from tests.spatial_reference import EPS, cells, draw_positions, reference


def make_case(B, N, T, Hf, Wf, K, seed):
    rng = np.random.default_rng(seed)
    y = rng.gamma(2.0, 1.0, size=(B, N, T))
    g = rng.normal(size=(B, T, Hf, Wf, K))
    pos = draw_positions(rng, N, Hf, Wf)
    weight = rng.normal(size=(N, K)) * 0.7 / np.sqrt(K)
    bias = rng.normal(size=(N,)) * 0.3
    dout = rng.normal(size=(B, N, T))
    return y, g, pos, weight, bias, dout


def torch_chain(y, g, pos, weight, bias, m, dout):
    ty, tg, tw, tb = (torch.tensor(np.asarray(v, dtype=np.float64), requires_grad=True) for v in (y, g, weight, bias))
    tp = torch.tensor(np.asarray(pos, dtype=np.float64), requires_grad=True)
    B, T, Hf, Wf, K = tg.shape
    N = ty.shape[1]
    inp = tg.permute(0, 1, 4, 2, 3).reshape(B * T, K, Hf, Wf)
    grid = tp[None, :, None, :].expand(B * T, N, 1, 2)
    samp = torch.nn.functional.grid_sample(inp, grid, mode="bilinear", padding_mode="border", align_corners=True)
    samp = samp.reshape(B, T, K, N)
    a = tb[None, :, None] + torch.einsum("btkn,nk->bnt", samp, tw)
    out = ty * torch.exp(m * torch.tanh(a))
    out.backward(torch.tensor(np.asarray(dout, dtype=np.float64)))
    return out.detach().numpy(), dict(dy=ty.grad.numpy(), dg=tg.grad.numpy(), dpos=tp.grad.numpy(), dweight=tw.grad.numpy(),
                                      dbias=tb.grad.numpy())


def assert_close(r, out, grads, names=("dy", "dg", "dpos", "dweight", "dbias")):
    assert np.allclose(r["out"], out, rtol=1e-12, atol=0)
    for name in names:
        want = grads[name]
        # a sum may cancel: the floor (eps times the sum of the absolute terms) sets the scale of what float64 can resolve
        scale = r["floor"][name] / EPS
        assert r[name].shape == want.shape
        assert np.all(np.abs(r[name] - want) <= 1e-12 * np.abs(want) + 1e-13 * scale), name
        assert np.all(r["floor"][name] >= 0)


@pytest.mark.parametrize("B,N,T,Hf,Wf,K,m", [(1, 1, 1, 1, 1, 1, 1.0), (2, 17, 3, 2, 2, 3, 1.0), (1, 40, 5, 3, 5, 8, 2.0),
                                               (2, 33, 2, 8, 8, 4, 0.7), (1, 9, 4, 1, 4, 5, 1.0), (1, 9, 4, 4, 1, 5, 1.0)])
def test_checker_matches_float64_grid_sample(B, N, T, Hf, Wf, K, m):
    y, g, pos, weight, bias, dout = make_case(B, N, T, Hf, Wf, K, seed=100 * Hf + Wf)
    r = reference(y, g, pos, weight, bias, m, dout)
    out, grads = torch_chain(y, g, pos, weight, bias, m, dout)
    assert_close(r, out, grads)
    if Wf == 1:
        assert not r["dpos"][:, 0].any()
    if Hf == 1:
        assert not r["dpos"][:, 1].any()
    if Hf > 1 and Wf > 1:
        assert np.all(r["dpos"] != 0)


def test_positions_outside_the_map_are_clamped_with_zero_gradient():
    B, N, T, Hf, Wf, K = 2, 8, 3, 3, 5, 4
    y, g, pos, weight, bias, dout = make_case(B, N, T, Hf, Wf, K, seed=5)
    pos[0] = (1.5, pos[0, 1]); pos[1] = (-1.5, pos[1, 1]); pos[2] = (pos[2, 0], 1.5); pos[3] = (pos[3, 0], -1e30)
    pos[4] = (1e30, -1.5)
    r = reference(y, g, pos, weight, bias, 1.0, dout)
    out, grads = torch_chain(y, g, np.clip(pos, -4.0, 4.0), weight, bias, 1.0, dout)    # (grid_sample itself overflows at 1e30)
    assert_close(r, out, grads)
    assert np.all(r["dpos"][[0, 1, 4], 0] == 0) and np.all(r["dpos"][[2, 3, 4], 1] == 0)
    assert np.all(r["dpos"][[0, 1], 1] != 0) and np.all(r["dpos"][[2, 3], 0] != 0)       # the other coordinate stays live
    assert np.all(r["floor"]["dpos"][[0, 1, 4], 0] == 0)


def test_boundary_positions_take_the_documented_side():
    """x = -1, an interior cell centre, +1 (Wf = 5: centres at -1, -0.5, 0, 0.5, 1, all exact).  Values and the gradients that do not
    depend on the side agree with grid_sample; dpos is the slope of the cell to the RIGHT of a centre (x0 = the centre's cell,
    fx = 0) and of the LAST cell at +1 (x0 = Wf - 2, fx = 1)."""
    B, N, T, Hf, Wf, K = 1, 6, 2, 3, 5, 3
    y, g, pos, weight, bias, dout = make_case(B, N, T, Hf, Wf, K, seed=9)
    pos[:, 0] = (-1.0, -0.5, 0.0, 0.5, 1.0, 1.0)
    pos[5, 1] = 1.0                                                         # a corner of the map: the last cell on both axes
    ce = cells(pos, Hf, Wf)
    assert list(ce["c"][0] % Wf) == [0, 1, 2, 3, 3, 3] and list(ce["fx"]) == [0, 0, 0, 0, 1, 1]
    assert ce["c"][0][5] // Wf == Hf - 2 and ce["fy"][5] == 1.0 and bool(ce["live_x"].all()) and bool(ce["live_y"].all())
    r = reference(y, g, pos, weight, bias, 1.0, dout)
    out, grads = torch_chain(y, g, pos, weight, bias, 1.0, dout)
    assert_close(r, out, grads, names=("dy", "dg", "dweight", "dbias"))
    h = 1e-6
    for n, side in enumerate((+1, +1, +1, +1, -1, -1)):
        p2 = pos.astype(np.float64).copy()
        p2[n, 0] += side * h
        quot = ((reference(y, g, p2, weight, bias, 1.0)["out"] - r["out"]) * dout).sum() / (side * h)
        assert quot == pytest.approx(r["dpos"][n, 0], rel=1e-4), (n, quot, r["dpos"][n, 0])
    p2 = pos.astype(np.float64).copy()
    p2[5, 1] -= h
    quot = ((reference(y, g, p2, weight, bias, 1.0)["out"] - r["out"]) * dout).sum() / (-h)
    assert quot == pytest.approx(r["dpos"][5, 1], rel=1e-4)


def test_gain_is_exactly_one_at_zero_heads():
    y, g, pos, weight, bias, dout = make_case(2, 5, 4, 3, 3, 3, seed=7)
    r = reference(y, g, pos, weight * 0, bias * 0, 1.5, dout)
    assert np.all(r["gain"] == 1.0) and np.array_equal(r["out"], y) and np.array_equal(r["dy"], dout)
    assert not r["dpos"].any() and not r["dg"].any()
    assert np.array_equal(r["dbias"], (dout * y * 1.5).sum(axis=(0, 2)))


def test_floor_has_the_operation_counts():
    """u = 0 and a saturated bias: the spread vanishes and the element floor is c0 eps |out|; with a single feature and a position on
    a cell centre the spread is m sech^2 ((4K + 3) A + WB D)."""
    y, g, pos, weight, bias, dout = make_case(1, 3, 2, 2, 2, 1, seed=3)
    sat = reference(y, g, pos, weight * 0, bias * 0 + 30.0, 1.0, dout)
    assert np.allclose(sat["floor"]["out"], EPS * np.abs(sat["out"]) * 13.0, rtol=1e-9)
    pos[:] = -1.0                                                          # w00 = 1: A is the first corner alone, D all four
    r = reference(y, g, pos, weight, bias * 0, 1.0, dout)
    corner = lambda i, j: np.abs(g[:, :, i, j, 0])[:, None, :] * np.abs(weight[:, 0])[None, :, None]
    A, D = corner(0, 0), corner(0, 0) + corner(0, 1) + corner(1, 0) + corner(1, 1)
    want = EPS * np.abs(r["out"]) * (13.0 + r["sech2"] * ((4 * 1 + 3) * A + (2 + 2 + 3) * D))
    assert np.allclose(r["floor"]["out"], want, rtol=1e-9)

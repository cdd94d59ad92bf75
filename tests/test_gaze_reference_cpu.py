"""CPU tests of tests/gaze_reference.py, the float64 checker the GPU tests of the gaze shifter compare with:
against float64 F.grid_sample and its autograd, the fill rule, the right derivative at integer shifts, and the exact
representability the bit-for-bit GPU cases rely on."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import gaze_reference as gr

SHAPES = [(2, 3, 5, 7), (1, 2, 2, 2), (2, 2, 36, 64)]


def random_shifts(gen, B, T, lo=-3.0, hi=3.0, away=1e-3):
    """Random shifts in [lo, hi] on the 2^-16 grid (so that the float32 subtraction dy - floor(dy) is exact and the float32 and
    float64 readings of the same shift agree), at least ``away`` from every integer."""
    s = torch.empty(B, T, 2, dtype=torch.float64)
    for i in range(s.numel()):
        while True:
            v = round(float(torch.empty(1).uniform_(lo, hi, generator=gen)) * 65536) / 65536
            if away <= v - math.floor(v) <= 1 - away:
                break
        s.view(-1)[i] = v
    return s


def grid_sample_shift(x, shift, video_channel=0):
    """The same translation by float64 grid_sample(bilinear, zeros, align_corners=True); differentiable in x and shift."""
    B, C, T, H, W = x.shape
    ys = torch.arange(H, dtype=torch.float64)[None, None, :, None]
    xs = torch.arange(W, dtype=torch.float64)[None, None, None, :]
    gx = ((xs + shift[:, :, 1, None, None]) * 2 / (W - 1) - 1).expand(B, T, H, W)
    gy = ((ys + shift[:, :, 0, None, None]) * 2 / (H - 1) - 1).expand(B, T, H, W)
    grid = torch.stack([gx, gy], dim=-1).reshape(B * T, H, W, 2)
    v = x[:, video_channel].reshape(B * T, 1, H, W)
    o = F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=True).view(B, T, H, W)
    return torch.cat([x[:, :video_channel], o[:, None], x[:, video_channel + 1:]], dim=1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_checker_equals_grid_sample(shape):
    B, T, H, W = shape
    gen = torch.Generator().manual_seed(B * 1000 + H * 10 + W)
    x = torch.randn(B, 2, T, H, W, dtype=torch.float64, generator=gen)
    dout = torch.randn(B, 2, T, H, W, dtype=torch.float64, generator=gen)
    shift = random_shifts(gen, B, T)
    xg, sg = x.clone().requires_grad_(True), shift.clone().requires_grad_(True)
    ref = grid_sample_shift(xg, sg, 1)
    (ref * dout).sum().backward()
    out = gr.resample(x, shift.float(), 1, 0.0)                     # the float32 reading of the shift, as the device takes it
    dx, _, ds, _ = gr.backward(x, shift.float(), dout, 1, 0.0)
    xa, sa = x.clone().requires_grad_(True), shift.clone().requires_grad_(True)
    (gr.resample(xa, sa, 1, 0.0) * dout).sum().backward()           # the checker's own autograd (what the model tests compose)
    errs = dict(forward=float((out - ref.detach()).abs().max()), dx=float((dx - xg.grad).abs().max()),
                dshift=float((ds - sg.grad).abs().max()), dx_autograd=float((xa.grad - xg.grad).abs().max()),
                dshift_autograd=float((sa.grad - sg.grad).abs().max()))
    print(f"gaze checker vs grid_sample {shape}: {errs}")
    assert all(e <= 1e-12 for e in errs.values()), errs
    assert float(sg.grad.abs().max()) > 0 and float(xg.grad[:, 1].abs().max()) > 0       # the case does exercise both gradients


def test_fill_is_a_shifted_zero_fill():
    gen = torch.Generator().manual_seed(3)
    B, T, H, W = 2, 3, 5, 7
    x = torch.randn(B, 3, T, H, W, dtype=torch.float64, generator=gen)
    dout = torch.randn(B, 3, T, H, W, dtype=torch.float64, generator=gen)
    shift = random_shifts(gen, B, T, -6.0, 6.0).float()
    out7 = gr.resample(x, shift, 0, 7.0)
    x0 = x.clone()
    x0[:, 0] -= 7.0
    out0 = gr.resample(x0, shift, 0, 0.0)
    out0[:, 0] += 7.0
    dx7, _, ds7, _ = gr.backward(x, shift, dout, 0, 7.0)
    dx0, _, ds0, _ = gr.backward(x0, shift, dout, 0, 0.0)
    errs = (float((out7 - out0).abs().max()), float((dx7 - dx0).abs().max()), float((ds7 - ds0).abs().max()))
    print(f"fill = 7 against fill = 0 on v - 7: forward {errs[0]:.2e}, dx {errs[1]:.2e}, dshift {errs[2]:.2e}")
    assert errs[0] <= 1e-12 and errs[1] == 0.0 and errs[2] <= 1e-11
    assert float((out7[:, 0] - gr.resample(x, shift, 0, 0.0)[:, 0]).abs().max()) > 1.0      # the fill does matter


def test_integer_shift_takes_the_right_derivative():
    gen = torch.Generator().manual_seed(5)
    B, T, H, W = 1, 4, 5, 6
    x = torch.randn(B, 1, T, H, W, dtype=torch.float64, generator=gen)
    dout = torch.randn(B, 1, T, H, W, dtype=torch.float64, generator=gen)
    shift = torch.tensor([[[0.0, 0.0], [1.0, -2.0], [-1.0, 3.0], [2.0, 0.0]]], dtype=torch.float32)
    _, _, ds, _ = gr.backward(x, shift, dout, 0, 2.0)
    base = gr.resample(x, shift, 0, 2.0)
    h = 0.25                                               # out is linear in the shift on [i, i + 1): the difference IS the slope
    right, left = torch.zeros(B, T, 2, dtype=torch.float64), torch.zeros(B, T, 2, dtype=torch.float64)
    for k in range(2):
        e = torch.zeros(2)
        e[k] = h
        right[..., k] = ((gr.resample(x, shift + e, 0, 2.0) - base) * dout).sum(dim=(1, 3, 4)) / h
        left[..., k] = ((base - gr.resample(x, shift - e, 0, 2.0)) * dout).sum(dim=(1, 3, 4)) / h
    err_r, err_l = float((ds - right).abs().max()), float((ds - left).abs().max())
    print(f"integer shifts: |dshift - right difference| {err_r:.2e}, |dshift - left difference| {err_l:.2e}")
    assert err_r <= 1e-12 and err_l > 1e-3


def test_dyadic_cases_are_exact_in_float32():
    """Integer video in 0...255, integer dout in -3...3, shifts on the 1/8 grid (and the special ones of the GPU tests): every value
    the checker returns is a float32, so the GPU tests may ask for equal bits."""
    gen = torch.Generator().manual_seed(7)
    for (B, T, H, W) in [(2, 3, 5, 7), (2, 4, 36, 64), (1, 2, 1, 9)]:
        x = torch.randint(0, 256, (B, 2, T, H, W), generator=gen).double()
        dout = torch.randint(-3, 4, (B, 2, T, H, W), generator=gen).double()
        pool = [0.0, 1.0, -1.0, 3.0, -3.0, 0.25, -0.25, 2.5, -1.75, -1e-9, H - 1.0, -(W - 1.0), max(H, W) + 2.0,
                -(max(H, W) + 2.0), 1e9, -1e9]
        pool += [k / 8 for k in range(-32, 33, 5)]
        idx = torch.randint(0, len(pool), (B, T, 2), generator=gen)
        shift = torch.tensor(pool, dtype=torch.float32)[idx]
        for fill in (0.0, 3.0):
            out = gr.resample(x, shift, 1, fill)
            dx, _, ds, _ = gr.backward(x, shift, dout, 1, fill)
            for name, v in (("out", out), ("dx", dx), ("dshift", ds)):
                exact = bool((v.float().double() == v).all())
                print(f"dyadic case {(B, T, H, W)} fill {fill}: {name} exactly representable in float32: {exact}")
                assert exact, name


def test_float32_reading_of_the_shift():
    x = torch.arange(24, dtype=torch.float64).view(1, 1, 1, 4, 6)
    tiny = torch.tensor([[[-1e-9, -1e-9]]], dtype=torch.float32)      # floor -1, the float32 fraction rounds to 1: the identity
    assert torch.equal(gr.resample(x, tiny, 0, 5.0), x)
    for big in (3e38, -3e38, 1e9):
        s = torch.tensor([[[big, 0.0]]], dtype=torch.float32)
        assert torch.equal(gr.resample(x, s, 0, 5.0), torch.full_like(x, 5.0))
        dx, _, ds, _ = gr.backward(x, s, torch.ones_like(x), 0, 5.0)
        assert float(dx.abs().max()) == 0.0 and float(ds.abs().max()) == 0.0
    for bad in (math.nan, math.inf):
        s = torch.tensor([[[0.5, bad]]], dtype=torch.float32)
        assert bool(torch.isnan(gr.resample(x, s, 0, 0.0)).all())

"""The gaze-shift kernels through the C-ABI (include/dwn.h dwn_gaze_shift_forward / _backward / dwn_plane_mean)
against the float64 checker tests/gaze_reference.py (itself held to float64 grid_sample on the CPU:
tests/test_gaze_reference_cpu.py).  u = 2^-24.  Every test prints what it measured before it asserts.

Bounds of the general cases, derived, not measured:
  out, dx   four terms w_ab * v, each with at most three roundings (1 - f, the product of the two factors, the product with v; a
            contraction into an FMA only removes one), plus three additions of partial sums no larger than sum |w v|: first order
            (3 + 3) u sum |w v|; asserted at 16 u sum |w v|.
  dshift    per pixel dout * ((1-f)(v_a - v_b) + f (v_c - v_d)): a difference, 1 - f, a product, the same again, an addition — about
            six roundings, each relative to a magnitude of the term; the float64 accumulation adds 2^-53 per addition and the
            final conversion one u of the result: asserted at 32 u sum |terms|.
The sums of magnitudes come from the checker.  Every output buffer sits between two guard bands that must come back untouched.
"""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gaze_reference as gr  # noqa: E402
from tests.det_child import deterministic_child  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

U = 2.0 ** -24
GUARD, SENTINEL = 64, -7777.0
# (B, Cin, T, H, W), video_channel, (c0, nc) of the plane mean
CASES = {
    "ragged":     ((2, 5, 3, 5, 7), 0, (3, 2)),       # ragged W, no 16-byte rows
    "one_row":    ((1, 5, 2, 1, 9), 0, (3, 2)),
    "one_column": ((1, 5, 1, 3, 1), 0, (3, 2)),
    "aligned":    ((2, 5, 2, 4, 8), 0, (3, 2)),       # 16-byte aligned planes
    "video_only": ((1, 1, 2, 6, 6), 0, (0, 1)),       # no copied channel
    "channel_3":  ((2, 8, 2, 5, 12), 3, (5, 3)),      # a non-zero video channel
    "frame":      ((2, 5, 4, 36, 64), 0, (3, 2)),     # the production frame
    "square":     ((1, 5, 2, 64, 64), 0, (3, 2)),     # the inference frame
}
FILLS = (0.0, 3.0)


def shift_set(H, W):
    m = float(max(H, W) + 2)
    return [0.0, 1.0, -1.0, 3.0, -3.0, 0.25, -0.25, 2.5, -1.75, -1e-9, float(H - 1), -float(W - 1), m, -m, 1e9, -1e9]


def shift_rounds(B, T, H, W):
    """Per-frame (dy, dx) drawn from the set so that one call mixes them; as many rounds as it takes for every value to have been a
    dy and a dx (7 is coprime to the size of the set)."""
    s = shift_set(H, W)
    n, F = len(s), B * T
    for r in range(math.ceil(n / F)):
        j = torch.arange(F) + r * F
        yield torch.tensor([[s[int(k) % n], s[(7 * int(k) + 3) % n]] for k in j], dtype=torch.float32).view(B, T, 2)


def guarded(shape, misalign=0):
    """A device tensor of `shape` between two guard bands (and optionally off the 16-byte grid by `misalign` floats)."""
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD + misalign,), SENTINEL, dtype=torch.float32, device=dev())
    return flat, flat[GUARD + misalign:GUARD + misalign + n].view(shape)


def guards_ok(flat, shape, misalign=0):
    n = math.prod(shape)
    lo, hi = flat[:GUARD + misalign], flat[GUARD + misalign + n:]
    return bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all())


def _args(L, shape, vc, fill):
    a = L.GazeArgs()
    a.B, a.Cin, a.T, a.H, a.W = shape
    a.video_channel, a.fill = vc, fill
    return a


def gpu_forward(x, shift, vc, fill, misalign=0):
    import sensorium_amd._lib as L
    if misalign:
        _, xd = guarded(tuple(x.shape), misalign)
        xd.copy_(x)
    else:
        xd = x.to(dev()).contiguous()
    sd = shift.to(dev()).contiguous()
    flat, out = guarded(tuple(x.shape), misalign)
    a = _args(L, tuple(x.shape), vc, fill)
    a.x, a.shift, a.out = xd.data_ptr(), sd.data_ptr(), out.data_ptr()
    L.check(L.lib.dwn_gaze_shift_forward(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_gaze_shift_forward")
    torch.cuda.synchronize()
    assert guards_ok(flat, tuple(x.shape), misalign), "dwn_gaze_shift_forward wrote outside out"
    return out.cpu()


def gpu_backward(x, shift, dout, vc, fill, want_dx=True, want_dshift=True, misalign=0):
    import sensorium_amd._lib as L
    xd, sd = x.to(dev()).contiguous(), shift.to(dev()).contiguous()
    if misalign:
        _, dd = guarded(tuple(x.shape), misalign)
        dd.copy_(dout)
    else:
        dd = dout.to(dev()).contiguous()
    fdx, dx = guarded(tuple(x.shape), misalign)
    fds, ds = guarded(tuple(shift.shape))
    a = _args(L, tuple(x.shape), vc, fill)
    a.x, a.shift, a.dout = xd.data_ptr(), sd.data_ptr(), dd.data_ptr()
    a.dx = dx.data_ptr() if want_dx else None
    a.dshift = ds.data_ptr() if want_dshift else None
    L.check(L.lib.dwn_gaze_shift_backward(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_gaze_shift_backward")
    torch.cuda.synchronize()
    assert guards_ok(fdx, tuple(x.shape), misalign) and guards_ok(fds, tuple(shift.shape)), "dwn_gaze_shift_backward wrote outside"
    if not want_dx:
        assert bool((dx == SENTINEL).all()), "dx == NULL must skip dx"
    if not want_dshift:
        assert bool((ds == SENTINEL).all()), "dshift == NULL must skip dshift"
    return (dx.cpu() if want_dx else None), (ds.cpu() if want_dshift else None)


def gpu_plane_mean(x, c0, nc):
    import sensorium_amd._lib as L
    B, Cin, T, H, W = x.shape
    xd = x.to(dev()).contiguous()
    flat, mean = guarded((B, T, nc))
    L.check(L.lib.dwn_plane_mean(xd.data_ptr(), B, Cin, T, H, W, c0, nc, mean.data_ptr(), 0,
                                 torch.cuda.current_stream().cuda_stream), "dwn_plane_mean")
    torch.cuda.synchronize()
    assert guards_ok(flat, (B, T, nc)), "dwn_plane_mean wrote outside mean"
    return mean.cpu()


def integer_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, shape, generator=g).float()
    dout = torch.randint(-3, 4, shape, generator=g).float()
    return x, dout


# ------------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", list(CASES))
def test_exact_cases_bit_for_bit(name, fill):
    """Integer video in 0...255, integer dout in -3...3, shifts from the set (multiples of 1/8, and -1e-9 whose float32 fraction is
    exactly 1): every product and sum is exact in float32, so out, dx and dshift EQUAL the checker's float64 results."""
    shape, vc, _ = CASES[name]
    B, Cin, T, H, W = shape
    x, dout = integer_case(shape, 11)
    seen = set()
    for r, shift in enumerate(shift_rounds(B, T, H, W)):
        seen |= set(shift.view(-1).tolist())
        ref = gr.resample(x, shift, vc, fill)
        rdx, _, rds, _ = gr.backward(x, shift, dout, vc, fill)
        assert bool((ref.float().double() == ref).all()) and bool((rdx.float().double() == rdx).all()) \
            and bool((rds.float().double() == rds).all()), "the case is not exactly representable"
        out = gpu_forward(x, shift, vc, fill)
        dx, ds = gpu_backward(x, shift, dout, vc, fill)
        copied = [c for c in range(Cin) if c != vc]
        res = dict(out=torch.equal(out, ref.float()), dx=torch.equal(dx, rdx.float()), dshift=torch.equal(ds, rds.float()),
                   copied=torch.equal(out[:, copied].view(torch.int32), x[:, copied].view(torch.int32)),
                   dcopied=torch.equal(dx[:, copied].view(torch.int32), dout[:, copied].view(torch.int32)))
        print(f"gaze exact {name} fill {fill} round {r}: {res}; max |dshift| {float(rds.abs().max()):.1f}")
        assert all(res.values()), res
    assert len(seen) == len(set(torch.tensor(shift_set(H, W), dtype=torch.float32).tolist())), "a shift of the set was never drawn"


def test_zero_shift_copies_the_bits():
    """Weights 1, 0, 0, 0: the resampled channel is the source bit for bit, -0.0, a denormal and an infinity included."""
    shape = (2, 5, 3, 5, 7)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(1))
    x[0, 0, 0, 0, :4] = torch.tensor([-0.0, 1e-42, math.inf, -math.inf])
    out = gpu_forward(x, torch.zeros(2, 3, 2), 0, 3.0)
    same = torch.equal(out.view(torch.int32), x.view(torch.int32))
    print(f"shift 0: out has the bits of x: {same}")
    assert same
    # -1e-9: floor -1, the float32 fraction is exactly 1, so the weights are 0, 0, 0, 1 — the identity again.  The taps of weight 0
    # (an infinite neighbour, an infinite fill outside the frame) contribute nothing: no 0 * Inf.
    out = gpu_forward(x, torch.full((2, 3, 2), -1e-9), 0, math.inf)
    same = torch.equal(out.view(torch.int32), x.view(torch.int32))
    print(f"shift -1e-9, fill Inf: out has the bits of x: {same}")
    assert same
    dx, ds = gpu_backward(x, torch.full((2, 3, 2), -1e-9), x, 0, 3.0)
    assert torch.equal(dx.view(torch.int32), x.view(torch.int32))       # the adjoint of the identity


# ----------------------------------------------------------------------------------------------------------------- 2. general
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name,misalign", [(n, 0) for n in CASES] + [("aligned", 1), ("frame", 3)])
def test_general_cases_within_the_derived_bounds(name, misalign, fill):
    shape, vc, _ = CASES[name]
    B, Cin, T, H, W = shape
    g = torch.Generator().manual_seed(5)
    x, dout = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    shift = torch.empty(B, T, 2).uniform_(-4.0, 4.0, generator=g)
    ref, mag = gr.resample(x, shift, vc, fill, magnitudes=True)
    rdx, dx_mag, rds, ds_mag = gr.backward(x, shift, dout, vc, fill)
    out = gpu_forward(x, shift, vc, fill, misalign)
    dx, ds = gpu_backward(x, shift, dout, vc, fill, misalign=misalign)
    copied = [c for c in range(Cin) if c != vc]
    assert torch.equal(out[:, copied], x[:, copied]) and torch.equal(dx[:, copied], dout[:, copied])
    tiny = 1e-300
    e_out = float(((out[:, vc].double() - ref[:, vc]).abs() / (mag[:, vc] + tiny)).max()) / U
    e_dx = float(((dx[:, vc].double() - rdx[:, vc]).abs() / (dx_mag[:, vc] + tiny)).max()) / U
    e_ds = float(((ds.double() - rds).abs() / (ds_mag + tiny)).max()) / U
    print(f"gaze general {name} misalign {misalign} fill {fill}: worst |out - ref| / sum|w v| = {e_out:.2f} u (bound 16), "
          f"|dx - ref| / sum|w dout| = {e_dx:.2f} u (bound 16), |dshift - ref| / sum|terms| = {e_ds:.2f} u (bound 32)")
    assert bool(((out[:, vc].double() - ref[:, vc]).abs() <= 16 * U * mag[:, vc]).all())
    assert bool(((dx[:, vc].double() - rdx[:, vc]).abs() <= 16 * U * dx_mag[:, vc]).all())
    assert bool(((ds.double() - rds).abs() <= 32 * U * ds_mag).all())
    if min(H, W) >= 4:      # (a one-row / one-column plane is mostly pushed out of the frame by shifts of up to 4 pixels)
        assert float(rds.abs().max()) > 0 and float(rdx[:, vc].abs().max()) > 0
    # a null dx or dshift skips that part, the other one is unchanged
    only_dx, none = gpu_backward(x, shift, dout, vc, fill, want_dshift=False)
    none2, only_ds = gpu_backward(x, shift, dout, vc, fill, want_dx=False)
    assert none is None and none2 is None and torch.equal(only_dx, gpu_backward(x, shift, dout, vc, fill)[0])
    assert torch.equal(only_ds, gpu_backward(x, shift, dout, vc, fill)[1])


# ---------------------------------------------------------------------------------------------------------- 3. extreme shifts
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("name", ["ragged", "frame", "one_column"])
def test_extreme_shifts(name, fill):
    """Finite huge shifts: the frame is `fill`, dx and dshift of that frame are 0.  NaN / Inf: that frame of out is NaN, and only
    that frame; every other frame and channel equals the checker's (an exact case: bit for bit)."""
    shape, vc, _ = CASES[name]
    shape = (2, shape[1], 4, shape[3], shape[4])
    x, dout = integer_case(shape, 13)
    shift = torch.tensor([[[3e38, -3e38], [-3e38, 0.3], [0.7, 3e38], [0.25, -1.75]],
                          [[math.nan, 0.5], [1.0, math.inf], [-math.inf, math.nan], [-0.25, 2.5]]], dtype=torch.float32)
    ref = gr.resample(x, shift, vc, fill)
    rdx, _, rds, _ = gr.backward(x, shift, dout, vc, fill)
    out = gpu_forward(x, shift, vc, fill)
    dx, ds = gpu_backward(x, shift, dout, vc, fill)
    huge, bad, plain = [(0, 0), (0, 1), (0, 2)], [(1, 0), (1, 1), (1, 2)], [(0, 3), (1, 3)]
    res = {}
    res["huge_out_is_fill"] = all(bool((out[b, vc, t] == fill).all()) for b, t in huge)
    res["huge_dx_zero"] = all(bool((dx[b, vc, t] == 0).all()) for b, t in huge)
    res["huge_dshift_zero"] = all(bool((ds[b, t] == 0).all()) for b, t in huge)
    res["bad_out_is_nan"] = all(bool(torch.isnan(out[b, vc, t]).all()) for b, t in bad)
    res["bad_dx_zero_dshift_nan"] = all(bool((dx[b, vc, t] == 0).all()) and bool(torch.isnan(ds[b, t]).all()) for b, t in bad)
    res["plain_frames_exact"] = all(torch.equal(out[b, vc, t], ref[b, vc, t].float()) and torch.equal(dx[b, vc, t], rdx[b, vc, t].float())
                                    and torch.equal(ds[b, t], rds[b, t].float()) for b, t in plain)
    copied = [c for c in range(shape[1]) if c != vc]
    res["other_channels"] = torch.equal(out[:, copied], x[:, copied]) and torch.equal(dx[:, copied], dout[:, copied])
    res["nan_nowhere_else"] = int(torch.isnan(out).sum()) == len(bad) * shape[3] * shape[4]
    print(f"gaze extreme shifts {name} fill {fill}: {res}")
    assert all(res.values()), res


# -------------------------------------------------------------------------------------------------------- 4. reproducibility
def repeat_report():
    """Forward and backward twice on the same inputs: (tensors compared, tensors that differ).  Shared with the child process that
    runs the deterministic build."""
    tensors = differing = 0
    for name, (shape, vc, _) in CASES.items():
        g = torch.Generator().manual_seed(9)
        x, dout = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
        shift = torch.empty(shape[0], shape[2], 2).uniform_(-4.0, 4.0, generator=g)
        runs = []
        for _ in range(2):
            out = gpu_forward(x, shift, vc, 3.0)
            dx, ds = gpu_backward(x, shift, dout, vc, 3.0)
            runs.append((out, dx, ds, gpu_plane_mean(x, *CASES[name][2])))
        for a, b in zip(*runs):
            tensors += 1
            differing += 0 if torch.equal(a.view(torch.int32), b.view(torch.int32)) else 1
    return tensors, differing


def test_two_calls_give_equal_bits():
    tensors, differing = repeat_report()
    print(f"gaze kernels, product build: {differing} of {tensors} outputs differ between two calls")
    assert tensors == 4 * len(CASES) and differing == 0


def test_deterministic_build_two_calls_give_equal_bits():
    import sensorium_amd._lib as L
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    deterministic, lib, (tensors, differing) = deterministic_child("tests.test_gpu_gaze_shift:repeat_report")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    assert tensors == 4 * len(CASES) and differing == 0


# --------------------------------------------------------------------------------------------------------------- 5. plane mean
@pytest.mark.parametrize("name", list(CASES))
def test_plane_mean(name):
    """Constant planes come back bit for bit (n copies of v sum to v n exactly in float64, and v n / n is v), -0.0 included; random
    planes are within 2 u mean|v| of float64 (the float64 sum is exact to 2^-53 n, the conversion rounds once: u |mean| <= u mean|v|)."""
    shape, _, (c0, nc) = CASES[name]
    B, Cin, T, H, W = shape
    consts = [123.456, -0.0, 0.0, -1e-3, 3.0e38, 1e-42, 70.25]
    x = torch.randn(shape, generator=torch.Generator().manual_seed(3))
    want = torch.empty(B, T, nc)
    for b in range(B):
        for t in range(T):
            for k in range(nc):
                v = torch.tensor(consts[(b * T * nc + t * nc + k) % len(consts)], dtype=torch.float32)
                x[b, c0 + k, t] = v
                want[b, t, k] = v
    got = gpu_plane_mean(x, c0, nc)
    same = torch.equal(got.view(torch.int32), want.view(torch.int32))
    print(f"plane mean {name}: constant planes bit for bit: {same}")
    assert same, (got, want)
    xr = torch.randn(shape, generator=torch.Generator().manual_seed(4)) * 20 + 5
    got = gpu_plane_mean(xr, c0, nc)
    ref = gr.plane_mean(xr, range(c0, c0 + nc))
    scale = torch.stack([xr[:, c].double().abs().mean(dim=(2, 3)) for c in range(c0, c0 + nc)], dim=2)
    e = float(((got.double() - ref).abs() / scale).max()) / U
    print(f"plane mean {name}: random planes worst |mean - ref| / mean|v| = {e:.3f} u (bound 2)")
    assert bool(((got.double() - ref).abs() <= 2 * U * scale).all())

"""The drifting-Gabor kernels through the C-ABI (include/dwn.h dwn_gabor_forward / _backward) and ops.GaborFn
against the float64 checker tests/gabor_reference.py (itself held to autograd of an independent form and to central differences:
tests/test_gabor_reference_cpu.py).  u = 2^-24.  Every test prints what it measured before it asserts.

Bounds of the general cases, as multiples K of a derived floor:
  forward   floor = u |amplitude| (1 + 2 pi Q) + ulp(out) per element, Q = |sf| (|dxp| + |dyp|) + |tf| t + |phase| / (2 pi): the
            rounding of the terms of q, carried through the carrier's slope 2 pi |amplitude|, plus the roundings of the product
            and the final sum.
  backward  floor_k = u sum_i (1 + 2 pi Q_i) |dout_i d out_i / d p_k|: the same relative floor on every term of the sum.
The expression has about ten roundings; K is twice the worst ratio measured over these cases on an MI355X (K_FORWARD, K_BACKWARD
below, the measurement beside each).  Every output buffer sits between two guard bands that must come back untouched.
"""
import ctypes as C
import hashlib
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gabor_reference as gb  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402
from tests.test_gabor_reference_cpu import CLAMP_BACKGROUND, CLAMP_PARAMS, CLAMP_RANGE, CLAMP_SHAPE  # noqa: E402

U = 2.0 ** -24
GUARD, SENTINEL = 64, -7777.0
# twice the worst ratio to the floor measured on an MI355X over CASES x envelopes x ranges, the two misaligned runs, the clamp case
# and the 1000-cycle case: forward 2.241 ("frame", envelope none), backward 0.873 ("single", envelope none)
K_FORWARD = 4.5
K_BACKWARD = 1.75

# (B, Cin, T, H, W), video_channel, window, pad
CASES = {
    "ragged":    ((2, 5, 3, 5, 7), 0, None, 0.0),                  # no 16-byte planes: the scalar copy path
    "ragged_c2": ((2, 5, 3, 5, 7), 2, None, 0.0),
    "single":    ((1, 1, 1, 1, 1), 0, None, 0.0),                  # one pixel, no copied channel
    "window":    ((3, 5, 4, 8, 12), 2, (2, 3, 4, 6), 0.5),
    "frame":     ((2, 5, 16, 36, 64), 0, None, 0.0),               # the production frame: three chunks of partial sums
    "square":    ((1, 5, 16, 64, 64), 0, (14, 0, 36, 64), 0.0),    # the inference window: the 36-row screen in a 64 x 64 input
}
ENVELOPES = ("gaussian", "none")
RANGES = ((0.0, 255.0), None)
BACKGROUND = 127.5


def case_params(name, seed=0):
    """[B][8] fp32: a Gabor inside the window, one to eight pixels per sigma, 3 to 30 pixels per cycle, no clamping at
    background 127.5 (amplitude below 100)."""
    shape, _, window, _ = CASES[name]
    B, _, T, H, W = shape
    if name == "single":
        return torch.tensor([[0.25, -0.25, 1.5, 0.6, 0.2, 0.1, 0.8, 50.0]], dtype=torch.float32)
    y0, x0, wh, ww = window if window is not None else (0, 0, H, W)
    g = torch.Generator().manual_seed(100 + seed)
    r = torch.rand(B, 8, generator=g)
    lo = torch.tensor([y0 + 0.2 * wh, x0 + 0.2 * ww, 1.0, -3.0, 0.03, -0.3, -3.0, 20.0])
    hi = torch.tensor([y0 + 0.8 * wh, x0 + 0.8 * ww, max(min(wh, ww) / 4.0, 2.0), 3.0, 0.3, 0.3, 3.0, 95.0])
    return (lo + (hi - lo) * r).float()


def case_tensors(name, seed=0):
    shape = CASES[name][0]
    g = torch.Generator().manual_seed(7 + seed)
    x = torch.randn(shape, generator=g) * 3.0
    dout = torch.randn(shape, generator=g)
    return x, dout


def guarded(shape, misalign=0, dtype=torch.float32):
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD + misalign,), SENTINEL, dtype=dtype, device=dev())
    return flat, flat[GUARD + misalign:GUARD + misalign + n].view(shape)


def guards_ok(flat, shape, misalign=0):
    n = math.prod(shape)
    return bool((flat[:GUARD + misalign] == SENTINEL).all()) and bool((flat[GUARD + misalign + n:] == SENTINEL).all())


def gabor_args(shape, vc, envelope, background, video_range, window, pad):
    import sensorium_amd._lib as L
    a = L.GaborArgs()
    a.B, a.Cin, a.T, a.H, a.W = shape
    a.video_channel, a.envelope = vc, {"gaussian": L.GABOR_GAUSSIAN, "none": L.GABOR_NONE}[envelope]
    a.background, a.pad = background, pad
    if video_range is not None:
        a.clamp, a.lo, a.hi = 1, video_range[0], video_range[1]
    if window is not None:
        a.y0, a.x0, a.wh, a.ww = window
    return a


def gpu_forward(params, x, vc=0, envelope="gaussian", background=BACKGROUND, video_range=(0.0, 255.0), window=None, pad=0.0,
                misalign=0):
    import sensorium_amd._lib as L
    shape = tuple(x.shape)
    if misalign:
        _, xd = guarded(shape, misalign)
        xd.copy_(x)
    else:
        xd = x.to(dev()).contiguous()
    pd = params.to(dev()).contiguous()
    flat, out = guarded(shape, misalign)
    a = gabor_args(shape, vc, envelope, background, video_range, window, pad)
    a.x, a.params, a.out = xd.data_ptr(), pd.data_ptr(), out.data_ptr()
    L.check(L.lib.dwn_gabor_forward(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_gabor_forward")
    torch.cuda.synchronize()
    assert guards_ok(flat, shape, misalign), "dwn_gabor_forward wrote outside out"
    return out.cpu()


def gpu_backward(params, dout, vc=0, envelope="gaussian", background=BACKGROUND, video_range=(0.0, 255.0), window=None):
    import sensorium_amd._lib as L
    shape = tuple(dout.shape)
    pd, dd = params.to(dev()).contiguous(), dout.to(dev()).contiguous()
    a = gabor_args(shape, vc, envelope, background, video_range, window, 0.0)
    need = L.lib.dwn_gabor_workspace_bytes(C.byref(a))
    assert need > 0 and need % 8 == 0
    fws, ws = guarded((need // 8,), dtype=torch.float64)
    fdp, dp = guarded((shape[0], 8))
    a.params, a.dout, a.dparams, a.ws, a.ws_bytes = pd.data_ptr(), dd.data_ptr(), dp.data_ptr(), ws.data_ptr(), need
    L.check(L.lib.dwn_gabor_backward(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_gabor_backward")
    torch.cuda.synchronize()
    assert guards_ok(fws, (need // 8,)) and guards_ok(fdp, (shape[0], 8)), "dwn_gabor_backward wrote outside ws / dparams"
    return dp.cpu()


def bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------------------- 1. exact
@pytest.mark.parametrize("name", list(CASES))
def test_exact_cases_bit_for_bit(name):
    shape, vc, window, pad = CASES[name]
    B, Cin, T, H, W = shape
    x, dout = case_tensors(name)
    if Cin > 1:
        c = (vc + 1) % Cin
        x[0, c, 0].view(-1)[:5] = torch.tensor([-0.0, 1e-42, math.inf, -math.inf, math.nan])[:min(5, H * W)]
    inside = gb.window_mask(H, W, window)
    copied = [c for c in range(Cin) if c != vc]
    res = {}
    # sf = tf = phase = 0, no envelope: the carrier is cos(0) = 1 on every pixel
    p = case_params(name)
    p[:, 4:7] = 0.0
    out = gpu_forward(p, x, vc, "none", 100.0, None, window, pad)
    want = (torch.tensor(100.0) + p[:, 7]).view(B, 1, 1, 1).expand(B, T, H, W)
    res["flat"] = torch.equal(out[:, vc][..., inside], want[..., inside]) and bool((out[:, vc][..., ~inside] == pad).all())
    res["copied"] = torch.equal(bits(out[:, copied]), bits(x[:, copied]))
    # theta = 0, sf = tf = 1/4, integer cx: q - rint(q) only takes multiples of 1/4, whose cosines are 1, 0, -1 exactly
    p = case_params(name)
    p[:, 3], p[:, 4], p[:, 5], p[:, 6] = 0.0, 0.25, 0.25, 0.0
    p[:, 1] = torch.round(p[:, 1])
    out = gpu_forward(p, x, vc, "none", 100.0, None, window, pad)
    t = torch.arange(T).view(1, T, 1, 1)
    xx = torch.arange(W).view(1, 1, 1, W)
    k = (xx - p[:, 1].long().view(B, 1, 1, 1) - t).expand(B, T, H, W) % 4            # quarter cycles
    A = p[:, 7].view(B, 1, 1, 1)
    want = torch.where(k == 0, 100.0 + A, torch.where(k == 2, 100.0 - A, torch.tensor(100.0))).expand(B, T, H, W)
    res["quarter"] = torch.equal(out[:, vc][..., inside], want[..., inside])
    res["copied2"] = torch.equal(bits(out[:, copied]), bits(x[:, copied]))
    # background above the range: hi everywhere, and no gradient
    for env in ENVELOPES:
        p = case_params(name)
        p[:, 7] = p[:, 7].clamp(max=40.0)                                            # raw >= 300 - 40 > hi on every pixel
        out = gpu_forward(p, x, vc, env, 300.0, (0.0, 255.0), window, pad)
        dp = gpu_backward(p, dout, vc, env, 300.0, (0.0, 255.0), window)
        res["saturated_" + env] = bool((out[:, vc][..., inside] == 255.0).all()) and bool((dp == 0).all())
    print(f"gabor exact {name}: {res}")
    assert all(res.values()), res


# ----------------------------------------------------------------------------------------------------------------- 2. general
def measure(name, envelope, video_range, misalign=0):
    shape, vc, window, pad = CASES[name]
    B, Cin, T, H, W = shape
    p = case_params(name)
    x, dout = case_tensors(name)
    ref = gb.render(p, x, vc, envelope, BACKGROUND, video_range, window, pad)
    out = gpu_forward(p, x, vc, envelope, BACKGROUND, video_range, window, pad, misalign)
    copied = [c for c in range(Cin) if c != vc]
    assert torch.equal(bits(out[:, copied]), bits(x[:, copied]))
    inside = gb.window_mask(H, W, window)
    assert bool((out[:, vc][..., ~inside] == pad).all())
    floor = gb.forward_floor(p, ref[:, vc], T, H, W)
    err = (out[:, vc].double() - ref[:, vc]).abs()
    k_fwd = float((err / floor)[..., inside].max())
    rdp, mag = gb.dparams(dout, p, vc, envelope, BACKGROUND, video_range, window, with_floor=True)
    dp = gpu_backward(p, dout, vc, envelope, BACKGROUND, video_range, window)
    derr = (dp.double() - rdp).abs()
    assert bool((derr[mag == 0] == 0).all()), "a gradient whose every term is 0 must be exactly 0"
    k_bwd = float((derr / (U * mag).clamp_min(1e-300)).max())
    if envelope == "none":
        assert bool((bits(dp[:, 2]) == 0).all()), "envelope none: dsigma must be exactly 0"
    return k_fwd, k_bwd


@pytest.mark.parametrize("video_range", RANGES, ids=["clamp", "raw"])
@pytest.mark.parametrize("envelope", ENVELOPES)
@pytest.mark.parametrize("name,misalign", [(n, 0) for n in CASES] + [("window", 1), ("frame", 3)])
def test_general_cases_within_the_bounds(name, misalign, envelope, video_range):
    k_fwd, k_bwd = measure(name, envelope, video_range, misalign)
    print(f"gabor general {name} misalign {misalign} {envelope} range {video_range}: worst |out - ref| / floor = {k_fwd:.3f} "
          f"(bound {K_FORWARD}), worst |dparams - ref| / floor = {k_bwd:.3f} (bound {K_BACKWARD})")
    assert k_fwd <= K_FORWARD and k_bwd <= K_BACKWARD


def test_many_cycles_do_not_cost_accuracy():
    """A phase of 1000 cycles and 3000 frames of drift: without the reduction in cycles the error would be that of an argument
    of 2 pi * 4000 radians; with it the same multiple of the floor holds, Q being the number of cycles."""
    shape = (1, 1, 2, 8, 8)
    p = torch.tensor([[3.3, 4.1, 2.0, 0.4, 0.45, -1.7, 6283.0, 80.0]], dtype=torch.float32)
    x = torch.zeros(shape)
    out = gpu_forward(p, x, 0, "gaussian", BACKGROUND, None)
    ref = gb.render(p, x, 0, "gaussian", BACKGROUND, None)
    k = float(((out[:, 0].double() - ref[:, 0]).abs() / gb.forward_floor(p, ref[:, 0], 2, 8, 8)).max())
    print(f"gabor 1000 cycles of phase: worst |out - ref| / floor = {k:.3f} (bound {K_FORWARD})")
    assert k <= K_FORWARD


# ------------------------------------------------------------------------------------------------------------------- 3. clamp
def test_clamp_case_against_the_checkers_mask():
    """tests/test_gabor_reference_cpu.py proves that 0.72 % of this clip is clamped and no element lies within 1e-3 of an edge, so
    the kernel's mask must be the checker's on every element: the forward is the clamped reference within the forward bound, and
    dparams follows the checker's mask within the backward bound (one flipped element would show: |dout| ~ 1 of ~ 3 10^4 terms)."""
    H, W, T = CLAMP_SHAPE
    shape = (1, 5, T, H, W)
    p = torch.tensor([CLAMP_PARAMS], dtype=torch.float32)
    g = torch.Generator().manual_seed(3)
    x, dout = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    ref = gb.render(p, x, 0, "gaussian", CLAMP_BACKGROUND, CLAMP_RANGE)
    raw = gb.raw_video(p, T, H, W, "gaussian", CLAMP_BACKGROUND)
    out = gpu_forward(p, x, 0, "gaussian", CLAMP_BACKGROUND, CLAMP_RANGE)
    clamped = (raw < CLAMP_RANGE[0]) | (raw > CLAMP_RANGE[1])
    same_mask = torch.equal((out[:, 0] == CLAMP_RANGE[0]) | (out[:, 0] == CLAMP_RANGE[1]), clamped)
    k_fwd = float(((out[:, 0].double() - ref[:, 0]).abs() / gb.forward_floor(p, ref[:, 0], T, H, W)).max())
    rdp, mag = gb.dparams(dout, p, 0, "gaussian", CLAMP_BACKGROUND, CLAMP_RANGE, None, with_floor=True)
    free = gb.dparams(dout, p, 0, "gaussian", CLAMP_BACKGROUND, None, None)
    dp = gpu_backward(p, dout, 0, "gaussian", CLAMP_BACKGROUND, CLAMP_RANGE)
    k_bwd = float(((dp.double() - rdp).abs() / (U * mag)).max())
    k_free = float(((dp.double() - free).abs() / (U * mag)).max())
    print(f"gabor clamp case: {int(clamped.sum())} clamped elements, masks agree: {same_mask}; forward {k_fwd:.3f} (bound {K_FORWARD}), "
          f"dparams {k_bwd:.3f} (bound {K_BACKWARD}); against the unmasked gradient {k_free:.1f}")
    assert int(clamped.sum()) > 0 and same_mask
    assert k_fwd <= K_FORWARD and k_bwd <= K_BACKWARD
    assert k_free > 100 * K_BACKWARD, "the case does not tell a masked gradient from an unmasked one"


# -------------------------------------------------------------------------------------------------------------- 4. degenerate
@pytest.mark.parametrize("bad", [("theta", math.nan), ("sigma", 0.0), ("sigma", -1.0), ("cx", math.inf), ("amplitude", -math.inf)],
                         ids=["nan_theta", "sigma_0", "sigma_neg", "inf_cx", "inf_amplitude"])
@pytest.mark.parametrize("name", ["ragged", "window", "frame"])
def test_degenerate_clip_next_to_a_healthy_one(name, bad):
    shape, vc, window, pad = CASES[name]
    B, Cin, T, H, W = shape
    p = case_params(name)
    good = p.clone()
    p[1, gb.PARAM_NAMES.index(bad[0])] = bad[1]
    x, dout = case_tensors(name)
    out = gpu_forward(p, x, vc, "gaussian", BACKGROUND, (0.0, 255.0), window, pad)
    dp = gpu_backward(p, dout, vc, "gaussian", BACKGROUND, (0.0, 255.0), window)
    out_good = gpu_forward(good, x, vc, "gaussian", BACKGROUND, (0.0, 255.0), window, pad)
    dp_good = gpu_backward(good, dout, vc, "gaussian", BACKGROUND, (0.0, 255.0), window)
    inside = gb.window_mask(H, W, window)
    others = [b for b in range(B) if b != 1]
    copied = [c for c in range(Cin) if c != vc]
    res = dict(nan_frame=bool(torch.isnan(out[1, vc][..., inside]).all()), pad_kept=bool((out[1, vc][..., ~inside] == pad).all()),
               nan_dparams=bool(torch.isnan(dp[1]).all()),
               others_out=torch.equal(bits(out[others]), bits(out_good[others])), others_dp=torch.equal(bits(dp[others]), bits(dp_good[others])),
               copied=torch.equal(bits(out[:, copied]), bits(x[:, copied])),
               nan_nowhere_else=int(torch.isnan(out).sum()) == T * int(inside.sum()))
    print(f"gabor degenerate {name} {bad}: {res}")
    assert all(res.values()), res
    if bad[0] == "sigma":          # sigma is not used without the envelope
        dp = gpu_backward(p, dout, vc, "none", BACKGROUND, (0.0, 255.0), window)
        assert bool(torch.isfinite(dp).all()) and bool((dp[:, 2] == 0).all())


# -------------------------------------------------------------------------------------------------------- 5. reproducibility
DIGEST_CASES = [(n, e) for n in CASES for e in ENVELOPES]


def gabor_digest():
    """(tensors, sha256) of out and dparams over the fixed cases; shared with the child process on the deterministic build."""
    h = hashlib.sha256()
    tensors = 0
    for name, env in DIGEST_CASES:
        shape, vc, window, pad = CASES[name]
        p = case_params(name, 1)
        x, dout = case_tensors(name, 1)
        for t in (gpu_forward(p, x, vc, env, BACKGROUND, (0.0, 255.0), window, pad),
                  gpu_backward(p, dout, vc, env, BACKGROUND, (0.0, 255.0), window)):
            h.update(t.numpy().tobytes())
            tensors += 1
    return tensors, h.hexdigest()


def test_two_launches_give_equal_bits():
    a, b = gabor_digest(), gabor_digest()
    print(f"gabor kernels, two passes over {a[0]} outputs: digests {a[1][:16]} / {b[1][:16]}")
    assert a[0] == 2 * len(DIGEST_CASES) and a == b


# ------------------------------------------------------------------------------------------------------------------ 6. GaborFn
@pytest.mark.parametrize("name", ["ragged_c2", "window", "square"])
def test_gabor_fn_matches_the_c_abi_and_routes_the_template_gradient(name):
    from sensorium_amd import ops
    shape, vc, window, pad = CASES[name]
    p = case_params(name)
    x, dout = case_tensors(name)
    pd, xd = p.to(dev()).requires_grad_(True), x.to(dev()).requires_grad_(True)
    out = ops.GaborFn.apply(pd, xd, vc, "gaussian", BACKGROUND, (0.0, 255.0), window, pad)
    out.backward(dout.to(dev()))
    torch.cuda.synchronize()
    assert torch.equal(bits(out.detach().cpu()), bits(gpu_forward(p, x, vc, "gaussian", BACKGROUND, (0.0, 255.0), window, pad)))
    assert torch.equal(bits(pd.grad.cpu()), bits(gpu_backward(p, dout, vc, "gaussian", BACKGROUND, (0.0, 255.0), window)))
    want = dout.clone()
    want[:, vc] = 0
    assert torch.equal(xd.grad.cpu(), want)
    # only the template requires a gradient: no reduction is launched, params gets none
    xd2 = x.to(dev()).requires_grad_(True)
    ops.GaborFn.apply(p.to(dev()), xd2, vc, "none", BACKGROUND, None, window, pad).backward(dout.to(dev()))
    assert torch.equal(xd2.grad.cpu(), want)


# ------------------------------------------------------------------------------------------------------------------ 7. capture
def test_forward_and_backward_in_a_captured_graph():
    """One torch.cuda.graph around both entries; replayed after `params` changed in place it returns the new values' result bit for
    bit: no host read-back, no parameter baked into the launch."""
    import sensorium_amd._lib as L
    name = "window"
    shape, vc, window, pad = CASES[name]
    first, second = case_params(name, 2), case_params(name, 3)
    x, dout = case_tensors(name)
    xd, dd, pd = x.to(dev()), dout.to(dev()), first.to(dev())
    out, dp = torch.empty_like(xd), torch.empty(shape[0], 8, device=dev())
    a = gabor_args(shape, vc, "gaussian", BACKGROUND, (0.0, 255.0), window, pad)
    need = L.lib.dwn_gabor_workspace_bytes(C.byref(a))
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev())
    a.x, a.params, a.out, a.dout, a.dparams, a.ws, a.ws_bytes = (xd.data_ptr(), pd.data_ptr(), out.data_ptr(), dd.data_ptr(),
                                                                 dp.data_ptr(), ws.data_ptr(), need)

    def both():
        s = torch.cuda.current_stream().cuda_stream
        L.check(L.lib.dwn_gabor_forward(C.byref(a), 0, s), "dwn_gabor_forward")
        L.check(L.lib.dwn_gabor_backward(C.byref(a), 0, s), "dwn_gabor_backward")

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    res = {}
    for tag, p in (("first", first), ("second", second)):
        pd.copy_(p.to(dev()))
        out.fill_(SENTINEL)
        dp.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        res[tag] = (torch.equal(bits(out.cpu()), bits(gpu_forward(p, x, vc, "gaussian", BACKGROUND, (0.0, 255.0), window, pad)))
                    and torch.equal(bits(dp.cpu()), bits(gpu_backward(p, dout, vc, "gaussian", BACKGROUND, (0.0, 255.0), window))))
    print(f"gabor captured graph: replays equal the direct calls: {res}")
    assert all(res.values()), res

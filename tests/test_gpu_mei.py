"""The regularised-MEI kernels (csrc/dwn_mei.hip) against the float64 checker of tests/mei_reference.py:
dwn_blur3d within its derived per-element bound and bit for bit on the exact cases, symmetric, NaN-local, reproducible and
capturable with a taps table that changes between replays; dwn_clip_moments within the a-priori float64 summation bounds of the
longdouble values; dwn_mei_update within one fp32 ulp and bit for bit on the degenerate clips.  Every test prints what it
measured before it asserts."""
import functools
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mei_reference as mr  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

SENTINEL = -777.25

# shape = (B, Cin_src, T, H, W)
BLUR_CASES = [
    dict(name="ragged", shape=(2, 5, 3, 5, 7), radii=(1, 2, 3), window=None, c_src=0, cin_dst=1, c_dst=0),
    dict(name="one-element", shape=(1, 1, 1, 1, 1), radii=(1, 2, 3), window=None, c_src=0, cin_dst=1, c_dst=0),
    dict(name="one-element-r0", shape=(1, 1, 1, 1, 1), radii=(0, 0, 0), window=None, c_src=0, cin_dst=1, c_dst=0),
    dict(name="radius>extent", shape=(1, 2, 2, 3, 5), radii=(4, 16, 2), window=None, c_src=1, cin_dst=1, c_dst=0),
    dict(name="windowed", shape=(3, 5, 4, 8, 12), radii=(1, 2, 3), window=(1, 2, 5, 7), c_src=2, cin_dst=5, c_dst=3),
    dict(name="channel0->5", shape=(2, 5, 3, 5, 8), radii=(1, 1, 2), window=None, c_src=0, cin_dst=5, c_dst=0),
    dict(name="tiles-2x2", shape=(1, 1, 2, 20, 70), radii=(1, 3, 5), window=None, c_src=0, cin_dst=1, c_dst=0),
    dict(name="tiles-window", shape=(1, 2, 2, 40, 72), radii=(0, 16, 16), window=(3, 4, 33, 66), c_src=1, cin_dst=2, c_dst=1),
    dict(name="production-64x64", shape=(1, 5, 16, 64, 64), radii=(2, 6, 6), window=None, c_src=0, cin_dst=1, c_dst=0),
    dict(name="production-36x64", shape=(2, 5, 32, 36, 64), radii=(2, 6, 6), window=None, c_src=0, cin_dst=1, c_dst=0),
]
BLUR_IDS = [c["name"] for c in BLUR_CASES]


def random_taps(rng, radii, symmetric=False):
    out = []
    for r in radii:
        k = torch.from_numpy(rng.normal(size=2 * r + 1) / np.sqrt(2 * r + 1))
        out.append(((k + k.flip(0)) / 2 if symmetric else k).float())
    return out


@functools.lru_cache(maxsize=None)
def blur_case_data(name, symmetric=False):
    """(source, taps, checker result, bound) of a case: computed once on the CPU and never changed."""
    case = next(c for c in BLUR_CASES if c["name"] == name)
    rng = np.random.default_rng(sum(map(ord, name)) + (7 if symmetric else 0))
    src = torch.from_numpy(rng.normal(size=case["shape"]) * 50 + 20).float()
    taps = random_taps(rng, case["radii"], symmetric)
    ref = mr.blur3d_ref(src[:, case["c_src"]], taps, case["window"])
    bound = mr.blur3d_bound(src[:, case["c_src"]], taps, case["window"])
    return src, taps, ref, bound


def device_blur(src, taps, *, c_src=0, cin_dst=1, c_dst=0, window=None):
    """dwn_blur3d on the device into a sentinel-filled destination; returns the whole destination on the CPU."""
    from sensorium_amd import ops
    table, radii = ops.blur_taps_table(taps, dev())
    x = src if src.is_cuda else src.to(dev())
    B, _, T, H, W = x.shape
    out = torch.full((B, cin_dst, T, H, W), SENTINEL, dtype=torch.float32, device=dev())
    ops.blur3d(x, table, radii, c_src=c_src, out=out, c_dst=c_dst, window=window)
    torch.cuda.synchronize()
    return out.cpu()


def run_case(case, symmetric=False):
    src, taps, _, _ = blur_case_data(case["name"], symmetric)
    return device_blur(src, taps, c_src=case["c_src"], cin_dst=case["cin_dst"], c_dst=case["c_dst"], window=case["window"])


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", BLUR_CASES, ids=BLUR_IDS)
def test_blur_against_checker(case):
    src, taps, ref, bound = blur_case_data(case["name"])
    out = run_case(case)
    got = out[:, case["c_dst"]].double()
    ratio = ((got - ref).abs() / bound.clamp_min(1e-300))[bound > 0]
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"blur {case['name']} radii {case['radii']}: worst |err| / bound {worst:.3f}, max |err| {float((got - ref).abs().max()):.3e}")
    assert bool(((got - ref).abs() <= bound).all())
    y0, x0, wh, ww = mr.resolve_window(case["shape"][3], case["shape"][4], case["window"])
    outside = torch.ones_like(got, dtype=torch.bool)
    outside[:, :, y0:y0 + wh, x0:x0 + ww] = False
    assert bool((bits(out[:, case["c_dst"]])[outside] == 0).all()), "outside the window the destination channel is +0"
    others = [c for c in range(case["cin_dst"]) if c != case["c_dst"]]
    assert bool((out[:, others] == SENTINEL).all()), "the other destination channels keep the sentinel"
    assert torch.equal(bits(run_case(case)), bits(out)), "two launches differ"


def test_blur_identity_copies_the_window_bit_for_bit():
    rng = np.random.default_rng(11)
    src = torch.from_numpy(rng.normal(size=(2, 5, 3, 8, 12)) * 1e3).float()
    src[0, 2, 1, 3, 4] = -0.0
    one = [torch.ones(1)] * 3
    for window in (None, (1, 2, 5, 7)):
        out = device_blur(src, one, c_src=2, window=window)[:, 0]
        want = torch.zeros_like(out)
        y0, x0, wh, ww = mr.resolve_window(8, 12, window)
        want[:, :, y0:y0 + wh, x0:x0 + ww] = src[:, 2, :, y0:y0 + wh, x0:x0 + ww]
        assert torch.equal(bits(out), bits(want))


@pytest.mark.parametrize("shape,window", [((2, 1, 5, 9, 13), None), ((1, 1, 3, 20, 70), (2, 1, 17, 68))])
def test_blur_quarter_taps_on_integers_is_exact(shape, window):
    """(1/4, 1/2, 1/4) on every axis over integers in [0, 255]: every partial sum is a multiple of 1/64 below 2^8."""
    rng = np.random.default_rng(12)
    src = torch.from_numpy(rng.integers(0, 256, size=shape)).float()
    taps = [torch.tensor([0.25, 0.5, 0.25])] * 3
    out = device_blur(src, taps, window=window)[:, 0]
    assert torch.equal(out.double(), mr.blur3d_ref(src[:, 0], taps, window))


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("side", [0, 2])
def test_blur_one_sided_delta_shifts(axis, side):
    """A delta on entry 0 (side 0) reads the element one step BEFORE, on entry 2 one step AFTER, zeros shifted in."""
    rng = np.random.default_rng(13)
    src = torch.from_numpy(rng.integers(0, 256, size=(2, 1, 4, 6, 9))).float()
    taps = [torch.tensor([0.0, 1.0, 0.0])] * 3
    delta = torch.zeros(3)
    delta[side] = 1.0
    taps[axis] = delta
    out = device_blur(src, taps)[:, 0]
    want = torch.zeros_like(out)
    dim = axis + 1
    L = src.shape[dim + 1]
    if side == 0:
        want.narrow(dim, 1, L - 1).copy_(src[:, 0].narrow(dim, 0, L - 1))
    else:
        want.narrow(dim, 0, L - 1).copy_(src[:, 0].narrow(dim, 1, L - 1))
    assert torch.equal(bits(out), bits(want))


def test_blur_symmetric_taps_give_a_symmetric_operator():
    case = next(c for c in BLUR_CASES if c["name"] == "windowed")
    rng = np.random.default_rng(14)
    a = torch.from_numpy(rng.normal(size=case["shape"])).float()
    b = torch.from_numpy(rng.normal(size=case["shape"])).float()
    taps = random_taps(rng, case["radii"], symmetric=True)
    y0, x0, wh, ww = case["window"]
    crop = (slice(None), slice(None), slice(y0, y0 + wh), slice(x0, x0 + ww))
    Ka = device_blur(a, taps, window=case["window"])[:, 0].double()
    Kb = device_blur(b, taps, window=case["window"])[:, 0].double()
    a0, b0 = a[:, 0].double(), b[:, 0].double()
    lhs, rhs = float((a0[crop] * Kb[crop]).sum()), float((Ka[crop] * b0[crop]).sum())
    slack = float((a0.abs() * mr.blur3d_bound(b[:, 0], taps, case["window"])).sum()
                  + (b0.abs() * mr.blur3d_bound(a[:, 0], taps, case["window"])).sum())
    print(f"<a, K b> = {lhs:.9e}, <K a, b> = {rhs:.9e}, difference {abs(lhs - rhs):.3e}, allowed {slack:.3e}")
    assert abs(lhs - rhs) <= slack


def test_blur_nan_reaches_exactly_its_tap_box():
    shape, radii, at = (2, 1, 6, 20, 70), (1, 2, 3), (1, 0, 3, 15, 63)
    rng = np.random.default_rng(15)
    src = torch.from_numpy(rng.normal(size=shape)).float()
    src[at] = float("nan")
    out = device_blur(src, random_taps(rng, radii))[:, 0]
    want = torch.zeros_like(out, dtype=torch.bool)
    want[1, 2:5, 13:18, 60:67] = True
    assert torch.equal(torch.isnan(out), want)


def test_blur_offset_view_takes_the_slow_path_to_the_same_values():
    from sensorium_amd import ops
    case = next(c for c in BLUR_CASES if c["name"] == "channel0->5")
    src, taps, ref, bound = blur_case_data(case["name"])
    table, radii = ops.blur_taps_table(taps, dev())
    n = src.numel()
    flat_in = torch.empty(n + 1, dtype=torch.float32, device=dev())
    flat_out = torch.full((n + 1,), SENTINEL, dtype=torch.float32, device=dev())
    x = flat_in[1:].view(src.shape)
    x.copy_(src)
    out = flat_out[1:].view(src.shape)
    assert x.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4 and x.is_contiguous()
    ops.blur3d(x, table, radii, c_src=0, out=out, c_dst=0)
    torch.cuda.synchronize()
    aligned = run_case(case)
    assert torch.equal(bits(out.cpu()), bits(aligned)) and float(flat_out[0]) == SENTINEL
    assert bool(((out[:, 0].cpu().double() - ref).abs() <= bound).all())


def test_captured_blur_follows_the_taps_table():
    from sensorium_amd import ops
    case = next(c for c in BLUR_CASES if c["name"] == "ragged")
    src, taps, _, _ = blur_case_data(case["name"])
    other = random_taps(np.random.default_rng(16), case["radii"])
    table, radii = ops.blur_taps_table(taps, dev())
    table2, _ = ops.blur_taps_table(other, dev())
    x = src.to(dev())
    out = torch.zeros(2, 1, 3, 5, 7, device=dev())
    ws = torch.empty(out.numel(), device=dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.blur3d(x, table, radii, out=out, ws=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.blur3d(x, table, radii, out=out, ws=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(device_blur(src, taps)))
    table.copy_(table2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out.cpu()), bits(device_blur(src, other)))
    assert not torch.equal(out.cpu(), device_blur(src, taps))


def test_blur_backward_is_the_reversed_kernel():
    from sensorium_amd import ops
    rng = np.random.default_rng(17)
    shape, radii, window = (2, 3, 3, 6, 9), (1, 2, 2), (1, 1, 4, 7)
    taps = random_taps(rng, radii)
    table, _ = ops.blur_taps_table(taps, dev())
    x = torch.from_numpy(rng.normal(size=shape)).float().to(dev()).requires_grad_(True)
    w = torch.from_numpy(rng.normal(size=(2, 1, 3, 6, 9))).float()
    y = ops.GaussianBlur3dFn.apply(x, table, radii, 1, window)
    (y * w.to(dev())).sum().backward()
    xd = x.detach().cpu()[:, 1].double().requires_grad_(True)
    y0, x0, wh, ww = window
    crop = xd[:, None, :, y0:y0 + wh, x0:x0 + ww]
    k = torch.einsum("i,j,k->ijk", *[t.double() for t in taps])[None, None]
    ref = torch.nn.functional.conv3d(crop, k, padding=radii)
    (ref * w[:, :, :, y0:y0 + wh, x0:x0 + ww].double()).sum().backward()
    got = x.grad.cpu()
    err = float((got[:, 1].double() - xd.grad).abs().max())
    print(f"blur backward: max abs err {err:.3e} (gradient scale {float(xd.grad.abs().max()):.3f})")
    assert err <= 1e-5 * float(xd.grad.abs().max()) and not bool(got[:, [0, 2]].any())


# ---------------------------------------------------------------------------------------------------------------------------
# moments
# ---------------------------------------------------------------------------------------------------------------------------
MOMENT_CASES = [
    dict(name="ragged", shape=(2, 5, 3, 5, 7), c=0, window=None),
    dict(name="one-element", shape=(1, 1, 1, 1, 1), c=0, window=None),
    dict(name="windowed", shape=(3, 5, 4, 8, 12), c=2, window=(1, 2, 5, 7)),
    dict(name="two-chunks-window", shape=(2, 1, 4, 40, 70), c=0, window=(3, 5, 32, 61)),
    dict(name="production-64x64", shape=(1, 5, 16, 64, 64), c=0, window=None),
    dict(name="production-36x64", shape=(2, 5, 32, 36, 64), c=0, window=None),
    dict(name="padded-screen", shape=(2, 1, 16, 64, 64), c=0, window=(14, 0, 36, 64)),
]


def device_moments(x, c=0, window=None):
    from sensorium_amd import ops
    stat = ops.clip_moments(x if x.is_cuda else x.to(dev()), c=c, window=window)
    torch.cuda.synchronize()
    return stat.cpu()


def longdouble_moments(x, window):
    y0, x0, wh, ww = mr.resolve_window(x.shape[2], x.shape[3], window)
    v = x.numpy()[:, :, y0:y0 + wh, x0:x0 + ww].reshape(x.shape[0], -1).astype(np.longdouble)
    n = v.shape[1]
    mean = v.sum(1) / n
    return n, mean, ((v - mean[:, None]) ** 2).sum(1), (v * v).sum(1), np.abs(v).max(1)


def check_moments(stat, x, window, what):
    n, mean, m2, s2, amax = longdouble_moments(x, window)
    got = stat.numpy().astype(np.longdouble)
    e_mean = np.abs(got[:, 1] - mean) / (n * 2.0 ** -53 * amax)
    e_m2 = np.abs(got[:, 2] - m2) / np.maximum(n * 2.0 ** -52 * m2, np.finfo(np.longdouble).tiny)
    e_s2 = np.abs(got[:, 3] - s2) / (n * 2.0 ** -52 * s2)
    print(f"moments {what}: n {n}, worst error / bound: mean {float(e_mean.max()):.3f}, M2 {float(e_m2.max()):.3f}, S2 {float(e_s2.max()):.3f}")
    assert np.all(got[:, 0] == n)
    assert np.all(e_mean <= 1) and np.all(e_m2 <= 1) and np.all(e_s2 <= 1)


@pytest.mark.parametrize("case", MOMENT_CASES, ids=[c["name"] for c in MOMENT_CASES])
def test_moments_against_longdouble(case):
    rng = np.random.default_rng(sum(map(ord, case["name"])))
    x = torch.from_numpy(rng.normal(size=case["shape"]) * 40 + 110).float()
    stat = device_moments(x, case["c"], case["window"])
    check_moments(stat, x[:, case["c"]], case["window"], case["name"])
    assert torch.equal(stat, device_moments(x, case["c"], case["window"])), "two launches differ"


def test_moments_large_offset_constant_and_non_finite_clips():
    T, H, W = 4, 40, 70
    k = torch.arange(T * H * W, dtype=torch.float64).reshape(T, H, W)
    rng = np.random.default_rng(21)
    x = torch.zeros(5, 1, T, H, W)
    x[0, 0] = (1e6 + (k % 4099) / 16.0).float()            # raw-sum formulas lose M2 here
    x[1, 0] = 0.1                                           # constant: mean bit for bit, M2 == 0
    x[2, 0] = torch.from_numpy(rng.normal(size=(T, H, W))).float()
    x[3, 0] = x[2, 0]
    x[3, 0, 1, 5, 9] = float("inf")
    x[4, 0] = x[2, 0]
    x[4, 0, 3, 39, 69] = float("nan")
    assert float(x[0, 0].double().sub(1e6).mul(16).frac().abs().max()) == 0
    for window in (None, (3, 5, 32, 61)):
        stat = device_moments(x, 0, window)
        check_moments(stat[:3], x[:3, 0], window, f"offset/constant/normal window {window}")
        assert float(stat[1, 1]) == float(np.float32(0.1)) and float(stat[1, 2]) == 0.0
        inside = window is None
        if inside:
            assert not bool(torch.isfinite(stat[3, 1:]).any()) and bool(torch.isnan(stat[4, 1:]).all())
        else:                                               # (the NaN of clip 4 is outside this window, the Inf of clip 3 is not)
            assert not bool(torch.isfinite(stat[3, 1:]).any()) and torch.equal(stat[4], stat[2])
        clean = device_moments(x[2:3], 0, window)
        assert torch.equal(stat[2], clean[0]), "a non-finite clip changed another clip's statistics"


def test_moments_offset_view_gives_the_bits_of_the_aligned_tensor():
    case = MOMENT_CASES[4]
    rng = np.random.default_rng(22)
    x = torch.from_numpy(rng.normal(size=case["shape"]) * 40 + 110).float()
    flat = torch.empty(x.numel() + 1, dtype=torch.float32, device=dev())
    view = flat[1:].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == 4
    assert torch.equal(device_moments(view), device_moments(x))


# ---------------------------------------------------------------------------------------------------------------------------
# update
# ---------------------------------------------------------------------------------------------------------------------------
UPDATE_CASES = [
    dict(name="fixed-mean", shape=(2, 5, 3, 5, 7), window=None, lr=3.0, mean=127.5, contrast=25.0, mode="fixed", lo=0.0, hi=255.0),
    dict(name="max-window", shape=(3, 5, 4, 8, 12), window=(1, 2, 5, 7), lr=8.0, mean=None, contrast=20.0, mode="max", lo=0.0, hi=255.0),
    dict(name="mean-only", shape=(2, 1, 4, 40, 70), window=(3, 5, 32, 61), lr=1.5, mean=100.0, contrast=None, mode="max", lo=0.0, hi=255.0),
    dict(name="production", shape=(2, 5, 16, 64, 64), window=None, lr=2.0, mean=127.5, contrast=30.0, mode="max", lo=0.0, hi=255.0),
]


def update_inputs(case):
    """(x, g) of a case on the CPU: x as the case's shape, g as a compact [B, 1, T, H, W] gradient."""
    rng = np.random.default_rng(sum(map(ord, case["name"])) + 100)
    B, _, T, H, W = case["shape"]
    x = torch.from_numpy(rng.normal(size=case["shape"]) * 35 + 125).float()
    g = torch.from_numpy(rng.normal(size=(B, 1, T, H, W)) * 1e-3).float()
    return x, g


def near_edge(v, lo, hi):
    """Elements of the unclamped checker result within one fp32 ulp of a clamp edge."""
    d = v.double()
    u = mr.ulp32(torch.maximum(d.abs(), torch.full_like(d, max(abs(lo), abs(hi)))))
    return ((d - lo).abs() <= u) | ((d - hi).abs() <= u)


def ulps(got, want):
    return (got.double() - want.double()).abs() / mr.ulp32(want.double())


@pytest.mark.parametrize("case", UPDATE_CASES, ids=[c["name"] for c in UPDATE_CASES])
def test_update_modes_within_one_ulp(case):
    from sensorium_amd import ops
    x, g = update_inputs(case)
    win = case["window"]
    lr = torch.tensor([case["lr"]], dtype=torch.float32, device=dev())
    # STEP
    xd, gd = x.to(dev()), g.to(dev())
    ops.mei_update(xd, ops.clip_moments(gd, window=win), "step", g=gd, lr=lr, window=win)
    torch.cuda.synchronize()
    want = mr.step_ref(x[:, 0], g[:, 0], mr.moments_ref(g[:, 0], win), case["lr"], win)
    e_step = float(ulps(xd[:, 0].cpu(), want).max())
    assert torch.equal(bits(xd[:, 1:].cpu()), bits(x[:, 1:])), "the other channels changed"
    # PROJECT, from the checker's stepped clip
    stepped = x.clone()
    stepped[:, 0] = want
    pd = stepped.to(dev())
    ops.mei_update(pd, ops.clip_moments(pd, window=win), "project", window=win, mean=case["mean"], contrast=case["contrast"],
                   contrast_mode=case["mode"], video_range=(case["lo"], case["hi"]))
    torch.cuda.synchronize()
    stat = mr.moments_ref(want, win)
    raw = mr.project_ref(want, stat, case["mean"], case["contrast"], case["mode"], case["lo"], case["hi"], win, clamp=False)
    ref = mr.project_ref(want, stat, case["mean"], case["contrast"], case["mode"], case["lo"], case["hi"], win)
    skip = near_edge(raw, case["lo"], case["hi"])
    e_proj = float(ulps(pd[:, 0].cpu(), ref)[~skip].max())
    print(f"update {case['name']}: step {e_step:.2f} ulp, project {e_proj:.2f} ulp, {float(skip.float().mean()):.4%} near an edge")
    assert float(skip.float().mean()) < 0.01
    assert e_step <= 1.0 and e_proj <= 1.0
    y0, x0, wh, ww = mr.resolve_window(x.shape[3], x.shape[4], win)
    outside = torch.ones_like(want, dtype=torch.bool)
    outside[:, :, y0:y0 + wh, x0:x0 + ww] = False
    assert torch.equal(bits(xd[:, 0].cpu())[outside], bits(x[:, 0])[outside])
    assert torch.equal(bits(pd[:, 0].cpu())[outside], bits(stepped[:, 0])[outside])
    assert torch.equal(bits(pd[:, 1:].cpu()), bits(x[:, 1:]))


@pytest.mark.parametrize("window", [None, (1, 2, 5, 7)])
def test_update_degenerate_clips_bit_for_bit(window):
    from sensorium_amd import ops
    rng = np.random.default_rng(31)
    shape = (4, 2, 3, 8, 12)
    x = torch.from_numpy(rng.normal(size=shape) * 60 + 125).float()      # some elements beyond [0, 255]
    x[2, 0] = 77.0                                                        # sd == 0
    x[3, 0, 2, 5, 6] = float("nan")
    y0, x0, wh, ww = mr.resolve_window(8, 12, window)
    crop = (slice(None), slice(None), slice(y0, y0 + wh), slice(x0, x0 + ww))
    inside = torch.zeros(shape[0], *shape[2:], dtype=torch.bool)
    inside[crop] = True

    def project(**kw):
        d = x.to(dev())
        ops.mei_update(d, ops.clip_moments(d, window=window), "project", window=window, video_range=(0.0, 255.0), **kw)
        torch.cuda.synchronize()
        return d.cpu()

    def expect(per_clip):
        want = x.clone()
        for b, fn in enumerate(per_clip):
            v = want[b, 0]
            v[inside[b]] = fn(v[inside[b]])
        return want
    nan = lambda v: torch.full_like(v, float("nan"))                     # noqa: E731
    clamp = lambda v: v.clamp(0.0, 255.0)                                # noqa: E731
    # a projection that does not bind only clamps: the unclamped bits are kept
    for kw in (dict(), dict(contrast=1e4, contrast_mode="max")):
        got = project(**kw)
        assert torch.equal(bits(got)[~torch.isnan(got)], bits(expect([clamp, clamp, clamp, nan]))[~torch.isnan(got)])
        assert torch.equal(torch.isnan(got), torch.isnan(expect([clamp, clamp, clamp, nan])))
    # sd == 0: FIXED collapses the clip onto m, MAX keeps it (s = 1)
    got = project(contrast=10.0, contrast_mode="fixed")
    assert bool((got[2, 0][inside[2]] == 77.0).all())
    got = project(contrast=10.0, contrast_mode="fixed", mean=90.0)
    assert bool((got[2, 0][inside[2]] == 90.0).all())
    got = project(contrast=10.0, contrast_mode="max")
    assert torch.equal(bits(got[2]), bits(x[2]))
    got = project(contrast=10.0, contrast_mode="max", mean=90.0)
    assert bool((got[2, 0][inside[2]] == 90.0).all()) and torch.equal(bits(got[2, 0][~inside[2]]), bits(x[2, 0][~inside[2]]))
    assert bool(torch.isnan(got[3, 0][inside[3]]).all()) and torch.equal(bits(got[3, 0][~inside[3]]), bits(x[3, 0][~inside[3]]))
    assert torch.equal(bits(got[:, 1]), bits(x[:, 1]))
    # STEP with S2 == 0 is a no-op; a NaN gradient clip becomes NaN inside its window; the rest moves
    g = torch.from_numpy(rng.normal(size=(4, 1, 3, 8, 12))).float()
    g[1] = 0.0
    g[2, 0, 0, y0, x0] = float("nan")
    d, gd = x.to(dev()), g.to(dev())
    ops.mei_update(d, ops.clip_moments(gd, window=window), "step", g=gd, window=window,
                   lr=torch.tensor([4.0], device=dev()))
    torch.cuda.synchronize()
    got = d.cpu()
    assert torch.equal(bits(got[1]), bits(x[1]))
    assert bool(torch.isnan(got[2, 0][inside[2]]).all()) and torch.equal(bits(got[2, 0][~inside[2]]), bits(x[2, 0][~inside[2]]))
    assert not torch.equal(got[0, 0][inside[0]], x[0, 0][inside[0]]) and torch.equal(bits(got[0, 0][~inside[0]]), bits(x[0, 0][~inside[0]]))
    assert torch.equal(bits(got[:, 1]), bits(x[:, 1]))


# ---------------------------------------------------------------------------------------------------------------------------
# one digest over fixed cases: tests/test_gpu_mei_det.py compares the two builds through it
# ---------------------------------------------------------------------------------------------------------------------------
DIGEST_CASES = ("ragged", "radius>extent", "windowed", "tiles-window", "production-64x64")


def mei_digest():
    """(number of tensors, sha256) of the blur, the moments and both updates over DIGEST_CASES."""
    from sensorium_amd import ops
    h, count = hashlib.sha256(), 0
    for name in DIGEST_CASES:
        case = next(c for c in BLUR_CASES if c["name"] == name)
        out = run_case(case)
        src, _, _, _ = blur_case_data(name)
        x = src.to(dev())
        win = case["window"]
        stat_g = ops.clip_moments(out.to(dev()), c=case["c_dst"], window=win)
        lr = torch.tensor([2.0], dtype=torch.float32, device=dev())
        ops.mei_update(x, stat_g, "step", c=case["c_src"], g=out.to(dev()), c_g=case["c_dst"], lr=lr, window=win)
        stat_x = ops.clip_moments(x, c=case["c_src"], window=win)
        ops.mei_update(x, stat_x, "project", c=case["c_src"], window=win, mean=20.0, contrast=30.0, contrast_mode="fixed",
                       video_range=(-200.0, 200.0))
        torch.cuda.synchronize()
        for t in (out, stat_g.cpu(), stat_x.cpu(), x.cpu()):
            h.update(t.contiguous().numpy().tobytes())
            count += 1
    return count, h.hexdigest()

"""The float64 checker of the regularised-MEI kernels (tests/mei_reference.py) held to independent definitions: the blur to
float64 conv3d with zero padding on the window-cropped input, the moments to numpy in longdouble, the projection to a direct
restatement per clip; and the rules of ops.gaussian_taps.  Also the inputs of the update tests of tests/test_gpu_mei.py: under
1 % of their elements sit within one ulp of a clamp edge.  No GPU here."""
import math

import numpy as np
import pytest
import torch

from tests import mei_reference as mr


def _taps(rng, radii, symmetric):
    out = []
    for r in radii:
        k = torch.from_numpy(rng.normal(size=2 * r + 1))
        out.append(((k + k.flip(0)) / 2 if symmetric else k).float())
    return out


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("radii", [(1, 2, 3), (0, 2, 3), (1, 0, 3), (1, 2, 0), (0, 0, 0), (4, 16, 2)])
@pytest.mark.parametrize("window", [None, (1, 2, 5, 7)])
def test_blur_against_conv3d(symmetric, radii, window):
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.normal(size=(2, 4, 8, 12))).float()
    taps = _taps(rng, radii, symmetric)
    got = mr.blur3d_ref(x, taps, window)
    y0, x0, wh, ww = mr.resolve_window(8, 12, window)
    crop = x[:, None, :, y0:y0 + wh, x0:x0 + ww].double()
    w = torch.einsum("i,j,k->ijk", *[k.double() for k in taps])[None, None]
    want = torch.nn.functional.conv3d(crop, w, padding=radii)[:, 0]
    err = float((got[:, :, y0:y0 + wh, x0:x0 + ww] - want).abs().max())
    print(f"blur checker vs conv3d radii {radii} window {window}: max abs err {err:.2e}")
    assert err < 1e-12
    outside = got.clone()
    outside[:, :, y0:y0 + wh, x0:x0 + ww] = 0
    assert not bool(outside.any())
    # the bound's scale dominates the result and is the result for non-negative data and taps
    assert bool((mr.blur3d_ref(x, taps, window, absolute=True) >= got.abs() - 1e-12).all())


def test_moments_against_longdouble():
    rng = np.random.default_rng(4)
    k = np.arange(3 * 4 * 5 * 6).reshape(3, 4, 5, 6)
    x = np.stack([rng.normal(size=(3, 4, 5, 6))[0] * 40 + 100, 1e6 + (k[0] % 977) / 16.0, np.full((4, 5, 6), 0.1)]).astype(np.float32)
    for window in (None, (1, 2, 3, 4)):
        got = mr.moments_ref(torch.from_numpy(x), window).numpy()
        y0, x0, wh, ww = mr.resolve_window(5, 6, window)
        v = x[:, :, y0:y0 + wh, x0:x0 + ww].reshape(3, -1).astype(np.longdouble)
        n = v.shape[1]
        mean = v.sum(1) / n
        m2 = ((v - mean[:, None]) ** 2).sum(1)
        s2 = (v * v).sum(1)
        assert np.all(got[:, 0] == n)
        assert np.all(np.abs(got[:, 1] - mean) <= n * 2.0 ** -53 * np.abs(v).max(1))
        assert np.all(np.abs(got[:, 2] - m2) <= n * 2.0 ** -52 * m2 + 1e-300) and np.all(np.abs(got[:, 3] - s2) <= n * 2.0 ** -52 * s2)
        assert got[2, 1] == np.float32(0.1) and got[2, 2] == 0.0


def _restated_projection(x, mean, contrast, mode, lo, hi):
    out = x.clone()
    for b in range(x.shape[0]):
        v = x[b].double()
        mu = v.mean()
        sd = math.sqrt(float(((v - mu) ** 2).sum()) / v.numel())
        m = mu if mean is None else mean
        if contrast is None:
            s = 1.0
        elif mode == "fixed":
            s = 0.0 if sd == 0 else contrast / sd
        else:
            s = 1.0 if sd == 0 else min(1.0, contrast / sd)
        out[b] = (m + s * (v - mu)).float().clamp(lo, hi)
    return out


@pytest.mark.parametrize("mean,contrast,mode", [(None, None, "max"), (120.0, None, "max"), (None, 10.0, "max"), (None, 100.0, "max"),
                                                (127.5, 12.0, "fixed"), (127.5, 12.0, "max"), (100.0, 0.0, "fixed")])
def test_projection_against_a_restatement(mean, contrast, mode):
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.normal(size=(3, 4, 5, 6)) * 30 + 128).float()
    x[2] = 77.0                                        # sd == 0
    stat = mr.moments_ref(x)
    got = mr.project_ref(x, stat, mean, contrast, mode, 0.0, 255.0)
    want = _restated_projection(x, mean, contrast, mode, 0.0, 255.0)
    ulps = ((got.double() - want.double()).abs() / mr.ulp32(want.double())).max()
    print(f"projection mean {mean} contrast {contrast} {mode}: worst {float(ulps):.2f} ulp")
    assert float(ulps) <= 1.0
    if contrast is not None and mode == "fixed":
        assert bool((got[2] == (77.0 if mean is None else mean)).all())          # s = 0: the clip collapses onto its mean
    if mean is None and (contrast is None or contrast == 100.0):
        assert torch.equal(got, x.clamp(0.0, 255.0))                            # not binding: bits kept
    if contrast is not None and mode == "max":
        assert torch.equal(got[2], x[2] if mean is None else torch.full_like(x[2], mean))


def test_step_rules():
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.normal(size=(3, 2, 4, 5)) * 30 + 128).float()
    g = torch.from_numpy(rng.normal(size=(3, 2, 4, 5))).float()
    g[1] = 0.0
    g[2, 0, 0, 0] = float("inf")
    stat = mr.moments_ref(g)
    got = mr.step_ref(x, g, stat, 2.5)
    rms = math.sqrt(float((g[0].double() ** 2).mean()))
    assert torch.allclose(got[0].double(), x[0].double() + 2.5 * g[0].double() / rms, rtol=1e-7)
    assert torch.equal(got[1], x[1]) and bool(torch.isnan(got[2]).all())
    w = mr.step_ref(x, g, mr.moments_ref(g, (1, 1, 2, 3)), 2.5, (1, 1, 2, 3))
    outside = torch.ones_like(x, dtype=torch.bool)
    outside[:, :, 1:3, 1:4] = False
    assert torch.equal(w[outside], x[outside]) and not torch.equal(w[0, :, 1:3, 1:4], x[0, :, 1:3, 1:4])


def test_gaussian_taps():
    from sensorium_amd import ops
    assert ops.gaussian_taps(0.0).tolist() == [1.0] and ops.gaussian_taps(0.0, 2).tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    for sigma in (0.3, 0.7, 1.0, 2.0, 2.5, 5.34):
        k = ops.gaussian_taps(sigma)
        R = k.numel() // 2
        assert k.dtype == torch.float32 and R == min(math.ceil(3 * sigma), 16)
        assert torch.equal(k, k.flip(0)) and abs(float(k.double().sum()) - 1.0) <= (2 * R + 1) * 2.0 ** -24
        want = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 / (2 * sigma * sigma))
        assert np.array_equal(k.numpy(), (want / want.sum()).astype(np.float32))
    assert ops.gaussian_taps(6.0).numel() == 33 and ops.gaussian_taps(50.0).numel() == 33          # the cap
    assert ops.gaussian_taps(2.0, 3).numel() == 7
    for bad in (dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=1.0, radius=17), dict(sigma=1.0, radius=-1)):
        with pytest.raises(ValueError):
            ops.gaussian_taps(**bad)


def test_update_inputs_stay_off_the_clamp_edges():
    """The inputs of the update tests on the GPU: elements the checker puts within 1 ulp of lo or hi are excluded there, and
    they are under 1 % of the elements."""
    from tests.test_gpu_mei import UPDATE_CASES, near_edge, update_inputs
    for case in UPDATE_CASES:
        x, g = update_inputs(case)
        stepped = mr.step_ref(x[:, 0], g[:, 0], mr.moments_ref(g[:, 0], case["window"]), case["lr"], case["window"])
        proj = mr.project_ref(stepped, mr.moments_ref(stepped, case["window"]), case["mean"], case["contrast"], case["mode"],
                              case["lo"], case["hi"], case["window"], clamp=False)
        share = float(near_edge(proj, case["lo"], case["hi"]).float().mean())
        clamped = float(((proj < case["lo"]) | (proj > case["hi"])).float().mean())
        print(f"update case {case['name']}: {share:.4%} of the elements within 1 ulp of an edge, {clamped:.2%} clamped")
        assert share < 0.01

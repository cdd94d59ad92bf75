"""DriftingGabor in front of the tiny model of tests/test_gpu_frozen_bn.py (randomised running statistics, inputs of order one:
grey levels times INPUT_SCALE), in fp32 and bf16: the parameter gradient through the eval-mode model against the float64 chain
checker render -> oracle, the `learn` mask, attribution.optimal_gabor and attribution.tuning_curve.
Every test prints what it measured before it asserts."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import gabor_reference as gb  # noqa: E402
from tests.gpu_helpers import dev, rel, tol  # noqa: E402
from tests.test_gpu_frozen_bn import BF16_DX, INPUT_SCALE, TINY, sd64, tiny_model  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
T, H, W = 6, 9, 11
WINDOW = (1, 1, 7, 9)
INDEX, NEURONS = 1, [0, 3, 4, 9]
# the reference's grey levels scaled to the tiny model's inputs of order one: mid-grey 1.275, range 0 ... 2.55
GEOM = dict(size=(H, W), background=127.5 * INPUT_SCALE, video_range=(0.0, 255.0 * INPUT_SCALE), window=WINDOW, pad=0.0,
            behavior=(0.3, -0.2), pupil_center=(0.1, 0.4))
INIT = dict(cy=[4.2, 3.6], cx=[5.3, 4.4], sigma=[2.0, 2.6], theta=[0.4, -1.1], sf=[0.12, 0.2], tf=[0.1, -0.15], phase=[0.3, -0.8],
            amplitude=[0.9, 0.7])
SCALES = dict(cy=0.5, cx=0.5, sigma=0.3, theta=0.2, sf=0.01, tf=0.01, phase=0.3, amplitude=0.05)


def reference_gradient(sd, params, geom=GEOM, envelope="gaussian"):
    """d (sum of the chosen responses) / d params through checker render -> oracle, float64, eval-mode statistics."""
    from sensorium_amd import DriftingGabor
    template = DriftingGabor(params.shape[0], T, **geom).template
    p = params.double().clone().requires_grad_(True)
    x = gb.render(p, template, 0, envelope, geom["background"], geom["video_range"], geom["window"], geom["pad"])
    out = orc.forward(sd64(sd), x, strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"], index=INDEX,
                      training=False)
    out[:, NEURONS].sum().backward()
    return p.grad, x.detach()


@pytest.mark.parametrize("dtype", DTYPES)
def test_parameter_gradient_through_the_model(dtype):
    from sensorium_amd import DriftingGabor
    model, sd = tiny_model(dtype)
    model.eval()
    g = DriftingGabor(2, T, init=INIT, **GEOM).to(dev())
    g_ref, x_ref = reference_gradient(sd, g.params.detach().cpu())
    assert not bool(((x_ref[:, 0] <= 0) | (x_ref[:, 0] >= GEOM["video_range"][1]))[..., 1:8, 1:10].any()), "the case must not clamp"
    x = g()
    assert x.shape == (2, 5, T, H, W) and rel(x, x_ref) < 1e-6
    model(x, index=INDEX)[:, NEURONS].sum().backward()
    torch.cuda.synchronize()
    e = rel(g.params.grad, g_ref)
    cols = {n: float((g.params.grad[:, k].double().cpu() - g_ref[:, k]).norm() / g_ref[:, k].norm()) for k, n in enumerate(gb.PARAM_NAMES)}
    print(f"model parameter gradient {dtype}: rel err {e:.3e}; per column " + ", ".join(f"{n} {v:.2e}" for n, v in cols.items()))
    assert float(g_ref.abs().min()) > 0
    assert e < (tol(dtype) if dtype == torch.float32 else BF16_DX["tiny"][1])


def test_learn_masks_columns():
    """The columns left out of `learn` receive exactly zero, through the model too; the kept ones are those of the full gradient
    (compared on one fixed incoming gradient: two backward passes of the model's product build may differ in the last bits)."""
    from sensorium_amd import DriftingGabor
    model, _ = tiny_model(torch.float32)
    model.eval()
    full = DriftingGabor(2, T, init=INIT, **GEOM).to(dev())
    some = DriftingGabor(2, T, init=INIT, learn=("theta", "sf", "amplitude"), **GEOM).to(dev())
    keep = [gb.PARAM_NAMES.index(n) for n in ("theta", "sf", "amplitude")]
    drop = [k for k in range(8) if k not in keep]
    dout = torch.randn(2, 5, T, H, W, generator=torch.Generator().manual_seed(1)).to(dev())
    for g in (full, some):
        g().backward(dout)
    assert torch.equal(some.params.grad[:, keep], full.params.grad[:, keep]) and bool((full.params.grad != 0).all())
    assert bool((some.params.grad[:, drop] == 0).all())
    assert torch.equal(some().detach(), full().detach())
    some.params.grad = None
    model(some(), index=INDEX)[:, NEURONS].sum().backward()
    assert bool((some.params.grad[:, drop] == 0).all()) and bool((some.params.grad[:, keep] != 0).all())


def _inside(params, lo, hi):
    return ((params > lo) & (params < hi)).all(dim=1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_optimal_gabor(dtype):
    from sensorium_amd import DriftingGabor, attribution
    model, _ = tiny_model(dtype)
    model.train()
    starts = dict(cy=[4.2, 3.6, 4.0, 4.5], cx=[5.3, 4.4, 5.0, 6.0], sigma=[2.0, 2.6, 1.8, 2.2], theta=[0.4, -1.1, 1.9, 2.8],
                  sf=[0.12, 0.2, 0.08, 0.15], tf=[0.1, -0.15, 0.05, 0.2], phase=[0.3, -0.8, 1.5, 0.0], amplitude=[0.9, 0.7, 0.8, 0.6])
    geometry = {k: v for k, v in GEOM.items() if k != "size"}
    params, trace = attribution.optimal_gabor(model, INDEX, NEURONS, starts=starts, steps=10, lr=0.05, scales=SCALES,
                                              shape=(T, H, W), **geometry)
    torch.cuda.synchronize()
    assert model.training and all(p.grad is None for p in model.parameters())
    assert params.shape == (4, 8) and trace.shape == (11, 4) and params.is_cuda and trace.is_cuda
    assert bool(torch.isfinite(params).all()) and bool(torch.isfinite(trace).all())
    lo, hi = (b.to(dev()) for b in attribution.gabor_bounds(DriftingGabor(4, T, **GEOM)))
    assert bool(((params >= lo) & (params <= hi)).all())
    free = _inside(params, lo, hi)
    start = torch.stack([torch.tensor(starts[n]) for n in gb.PARAM_NAMES], dim=1).to(dev())
    print(f"optimal_gabor {dtype}: trace first {trace[0].tolist()} last {trace[-1].tolist()}; inside the bounds {free.tolist()}; "
          f"moved by {(params - start).abs().max(dim=0).values.tolist()}")
    assert bool(free.any()) and bool((params != start).any(dim=1).all())
    assert bool((trace[-1] >= trace[0])[free].all())
    # the trace's last entry is the response at the returned parameters
    model.eval()
    g = DriftingGabor(4, T, init={n: params[:, k] for k, n in enumerate(gb.PARAM_NAMES)}, **GEOM).to(dev())
    with torch.no_grad():
        again = model(g(), index=INDEX)[:, NEURONS].float().sum(dim=(1, 2))
    e = rel(again, trace[-1])
    print(f"optimal_gabor {dtype}: re-evaluated {again.tolist()}, rel diff to the trace {e:.3e}")
    assert e < tol(dtype)


def antipodal_pair():
    """(theta, theta') in float32 with theta' = theta + pi to within 2e-11 rad (the float32 grid near pi is 2.4e-7 wide, so the sum
    theta + float32(pi) is in general 1e-7 off; small angles, whose own grid is fine, can land on it)."""
    best = None
    cand = torch.tensor(math.pi + 2.0 ** -11, dtype=torch.float32)
    for _ in range(2048):
        cand = torch.nextafter(cand, torch.tensor(4.0))
        th = torch.tensor(float(cand) - math.pi, dtype=torch.float32)
        d = abs(float(th) + math.pi - float(cand))
        if best is None or d < best[0]:
            best = (d, float(th), float(cand))
    assert best[0] < 2e-11
    return best[1], best[2]


@pytest.mark.parametrize("dtype", DTYPES)
def test_tuning_curve(dtype):
    from sensorium_amd import DriftingGabor, attribution
    model, _ = tiny_model(dtype)
    model.train()
    th0, th0_pi = antipodal_pair()
    thetas = [th0] + [k * math.pi / 8 for k in range(1, 8)]
    # a full-field grating on the whole plane, centred so that the plane is symmetric about the centre
    geom = dict(GEOM, window=None)
    base = dict(frames=T, envelope="none", cy=4.0, cx=5.0, sf=0.15, tf=0.2, phase=0.7, amplitude=0.9, **geom)
    curve = attribution.tuning_curve(model, INDEX, base, dict(theta=thetas), neurons=NEURONS, frames=[2, 3, 4, 5])
    torch.cuda.synchronize()
    assert model.training and all(p.grad is None for p in model.parameters())
    assert curve.shape == (8, 4) and curve.is_cuda and bool(torch.isfinite(curve).all())
    model.eval()
    rows = []
    for th in thetas:
        g = DriftingGabor(1, T, envelope="none", init=dict(cy=4.0, cx=5.0, sf=0.15, tf=0.2, phase=0.7, amplitude=0.9, theta=th), **geom).to(dev())
        with torch.no_grad():
            rows.append(model(g(), index=INDEX)[:, NEURONS][:, :, [2, 3, 4, 5]].float().mean(dim=2))
    loop = torch.cat(rows)
    chunked = attribution.tuning_curve(model, INDEX, base, dict(theta=thetas), neurons=NEURONS, frames=[2, 3, 4, 5], chunk=3)
    e, ec = rel(curve, loop), rel(chunked, loop)
    spread = float((curve.max(dim=0).values - curve.min(dim=0).values).max())
    print(f"tuning_curve {dtype}: rel diff to the explicit loop {e:.3e} (chunk 3: {ec:.3e}); spread over theta {spread:.3e}")
    assert e < tol(dtype) and ec < tol(dtype) and spread > 0
    # theta + pi with the drift and the phase negated is the same grating: q -> -q, and the cosine is even
    kw = dict(cy=4.0, cx=5.0, sf=0.15, amplitude=0.9)
    a = DriftingGabor(1, T, envelope="none", init=dict(theta=th0, tf=0.2, phase=0.7, **kw), **geom).to(dev())().detach()
    b = DriftingGabor(1, T, envelope="none", init=dict(theta=th0_pi, tf=-0.2, phase=-0.7, **kw), **geom).to(dev())().detach()
    same_clip = torch.equal(a.view(torch.int32), b.view(torch.int32))
    flipped = attribution.tuning_curve(model, INDEX, dict(base, tf=-0.2, phase=-0.7), dict(theta=[th0_pi] + thetas[1:]),
                                       neurons=NEURONS, frames=[2, 3, 4, 5])
    same_row = torch.equal(flipped[0], curve[0])
    print(f"tuning_curve {dtype}: theta {th0!r} and {th0_pi!r}: same clip {same_clip}, same row {same_row}")
    assert same_clip and same_row
    assert not torch.equal(flipped[1], curve[1])

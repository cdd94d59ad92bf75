"""The parametric receptive-field fits at model level: the planted-filter experiment of section 12q end to
end on the device, then ``.fit()`` — the conditions of tests/test_rf_fit_reference_cpu.py, and the row against the checker on the
device's own map at the bounds of tests/test_gpu_rf_fit.py —; ``attribution.receptive_fields(..., fit={})`` = ``.fit()`` =
``fit_gaussian2d`` on the selected slices, bit for bit, on the tiny model; and the fitted centres written into a tiny
``DwiseNeuroSpatial`` and read back.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rf_fit_reference as gf  # noqa: E402
from tests import rf_reference as rf  # noqa: E402
from tests.gpu_helpers import dev, rel, tol  # noqa: E402
from tests.test_gpu_frozen_bn import INPUT_SCALE, TINY, tiny_model  # noqa: E402
from tests.test_gpu_model_rf import Recorder, Replay  # noqa: E402
from tests.test_gpu_rf_fit import FTOL, TAU, XTOL  # noqa: E402
from tests.test_rf_fit_reference_cpu import check_planted_fit, planted_fit_figures  # noqa: E402
from tests.test_rf_reference_cpu import PLANTED  # noqa: E402


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("kind", ["binary", "sparse"])
def test_planted_filter_fitted_on_the_device(kind):
    from sensorium_amd import NoiseStimulus, StaAccumulator
    p = PLANTED
    ft = torch.from_numpy(rf.planted_filter(p["gh"], p["gw"])).to(dev())
    stim = NoiseStimulus(32, p["T"], (p["gh"], p["gw"]), kind=kind, contrast=p["contrast"], density=0.1, seed=p["seed"]).to(dev())
    acc = None
    for k0 in range(0, p["clips"], 32):
        x = stim(first_clip=k0)
        d = x[:, 0].double() - 127.5
        drive = torch.zeros(32, p["T"], dtype=torch.float64, device=dev())
        for l in range(p["L"]):
            drive[:, l:] += torch.einsum("btyx,yx->bt", d[:, :p["T"] - l], ft[l])
        r = torch.nn.functional.softplus(0.5 + (0.3 / p["contrast"]) * drive).float()[:, None, :]
        if acc is None:
            acc = StaAccumulator(1, p["L"], (p["gh"], p["gw"]), skip=0, response_centre=r.mean(dim=(0, 2)), device=dev())
        acc.add(x, r)
    got = acc.compute()
    fits = got.fit()
    torch.cuda.synchronize()
    assert fits is got.fits and fits.lag.tolist() == [2] and fits.table[0, 15].item() == 2.0       # row n L + lag of the map
    t, par = fits.table[0].cpu().numpy(), fits.params[0].cpu().numpy()
    prof = fits.profile[0].cpu().numpy()
    res = dict(status=int(t[0]), iterations=int(t[1]), cy=float(t[4]), cx=float(t[5]), sigma_major=float(t[6]), sigma_minor=float(t[7]),
               r2=float(t[10]), profile=(prof / prof[2]).round(4).tolist(), separability=float(fits.separability[0]))
    print(f"planted filter fitted on the device ({kind}): {res}")
    check_planted_fit(res)
    # the row against the checker on the device's own map
    cov32 = got.sta.cpu().numpy()
    m = cov32[0, 2].astype(np.float64).ravel()
    P, T, _, Cv = gf.fit_one(cov32[0, 2], p["gh"], p["gw"])
    excess = (gf.sse(par, m, p["gh"], p["gw"]) - gf.sse(P, m, p["gh"], p["gw"])) / T[9]
    ratio = float((np.abs(par - P) / gf.param_bound(P, T[9], Cv, XTOL, FTOL)).max())
    wprof, wsep, bound = gf.profile(par[None], cov32)
    pratio = float((np.abs(prof - wprof[0]) / bound[0]).max())
    print(f"  against the checker: relative excess of S {excess:.2e}, worst |p difference| / bound {ratio:.3g}, iterations {int(t[1])} / "
          f"{int(T[1])}, profile |difference| / bound {pratio:.3g}")
    assert T[0] == 0 and excess <= TAU[True] and ratio <= 1.0 and pratio <= 1.0
    assert abs(float(fits.separability[0]) - wsep[0]) <= 8 * m.size * p["L"] * gf.EPS64
    assert planted_fit_figures(cov32, 2)["iterations"] == int(T[1])
    # cell 1, window at the origin: pixels are cells; the rendered model is the checker's model
    assert torch.equal(fits.centres("input"), fits.centres("cells")) and torch.equal(fits.sigmas("input"), fits.sigmas("cells"))
    img = fits.render()[0].cpu().numpy().ravel()
    assert np.allclose(img, gf.model(par, p["gh"], p["gw"]), rtol=0, atol=1e-15 + 8 * gf.EPS64 * np.abs(img).max())


T_, H, W = 8, 9, 11
WINDOW = (1, 1, 6, 8)
INDEX, N, LAGS, CLIPS, BATCH, SEED = 1, 10, 3, 6, 3, 9
NOISE = dict(cell=1, contrast=64.0 * INPUT_SCALE, background=127.5 * INPUT_SCALE, video_range=(0.0, 255.0 * INPUT_SCALE))
KW = dict(clips=CLIPS, frames=T_, lags=LAGS, batch=BATCH, noise=NOISE, seed=SEED, size=(H, W), window=WINDOW, behavior=(0.3, -0.2),
          pupil_center=(0.1, 0.4))


def test_fit_through_attribution_equals_fit_equals_fit_gaussian2d():
    from sensorium_amd import attribution, fit_gaussian2d
    model, _ = tiny_model(torch.float32)
    rec = Recorder(model)
    plain = attribution.receptive_fields(rec, INDEX, **KW)
    outs = [out for _, out in rec.seen]
    assert plain.fits is None
    fitted = attribution.receptive_fields(Replay(outs), INDEX, fit={}, **KW)
    mine = plain.fit()
    torch.cuda.synchronize()
    assert torch.equal(fitted.sta, plain.sta) and torch.equal(bits(fitted.summary), bits(plain.summary))      # fit=None ran what it ran before
    a, b = fitted.fits, mine
    lag = plain.peak_lag
    slices = plain.sta[torch.arange(N, device=dev()), lag].contiguous()
    direct = fit_gaussian2d(slices, window=WINDOW, cell=1, size=(H, W))
    torch.cuda.synchronize()
    print(f"tiny model: peak lags {lag.tolist()}, statuses {a.table[:, 0].tolist()}, r2 {[round(v, 3) for v in a.r2.tolist()]}, "
          f"iterations {a.table[:, 1].tolist()}")
    for name in ("table", "params", "profile", "separability", "start"):
        assert torch.equal(bits(getattr(a, name)), bits(getattr(b, name))), name
    assert torch.equal(bits(direct.params), bits(a.params)) and torch.equal(bits(direct.table[:, :15]), bits(a.table[:, :15]))
    assert a.table[:, 15].tolist() == [float(n * LAGS + int(l)) for n, l in enumerate(lag.tolist())] and a.lag.tolist() == lag.tolist()
    assert direct.profile is None and a.profile.shape == (N, LAGS) and a.grid == (6, 8)
    # a fixed lag, as an int and as a tensor; other options reach the kernel
    one = plain.fit(lag=1, profile=False, baseline="zero", max_iter=2)
    same = plain.fit(lag=torch.ones(N, dtype=torch.long), profile=False, baseline="zero", max_iter=2)
    assert torch.equal(bits(one.table), bits(same.table)) and one.profile is None and plain.fits is same
    assert bool((one.table[:, 2] == 0).all()) and bool((one.table[:, 1] <= 2).all()) and one.table[:, 15].tolist() == [n * LAGS + 1.0 for n in range(N)]
    # the centres convert as the summary's do, and good() indexes like significant()
    c = a.centres("input")
    ok = ~torch.isnan(c[:, 0])
    assert bool(((c[ok, 0] >= 0.0) & (c[ok, 0] <= 7.0) & (c[ok, 1] >= 0.0) & (c[ok, 1] <= 9.0)).all())      # the clamp [-1, g] plus the origin
    idx = a.good(-1e9)
    assert idx.is_cuda and idx.dtype == torch.long and idx.tolist() == torch.nonzero(a.converged).flatten().tolist()
    assert idx.numel() > 0, "no fit of the tiny model converged: the test has nothing to feed on"
    x = rec.seen[0][0]
    g = attribution.input_gradient(model, x, INDEX, neurons=idx)
    torch.cuda.synchronize()
    print(f"input_gradient on the converged fits {idx.tolist()}: norm {float(g.norm()):.3e}")
    assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.norm()) > 0


def test_fitted_centres_into_a_tiny_spatial_model_and_back():
    from sensorium_amd import DwiseNeuroSpatial, fit_gaussian2d
    _, sd = tiny_model(torch.float32)

    def build():
        torch.manual_seed(5)
        m = DwiseNeuroSpatial(**TINY)
        m.load_state_dict(sd, strict=False)
        return m.to(dev())
    model = build()
    with torch.no_grad():                                        # the gain starts flat (zero weights): give the positions something to move
        head = model.spatial.heads[INDEX]
        head.weight.copy_(torch.randn(head.weight.shape, generator=torch.Generator().manual_seed(7)) * 0.5)
    # ten maps over the 9 x 9 pixels the 3 x 3 core map (stride 4) spans: planted fields, but neuron 2 is constant (no fit) and
    # neurons 5 and 7 are noise (low R2)
    maps, truth = gf.planted_maps(H, H, N, 0.02, 31)
    maps[2] = 0.25
    maps[5] = np.random.default_rng(1).normal(size=(H, H)).astype(np.float32)
    maps[7] = np.random.default_rng(2).normal(size=(H, H)).astype(np.float32)
    geometry = dict(window=(0, 0, H, H), size=(H, W))
    fits = fit_gaussian2d(torch.from_numpy(maps).to(dev()), **geometry)
    before = model.positions(INDEX, "input", (H, W)).clone()
    raw_before = model.spatial.heads[INDEX].pos.detach().clone()
    other_before = model.spatial.heads[0].pos.detach().clone()
    err_before = model.position_error(fits, INDEX, (H, W))
    wrote = model.set_positions_from(fits, INDEX, input_size=(H, W), min_r2=0.5)
    torch.cuda.synchronize()
    after = model.positions(INDEX, "input", (H, W))
    err = model.position_error(fits, INDEX, (H, W))
    want = fits.centres("input").flip(1)
    rest = [n for n in range(N) if n not in wrote.tolist()]
    print(f"written {wrote.tolist()}, left {rest}; r2 {[round(v, 3) for v in fits.r2.tolist()]}; position error before "
          f"{[round(v, 2) for v in err_before.tolist()]}, after {[float('%.2e' % v) for v in err.tolist()]}")
    assert wrote.tolist() == fits.good(0.5).tolist() and 2 in rest and 5 in rest and 7 in rest and len(wrote) == 7
    # fp32 rounding of a normalised coordinate of magnitude <= 1, carried to pixels: half the plane's span per unit
    eps = 2.0 ** -24 * 4 * max(H, W)
    assert float((after[wrote].double() - want[wrote]).abs().max()) <= eps and float(err[wrote].max()) <= 2 * eps
    assert torch.equal(after[rest], before[rest]) and torch.equal(model.spatial.heads[INDEX].pos.detach()[rest], raw_before[rest])
    assert torch.equal(model.spatial.heads[0].pos.detach(), other_before)
    assert bool(torch.isnan(err[2])) and bool(torch.isnan(err_before[2])) and bool(torch.isfinite(err[[5, 7]]).all())
    assert torch.equal(err[rest][1:], err_before[rest][1:]) and model.spatial.heads[INDEX].pos.requires_grad
    # a forward and backward step after it matches a model constructed with those positions
    twin = build()
    twin.load_state_dict(model.state_dict(), strict=True)
    x = torch.from_numpy(rf.noise(2, T_, (H, W), window=WINDOW, contrast=64.0, seed=3)).to(dev()) * INPUT_SCALE
    outs = []
    for m in (model, twin):
        m.train()
        y = m(x, index=INDEX)
        y.square().mean().backward()
        named = dict(m.named_parameters())
        outs.append((y.detach(), m.spatial.heads[INDEX].pos.grad.clone(), named[f"readouts.{INDEX}.layer.1.weight"].grad.clone()))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), twin.state_dict().values()) if a.is_floating_point() and a.dim() == 2)
    diffs = [rel(a, b) for a, b in zip(*outs)]
    print(f"step after set_positions_from: |y| {float(outs[0][0].norm()):.3e}, |dpos| {float(outs[0][1].norm()):.3e}; relative differences "
          f"to the twin (output, dpos, readout dweight) {[float('%.2e' % v) for v in diffs]}")
    # two training steps of one model differ by the order of the batch-statistics sums: the standing fp32 bound of the suite
    assert max(diffs) <= tol(torch.float32)
    assert bool(torch.isfinite(outs[0][1]).all()) and float(outs[0][1].abs().sum()) > 0
    # explicit rows: fits of a subset of neurons
    sub = fit_gaussian2d(torch.from_numpy(maps[[0, 2, 4]]).to(dev()), **geometry)
    w2 = model.set_positions_from(sub, 0, input_size=(H, W), neurons=[6, 1, 3])
    assert w2.tolist() == [6, 3] and torch.equal(model.spatial.heads[0].pos.detach()[[0, 1, 2, 4, 5]], other_before[[0, 1, 2, 4, 5]])

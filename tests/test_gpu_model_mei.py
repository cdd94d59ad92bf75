"""attribution.most_exciting_input with the regularised ascent on the tiny model of
tests/test_gpu_frozen_bn.py: the plain loop is untouched, one regularised step equals the checker's step on the library's own
gradient, the mean / contrast constraints hold after every step, per-clip objectives give each clip the gradient of its own neuron
set, and the captured graph gives the bits of the eager loop.  Every test prints what it measured before it asserts.

Bit-for-bit statements about two runs THROUGH THE MODEL are made in the ordered-reduction build (DWN_DETERMINISTIC=1, a child
process: tests/det_child.py runs bitwise_report()).  The product build leaves the order of some of the model's sums to the arrival of waves and
workgroups (csrc/dwn_common.h), so there the same ascent run twice differs in the last bits — measured here with the verbatim copy
of the plain loop against the plain loop itself — and equal bits would say nothing about the code under test.  In the product build
the graph is held to the eager loop at the standing fp32 bound instead."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import mei_reference as mr  # noqa: E402
from tests.det_child import deterministic_child  # noqa: E402
from tests.gpu_helpers import dev, rel  # noqa: E402
from tests.test_gpu_frozen_bn import _model_input, tiny_model  # noqa: E402

INDEX, NEURONS = 1, [0, 3, 4, 9]
T, H, W = 6, 9, 11
WINDOW = (1, 1, 7, 9)
WIDE = (-1e4, 1e4)           # a video range that never clamps


def start(batch, seed=4):
    init = _model_input(batch, T, H, W, seed=seed)
    init[:, 0] = init[:, 0] * 0.25 + 96          # a start well inside 0 ... 255
    return init


def legacy_ascent(model, mouse_index, neurons, init, steps, lr, video_range=(0.0, 255.0), norm_budget=None):
    """The ascent loop of most_exciting_input as it stood before the regularised options, copied verbatim."""
    from sensorium_amd.attribution import _as_index, _eval_mode, _response
    lo, hi = float(video_range[0]), float(video_range[1])
    mid = 0.5 * (lo + hi)
    device = next(model.parameters()).device
    x = init.detach().to(device=device, dtype=torch.float32).clone()
    x = x.contiguous()
    nsel = _as_index(neurons, device)
    fsel = _as_index(None, device)
    trace = torch.zeros(steps + 1, dtype=torch.float32, device=device)
    per_clip = x[0, 0].numel()
    with _eval_mode(model):
        for i in range(steps):
            xg = x.detach().requires_grad_(True)
            with torch.enable_grad():
                r = _response(model, xg, mouse_index, nsel, fsel, "sum")
                (g,) = torch.autograd.grad(r, xg)
            trace[i] = r.detach()
            gv = g[:, 0]
            rms = gv.flatten(1).norm(dim=1).div_(per_clip ** 0.5).clamp_min_(1e-20)
            video = x[:, 0] + lr * gv / rms.view(-1, 1, 1, 1)
            if norm_budget is not None:
                dev_ = video - mid
                n = dev_.flatten(1).norm(dim=1).clamp_min_(1e-20)
                video = mid + dev_ * (float(norm_budget) / n).clamp_max_(1.0).view(-1, 1, 1, 1)
            x[:, 0] = video.clamp_(lo, hi)          # channels 1-4 are never written
        with torch.enable_grad():
            trace[steps] = _response(model, x.detach().requires_grad_(True), mouse_index, nsel, fsel, "sum").detach()
    return x, trace


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def plain_path_pair(norm_budget):
    """(library, verbatim copy) of the plain ascent: final inputs and traces."""
    from sensorium_amd import attribution
    model, _ = tiny_model()
    init = start(2)
    want_x, want_t = legacy_ascent(model, INDEX, NEURONS, init, 4, 2.0, norm_budget=norm_budget)
    got_x, got_t = attribution.most_exciting_input(model, INDEX, NEURONS, steps=4, lr=2.0, init=init.to(dev()), norm_budget=norm_budget)
    torch.cuda.synchronize()
    assert got_t.shape == (5,) and not torch.equal(got_x[:, 0].cpu(), init[:, 0])
    return (got_x, got_t), (want_x, want_t)


@pytest.mark.parametrize("norm_budget", [None, 300.0])
def test_plain_path_is_unchanged(norm_budget):
    """Without the new options the function runs the loop it ran before: bit for bit in the deterministic build; in this process
    (product build: run-to-run reordering) within the standing fp32 bound."""
    (got_x, got_t), (want_x, want_t) = plain_path_pair(norm_budget)
    print(f"plain path, norm_budget {norm_budget}: rel diff of the videos {rel(got_x[:, 0], want_x[:, 0]):.3e}, of the traces {rel(got_t, want_t):.3e}")
    assert rel(got_x[:, 0], want_x[:, 0]) < 1e-3 and rel(got_t, want_t) < 1e-3 and same_bits(got_x[:, 1:], want_x[:, 1:])
    assert deterministic_report()[f"plain[{norm_budget}]"] == "1"


def test_one_regularised_step_equals_the_checker_on_the_library_gradient():
    from sensorium_amd import attribution, ops
    model, _ = tiny_model()
    init = start(2)
    sigma, lr = (0.6, 1.0, 1.2), 2.0
    got, trace = attribution.most_exciting_input(model, INDEX, NEURONS, steps=1, lr=lr, init=init.to(dev()), video_range=WIDE,
                                                 blur_sigma=sigma, window=WINDOW)
    g = attribution.input_gradient(model, init.to(dev()), INDEX, NEURONS).cpu()
    torch.cuda.synchronize()
    radii = tuple(min(math.ceil(3 * s), 16) for s in sigma)
    taps = [ops.gaussian_taps(s, r) for s, r in zip(sigma, radii)]
    gb = mr.blur3d_ref(g[:, 0], taps, WINDOW)
    bound = mr.blur3d_bound(g[:, 0], taps, WINDOW)
    stat = mr.moments_ref(gb, WINDOW)
    n, s2 = stat[:, 0], stat[:, 3]
    c = 1.0 / torch.sqrt(s2 / n)
    y0, x0, wh, ww = WINDOW
    crop = (slice(None), slice(None), slice(y0, y0 + wh), slice(x0, x0 + ww))
    want = init[:, 0].double().clone()
    want[crop] = (init[:, 0].double() + lr * gb * c.view(-1, 1, 1, 1))[crop]
    # the blur's bound through the step: |c gb - c' gb'| <= c |gb - gb'| + |gb| |c - c'|, |c - c'| / c <= sum |gb| bound / S2
    dc = ((gb.abs() * bound)[crop].flatten(1).sum(1) / s2) * 1.01
    allowed = lr * c.view(-1, 1, 1, 1) * (bound + gb.abs() * dc.view(-1, 1, 1, 1)) + mr.ulp32(want)
    err = (got[:, 0].cpu().double() - want).abs()
    print(f"one regularised step: worst error / allowed {float((err / allowed).max()):.3f}; step size {float((want - init[:, 0].double()).abs().max()):.3f} "
          f"grey levels, allowed at most {float(allowed.max()):.3e}")
    assert bool((err <= allowed).all())
    outside = torch.ones_like(err, dtype=torch.bool)
    outside[crop] = False
    assert torch.equal(got[:, 0].cpu()[outside], init[:, 0][outside]) and torch.equal(got[:, 1:].cpu(), init[:, 1:])
    assert trace.shape == (2,) and bool(torch.isfinite(trace).all())


@pytest.mark.parametrize("mode", ["max", "fixed"])
@pytest.mark.parametrize("window", [None, WINDOW])
def test_constraints_hold_after_every_step(mode, window):
    from sensorium_amd import attribution
    model, _ = tiny_model()
    mean, contrast = 120.0, 6.0
    y0, x0, wh, ww = mr.resolve_window(H, W, window)
    x = start(2).to(dev())
    first = last = None
    for i in range(5):
        x, trace = attribution.most_exciting_input(model, INDEX, NEURONS, steps=1, lr=3.0, init=x, video_range=WIDE,
                                                   blur_sigma=(0.5, 0.8, 0.8), mean=mean, contrast=contrast, contrast_mode=mode,
                                                   window=window)
        v = x[:, 0, :, y0:y0 + wh, x0:x0 + ww].double().flatten(1).cpu()
        n = v.shape[1]
        mu, sd = v.mean(1), v.std(1, unbiased=False)
        print(f"{mode} window {window} step {i}: mean {mu.tolist()}, sd {sd.tolist()}, response {trace.tolist()}")
        assert bool(((mu - mean).abs() <= n * 2.0 ** -24 * mean).all())
        assert bool((sd <= contrast * (1 + 1e-6)).all())
        if mode == "fixed":
            assert bool(((sd - contrast).abs() <= contrast * 1e-6).all())
        assert bool(torch.isfinite(trace).all())
        first = float(trace[0]) if first is None else first
        last = float(trace[1])
    assert last > first


def test_per_clip_objectives():
    from sensorium_amd import attribution
    model, _ = tiny_model()
    sets = [[0, 3], [4], [1, 2, 9]]
    x = start(3).to(dev())
    g = attribution.input_gradient(model, x, INDEX, sets)
    for b, own in enumerate(sets):
        alone = attribution.input_gradient(model, x[b:b + 1], INDEX, own)
        e = rel(g[b:b + 1], alone)
        print(f"per-clip objective, clip {b} with neurons {own}: rel err to the clip alone {e:.3e}")
        assert e < 1e-3
    assert rel(g[0:1], attribution.input_gradient(model, x[0:1], INDEX, sets[1])) > 1e-2, "the sets must matter"
    as_tensor = attribution.input_gradient(model, x[:2], INDEX, torch.tensor([[0, 3], [4, 4]]))
    assert rel(as_tensor[0:1], g[0:1]) < 1e-3
    video, trace = attribution.most_exciting_input(model, INDEX, sets, steps=3, lr=2.0, init=x, blur_sigma=(0.5, 0.8, 0.8))
    assert trace.shape == (4, 3) and bool((trace[-1] > trace[0]).all()) and video.shape == x.shape
    out = model.eval()(video, index=INDEX).float()
    model.train()
    want = torch.stack([out[b, own].sum() for b, own in enumerate(sets)])
    assert rel(trace[-1], want) < 1e-4
    # one start, three sets: the start is repeated
    video1, trace1 = attribution.most_exciting_input(model, INDEX, sets, steps=1, lr=2.0, init=x[0], mean=100.0)
    assert video1.shape == x.shape and trace1.shape == (2, 3)
    # a flat list keeps its meaning: one objective summed over the batch
    flat_x, flat_t = attribution.most_exciting_input(model, INDEX, NEURONS, steps=2, lr=2.0, init=x, blur_sigma=(0.5, 0.8, 0.8))
    assert flat_t.shape == (3,)
    g_flat = attribution.input_gradient(model, x, INDEX, NEURONS)
    assert rel(g_flat, attribution.input_gradient(model, x, INDEX, [NEURONS] * 3)) < 1e-3


SCHEDULES = [([[1.0, 1.5, 1.5], [0.8, 1.2, 1.2], [0.5, 0.9, 1.0], [0.0, 0.6, 0.7]], [4.0, 3.0, 2.0, 1.0]),
             ([[0.0, 0.5, 0.5], [0.3, 1.0, 0.4], [0.9, 0.2, 1.3], [0.6, 0.6, 0.6]], [1.0, 2.5, 0.5, 3.0])]
GRAPH_KW = dict(mean=118.0, contrast=8.0, contrast_mode="max", window=WINDOW)
GRAPH_SETS = [[0, 3], [4, 1, 2]]


def _scheduled(model, use_graph, sigmas, lrs, **kw):
    from sensorium_amd import attribution
    x, trace = attribution.most_exciting_input(model, INDEX, kw.pop("neurons", NEURONS), steps=4, lr=lrs, init=start(2).to(dev()),
                                               blur_sigma=sigmas, use_graph=use_graph, **kw)
    torch.cuda.synchronize()
    return x.cpu(), trace.cpu()


def graph_pairs(model):
    """[(name, eager (x, trace), graph (x, trace))]: four steps with a sigma and an lr schedule that change every step, twice with
    different schedules on the same model, then per-clip objectives."""
    out = []
    for i, (sigmas, lrs) in enumerate(SCHEDULES):
        out.append((f"graph[{i}]", _scheduled(model, False, sigmas, lrs, **GRAPH_KW), _scheduled(model, True, sigmas, lrs, **GRAPH_KW)))
    out.append(("graph[sets]", _scheduled(model, False, *SCHEDULES[0], neurons=GRAPH_SETS), _scheduled(model, True, *SCHEDULES[0], neurons=GRAPH_SETS)))
    return out


def test_graph_replay_follows_the_eager_loop():
    model, _ = tiny_model()
    pairs = graph_pairs(model)
    for name, (ex, et), (gx, gt) in pairs:
        print(f"{name}: graph vs eager rel diff video {rel(gx[:, 0], ex[:, 0]):.3e}, trace {rel(gt, et):.3e}; trace {gt.flatten().tolist()}")
        assert rel(gx[:, 0], ex[:, 0]) < 1e-3 and rel(gt, et) < 1e-3 and same_bits(gx[:, 1:], ex[:, 1:])
        assert gt.shape == ((5, 2) if name == "graph[sets]" else (5,)) and bool((gt[-1] > gt[0]).all())
    assert rel(pairs[0][2][0][:, 0], pairs[1][2][0][:, 0]) > 1e-3, "the second call must follow its own schedules"
    report = deterministic_report()
    assert all(report[name] == "1" for name, _, _ in pairs) and report["schedules_differ"] == "1"


def five_calls_and_one_call(model):
    """Five calls of one step against one call of five steps: the constraints are part of every step."""
    from sensorium_amd import attribution
    kw = dict(lr=3.0, video_range=WIDE, blur_sigma=(0.5, 0.8, 0.8), mean=120.0, contrast=6.0, contrast_mode="fixed", window=WINDOW)
    x = start(2).to(dev())
    for _ in range(5):
        x, trace = attribution.most_exciting_input(model, INDEX, NEURONS, steps=1, init=x, **kw)
    x5, trace5 = attribution.most_exciting_input(model, INDEX, NEURONS, steps=5, init=start(2).to(dev()), **kw)
    torch.cuda.synchronize()
    return (x, trace[-1:]), (x5, trace5[-1:])


def test_five_calls_of_one_step_are_one_call_of_five_steps():
    model, _ = tiny_model()
    (x, t), (x5, t5) = five_calls_and_one_call(model)
    print(f"five calls vs one call: rel diff video {rel(x5[:, 0], x[:, 0]):.3e}, last response {float(t):.6f} / {float(t5):.6f}")
    assert rel(x5[:, 0], x[:, 0]) < 1e-3 and rel(t5, t) < 1e-3
    assert deterministic_report()["five_calls"] == "1"


def bitwise_report():
    """What must hold bit for bit when the model itself is reproducible: name -> bool.  Run in a child process (tests/det_child.py)."""
    out = {}
    for nb in (None, 300.0):
        (gx, gt), (wx, wt) = plain_path_pair(nb)
        out[f"plain[{nb}]"] = same_bits(gx, wx) and same_bits(gt, wt)
    model, _ = tiny_model()
    pairs = graph_pairs(model)
    for name, (ex, et), (gx, gt) in pairs:
        out[name] = same_bits(gx, ex) and same_bits(gt, et)
    out["schedules_differ"] = not torch.equal(pairs[0][2][0], pairs[1][2][0])
    (x, t), (x5, t5) = five_calls_and_one_call(model)
    out["five_calls"] = same_bits(x, x5) and same_bits(t, t5)
    return out


@functools.lru_cache(maxsize=None)
def deterministic_report():
    """bitwise_report() of a child process on the ordered-reduction build: name -> "1" / "0"."""
    import sensorium_amd._lib as L
    if not (L._HERE / "csrc" / "libdwiseneuro_hip_det.so").exists():
        pytest.skip("libdwiseneuro_hip_det.so is not built")
    deterministic, lib, report = deterministic_child("tests.test_gpu_model_mei:bitwise_report")
    assert deterministic == "1" and lib == "libdwiseneuro_hip_det.so"
    return {k: str(int(v)) for k, v in report.items()}

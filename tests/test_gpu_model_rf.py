"""attribution.receptive_fields on the tiny model of tests/test_gpu_frozen_bn.py (randomised running statistics, inputs of order
one: grey levels times INPUT_SCALE), in fp32 and bf16.  The new code is isolated by recording what the
model was given and what it answered: the map must be the checker's from those very responses and the bit-identical checker
noise, at the kernel bounds.  The model's own error enters only in the comparison with the float64 oracle, at the propagated form
of the bound its output already meets.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import rf_reference as rf  # noqa: E402
from tests.gpu_helpers import dev, tol  # noqa: E402
from tests.test_gpu_frozen_bn import INPUT_SCALE, TINY, sd64, tiny_model  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
T, H, W = 8, 9, 11
WINDOW = (1, 1, 6, 8)
INDEX, N, LAGS, CLIPS, BATCH, SEED, CELL = 1, 10, 3, 5, 2, 9, 2
BACKGROUND, CONTRAST = 127.5 * INPUT_SCALE, 64.0 * INPUT_SCALE
NOISE = dict(cell=CELL, contrast=CONTRAST, background=BACKGROUND, video_range=(0.0, 255.0 * INPUT_SCALE))
KW = dict(clips=CLIPS, frames=T, lags=LAGS, batch=BATCH, noise=NOISE, seed=SEED, size=(H, W), window=WINDOW, behavior=(0.3, -0.2),
          pupil_center=(0.1, 0.4))


class Recorder(torch.nn.Module):
    """Passes calls on to ``inner`` and keeps what went in and what came out."""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.seen = inner, []

    def forward(self, x, index=None):
        out = self.inner(x, index=index)
        self.seen.append((x.detach().clone(), out.detach().clone()))
        return out


class Replay(torch.nn.Module):
    """Answers the recorded outputs in order: two runs then see the same responses bit for bit, whatever the model's kernels do."""

    def __init__(self, outs):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1, device=outs[0].device))
        self.outs, self.at = outs, 0

    def forward(self, x, index=None):
        out = self.outs[self.at]
        assert out.shape[0] == x.shape[0]
        self.at += 1
        return out


def checker_noise(first, count):
    return rf.noise(count, T, (H, W), kind="binary", cell=CELL, contrast=CONTRAST, background=BACKGROUND, window=WINDOW,
                    behavior=(0.3, -0.2), pupil_center=(0.1, 0.4), seed=SEED, first_clip=first)


def checker_state(batches, r0):
    """The checker's state from (x, r) batches (numpy), centred as the library centres."""
    st = rf.State(batches[0][1].shape[1], LAGS, WINDOW[2] // CELL, WINDOW[3] // CELL)
    for x, r in batches:
        rf.accumulate(st, x, r, channel=0, window=WINDOW, cell=CELL, skip=LAGS - 1, s0=np.float32(BACKGROUND), r0=r0)
    return st


def kernel_tolerance(st, cov):
    """What separates the device's cov from the checker's on the same operands: the fp32 chain of the cross term and the float64
    sums of the moments, propagated through cov = (Cuv - U1 V1 / K) / K, the float64 evaluation itself and one fp32 ulp."""
    K = float(st.K)
    prop = (st.bound_C + 2 * (st.bound_U1[:, None, None] * np.abs(st.V1)[None] + np.abs(st.U1)[:, None, None] * st.bound_V1[None]) / K) / K
    a = np.maximum(np.abs(cov), np.finfo(np.float32).tiny).astype(np.float32)
    ulp = (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)
    return prop + rf.cov_f64_bound(st) + ulp


def recorded_run(dtype, **kw):
    from sensorium_amd import attribution
    model, sd = tiny_model(dtype)
    model.train()
    rec = Recorder(model)
    got = attribution.receptive_fields(rec, INDEX, **{**KW, **kw})
    torch.cuda.synchronize()
    assert model.training and all(p.grad is None for p in model.parameters())
    return got, rec, sd


@pytest.mark.parametrize("dtype", DTYPES)
def test_map_equals_the_checker_on_the_library_s_own_responses(dtype):
    got, rec, _ = recorded_run(dtype)
    assert [int(x.shape[0]) for x, _ in rec.seen] == [2, 2, 1]                  # the last batch is smaller
    first = 0
    batches = []
    for x, out in rec.seen:
        want = checker_noise(first, x.shape[0])
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want.view(np.uint32)), "the noise must be the checker's bit for bit"
        assert out.dtype == torch.float32 or out.dtype == dtype
        batches.append((want, out.float().cpu().numpy()))
        first += x.shape[0]
    r0 = rec.seen[0][1].float().mean(dim=(0, 2)).cpu().numpy()
    st = checker_state(batches, r0)
    cov, z, summary = rf.finalize(st)
    G = st.gh * st.gw
    dev_cov = got.sta.cpu().numpy().astype(np.float64).reshape(N, LAGS, G)
    ratio = float((np.abs(dev_cov - cov.reshape(N, LAGS, G)) / kernel_tolerance(st, cov.reshape(N, LAGS, G))).max())
    print(f"receptive_fields {dtype}: K {got.samples}, max |sta| {np.abs(cov).max():.3e}, worst |error| / kernel tolerance {ratio:.3f}; "
          f"peak lags {got.peak_lag.tolist()}, peak z {[round(v, 2) for v in got.summary[:, 1].tolist()]}")
    assert got.samples == st.K == CLIPS * (T - (LAGS - 1)) and got.sta.shape == (N, LAGS, 3, 4) and got.z.shape == got.sta.shape
    assert ratio <= 1.0 and float(np.abs(cov).max()) > 0
    assert torch.equal(got.accumulator.r0.cpu(), torch.from_numpy(r0))


@pytest.mark.parametrize("dtype", DTYPES)
def test_map_against_the_float64_oracle(dtype):
    """|sta - sta_oracle| <= tol max |r| sum |v| / K element by element: the model's output error, bounded by the standing model
    tolerance relative to the largest response, weighted by the stimulus deviations it is correlated with."""
    got, rec, sd = recorded_run(dtype)
    x64 = torch.from_numpy(checker_noise(0, CLIPS)).double()
    r64 = orc.forward(sd64(sd), x64, strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"], index=INDEX,
                      training=False).detach().numpy()
    r0 = rec.seen[0][1].float().mean(dim=(0, 2)).cpu().numpy()
    st = checker_state([(x64.numpy().astype(np.float32), r64.astype(np.float32))], r0)
    cov = rf.covariance(st)
    bound = tol(dtype) * float(np.abs(r64).max()) * st.absV[None] / st.K
    dev_cov = got.sta.cpu().numpy().astype(np.float64).reshape(cov.shape)
    ratio = float((np.abs(dev_cov - cov) / bound).max())
    print(f"receptive_fields {dtype} against the oracle: max |r| {np.abs(r64).max():.3e}, max |sta| {np.abs(cov).max():.3e}, "
          f"worst |difference| / bound {ratio:.3f}")
    assert ratio <= 1.0


def test_neuron_selection_split_runs_and_last_batch():
    from sensorium_amd import attribution
    full, rec, _ = recorded_run(torch.float32)
    outs = [out for _, out in rec.seen]
    rows = [0, 3, 4, 9]
    sel = attribution.receptive_fields(Replay(outs), INDEX, neurons=rows, **KW)
    same = attribution.receptive_fields(Replay(outs), INDEX, **KW)
    torch.cuda.synchronize()
    print("selected rows: sta equal", torch.equal(sel.sta, full.sta[rows]), "summary equal", torch.equal(sel.summary, full.summary[rows]))
    assert torch.equal(same.sta, full.sta) and torch.equal(same.accumulator.state, full.accumulator.state)
    assert sel.sta.shape[0] == 4 and sel.accumulator.state.numel() < full.accumulator.state.numel()
    assert torch.equal(sel.sta, full.sta[rows]) and torch.equal(sel.z, full.z[rows])
    assert torch.equal(sel.summary.view(torch.int64), full.summary[rows].contiguous().view(torch.int64))
    # the same clips over two calls: the second continues the first's accumulator
    replay = Replay(outs)
    part = attribution.receptive_fields(replay, INDEX, **{**KW, "clips": 4})
    assert part.samples == 4 * (T - (LAGS - 1))
    both = attribution.receptive_fields(replay, INDEX, first_clip=4, accumulator=part.accumulator, **{**KW, "clips": 1})
    torch.cuda.synchronize()
    print("split over two calls: K", both.samples, "of", full.samples)
    assert both.samples == full.samples and torch.equal(both.sta, full.sta) and torch.equal(both.accumulator.state, full.accumulator.state)


def test_significant_indices_feed_input_gradient():
    from sensorium_amd import attribution
    got, rec, _ = recorded_run(torch.float32)
    idx = got.significant(0.0)
    some = got.significant(float(got.summary[:, 1].abs().median()))
    assert idx.is_cuda and idx.dtype == torch.long and idx.tolist() == list(range(N)) and 0 < some.numel() < N
    x = rec.seen[0][0]
    g = attribution.input_gradient(rec.inner, x, INDEX, neurons=some)
    torch.cuda.synchronize()
    print(f"input_gradient on {some.tolist()}: norm {float(g.norm()):.3e}")
    assert g.shape == x.shape and bool(torch.isfinite(g).all()) and float(g.norm()) > 0
    c = got.centres("input")
    assert c.shape == (N, 2) and bool(((c[:, 0] >= 1.5 - 1e-9) & (c[:, 0] <= 5.5 + 1e-9) & (c[:, 1] >= 1.5 - 1e-9) & (c[:, 1] <= 7.5 + 1e-9)).all())
    n = got.centres("normalised")
    assert bool((n.abs() <= 1).all())


@pytest.mark.parametrize("kind", ["spatial", "gaze"])
def test_other_model_classes_run_through_the_same_call(kind):
    from sensorium_amd import DwiseNeuroGaze, DwiseNeuroSpatial, attribution
    _, sd = tiny_model(torch.float32)
    torch.manual_seed(5)
    model = (DwiseNeuroSpatial if kind == "spatial" else DwiseNeuroGaze)(**TINY)
    model.load_state_dict(sd, strict=False)
    model = model.to(dev())
    got = attribution.receptive_fields(model, INDEX, **KW)
    torch.cuda.synchronize()
    print(f"{kind}: peak lags {got.peak_lag.tolist()}, max |z| {float(got.z.abs().max()):.2f}")
    assert got.sta.shape == (N, LAGS, 3, 4) and bool(torch.isfinite(got.sta).all()) and bool(torch.isfinite(got.z).all())
    assert got.samples == CLIPS * (T - (LAGS - 1)) and float(got.sta.abs().max()) > 0

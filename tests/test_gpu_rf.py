"""The receptive-field kernels against the float64 checker tests/rf_reference.py: the noise stimulus bit
for bit; the accumulator on the smallest shapes at which a tiled matrix-instruction kernel can go wrong — bit for bit on data
whose sums are exact in fp32, within the derived bound (K_call + 2) 2^-24 sum |u| |v| on real-valued data —; the containment of
non-finite values; the finaliser from the device's own state; and the planted-filter case end to end on the device.
Every test prints what it measured before it asserts."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rf_reference as rf  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402
from tests.test_rf_reference_cpu import PLANTED, planted_condition  # noqa: E402

# ------------------------------------------------------------------------------------------------------------------------ noise
GEOMS = {
    "cell2-hold2": dict(B=3, T=5, size=(9, 11), window=(1, 1, 6, 8), cell=2, hold=2),
    "ragged-63-cells": dict(B=2, T=3, size=(9, 11), window=(1, 1, 7, 9), cell=1, hold=1),
    "window-is-plane": dict(B=2, T=4, size=(8, 12), window=None, cell=2, hold=3),
    "last-clips": dict(B=3, T=2, size=(6, 8), window=(0, 1, 6, 6), cell=3, hold=1, first_clip=2 ** 32 - 3),
    "seed-high-bits": dict(B=2, T=3, size=(6, 8), window=(1, 0, 4, 8), cell=1, hold=1, seed=0xFEDCBA9876543210, first_clip=5),
}


def device_noise(kind, B, T, size, window, cell, hold, seed=3, first_clip=0, density=0.3):
    from sensorium_amd import NoiseStimulus
    stim = NoiseStimulus(B, T, size, kind=kind, cell=cell, hold=hold, contrast=60.25, density=density, background=120.5, window=window,
                         pad=3.0, behavior=(0.5, -1.5), pupil_center=(2.0, 4.0), seed=seed).to(dev())
    return stim(first_clip=first_clip)


def checker_noise(kind, B, T, size, window, cell, hold, seed=3, first_clip=0, density=0.3):
    return rf.noise(B, T, size, kind=kind, cell=cell, hold=hold, contrast=60.25, density=density, background=120.5, window=window,
                    pad=3.0, behavior=(0.5, -1.5), pupil_center=(2.0, 4.0), seed=seed, first_clip=first_clip)


@pytest.mark.parametrize("kind", ["binary", "sparse"])
@pytest.mark.parametrize("name", list(GEOMS))
def test_noise_is_the_checker_bit_for_bit(name, kind):
    got = device_noise(kind, **GEOMS[name]).cpu().numpy()
    want = checker_noise(kind, **GEOMS[name])
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"noise {name} {kind}: {diff} of {want.size} words differ; levels {np.unique(got[:, 0]).tolist()}")
    assert got.shape == want.shape and diff == 0


def test_noise_sparse_extremes_and_chunks():
    g = GEOMS["cell2-hold2"]
    zero = device_noise("sparse", density=0.0, **g).cpu().numpy()
    one = device_noise("sparse", density=1.0, **g).cpu().numpy()
    assert np.array_equal(zero, checker_noise("sparse", density=0.0, **g)) and np.array_equal(one, checker_noise("sparse", density=1.0, **g))
    win = (slice(None), 0, slice(None), slice(1, 7), slice(1, 9))
    assert np.all(zero[win] == 120.5) and not np.any(one[win] == 120.5)
    whole = device_noise("binary", **dict(g, B=3))
    tail = device_noise("binary", **dict(g, B=2, first_clip=1))
    assert torch.equal(tail, whole[1:])


# ------------------------------------------------------------------------------------------------------------------- accumulate
# (N, gh, gw, cell, L, skip, T, B): N on both sides of the 32-row tile and past one 64-row workgroup; 1, 35, 63 and 65 cells (the
# last one needs a second workgroup column); 1, 2, 3, 5 valid frames per clip (odd sample counts against the x2 step of the matrix
# instruction, and sample totals 1 ... 15 below one staged chunk); skip below and above L - 1.  The window starts at an odd column
# and is narrower than the plane: its rows are neither aligned nor contiguous.
CASES = {
    "n1-g1-c3-k1": (1, 1, 1, 3, 1, 0, 1, 1),
    "n31-g35-c1-k6": (31, 5, 7, 1, 3, 0, 4, 3),
    "n33-g63-c2-k3": (33, 7, 9, 2, 5, 2, 7, 1),
    "n70-g65-c1-k15": (70, 5, 13, 1, 3, 4, 9, 3),
    "n70-g65-c3-k15": (70, 5, 13, 3, 1, 0, 5, 3),
    "n33-g35-c2-k70": (33, 5, 7, 2, 3, 1, 16, 5),       # 70 samples: two full staged chunks and a ragged third
}
Y0, X0, CIN, CH = 2, 3, 2, 1


def make_case(name, exact, seed=0):
    N, gh, gw, cell, L, skip, T, B = CASES[name]
    rng = np.random.default_rng(seed)
    H, W = Y0 + gh * cell + 1, X0 + gw * cell + 2
    window = (Y0, X0, gh * cell, gw * cell)
    if exact:
        # r in [-8, 8], x in 0 .. 255, s0 = 128, integer centres: every product and every sum is exact in fp32.  With cell = 3 the
        # factor 1 / 9 is not a power of two: the cells are then constant (9 m * fl(1 / 9) rounds to m), so v stays an integer
        x = rng.integers(0, 256, size=(B, CIN, T, H, W)).astype(np.float32)
        if cell == 3:
            vals = rng.integers(0, 256, size=(B, T, gh, gw)).astype(np.float32)
            x[:, CH, :, Y0:Y0 + gh * cell, X0:X0 + gw * cell] = np.repeat(np.repeat(vals, 3, axis=2), 3, axis=3)
        r = rng.integers(-8, 9, size=(B, N, T)).astype(np.float32)
        r0 = rng.integers(-2, 3, size=N).astype(np.float32)
        s0 = 128.0
    else:
        x = (rng.random(size=(B, CIN, T, H, W)) * 255).astype(np.float32)
        r = (np.abs(rng.normal(size=(B, N, T))) * 3).astype(np.float32)
        r0 = (np.round(r.mean(axis=(0, 2)) * 2) / 2).astype(np.float32)     # near the mean, and never equal to a lone response
        s0 = 127.5
    return dict(N=N, gh=gh, gw=gw, cell=cell, L=L, skip=skip, T=T, B=B, H=H, W=W, window=window, x=x, r=r, r0=r0, s0=s0)


def device_accumulate(c, splits=None, r0=True, x=None, r=None):
    """The device state (numpy float64, flat) and K after accumulating the case in the given clip ranges."""
    from sensorium_amd import ops
    x = c["x"] if x is None else x
    r = c["r"] if r is None else r
    state = torch.zeros(ops.sta_state_numel(c["N"], c["L"], c["window"], c["cell"]), dtype=torch.float64, device=dev())
    r0t = torch.from_numpy(c["r0"]).to(dev()) if r0 else None
    K = 0
    for lo, hi in (splits or [(0, c["B"])]):
        K += ops.sta_accumulate(state, torch.from_numpy(x[lo:hi]).to(dev()), torch.from_numpy(r[lo:hi]).to(dev()), lags=c["L"],
                                window=c["window"], cell=c["cell"], channel=CH, skip=c["skip"], s0=c["s0"], r0=r0t)
    torch.cuda.synchronize()
    return state, K


def checker_accumulate(c, splits=None, r0=True):
    st = rf.State(c["N"], c["L"], c["gh"], c["gw"])
    for lo, hi in (splits or [(0, c["B"])]):
        rf.accumulate(st, c["x"][lo:hi], c["r"][lo:hi], channel=CH, window=c["window"], cell=c["cell"], skip=c["skip"], s0=c["s0"],
                      r0=c["r0"] if r0 else None)
    return st


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_exact_data_bit_for_bit(name):
    c = make_case(name, exact=True)
    want = checker_accumulate(c)
    runs = [("one call", None)]
    if c["B"] >= 3:
        runs.append(("three calls", [(0, 1), (1, 2), (2, c["B"])]))
    for label, splits in runs:
        state, K = device_accumulate(c, splits)
        got = state.cpu().numpy()
        diff = int((got != want.flat()).sum())
        print(f"accumulate exact {name}, {label}: K {K}, {diff} of {got.size} state elements differ; max |Cuv| {np.abs(want.Cuv).max()}")
        assert K == want.K == c["B"] * (c["T"] - max(c["skip"], c["L"] - 1)) and diff == 0
    # without response centres (a null r0) the same holds
    got = device_accumulate(c, r0=False)[0].cpu().numpy()
    assert np.array_equal(got, checker_accumulate(c, r0=False).flat())


@pytest.mark.parametrize("name", list(CASES))
def test_accumulate_real_data_within_the_derived_bounds(name):
    """Cross term: an fp32 fma chain of K_call terms, one conversion and one float64 add per call: (K_call + 2) 2^-24 sum |u||v|,
    summed over the calls.  Moments: float64 sums of K_call terms on both sides (device and checker), (K_call + 2) 2^-53 sum |term|
    each: twice that between them."""
    c = make_case(name, exact=False, seed=1)
    for label, splits in (("one call", None), ("per clip", [(b, b + 1) for b in range(c["B"])])):
        want = checker_accumulate(c, splits)
        got = rf.State.from_flat(device_accumulate(c, splits)[0].cpu().numpy(), c["N"], c["L"], c["gh"], c["gw"], want.K)
        ratio = float((np.abs(got.Cuv - want.Cuv) / want.bound_C).max())
        mom = {k: float((np.abs(getattr(got, k) - getattr(want, k)) / (2 * getattr(want, "bound_" + k))).max()) for k in ("U1", "U2", "V1", "V2")}
        print(f"accumulate real {name}, {label}: K {want.K}, worst |error| / bound: cross {ratio:.3f}, moments {mom}")
        assert ratio <= 1.0 and all(v <= 1.0 for v in mom.values())
        assert float(np.abs(want.Cuv).max()) > 0


def test_non_finite_values_stay_where_they_are():
    c = make_case("n70-g65-c1-k15", exact=False, seed=2)
    N, L, G = c["N"], c["L"], c["gh"] * c["gw"]
    clean = rf.State.from_flat(device_accumulate(c)[0].cpu().numpy(), N, L, c["gh"], c["gw"], 0)
    # a NaN and an Inf in the responses of neurons 5 and 66 (valid frames): only their rows
    r = c["r"].copy()
    r[1, 5, 6] = np.nan
    r[2, 66, 8] = np.inf
    got = rf.State.from_flat(device_accumulate(c, r=r)[0].cpu().numpy(), N, L, c["gh"], c["gw"], 0)
    others = np.setdiff1d(np.arange(N), [5, 66])
    print("non-finite rows:", np.unique(np.nonzero(~np.isfinite(got.Cuv))[0]).tolist())
    assert not np.isfinite(got.Cuv[[5, 66]]).any() and not np.isfinite(got.U1[[5, 66]]).any() and not np.isfinite(got.U2[[5, 66]]).any()
    assert np.array_equal(got.Cuv[others], clean.Cuv[others]) and np.array_equal(got.U1[others], clean.U1[others])
    assert np.array_equal(got.V1, clean.V1) and np.array_equal(got.V2, clean.V2)
    # a NaN in one pixel of cell (2, 11) of frame 5 of clip 0: only that cell's columns, at the lags that reach the frame
    x = c["x"].copy()
    g = 2 * c["gw"] + 11
    x[0, CH, 5, Y0 + 2, X0 + 11] = np.nan
    got = rf.State.from_flat(device_accumulate(c, x=x)[0].cpu().numpy(), N, L, c["gh"], c["gw"], 0)
    cols = np.setdiff1d(np.arange(G), [g])
    bad_lags = np.unique(np.nonzero(~np.isfinite(got.Cuv[:, :, g]))[1]).tolist()
    print("non-finite columns:", np.unique(np.nonzero(~np.isfinite(got.Cuv))[2]).tolist(), "lags", bad_lags)
    assert bad_lags == [0, 1, 2]                                # t0 = 4: frame 5 is read as t - l for t = 5, 6, 7
    assert np.isnan(got.Cuv[:, :, g]).all() and np.isnan(got.V1[:, g]).all() and np.isnan(got.V2[:, g]).all()
    assert np.array_equal(got.Cuv[:, :, cols], clean.Cuv[:, :, cols]) and np.array_equal(got.V1[:, cols], clean.V1[:, cols])
    assert np.array_equal(got.V2[:, cols], clean.V2[:, cols]) and np.array_equal(got.U1, clean.U1) and np.array_equal(got.U2, clean.U2)


# --------------------------------------------------------------------------------------------------------------------- finalise
def ulp32(ref):
    """One fp32 ulp at |ref| (the spacing of fp32 above it), at least the smallest normal's."""
    a = np.maximum(np.abs(ref), np.finfo(np.float32).tiny).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def compare_finalize(label, state, K, N, L, gh, gw, window, cell, rel=0.5, skip_summary=()):
    """Device finaliser against the checker's on the DEVICE's state (read back): the state bound does not enter.  cov and z: one
    fp32 ulp (the rounding of the store is half of one; the float64 formulas are the same, operation by operation).  summary:
    lag and count exact, the rest at the float64 bound of a sum over G cells in another order (rf.summary_tolerance)."""
    from sensorium_amd import ops
    cov, z, summary = ops.sta_finalize(state, K, N=N, lags=L, window=window, cell=cell, rel_threshold=rel)
    cov_only, none, summary2 = ops.sta_finalize(state, K, N=N, lags=L, window=window, cell=cell, rel_threshold=rel, z=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(cov_only, cov) and torch.equal(summary2.view(torch.int64), summary.view(torch.int64))
    st = rf.State.from_flat(state.cpu().numpy(), N, L, gh, gw, K)
    wc, wz, ws = rf.finalize(st, rel)
    cov, z, summary = cov.cpu().numpy().astype(np.float64), z.cpu().numpy().astype(np.float64), summary.cpu().numpy()
    ec, ez = float((np.abs(cov - wc) / ulp32(wc)).max()), float((np.abs(z - wz) / ulp32(wz)).max())
    keep = np.setdiff1d(np.arange(N), list(skip_summary))
    tol = rf.summary_tolerance(gh, gw)
    es = np.abs(summary[keep] - ws[keep])
    print(f"finalise {label}: cov {ec:.3f} ulp, z {ez:.3f} ulp; summary max abs diff per column {np.nanmax(es, axis=0).tolist()} (tol {tol:.2e})")
    assert ec <= 1.0 and ez <= 1.0
    assert np.array_equal(summary[keep][:, [0, 7]], ws[keep][:, [0, 7]])
    assert np.array_equal(np.isnan(summary[keep]), np.isnan(ws[keep]))
    assert np.allclose(summary[keep][:, 1], ws[keep][:, 1], rtol=1e-12, atol=0)
    assert np.allclose(summary[keep][:, 2:6], ws[keep][:, 2:6], rtol=0, atol=tol, equal_nan=True)
    assert np.allclose(summary[keep][:, 6], ws[keep][:, 6], rtol=gh * gw * 2.0 ** -50, atol=0)
    return cov, z, summary


@pytest.mark.parametrize("name", ["n33-g63-c2-k3", "n70-g65-c1-k15", "n33-g35-c2-k70", "n1-g1-c3-k1"])
@pytest.mark.parametrize("rel", [0.5, 0.0, 1.0])
def test_finalize_against_the_checker(name, rel):
    c = make_case(name, exact=False, seed=4)
    state, K = device_accumulate(c)
    compare_finalize(f"{name} rel {rel}", state, K, c["N"], c["L"], c["gh"], c["gw"], c["window"], c["cell"], rel)


def test_finalize_special_neurons_and_cells():
    """Neuron 0 responds to the stimulus; neuron 1 always answers its centre (cov exactly zero: the degenerate summary, decided on
    the device); neuron 2 is constant off its centre (var_u = 0: z = 0 everywhere).  The stimulus window is wider than the noise:
    the last two columns of cells hold the pad (var_v = 0: z = 0 there)."""
    from sensorium_amd import NoiseStimulus, ops
    B, T, L, gh, gw = 16, 16, 3, 6, 10
    stim = NoiseStimulus(B, T, (gh, gw), window=(0, 0, 6, 8), seed=5, pad=0.0).to(dev())
    x = stim()
    r = torch.zeros(B, 3, T, device=dev())
    r[:, 0] = 1.0 + 0.01 * (x[:, 0, :, 2, 3] - 127.5) + 0.005 * (x[:, 0, :, 2, 4] - 127.5)
    r[:, 1] = 2.0
    r[:, 2] = 1.5
    r0 = torch.tensor([1.0, 2.0, 0.0], device=dev())
    window = (0, 0, gh, gw)
    state = torch.zeros(ops.sta_state_numel(3, L, window, 1), dtype=torch.float64, device=dev())
    K = ops.sta_accumulate(state, x, r, lags=L, window=window, skip=0, s0=127.5, r0=r0)
    cov, z, summary = compare_finalize("special", state, K, 3, L, gh, gw, window, 1, skip_summary=(2,))
    print("special summary\n", summary)
    assert K == B * (T - 2)
    assert np.all(cov[1] == 0) and np.all(z[1] == 0)
    assert summary[1, :2].tolist() == [0.0, 0.0] and np.isnan(summary[1, 2:6]).all() and summary[1, 6:].tolist() == [0.0, 0.0]
    assert np.all(z[2] == 0) and float(np.abs(cov[2]).max()) < 1e-9
    assert np.all(z[:, :, :, 8:] == 0) and np.any(z[0, :, :, :8] != 0)
    assert summary[0, 0] == 0 and summary[0, 1] > 0 and abs(summary[0, 2] - 2.0) < 0.1 and 2.9 <= summary[0, 3] <= 3.5


@pytest.mark.parametrize("kind", ["binary", "sparse"])
def test_planted_filter_end_to_end_on_the_device(kind):
    """noise kernel -> torch responder on the GPU -> accumulate in 16 calls -> finalise: the condition of the issue (peak lag 2,
    cosine >= 0.9, centre within 0.25 cell of (3, 7)), and the summary equal to the checker's on the same state."""
    from sensorium_amd import NoiseStimulus, StaAccumulator
    p = PLANTED
    f = rf.planted_filter(p["gh"], p["gw"])
    ft = torch.from_numpy(f).to(dev())
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
    torch.cuda.synchronize()
    cov, z, summary = compare_finalize(f"planted {kind}", acc.state, acc.samples, 1, p["L"], p["gh"], p["gw"], (0, 0, p["gh"], p["gw"]), 1)
    assert np.array_equal(got.sta.cpu().numpy().astype(np.float64), cov) and got.samples == 6144
    cos, lag, cy, cx = planted_condition(cov, summary, f)
    print(f"planted filter on the device ({kind}): K {acc.samples}, cosine {cos:.3f}, peak lag {lag}, centre ({cy:.2f}, {cx:.2f}), "
          f"peak z {summary[0, 1]:.1f}, polarity {got.polarity.tolist()}")
    assert lag == 2 == int(got.peak_lag[0]) and cos >= 0.9 and abs(cy - 3.0) <= 0.25 and abs(cx - 7.0) <= 0.25
    assert got.polarity.tolist() == [1.0] and got.significant(5.0).tolist() == [0]
    assert torch.allclose(got.centres("input"), got.centres("cells"))          # cell 1, window at the origin: pixels are cells


# ------------------------------------------------------------------------------------------------------------------ determinism
def rf_digest():
    """(number of tensors, sha256) over the noise of every geometry and kind, and the state, cov, z and summary of two cases."""
    from sensorium_amd import ops
    h, n = hashlib.sha256(), 0
    for name, g in GEOMS.items():
        for kind in ("binary", "sparse"):
            h.update(device_noise(kind, **g).cpu().numpy().tobytes()); n += 1
    for name in ("n70-g65-c1-k15", "n33-g35-c2-k70"):
        c = make_case(name, exact=False, seed=7)
        state, K = device_accumulate(c, [(0, 2), (2, c["B"])])
        outs = ops.sta_finalize(state, K, N=c["N"], lags=c["L"], window=c["window"], cell=c["cell"])
        torch.cuda.synchronize()
        for t in (state, *outs):
            h.update(t.cpu().numpy().tobytes()); n += 1
    return n, h.hexdigest()

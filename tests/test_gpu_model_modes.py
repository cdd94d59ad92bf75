"""Population modes from the accumulators up: planted shared noise modes through PairwiseCorrelation and
CorrelationMatrices.modes, held to eigh of the same state at the bounds of tests/modes_reference.py; compare_modes against an
accumulator that lacks one of the modes; and the tiny model behind Predictor through population_structure, whose noise state is
exact zeros."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests import modes_reference as ref  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

pytestmark = pytest.mark.gpu
N, FRAMES, GROUPS, REPEATS = 130, 40, 4, 6
AMPLITUDES = (3.0, 2.0, 1.5)


def planted_trials(n_modes, seed=21):
    """[(responses [N, FRAMES] fp32, group)]: a per-video signal, ``n_modes`` shared noise sources along fixed orthonormal
    directions and a small private noise.  The random draws do not depend on ``n_modes``."""
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.normal(size=(N, len(AMPLITUDES))))
    out = []
    for g in range(GROUPS):
        signal = rng.gamma(2.0, 1.0, size=(N, FRAMES))
        for _ in range(REPEATS):
            z = rng.normal(size=(len(AMPLITUDES), FRAMES)) * np.array(AMPLITUDES)[:, None]
            private = 0.1 * rng.normal(size=(N, FRAMES))
            out.append(((signal + U[:, :n_modes] @ z[:n_modes] + private).astype(np.float32), g))
    return out


def accumulate(trials):
    from sensorium_amd.population import PairwiseCorrelation
    acc = PairwiseCorrelation(N, dev(), kinds=("noise",))
    for y, g in trials:
        acc.add(torch.from_numpy(y).to(dev()), group=g)
    return acc.compute()


def subspace_sine(A, vectors, k):
    lam, E = np.linalg.eigh(A)
    Ek = E[:, ::-1][:, :k]
    return np.linalg.norm(vectors - Ek @ (Ek.T @ vectors), 2), Ek


def test_planted_noise_modes_and_a_model_that_lacks_one():
    from sensorium_amd.population import compare_modes
    k, p = 3, 11
    full, lacking = accumulate(planted_trials(3)), accumulate(planted_trials(2))
    sides = []
    for name, cm in (("data", full), ("model", lacking)):
        m = cm.modes("noise", of="covariance", k=k)
        A = cm.comoments("noise").cpu().numpy() / cm.counts["noise"]
        assert np.array_equal(A, A.T)
        values, vectors, residuals = (t.cpu().numpy() for t in (m.values, m.vectors, m.residuals))
        ratios = ref.check_pairs(A, values, vectors, residuals, k, p, name == "data", name)
        s = m.summary()
        print(f"{name}: values {values}, rounds {s['rounds']}, participation ratio {s['participation_ratio']:.3f}, ratios "
              f"{({a: float(f'{b:.3g}') for a, b in ratios.items()})}")
        assert s["converged"] == (name == "data")               # the model's third mode lies in the private noise: no gap, no stop
        sine, Ek = subspace_sine(A, vectors, k)
        sides.append((m, A, vectors, sine, Ek))
    (mb, B, Vb, sine_b, Eb), (ma, _, Va, sine_a, Ea) = sides
    # the three planted variances stand out of the private noise in the data
    assert mb.values[2] > 20 * 0.01 * 2 and float(mb.explained().sum()) > 0.9
    cmp_ = compare_modes(ma, mb, full.comoments("noise"), 1.0 / full.counts["noise"])
    got = cmp_.cosines.cpu().numpy()
    assert (np.abs(got - ref.cosines(Va, Vb)) <= 2 * ref.cosine_bound(ref.cosines(Va, Vb), N, k)).all()
    want = ref.cosines(Ea, Eb)                                  # the checker's own claim, from eigh of both states
    print(f"cosines {got}, from eigh {want}; sines to eigh's subspaces {sine_a:.2e} {sine_b:.2e}")
    assert (np.abs(got[:2] - want[:2]) <= 2 * (ref.cosine_bound(want, N, k)[:2] + sine_b) + 1e-6).all()
    assert want[0] > 0.99 and want[1] > 0.99 and want[2] < 0.5                         # two modes shared, the third is not there:
    assert got[0] > 0.99 and got[1] > 0.99 and got[2] < 0.5                            # the same cut on the device's numbers
    share, bound = ref.captured(Va, B)
    s = cmp_.summary()
    assert abs(s["captured"] - share) <= 2 * bound and abs(s["own"] - float(mb.values.sum() / mb.trace)) <= 1e-15
    assert s["captured"] < s["own"] and set(s) == {"k", "max_cosine", "min_cosine", "own", "captured"}
    # the time courses of the modes: plain torch
    y = torch.from_numpy(planted_trials(3)[0][0]).to(dev())
    tc = mb.project(y, full.mean("noise"))
    assert tc.shape == (k, FRAMES) and tc.dtype == torch.float64
    # the correlation matrix goes the same way
    mc = full.modes("noise", k=2, oversample=6)
    R = full.noise.cpu().numpy()
    ref.check_pairs(R, mc.values.cpu().numpy(), mc.vectors.cpu().numpy(), mc.residuals.cpu().numpy(), 2, 8, False, "correlation")


def test_tiny_model_end_to_end():
    from sensorium_amd import population_structure
    from sensorium_amd.evaluation import FrameCut
    from sensorium_amd.population import compare_modes
    from tests.test_gpu_model_trial_score import MOUSE, predictor, trials_with_repeats
    pred = predictor("single", False)
    trials = trials_with_repeats((20, 22, 37, 22), (3, 1, 2, 1), seed=40)
    model, data, _ = population_structure(pred, trials, MOUSE, cut=FrameCut(5, None, 1))
    n = model.signal.shape[0]
    # a deterministic model has no noise: exact zeros in, exact zeros out, converged, nothing NaN
    zero = model.modes("noise", of="covariance", k=3)
    assert int(torch.count_nonzero(model.comoments("noise"))) == 0
    assert int(torch.count_nonzero(zero.values)) == 0 and int(torch.count_nonzero(zero.vectors)) == 0
    assert bool(zero.converged) and int(torch.count_nonzero(zero.residuals)) == 0 and float(zero.trace) == 0.0
    for side, kind in ((data, "noise"), (data, "signal"), (model, "signal")):
        m = side.modes(kind, of="covariance", k=3)
        A = side.comoments(kind).cpu().numpy() / side.counts[kind]
        ref.check_pairs(A, m.values.cpu().numpy(), m.vectors.cpu().numpy(), m.residuals.cpu().numpy(), 3, min(11, n), False, kind)
        assert bool(m.converged)
    a, b = model.modes("signal", k=3), data.modes("signal", k=3)
    s = compare_modes(a, b, data.signal).summary()
    assert 0.0 <= s["min_cosine"] <= s["max_cosine"] <= 1.0 + 1e-12 and 0.0 < s["captured"] <= s["own"] + 1e-12

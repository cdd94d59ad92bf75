"""Synthetic trials shared by the trial-score tests (imported only by tests): built here because tests/test_gpu_trial_score.py
runs them on the device and tests/test_trial_score_reference_cpu.py checks on the CPU that the generators have the properties
the GPU tests rely on.  A case is a list of trials ``(P, Y, group)``, fp32 ``[N, K]`` over the kept frames, in table order
(the trials of a group are consecutive)."""
import numpy as np

TILE = 4                                   # DWN_TRIAL_TILE: neurons per workgroup
NS = (1, TILE - 1, TILE, TILE + 1, 64, 67)
KS = (1, 63, 64, 65, 249)
RS = (1, 2, 3, 10)
FEV_THRESHOLD = 0.15
FEV_TARGETS = (0.12, 0.13, 0.17, 0.2, 0.4, 0.7, 0.9)


def random_case(seed, N, units, offset=0.0):
    """units: [(R, K), ...].  Y = signal of the video + noise, P = a scaled signal + its own noise (responses about 0 .. 10)."""
    rng = np.random.default_rng(seed)
    trials = []
    for g, (R, K) in enumerate(units):
        s = rng.gamma(2.0, 1.0, size=(N, K))
        for _ in range(R):
            y = s + rng.normal(size=(N, K)) * 0.8
            p = 0.7 * s + 0.5 + rng.normal(size=(N, K)) * 0.3
            trials.append(((p + offset).astype(np.float32), (y + offset).astype(np.float32), g if R > 1 else None))
    return trials


def shape_case(N, K, R, seed=0):
    """Two units of R repeats around a single trial; R = 1: three single trials."""
    return random_case(seed + 1000 * N + 10 * K + R, N, [(R, K), (1, K), (R, K)])


def mixed_case(N=67, seed=5):
    """Groups of different R and K and ungrouped trials, in one table."""
    return random_case(seed, N, [(3, 65), (1, 249), (2, 1), (1, 63), (10, 64), (1, 1), (4, 130)])


def hard_case(N=5, seed=7):
    """Values 10^6 + k / 16, k integer: exactly representable in fp32, and a raw sum of squares (10^12 per term, spacing 2^-13 in
    float64) would lose what a centred sum keeps (deviations of a few units, exact)."""
    rng = np.random.default_rng(seed)
    trials = []
    for g, (R, K) in enumerate([(3, 65), (1, 249), (2, 64)]):
        s = rng.integers(0, 128, size=(N, K))
        for _ in range(R):
            y = 1e6 + (s + rng.integers(0, 64, size=(N, K))) / 16.0
            p = 1e6 + (s + rng.integers(0, 32, size=(N, K))) / 16.0
            trials.append((p.astype(np.float32), y.astype(np.float32), g if R > 1 else None))
    for p, y, _ in trials:
        assert np.array_equal(p.astype(np.float64) * 16, np.round(p.astype(np.float64) * 16)) and p.min() >= 1e6
    return trials


def exact_case(N=5, seed=11):
    """Small integers, R = 2 and counts that are powers of two after every merge (128, 256, 512, 1024): every mean is a dyadic
    rational and every moment an exactly representable number, whatever the order of summation."""
    rng = np.random.default_rng(seed)
    trials = []
    for g, (R, K) in enumerate([(2, 64), (2, 64), (1, 256), (1, 512)]):
        for _ in range(R):
            trials.append((rng.integers(0, 16, size=(N, K)).astype(np.float32), rng.integers(0, 16, size=(N, K)).astype(np.float32),
                           g if R > 1 else None))
    return trials


def fev_case(N=67, seed=13):
    """Repeat groups whose per-neuron noise amplitude is solved for (in float64, before rounding to fp32) so that neuron j's fev is
    FEV_TARGETS[j % 7]: no fev near the threshold, none below 0.1.  Y = s + c_j e; NV = c^2 NV_e and
    TV = Var(s) + 2 c Cov(s, e) + c^2 Var(e) are quadratics in c, and fev = f is (1 - f) TV = NV."""
    rng = np.random.default_rng(seed)
    units = [(3, 65), (2, 64), (5, 63), (3, 64)]
    S = [rng.gamma(2.0, 1.0, size=(N, K)) for _, K in units]
    E = [rng.normal(size=(R, N, K)) for R, K in units]
    s_all = np.concatenate([np.tile(s, (1, R)) for s, (R, _) in zip(S, units)], axis=1)                    # [N, n]
    e_all = np.concatenate([np.concatenate(list(e), axis=1) for e in E], axis=1)
    n = s_all.shape[1]
    Vs, Ve = s_all.var(axis=1, ddof=1), e_all.var(axis=1, ddof=1)
    Cov = ((s_all - s_all.mean(1, keepdims=True)) * (e_all - e_all.mean(1, keepdims=True))).sum(1) / (n - 1)
    NVe = np.concatenate([e.var(axis=0, ddof=1) for e in E], axis=1).mean(axis=1)
    f = np.array([FEV_TARGETS[j % len(FEV_TARGETS)] for j in range(N)])
    a, b, c0 = NVe - (1 - f) * Ve, -2 * (1 - f) * Cov, -(1 - f) * Vs
    c = (-b + np.sqrt(b * b - 4 * a * c0)) / (2 * a)
    assert (a > 0).all() and (c > 0).all()
    trials = []
    for g, (s, e) in enumerate(zip(S, E)):
        for r in range(e.shape[0]):
            y = s + c[:, None] * e[r]
            p = 0.8 * s + 0.3 + rng.normal(size=s.shape) * 0.4
            trials.append((p.astype(np.float32), y.astype(np.float32), g))
    return trials, f

"""Generators of the population-structure cases shared by the CPU and the GPU tests.  A case is a list of trials
``(Y, group)``: fp32 ``[N, K]`` responses over the kept frames and a group id or None, in the order they are added."""
import numpy as np

CONSTANT, OFFSET = 1, 2          # in the mixed case: a constant neuron, and one at mean = 1e4 sigma (when N allows)


def shape_case(N, K, groups, repeats=2, seed=0):
    """``groups`` repeat groups of ``repeats`` trials of K frames: a shared signal per group plus noise per trial."""
    rng = np.random.default_rng(seed + 1000 * N + 10 * K + groups)
    out = []
    for g in range(groups):
        s = rng.gamma(2.0, 1.0, size=(N, K)) + g
        out.extend(((s + 0.5 * rng.normal(size=(N, K))).astype(np.float32), f"g{g}") for _ in range(repeats))
    return out


def mixed_case(N=23, K=9, seed=1):
    """Groups of 2, 3 and 5 repeats mixed with single trials (one of them under a group id nobody else carries), the trials of the
    3-group not adjacent, lengths that differ between units; a constant neuron and a neuron at mean = 1e4 sigma."""
    rng = np.random.default_rng(seed)
    lengths = {"a": K, "b": K + 2, "c": max(K - 1, 1)}
    sig = {k: rng.gamma(2.0, 1.0, size=(N, L)) for k, L in lengths.items()}
    mix = rng.normal(size=(N, N)) / np.sqrt(N)

    def trial(key, L=None):
        base = sig[key] if key in sig else rng.gamma(2.0, 1.0, size=(N, L))
        y = base + 0.6 * (mix @ rng.normal(size=base.shape))
        if N > OFFSET:
            y[OFFSET] = 1e4 + rng.normal(size=base.shape[1])
        if N > CONSTANT:
            y[CONSTANT] = 3.25
        return y.astype(np.float32)
    plan = [("a", "a"), (None, K + 1), ("b", "b"), ("a", "a"), ("c", "c"), ("b", "b"), ("lonely", K + 3), ("c", "c"), ("b", "b"),
            ("c", "c"), (None, K), ("c", "c"), ("c", "c")]
    return [(trial(key, L) if key in sig else trial("-", L), key) for key, L in plan]


def _with_mean(rng, N, k, m):
    """integer [N, k] whose row means are exactly the integers m [N]"""
    x = rng.integers(-6, 7, size=(N, k)).astype(np.int64)
    x[:, -1] += m * k - x.sum(axis=1)
    return x


def integer_case(N, K=8, groups=3, repeats=2, equal_means=True, seed=5):
    """Exact-integer data on which every operation of the kernels is exact: small integers, every trial's mean over frames an
    integer, every repeat average an integer array whose mean is an integer (the noise residuals are then integers of mean 0).
    ``equal_means``: every chunk of every kind has mean m_i = i % 5 - 2, so every merge column is an exact zero.  Otherwise the
    group means differ by even integers: exact for the SIGNAL set of two groups of K = 8 frames (n_a = n_b = 8: the merge
    coefficient is sqrt(4) = 2 and the mean moves by half an even integer) and for the noise set; the total set of such a case
    is not exact (its third chunk meets n_a = 16) and is left to ``integer_pair_case``.  All rows differ."""
    rng = np.random.default_rng(seed + N)
    base = (np.arange(N) % 5 - 2).astype(np.int64)
    out = []
    for g in range(groups):
        m = base if equal_means else base + 2 * g * (1 + np.arange(N) % 3)
        ybar = _with_mean(rng, N, K, m)
        parts = [_with_mean(rng, N, K, m) for _ in range(repeats - 1)]
        parts.append(repeats * ybar - sum(parts))                      # the repeats average to ybar exactly
        out.extend((p.astype(np.float32), f"g{g}") for p in parts)
    for y, _ in out:
        assert np.abs(y).max() < 2 ** 20 and np.array_equal(y, np.round(y))
    return out


def integer_pair_case(N, K=8, seed=6):
    """Two single trials of K = 8 integer frames whose integer means differ by an even integer: the TOTAL set's one merge has
    n_a = n_b = 8, coefficient 2, every operation exact."""
    rng = np.random.default_rng(seed + N)
    base = (np.arange(N) % 5 - 2).astype(np.int64)
    return [(_with_mean(rng, N, K, base).astype(np.float32), None),
            (_with_mean(rng, N, K, base + 2 * (1 + np.arange(N) % 3)).astype(np.float32), None)]


def planted_case(N=12, K=40, groups=3, repeats=4, seed=9):
    """Targets from two latent signals (neurons [0, N/2) follow the first, the rest the second) and ONE noise source shared by
    all neurons of a trial's frame.  Returns (trials, block labels [N])."""
    rng = np.random.default_rng(seed)
    block = (np.arange(N) >= N // 2).astype(int)
    gain = 1.0 + 0.2 * rng.random(N)
    out = []
    for g in range(groups):
        latent = rng.normal(size=(2, K))
        for _ in range(repeats):
            shared = rng.normal(size=K)
            y = 5.0 + gain[:, None] * latent[block] + 0.8 * shared[None] + 0.1 * rng.normal(size=(N, K))
            out.append((y.astype(np.float32), f"v{g}"))
    return out, block

"""The checker of the population modes (tests/modes_reference.py) against numpy.linalg.eigh, on every case of the GPU tests: its
restated iteration must satisfy the bounds the GPU is held to, must stop within half of the rounds the GPU is given wherever the
GPU test asserts `converged`, and the bounds must catch the mistakes a kernel could make.  No device."""
import numpy as np
import pytest

from tests import modes_reference as ref
from tests import rf_reference as rf


def test_start_block_is_philox_word_by_word():
    Q = ref.start_block(9, 7, seed=(5 << 32) | 3)
    for i, c in ((0, 0), (8, 6), (3, 5), (4, 3)):
        w = rf.philox_scalar((i, c >> 2, 0, 0), (3, 5))[c & 3]
        assert Q[i, c] == (w + 0.5) * 2.0 ** -31 - 1.0
    assert np.abs(Q).max() < 1 and not np.array_equal(Q, ref.start_block(9, 7, seed=1))
    assert np.array_equal(ref.start_block(9, 7, 4)[:5, :3], ref.start_block(5, 3, 4))           # a function of (seed, row, column)


@pytest.mark.parametrize("case", ref.SOLVE_CASES, ids=[c[0] for c in ref.SOLVE_CASES])
def test_restated_iteration_meets_the_bounds_and_stops_in_half_the_rounds(case):
    name, N, build, k, oversample, gapped, converges = case
    A = build()
    assert np.array_equal(A, A.T)
    res = ref.iterate(A, k, oversample, ref.MAX_ITERS, ref.TOL)
    p = min(k + oversample, N)
    ratios = ref.check_pairs(A, res["values"], res["vectors"], res["residuals"], k, p, gapped, name)
    print(f"{name}: rounds {res['rounds']}, ratios to the single bounds {({a: float(f'{b:.3g}') for a, b in ratios.items()})}")
    if converges:
        assert res["converged"] and res["rounds"] <= ref.MAX_ITERS // 2, f"{name}: {res['rounds']} rounds"
    lam = np.linalg.eigvalsh(A)[::-1]
    assert np.abs(res["values"] - lam[:k]).max() <= 1e-8 * max(1.0, lam[0])


def test_rank_deficient_modes_are_exact_zeros():
    A = ref.SOLVE_CASES[[c[0] for c in ref.SOLVE_CASES].index("rank3-40")][2]()
    res = ref.iterate(A, 5, 8, ref.MAX_ITERS, ref.TOL)
    assert (res["values"][3:] == 0).all() and (res["vectors"][:, 3:] == 0).all() and res["converged"]
    Z = ref.iterate(np.zeros((12, 12)), 3, 8)
    assert Z["converged"] and (Z["values"] == 0).all() and (Z["vectors"] == 0).all() and Z["rounds"] == 1


def test_nan_gives_nan_and_stops():
    A = ref.planted(17, ref.GAPPED, 3)
    A[2, 5] = A[5, 2] = np.nan
    res = ref.iterate(A, 3, 8)
    assert not res["converged"] and np.isnan(res["values"]).all()


def test_orth_bound_and_drop_rule():
    rng = np.random.default_rng(5)
    for N, p in ((17, 16), (130, 24), (65, 64)):
        Y = rng.normal(size=(N, p)) * np.logspace(0, -6, p)
        Q = ref.orth(Y)
        assert np.abs(Q.T @ Q - np.eye(p)).max() <= 2 * ref.orth_bound(N, p)
    Y = rng.normal(size=(40, 6))
    Y[:, 3] = Y[:, 0] - 2 * Y[:, 1]
    Q = ref.orth(Y)
    assert (Q[:, 3] == 0).all() and np.abs(Q[:, [0, 1, 2, 4, 5]].T @ Q[:, [0, 1, 2, 4, 5]] - np.eye(5)).max() <= 2 * ref.orth_bound(40, 6)


def test_bounds_catch_the_mutations():
    for N, p in ((17, 16), (65, 17), (130, 32)):
        store, Q, scale = ref.lane_pin_operands(N, p, 3, -2, seed=N + p)
        A = store[:, :N]
        want = scale * (A @ Q)
        for name, Y in ref.symm_mutants(A, Q, scale).items():
            assert not np.array_equal(Y, want), f"lane pin misses {name} at N = {N}, p = {p}"
            assert (np.abs(Y - want) > 2 * ref.symm_bound(A, Q, scale)).any(), name
    A = ref.planted(65, ref.GAPPED, 165)
    for mutate in ("raw_residual", "unsorted", "no_scale"):
        res = ref.iterate(A, 6, 10, 8, ref.TOL, scale=0.5, mutate=mutate)
        with pytest.raises(AssertionError):
            ref.check_pairs(0.5 * A, res["values"], res["vectors"], res["residuals"], 6, 16, True, mutate)


def test_overlap_claims():
    rng = np.random.default_rng(9)
    E, _ = np.linalg.qr(rng.normal(size=(40, 40)))
    phi = np.array([0.1, 0.7, 1.3])
    Va, Vb = E[:, :3], E[:, :3] * np.cos(phi) + E[:, 3:6] * np.sin(phi)
    assert np.abs(ref.cosines(Va, Vb) - np.sort(np.cos(phi))[::-1]).max() < 1e-14
    B = ref.planted(40, ref.GAPPED, 2)
    lam, F = np.linalg.eigh(B)
    share, bound = ref.captured(F[:, -3:], B, 0.25)
    assert abs(share - lam[-3:].sum() / lam.sum()) <= bound + 1e-15

"""CPU tests that hold the checker tests/pairwise_reference.py itself: against ``numpy.cov`` /
``numpy.corrcoef`` on well-conditioned data and against a brute-force triple loop; that a float64 emulation of the kernels' chunked
path stays inside the derived bounds while the mistakes the GPU tests must catch fall outside them; and that the generators of
tests/pairwise_cases.py have the properties the GPU tests rely on."""
import numpy as np
import pytest

from tests import pairwise_cases as pc
from tests import pairwise_reference as ref


def test_sample_sets_and_counts():
    trials = pc.mixed_case(N=7, K=6)
    sets = ref.sample_sets(trials)
    lengths = {"a": 6, "b": 8, "c": 5}
    assert sets["total"].shape == (7, sum(y.shape[1] for y, _ in trials))
    assert sets["signal"].shape == (7, sum(lengths.values()))                      # 'lonely' is no group
    assert sets["noise"].shape == (7, 2 * 6 + 3 * 8 + 5 * 5)
    # the residuals of a group average to zero over its repeats, frame by frame
    assert np.abs(np.asarray(sets["noise"][:, :12], dtype=np.float64).reshape(7, 2, 6).sum(axis=1)).max() < 1e-12
    for kind in ref.KINDS:
        n, G, n_src, Rmax, A = ref.set_stats(trials, kind)
        assert n == sets[kind].shape[1] and A.shape == (7,)
        assert (G, Rmax) == {"total": (13, 1), "signal": (3, 5), "noise": (3, 5)}[kind]


def test_checker_is_numpy_cov_and_corrcoef_and_the_triple_loop():
    rng = np.random.default_rng(3)
    trials = pc.shape_case(6, 11, 3, repeats=3)
    for kind in ref.KINDS:
        X = ref.sample_sets(trials)[kind]
        n = X.shape[1]
        m, C = ref.comoments(X)
        Xd = np.asarray(X, dtype=np.float64)
        np.testing.assert_allclose(np.asarray(C, dtype=np.float64) / n, np.cov(Xd, bias=True), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(ref.corr_matrix(C, n, eps=1e-300), np.corrcoef(Xd), rtol=0, atol=1e-12)
        ml, Cl = ref.comoments_loop(Xd)
        np.testing.assert_allclose(np.asarray(m, dtype=np.float64), ml, rtol=1e-14, atol=1e-15)      # (noise: a mean of zero)
        np.testing.assert_allclose(np.asarray(C, dtype=np.float64), Cl, rtol=1e-12, atol=1e-12)
        assert np.array_equal(C, C.T)
    assert np.isnan(ref.corr_matrix(np.zeros((3, 3)), 0)).all()
    # the comparison, against numpy on the off-diagonal entries
    A, B = rng.normal(size=(9, 9)), rng.normal(size=(9, 9))
    sel = np.array([7, 0, 3, 4, 8])
    for s in (None, sel):
        per, summ = ref.compare(A, B, s, eps=1e-300)
        idx = np.arange(9) if s is None else s
        for m, i in enumerate(idx):
            others = [j for j in idx if j != i]
            assert per[m] == pytest.approx(np.corrcoef(A[i, others], B[i, others])[0, 1], abs=1e-12)
        a = np.concatenate([A[i, [j for j in idx if j != i]] for i in idx])
        b = np.concatenate([B[i, [j for j in idx if j != i]] for i in idx])
        want = [len(a), np.corrcoef(a, b)[0, 1], a.mean(), b.mean(), a.std(), b.std(), np.abs(a - b).mean(), np.sqrt(((a - b) ** 2).mean())]
        np.testing.assert_allclose(summ, want, rtol=1e-12, atol=1e-13)
    A[3, 4] = np.nan
    per, summ = ref.compare(A, B)
    assert np.isnan(per[3]) and np.isfinite(np.delete(per, 3)).all() and np.isnan(summ[1:]).all() and summ[0] == 72
    per, summ = ref.compare(A, B, np.array([2]))
    assert np.isnan(per).all() and summ[0] == 0


CASES = {"mixed": lambda: pc.mixed_case(), "shape": lambda: pc.shape_case(9, 5, 3), "one group": lambda: pc.shape_case(4, 3, 1, repeats=5),
         "long": lambda: pc.shape_case(5, 250, 2)}


@pytest.mark.parametrize("name", list(CASES))
def test_emulated_chunked_path_stays_inside_the_bounds(name):
    trials = CASES[name]()
    for kind in ref.KINDS:
        X = ref.sample_sets(trials)[kind]
        m, C = ref.comoments(X)
        Ce, me, n = ref.emulate(trials, kind)
        assert n == X.shape[1] == ref.set_stats(trials, kind)[0]
        bound = ref.comoment_bound(trials, kind, C)
        ratio = np.abs(Ce - np.asarray(C, dtype=np.float64)) / bound
        R = ref.corr_matrix(C, n)
        cb = ref.corr_bound(trials, kind, C)
        claim = np.isfinite(cb)
        rratio = np.abs(ref.corr_matrix(Ce, n) - R)[claim] / cb[claim]
        print(f"{name} {kind}: n {n}, worst |dC| / bound {np.nanmax(ratio):.3g}, worst |dr| / bound {rratio.max():.3g}")
        assert np.nanmax(ratio) <= 1.0 and rratio.max() <= 1.0
        _, G, n_src, Rmax, A = ref.set_stats(trials, kind)
        assert np.all(np.abs(me - np.asarray(m, dtype=np.float64)) <= ref.value_err(n_src, G, Rmax, A))
        if name == "mixed":
            assert not claim[pc.CONSTANT].any() and np.all(Ce[pc.CONSTANT] == 0) and np.all(Ce[:, pc.CONSTANT] == 0)


def test_several_flushes_equal_one_in_the_emulation():
    trials = pc.mixed_case()
    for kind in ref.KINDS:
        one = ref.emulate(trials, kind)
        nch = len(ref.chunks(trials, kind))
        for cuts in ((1,), (1, 2), tuple(range(1, nch))):
            many = ref.emulate(trials, kind, flush_after=cuts)
            assert np.array_equal(one[0], many[0]) and np.array_equal(one[1], many[1]) and one[2] == many[2], (kind, cuts)


def _outside(trials, kind, C_mut):
    _, C = ref.comoments(ref.sample_sets(trials)[kind])
    ratio = np.abs(C_mut - np.asarray(C, dtype=np.float64)) / ref.comoment_bound(trials, kind, C)
    return float(np.nanmax(ratio))


def test_mutations_fall_outside_twice_the_bound():
    trials = pc.mixed_case()
    # a dropped merge term
    for kind in ("total", "signal"):
        r = _outside(trials, kind, ref.emulate(trials, kind, drop_merge=True)[0])
        print(f"dropped merge term, {kind}: {r:.3g} bounds")
        assert r > 2.0
    # raw-sum products at mean = 1e4 sigma
    X = np.asarray(ref.sample_sets(trials)["total"], dtype=np.float64)
    r = _outside(trials, "total", ref.raw_sum_comoments(X))
    print(f"raw sums at mean = 1e4 sigma: {r:.3g} bounds")
    assert r > 2.0
    # noise residuals about the grand mean instead of the group mean
    r = _outside(trials, "noise", ref.emulate(trials, "noise", noise_about_grand_mean=True)[0])
    print(f"noise about the grand mean: {r:.3g} bounds")
    assert r > 2.0


def test_lane_map_mutations_fall_outside_on_integer_rows_that_all_differ():
    trials = pc.integer_case(129)
    X = np.asarray(ref.sample_sets(trials)["total"], dtype=np.float64)
    assert len({tuple(row) for row in X}) == 129                                  # all rows differ
    _, C = ref.comoments(ref.sample_sets(trials)["total"])
    C = np.asarray(C, dtype=np.float64)
    bound = ref.comoment_bound(trials, "total", C)
    assert np.array_equal(ref.emulate(trials, "total")[0], C)                      # every operation is exact
    # the right map is the identity; the f32 row map on one 16 x 16 tile (a diagonal one: the symmetry of Z Z^T does not hide it)
    for r0, c0 in ((64, 64), (80, 16)):
        tile = C[r0:r0 + 16, c0:c0 + 16]
        assert np.array_equal(ref.mfma_f64_store(tile, "f64"), tile)
        bad = C.copy()
        bad[r0:r0 + 16, c0:c0 + 16] = ref.mfma_f64_store(tile, "f32")
        wrong = np.abs(bad - C) > 2 * bound
        print(f"f32 row map on tile ({r0}, {c0}): {int(wrong.sum())} of 256 elements outside twice the bound")
        assert wrong.sum() >= 128                                                # three of every four rows are wrong rows
    # a transposed off-diagonal tile; on a diagonal tile the transpose hides (which is why the pin needs two tile rows)
    bad = C.copy()
    bad[64:128, 0:64] = C[64:128, 0:64].T
    assert (np.abs(bad - C) > 2 * bound).sum() > 2000
    diag = C.copy()
    diag[64:128, 64:128] = C[64:128, 64:128].T
    assert np.array_equal(diag, C)


def test_generators_have_the_properties_the_gpu_tests_rely_on():
    trials = pc.mixed_case()
    sizes = {}
    for _, g in trials:
        sizes[g] = sizes.get(g, 0) + 1
    assert sorted(v for k, v in sizes.items() if k not in (None, "lonely")) == [2, 3, 5] and sizes["lonely"] == 1 and sizes[None] == 2
    Y = np.concatenate([y for y, _ in trials], axis=1).astype(np.float64)
    assert np.all(Y[pc.CONSTANT] == 3.25) and 0.5e4 < Y[pc.OFFSET].mean() / Y[pc.OFFSET].std() < 2e4
    for case, kinds in ((pc.integer_case(17), ref.KINDS), (pc.integer_case(17, groups=2, equal_means=False), ("signal", "noise")),
                        (pc.integer_pair_case(17), ("total",))):
        for kind in kinds:
            m, C = ref.comoments(ref.sample_sets(case)[kind])
            Ce, me, _ = ref.emulate(case, kind)
            assert np.array_equal(Ce, np.asarray(C, dtype=np.float64)) and np.array_equal(me, np.asarray(m, dtype=np.float64))
            assert np.array_equal(C * 4, np.round(C * 4))
    Z, mean, n = ref.stage(ref.chunks(pc.integer_case(5, groups=2, equal_means=False), "signal"), np.zeros(5), 0)
    assert Z.shape == (2 * 12, 5) and n == 16 and np.all(Z[8] == 0) and np.all(Z[9:12] == 0) and np.all(Z[21:] == 0)
    assert np.array_equal(Z[20], 2.0 * 2 * (1 + np.arange(5) % 3))                # coefficient sqrt(8 * 8 / 16) = 2, exactly
    planted, block = pc.planted_case()
    sets = ref.sample_sets(planted)
    Rs = ref.corr_matrix(ref.comoments(sets["signal"])[1], sets["signal"].shape[1])
    Rn = ref.corr_matrix(ref.comoments(sets["noise"])[1], sets["noise"].shape[1])
    same = block[:, None] == block[None, :]
    assert Rs[same].min() > 0.9 and np.abs(Rs[~same]).max() < 0.6 and Rn[~np.eye(len(block), dtype=bool)].min() > 0.8

"""CPU tests that hold the float64 checker tests/trial_score_reference.py itself: to
``sensorium_amd.metrics.corr`` (pinned to the reference by tests/golden/corr.npz), ``FrameCut`` to the reference's slicing, to
cases that can be computed by hand, and to a second, loop-form statement of the repeat scores; and that confirm the generators of
tests/trial_score_cases.py have the properties the GPU tests rely on."""
import numpy as np
import pytest

from tests import trial_score_cases as tc
from tests import trial_score_reference as ref


def test_single_trial_corr_is_metrics_corr_on_the_concatenation():
    from sensorium_amd.metrics import corr
    for trials in (tc.mixed_case(N=9), tc.shape_case(5, 63, 1), tc.shape_case(4, 1, 3)):
        sc = ref.scores(trials)
        P = np.concatenate([p for p, _, _ in trials], axis=1).astype(np.float64)
        Y = np.concatenate([y for _, y, _ in trials], axis=1).astype(np.float64)
        want = corr(P, Y, axis=1)
        assert sc["n_all"] == P.shape[1]
        np.testing.assert_allclose(sc["single_trial_corr"], want, rtol=0, atol=1e-12)
        # the order of the trials does not matter to a concatenation
        back = ref.scores(trials[::-1])
        np.testing.assert_allclose(back["single_trial_corr"], want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("L", [1, 50, 51, 52, 299, 300, 301, 400])
def test_frame_cut_is_the_slicing_of_the_reference(L):
    from sensorium_amd.evaluation import FrameCut
    frames = np.arange(L)
    for cut in (FrameCut.submission(), FrameCut(), FrameCut(0, 300, 0), FrameCut(3, None, 2), FrameCut(50, 60, 1), FrameCut(0, 0, 0),
                FrameCut(1, 1000, 0)):
        want = frames[:cut.limit_length] if cut.limit_length is not None else frames
        want = want[cut.skip_first:]
        if cut.skip_last:
            want = want[:-cut.skip_last]
        assert np.array_equal(ref.frame_cut(frames, cut.skip_first, cut.limit_length, cut.skip_last), want)
        if len(want) == 0:
            with pytest.raises(ValueError, match="keeps no frame"):
                cut.bounds(L)
        else:
            start, stop = cut.bounds(L)
            assert np.array_equal(frames[start:stop], want), (cut, L)
    assert FrameCut.submission() == FrameCut(50, 300, 1)
    if L == 300:
        assert FrameCut.submission().bounds(L) == (50, 299)
    with pytest.raises(ValueError):
        FrameCut(-1)


def _t(p, y, g=None):
    return (np.array([p], dtype=np.float32), np.array([y], dtype=np.float32), g)


def test_two_repeats_by_hand():
    # target repeats [0, 2] and [2, 0]: ybar = [1, 1], within-frame variance (ddof 1) = 2 in both frames, TV = Var([0,2,2,0], ddof 1)
    # = 4/3 < NV = 2: fev and feve undefined; the leave-one-out mean is the other repeat: oracle correlation -1.
    trials = [_t([1, 3], [0, 2], "a"), _t([1, 3], [2, 0], "a")]
    sc = ref.scores(trials, eps=1e-8)
    assert (sc["n_all"], sc["n_repeat"], sc["n_group_frames"]) == (4, 4, 2)
    assert float(sc["TV"][0]) == pytest.approx(4 / 3, abs=1e-15) and float(sc["NV"][0]) == 2.0
    assert float(sc["MSE"][0]) == pytest.approx((1 + 1 + 1 + 9) / 4, abs=1e-15)
    assert np.isnan(sc["fev"][0]) and np.isnan(sc["feve"][0])
    assert sc["oracle_corr"][0] == pytest.approx(-1.0, abs=1e-7)
    assert sc["corr_to_average"][0] == 0.0                                        # ybar is constant
    assert sc["single_trial_corr"][0] == 0.0                                      # C = 0: p - 2 = (-1, 1, -1, 1), y - 1 = (-1, 1, 1, -1)
    st = ref.moments(trials)[:, 0]
    assert st.tolist() == [2, 1, 4, 4, 0, 1, 4, 12, 4, 2, 1, 2, 0, 0, 1, 4, -4]


def test_prediction_equal_to_target_and_to_the_repeat_average():
    rng = np.random.default_rng(0)
    s = rng.normal(size=(3, 40)) * 2
    ys = [(s + rng.normal(size=s.shape)).astype(np.float32) for _ in range(4)]
    same = ref.scores([(y, y, "v") for y in ys])
    np.testing.assert_allclose(same["single_trial_corr"], 1.0, atol=1e-7)
    assert np.all(same["MSE"] == 0)
    # MSE = 0: feve = 1 + NV / (TV - NV) = 1 / fev ... - : (0 - NV) / (TV - NV) = -(1 - fev) / fev
    np.testing.assert_allclose(same["feve"], 1 + (1 - same["fev"]) / same["fev"], rtol=1e-12)
    ybar = np.mean([y.astype(np.float64) for y in ys], axis=0)
    avg = ref.scores([(ybar.astype(np.float32), y, "v") for y in ys])
    np.testing.assert_allclose(avg["corr_to_average"], 1.0, atol=1e-6)
    # prediction = repeat average: MSE = (R - 1) / R * NV exactly, so feve = 1 + (NV / R) / (TV - NV), just above 1
    TV, NV, MSE = (np.asarray(avg[k], dtype=np.float64) for k in ("TV", "NV", "MSE"))
    np.testing.assert_allclose(MSE, 0.75 * NV, rtol=1e-6)
    np.testing.assert_allclose(avg["feve"], 1 + (NV / 4) / (TV - NV), rtol=1e-5)
    assert np.all(avg["feve"] > 1)


def test_constant_neuron():
    trials = tc.random_case(3, 4, [(3, 20), (1, 7), (2, 5)])
    for _, y, _ in trials:
        y[2] = 4.25
    sc = ref.scores(trials)
    assert sc["single_trial_corr"][2] == 0 and sc["corr_to_average"][2] == 0 and sc["oracle_corr"][2] == 0
    assert np.isnan(sc["fev"][2]) and np.isnan(sc["feve"][2])
    other = [0, 1, 3]
    assert np.isfinite(sc["fev"][other]).all() and (np.abs(sc["single_trial_corr"][other]) > 0.05).all()
    st = ref.moments(trials)
    assert st[1, 2] == 4.25 and st[3, 2] == 0 and st[6, 2] == 0 and st[8, 2] == 0 and st[15, 2] == 0
    assert np.isinf(ref.score_bounds(trials)["single_trial_corr"][2])            # no bound claimed: asserted exactly instead
    assert np.isfinite(ref.summary(sc)[0]) and np.isfinite(ref.summary(sc)[3])     # r = 0 counts in the mean; NaN fev is masked out


def test_loop_form_agrees_with_the_array_form():
    for trials in (tc.mixed_case(N=3), tc.shape_case(3, 1, 2), tc.shape_case(2, 65, 10), tc.hard_case(N=2)):
        a, b = ref.scores(trials), ref.scores_loop(trials)
        for k in ("corr_to_average", "fev", "feve", "oracle_corr"):
            assert np.array_equal(np.isnan(a[k]), np.isnan(b[k])), k
            ok = ~np.isnan(a[k])
            np.testing.assert_allclose(a[k][ok], b[k][ok], rtol=0, atol=2e-9 if trials[0][0].max() < 1e5 else 2e-6, err_msg=k)
    none = tc.shape_case(3, 64, 1)
    a, b = ref.scores(none), ref.scores_loop(none)
    assert (a["n_repeat"], a["n_group_frames"]) == (0, 0) and np.isfinite(a["single_trial_corr"]).all()
    for k in ("corr_to_average", "fev", "feve", "oracle_corr"):
        assert np.isnan(a[k]).all() and np.isnan(b[k]).all()
    assert np.isnan(ref.summary(a)[1:4]).all() and ref.summary(a)[4] == 0


def test_moments_are_consistent_with_the_scores_and_group_ids_seen_once_are_no_groups():
    trials = tc.mixed_case(N=6)
    st, sc = ref.moments(trials), ref.scores(trials)
    n, nr, ngf = sc["n_all"], sc["n_repeat"], sc["n_group_frames"]
    assert (n, nr, ngf) == (3 * 65 + 249 + 2 + 63 + 640 + 1 + 4 * 130, 3 * 65 + 2 + 640 + 520, 65 + 1 + 64 + 130)
    eps = 1e-8
    pear = lambda Ma, Mb, Cab, m: (Cab / m) / ((np.sqrt(Ma / m) + eps) * (np.sqrt(Mb / m) + eps))
    np.testing.assert_allclose(pear(st[2], st[3], st[4], n), sc["single_trial_corr"], atol=1e-13)
    np.testing.assert_allclose(pear(st[11], st[12], st[13], ngf), sc["corr_to_average"], atol=1e-13)
    np.testing.assert_allclose(pear(st[6], st[15], st[16], nr), sc["oracle_corr"], atol=1e-13)
    TV, NV, MSE = st[6] / (nr - 1), st[8] / ngf, st[7] / nr
    np.testing.assert_allclose((TV - NV) / TV, sc["fev"], atol=1e-13)
    np.testing.assert_allclose(1 - (MSE - NV) / (TV - NV), sc["feve"], atol=1e-12)
    assert np.array_equal(st[5], st[14]) or np.allclose(st[5], st[14], rtol=1e-15)       # mean of the leave-one-out means = mean y
    lonely = [(p, y, ("only", i) if g is None else g) for i, (p, y, g) in enumerate(trials)]
    assert np.array_equal(ref.moments(lonely), st)


def test_generators_have_the_properties_the_gpu_tests_rely_on():
    trials, f = tc.fev_case()
    sc = ref.scores(trials)
    fev, TV, NV = sc["fev"], np.asarray(sc["TV"], dtype=np.float64), np.asarray(sc["NV"], dtype=np.float64)
    assert np.isfinite(fev).all()
    assert (np.abs(fev - tc.FEV_THRESHOLD) > 1e-6).all() and (TV - NV >= 0.1 * TV).all()
    np.testing.assert_allclose(fev, f, atol=1e-5)                                  # the solve survives the rounding to fp32
    above = int((fev >= tc.FEV_THRESHOLD).sum())
    assert 0 < above < len(fev) and ref.summary(sc, tc.FEV_THRESHOLD)[4] == above
    b = ref.score_bounds(trials)
    assert np.isfinite(b["fev"]).all() and np.isfinite(b["feve"]).all() and b["fev"].max() < 1e-9 and b["feve"].max() < 1e-8
    # the exact case: every state row is the same number in float64 and in the checker's precision, whatever the summation order
    ex = tc.exact_case()
    st = ref.moments(ex)
    assert np.array_equal(st * 2.0 ** 20, np.round(st * 2.0 ** 20))
    assert np.array_equal(st, ref.moments([(p.astype(np.float64), y.astype(np.float64), g) for p, y, g in ex]))
    # the hard case: a raw sum of squares in float64 is off by more than the bound of the centred one
    hard = tc.hard_case()
    hs, hb = ref.moments(hard), ref.state_bounds(hard)
    Y = np.concatenate([y for _, y, _ in hard], axis=1).astype(np.float64)
    raw = (Y * Y).sum(axis=1) - Y.sum(axis=1) ** 2 / Y.shape[1]
    assert (np.abs(raw - hs[3]) > hb[3]).all(), (np.abs(raw - hs[3]), hb[3])
    for name, bound in ref.score_bounds(hard).items():
        if name != "kappa":
            assert np.isfinite(bound).all() and bound.max() < 1e-4, (name, bound.max())
    for name, bound in ref.score_bounds(tc.mixed_case()).items():
        if name != "kappa":
            assert np.isfinite(bound).all() and bound.max() < 1e-8, (name, bound.max())

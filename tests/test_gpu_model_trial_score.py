"""Trial-level evaluation at model level: the tiny model of tests/test_gpu_frozen_bn.py behind ``Predictor``
and ``EnsemblePredictor``, eager and with graph replay, trial lengths on both sides of a window batch.  Ground truth is the float64
checker tests/trial_score_reference.py applied to the predictions the same predictor returns as numpy, at the checker's derived
bounds.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import trial_score_reference as ref  # noqa: E402
from tests.gpu_helpers import dev, synth_inputs  # noqa: E402
from tests.test_gpu_frozen_bn import INPUT_SCALE, TINY, TINY_SD  # noqa: E402

MOUSE, N = 1, 10
STACK = dict(frame_stack_size=6, frame_stack_step=1, windows_per_batch=16)
LENGTHS = (20, 22, 37)                      # 15, 17 and 32 windows of 6 frames: below, above and twice a batch of 16


def mouse_model(seed):
    from sensorium_amd.argus_models import MouseModel
    params = {"nn_module": ("dwiseneuro", dict(TINY)), "loss": ("mice_poisson", {}), "optimizer": ("AdamW", {"lr": 1e-3}),
              "device": str(dev()), "amp": False, "iter_size": 1, "frame_stack": {"size": 6, "step": 1, "position": "last"}}
    m = MouseModel(params)
    m.nn_module.load_state_dict(orc.make_state_dict(seed=seed, randomize_bn=True, **TINY_SD), strict=True)
    return m


def video(length, seed):
    xn, _, _ = synth_inputs(np.random.default_rng(seed), 1, length, 9, 11, (1,))
    return torch.from_numpy(xn)[0] * INPUT_SCALE                      # (5, L, H, W)


def predictor(kind, graph, seeds=(3, 4)):
    from sensorium_amd.predictors import EnsemblePredictor, Predictor
    if kind == "single":
        return Predictor(mouse_model(seeds[0]), str(dev()), use_graph=graph, **STACK)
    return EnsemblePredictor([mouse_model(s) for s in seeds], str(dev()), use_graph=graph, **STACK)


def trials_with_repeats(lengths, repeats, seed):
    """[(inputs, target, group)]: video g is shown repeats[g] times; the targets are a per-video signal plus noise."""
    rng = np.random.default_rng(seed)
    out = []
    for g, (L, R) in enumerate(zip(lengths, repeats)):
        x = video(L, seed + g)
        s = rng.gamma(2.0, 1.0, size=(N, L + 3))                      # stored targets are longer than the video: the tail is cut
        for _ in range(R):
            y = (s + rng.normal(size=s.shape) * 0.5).astype(np.float32)
            out.append((x, y, f"video {g}" if R > 1 else None))
    return out


def checker_trials(pred, trials, cut):
    """(P, Y, group) over the kept frames, from the predictor's numpy predictions and the reference's slicing."""
    out = []
    for x, y, g in trials:
        p = pred.predict_trial(x, MOUSE)
        L = p.shape[1]
        out.append((ref.frame_cut(p, *cut), ref.frame_cut(y[:, :L], *cut), g))
    return out


def compare(res, want_trials, label):
    sc, bb = ref.scores(want_trials), ref.score_bounds(want_trials)
    assert (res.n_all, res.n_repeat, res.n_group_frames) == (sc["n_all"], sc["n_repeat"], sc["n_group_frames"])
    got = res.scores.cpu().numpy()
    worst = {}
    for i, name in enumerate(ref.SCORE_NAMES):
        claim = np.isfinite(bb[name])
        assert np.array_equal(np.isnan(got[i][claim]), np.isnan(sc[name][claim])), name
        ok = claim & ~np.isnan(sc[name])
        worst[name] = float((np.abs(got[i][ok] - sc[name][ok]) / bb[name][ok]).max()) if ok.any() else 0.0
    print(f"model trial_score {label}: counts {(res.n_all, res.n_repeat, res.n_group_frames)}, worst ratio to the derived bounds "
          + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    return sc, bb


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("kind", ["single", "ensemble"])
def test_device_predictions_equal_the_numpy_return_and_score_like_the_checker(kind, graph):
    from sensorium_amd.evaluation import FrameCut, evaluate_trials
    pred = predictor(kind, graph)
    for L in LENGTHS:
        x = video(L, 20 + L)
        a, b = pred.predict_trial(x, MOUSE), pred.predict_trial(x, MOUSE, to_numpy=False)
        assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == (N, L)
        assert torch.is_tensor(b) and b.is_cuda and b.dtype == torch.float32 and tuple(b.shape) == (N, L)
        assert np.array_equal(a, b.cpu().numpy()), L
    assert not graph or len(pred._graphs) == 1
    empty = pred.predict_trial(video(3, 1), MOUSE, num_neurons=N, to_numpy=False)          # shorter than a window
    assert torch.is_tensor(empty) and tuple(empty.shape) == (N, 3) and float(empty.abs().sum()) == 0
    trials = trials_with_repeats(LENGTHS + (22,), (3, 1, 2, 1), seed=40)
    cut = FrameCut(5, 30, 1)
    scorer = evaluate_trials(pred, trials, MOUSE, cut=cut)
    res = scorer.compute()
    sc, bb = compare(res, checker_trials(pred, trials, (5, 30, 1)), f"{kind} {'graph' if graph else 'eager'}")
    s, want = res.summary(), ref.summary(sc)
    assert s["n_feve_neurons"] == int(want[4]) and (s["n_all"], s["n_repeat"], s["n_group_frames"]) == (3 * 14 + 16 + 2 * 24 + 16, 90, 38)
    assert abs(s["single_trial_corr"] - want[0]) <= bb["single_trial_corr"].mean() + (N + 2) * ref.U


def test_submission_cut_equals_metrics_corr_on_the_cut_concatenation():
    from sensorium_amd.evaluation import FrameCut, evaluate_trials, summarise
    from sensorium_amd.metrics import corr
    pred = predictor("single", False)
    trials = trials_with_repeats((56, 60, 75), (1, 1, 1), seed=50)
    assert FrameCut.submission() == FrameCut(50, 300, 1)
    res = evaluate_trials(pred, trials, MOUSE).compute()                # the default cut is the submission's
    want_trials = checker_trials(pred, trials, (50, 300, 1))
    P = np.concatenate([p for p, _, _ in want_trials], axis=1).astype(np.float64)
    Y = np.concatenate([y for _, y, _ in want_trials], axis=1).astype(np.float64)
    assert P.shape == (N, 5 + 9 + 24) and res.n_all == 38 and res.n_repeat == 0
    want = corr(P, Y, axis=1)
    # the derived bound of the kernel plus the float64 sums of metrics.corr itself: three sums of n terms, (n + 16) u each
    bound = ref.score_bounds(want_trials)["single_trial_corr"] + 3 * (P.shape[1] + 16) * ref.U
    got = res.single_trial_corr.cpu().numpy()
    print(f"model trial_score submission cut: |r - corr| at most {np.abs(got - want).max():.3g}, "
          f"{(np.abs(got - want) / bound).max():.3g} of the bound; mean {got.mean():.6f}")
    assert (np.abs(got - want) <= bound).all()
    assert np.isnan(res.corr_to_average.cpu().numpy()).all() and np.isnan(res.summary()["feve"])
    out = summarise({"mouse a": res, "mouse b": res})
    assert set(out) == {"correlations", "mean_correlation"} and list(out["correlations"]) == ["mouse a", "mouse b"]
    assert abs(out["correlations"]["mouse a"] - float(want.mean())) <= bound.mean() + (N + 2) * ref.U
    assert out["mean_correlation"] == out["correlations"]["mouse a"]


def test_a_scorer_shared_by_two_fold_models_gives_the_pooled_number():
    from sensorium_amd.evaluation import FrameCut, TrialScorer, evaluate_trials
    folds = [predictor("single", False, seeds=(3,)), predictor("single", False, seeds=(4,))]
    held_out = [trials_with_repeats((20, 37), (2, 1), seed=60), trials_with_repeats((22, 25), (1, 3), seed=70)]
    held_out[1] = [(x, y, None if g is None else g + " of fold 1") for x, y, g in held_out[1]]
    cut = FrameCut(5, None, 1)
    scorer = TrialScorer(N, dev(), cut=cut)
    for p, t in zip(folds, held_out):
        assert evaluate_trials(p, t, MOUSE, scorer=scorer) is scorer
    res = scorer.compute()
    pooled = checker_trials(folds[0], held_out[0], (5, None, 1)) + checker_trials(folds[1], held_out[1], (5, None, 1))
    compare(res, pooled, "two folds")
    alone = evaluate_trials(folds[0], held_out[0], MOUSE, cut=cut).compute()
    assert res.n_all == alone.n_all + 16 + 3 * 19 and not torch.equal(res.single_trial_corr, alone.single_trial_corr)


def test_reliable_neurons_feed_the_attribution_tools_without_a_copy():
    from sensorium_amd import attribution
    from sensorium_amd.evaluation import FrameCut, TrialScorer
    rng = np.random.default_rng(5)
    scorer = TrialScorer(N, dev(), cut=FrameCut())
    s = rng.gamma(2.0, 1.0, size=(N, 40))
    noise = np.where(np.arange(N)[:, None] % 2 == 0, 0.1, 5.0)          # even neurons repeat, odd ones do not
    keep = []
    for _ in range(4):
        y = torch.from_numpy((s + rng.normal(size=s.shape) * noise).astype(np.float32)).to(dev())
        keep.append(y)
        scorer.add(y, y, group="video")
    res = scorer.compute()
    idx = res.reliable(0.5)
    print(f"model trial_score reliable: oracle_corr {np.round(res.oracle_corr.cpu().numpy(), 3).tolist()} -> neurons {idx.tolist()}")
    assert idx.tolist() == [0, 2, 4, 6, 8] and idx.is_cuda and idx.dtype == torch.int64
    assert attribution._as_index(idx, idx.device) is idx                 # taken as is: no conversion, no copy
    model = mouse_model(3).nn_module
    x = video(6, 9)[None].to(dev())
    g = attribution.input_gradient(model, x, MOUSE, neurons=idx)
    g_list = attribution.input_gradient(model, x, MOUSE, neurons=idx.tolist())
    g_all = attribution.input_gradient(model, x, MOUSE)
    assert g.shape == x.shape and float(g.abs().max()) > 0
    assert float((g - g_list).norm() / g_list.norm()) < 1e-3 and float((g - g_all).norm() / g_all.norm()) > 1e-2

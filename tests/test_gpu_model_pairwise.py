"""Population structure at model level: the tiny model of tests/test_gpu_frozen_bn.py behind ``Predictor``
and ``EnsemblePredictor``.  Ground truth is the longdouble checker tests/pairwise_reference.py applied to the predictions the same
predictor returns as numpy and to the targets, at twice the checker's derived bounds; the planted case is judged by the checker's
own numbers, not by thresholds picked in advance.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import pairwise_cases as pc  # noqa: E402
from tests import pairwise_reference as ref  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402
from tests.test_gpu_frozen_bn import TINY, TINY_SD  # noqa: E402
from tests.test_gpu_model_trial_score import MOUSE, N, STACK, predictor, trials_with_repeats, video  # noqa: E402
from tests.test_gpu_pairwise import EPS, check  # noqa: E402
from tests.trial_score_reference import frame_cut  # noqa: E402

CUT = (5, 30, 1)


def checker_sides(pred, trials, cut=CUT):
    """([(P, group)], [(Y, group)]) over the kept frames, from the predictor's numpy predictions and the reference's slicing."""
    model, data = [], []
    for x, y, g in trials:
        p = pred.predict_trial(x, MOUSE)
        L = min(p.shape[1], y.shape[1])
        model.append((frame_cut(p[:, :L], *cut), g))
        data.append((frame_cut(np.asarray(y)[:, :L], *cut), g))
    return model, data


def check_comparison(cmp_, A_trials, B_trials, kind, label):
    """per_neuron against the checker's comparison of the CHECKER's matrices, at twice the bound that carries the matrices' own
    bounds through the Pearson formula; where the checker's row has no spread (a model without noise) the kernels' 0 is exact."""
    mats, errs = [], []
    for trials in (A_trials, B_trials):
        X = ref.sample_sets(trials)[kind]
        _, C = ref.comoments(X)
        C64 = np.asarray(C, dtype=np.float64)
        mats.append(ref.corr_matrix(C, X.shape[1], EPS))
        errs.append(ref.corr_bound(trials, kind, C64, EPS))
    per, summ = ref.compare(mats[0], mats[1], None, EPS)
    errs = [np.where(np.isfinite(e), e, 0.0) for e in errs]              # a constant neuron's entries are exact zeros on both sides
    bound = ref.compare_propagated_bound(mats[0], mats[1], errs[0], errs[1], None, EPS)
    got = cmp_.per_neuron.cpu().numpy()
    claim = np.isfinite(bound)
    ratio = float((np.abs(got - per)[claim] / bound[claim]).max()) if claim.any() else 0.0
    print(f"model pairwise {label} {kind}: per-neuron similarity {np.round(got, 4).tolist()}, worst ratio to the derived bound {ratio:.3g}")
    assert ratio <= 2.0
    assert np.all(got[~claim] == 0.0) and np.all(per[~claim] == 0.0)
    s = cmp_.summary()
    assert s["pairs"] == N * (N - 1) == summ[0]
    return per


@pytest.mark.parametrize("kind,graph", [("single", False), ("single", True), ("ensemble", False)], ids=["single-eager", "single-graph", "ensemble-eager"])
def test_population_structure_matches_the_checker_on_the_read_back_predictions(kind, graph):
    from sensorium_amd import population_structure
    from sensorium_amd.evaluation import FrameCut
    pred = predictor(kind, graph)
    trials = trials_with_repeats((20, 22, 37, 22), (3, 1, 2, 1), seed=40)
    model, data, cmp_ = population_structure(pred, trials, MOUSE, cut=FrameCut(*CUT))
    want_model, want_data = checker_sides(pred, trials)
    check(want_model, model, f"{kind} {'graph' if graph else 'eager'} model")
    check(want_data, data, f"{kind} {'graph' if graph else 'eager'} data")
    assert model.counts == data.counts == {"total": 3 * 14 + 16 + 2 * 24 + 16, "signal": 38, "noise": 90}
    assert set(cmp_) == set(ref.KINDS)
    for k in ref.KINDS:
        assert getattr(model, k).is_cuda and getattr(model, k).dtype == torch.float64 and tuple(getattr(model, k).shape) == (N, N)
        check_comparison(cmp_[k], want_model, want_data, k, kind)
    # the model is deterministic given its inputs: the repeats of a video predict the same bits, its noise co-moments are exact zeros
    assert int(torch.count_nonzero(model.comoments("noise"))) == 0 and int(torch.count_nonzero(model.noise)) == 0
    assert float(data.comoments("noise").diagonal().min()) > 0
    worst = cmp_["signal"].worst(3)
    assert worst.is_cuda and worst.dtype == torch.int64 and worst.numel() == 3
    # several launches (flush_frames below one group) and a subset of kinds give the same bits
    m2, d2, c2 = population_structure(pred, trials, MOUSE, cut=FrameCut(*CUT), kinds=("signal", "total"), flush_frames=20)
    assert m2.noise is None and set(c2) == {"signal", "total"}
    for k in ("signal", "total"):
        assert torch.equal(m2.comoments(k), model.comoments(k)) and torch.equal(getattr(d2, k), getattr(data, k))
        assert torch.equal(c2[k].per_neuron, cmp_[k].per_neuron)


def behavior_predictor():
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.predictors import Predictor
    from tests.test_gpu_model_modulator import MODULATOR, randomize_heads
    params = {"nn_module": ("dwiseneuro_behavior", dict(TINY, modulator=dict(MODULATOR))), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", {"lr": 1e-3}), "device": str(dev()), "amp": False, "iter_size": 1,
              "frame_stack": {"size": 6, "step": 1, "position": "last"}}
    torch.manual_seed(29)
    m = MouseModel(params)
    m.nn_module.load_state_dict(orc.make_state_dict(seed=3, randomize_bn=True, **TINY_SD), strict=False)
    randomize_heads(m.nn_module)
    return Predictor(m, str(dev()), use_graph=False, **STACK)


def test_planted_signal_blocks_shared_noise_and_the_models_noise_through_behaviour():
    from sensorium_amd import population_structure
    from sensorium_amd.evaluation import FrameCut
    L, groups, repeats = 30, 3, 4
    planted, block = pc.planted_case(N=N, K=L, groups=groups, repeats=repeats)
    videos = [video(L, 80 + g) for g in range(groups)]
    trials = [(videos[i // repeats], y, g) for i, (y, g) in enumerate(planted)]
    pred = behavior_predictor()
    cut = FrameCut(5, None, 0)
    model, data, cmp_ = population_structure(pred, trials, MOUSE, cut=cut)
    want_model, want_data = checker_sides(pred, trials, (5, None, 0))
    check(want_data, data, "planted data")
    check(want_model, model, "planted, behaviour equal across repeats: model")
    # what the data show, by the checker's own numbers: two signal blocks, one shared noise source
    sets = ref.sample_sets(want_data)
    Rs = ref.corr_matrix(ref.comoments(sets["signal"])[1], sets["signal"].shape[1], EPS)
    Rn = ref.corr_matrix(ref.comoments(sets["noise"])[1], sets["noise"].shape[1], EPS)
    same, off = block[:, None] == block[None, :], ~np.eye(N, dtype=bool)
    got_s, got_n = data.signal.cpu().numpy(), data.noise.cpu().numpy()
    print(f"planted data: signal within blocks >= {got_s[same].min():.4f} (checker {Rs[same].min():.4f}), across <= "
          f"{np.abs(got_s[~same]).max():.4f} (checker {np.abs(Rs[~same]).max():.4f}); noise off-diagonal >= {got_n[off].min():.4f} "
          f"(checker {Rn[off].min():.4f})")
    assert Rs[same].min() > np.abs(Rs[~same]).max() and got_s[same].min() > np.abs(got_s[~same]).max()
    assert np.array_equal(got_s > np.abs(Rs[~same]).max(), same)                       # the two blocks, cut at the checker's level
    assert Rn[off].min() > 0 and got_n[off].min() > 0
    # the repeats of a video carry the same behaviour planes: the model has no noise at all
    assert int(torch.count_nonzero(model.comoments("noise"))) == 0
    check_comparison(cmp_["noise"], want_model, want_data, "noise", "planted, behaviour equal")
    # different behaviour on every repeat: the behaviour model's noise matrix is no longer zero, and is the checker's
    rng = np.random.default_rng(12)
    moved = []
    for x, y, g in trials:
        x = x.clone()
        x[1:3] = x[1:3] * torch.from_numpy(rng.uniform(0.5, 1.5, size=(2, L, 1, 1)).astype(np.float32))
        moved.append((x, y, g))
    model2, data2, cmp2 = population_structure(pred, moved, MOUSE, cut=cut)
    want_model2, want_data2 = checker_sides(pred, moved, (5, None, 0))
    check(want_model2, model2, "planted, behaviour differs across repeats: model")
    want_noise = np.asarray(ref.comoments(ref.sample_sets(want_model2)["noise"])[1], dtype=np.float64)
    got_noise = model2.comoments("noise").cpu().numpy()
    print(f"planted, behaviour differs: the model's noise co-moment diagonal lies in [{got_noise.diagonal().min():.3g}, "
          f"{got_noise.diagonal().max():.3g}] (checker [{want_noise.diagonal().min():.3g}, {want_noise.diagonal().max():.3g}])")
    assert want_noise.diagonal().min() > 0 and got_noise.diagonal().min() > 0
    assert torch.equal(data2.noise, data.noise)                                        # the data did not change
    check_comparison(cmp2["noise"], want_model2, want_data2, "noise", "planted, behaviour differs")
    check_comparison(cmp2["signal"], want_model2, want_data2, "signal", "planted, behaviour differs")

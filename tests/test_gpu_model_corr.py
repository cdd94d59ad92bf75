"""The correlation objective at loss and model level: MiceCorrelationLoss / MicePoissonCorrelationLoss against the
float64 checker tests/corr_reference.py, the tiny model's parameter gradients against oracle.dwiseneuro_oracle.forward + the checker
loss under float64 autograd, MouseModel's steps, graph capture, a short fine-tuning run and CorrelationMetric(fused=True).
Every test prints what it measured before it asserts."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import corr_reference as cr  # noqa: E402
from tests.gpu_helpers import analytically_zero_grad, dev, rel  # noqa: E402

OUTS, STRIDES = (7, 10), (2, 1, 2)
CFG = dict(readout_outputs=OUTS, core_features=(8, 8, 16), spatial_strides=STRIDES, expansion_ratio=3, se_reduce_ratio=4,
           cortex_features=(32, 64), drop_rate=0.0, drop_path_rate=0.0)          # the tiny model of smoke()
FT_LR, FT_STEPS, FT_WD, FT_MARGIN = 2e-3, 6, 0.05, 0.03


def tiny_sd():
    return orc.make_state_dict(readout_outputs=OUTS, core_features=(8, 8, 16), expansion_ratio=3, se_reduce_ratio=4,
                               cortex_features=(32, 64), seed=1, randomize_bn=True)


def tiny_inputs(B=4, seed=0):
    """smoke()'s input statistics with two samples per mouse: n = 2 x 6 values per neuron."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.normal(size=(B, 5, 6, 9, 11)).astype(np.float32) * 30 + 60)
    targets = [torch.from_numpy(np.maximum(rng.normal(size=(B, n, 6)), 0).astype(np.float32) * 10) for n in OUTS]
    w = torch.eye(2)[torch.arange(B) % 2].contiguous()
    return x, targets, w


def tiny_model(loss, opt=None, ema=None):
    from sensorium_amd.argus_models import MouseModel
    m = MouseModel({"nn_module": ("dwiseneuro", dict(CFG)), "loss": loss, "device": str(dev()), "amp": False, "iter_size": 1,
                    "optimizer": ("AdamW", dict({"lr": 1e-3, "weight_decay": 0.05}, **(opt or {})))})
    m.nn_module.load_state_dict(tiny_sd(), strict=True)
    if ema:
        m.set_ema(ema)
    return m


def oracle_step(x, targets, w, training=True, poisson_weight=0.0, correlation_weight=1.0):
    """Float64 oracle forward + checker loss under autograd: (loss, predictions, {name: grad})."""
    sd = tiny_sd()
    sdo = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and "inv_freq" not in k
               else (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}
    po = orc.forward(sdo, x.double(), strides=STRIDES, readout_outputs=OUTS, training=training)
    lo = correlation_weight * cr.torch_loss(po, targets, w)
    if poisson_weight:
        lo = lo + poisson_weight * orc.mice_poisson_loss(po, [t.double() for t in targets], w.double())
    grads = {}
    if training:
        lo.backward()
        grads = {k: v.grad for k, v in sdo.items() if v.requires_grad}
    return float(lo.detach()), [p.detach() for p in po], grads


def worst_grad_error(named, grads):
    """tests/test_gpu_model.py's rule: per parameter, norm of the difference over (norm of the reference + 1e-4 of the global
    gradient norm) — the floor is what the analytically zero BatchNorm biases (summation noise in both) are measured against."""
    gnorm = math.sqrt(sum(float((g ** 2).sum()) for g in grads.values()))
    worst = ("", 0.0)
    for k, g in grads.items():
        assert named[k].grad is not None, k
        err = float((named[k].grad.double().cpu() - g).norm()) / (float(g.norm()) + 1e-4 * gnorm)
        if err > worst[1]:
            worst = (k, err)
    return worst


# ---------------------------------------------------------------------------------------------------------------- 1. the losses
def _loss_case(n_mice, seed):
    """B = 8, one-hot owners with shares that are exact in fp32; the LAST mouse owns no row."""
    rng = np.random.default_rng(seed)
    owner = np.array([0, 1, 0, 0, 1, 0, 0, 0]) if n_mice == 3 else np.array([0, 0, 0, 0, 0, 0, 0, 0])
    sizes = (65, 9, 5)[:n_mice] if n_mice == 3 else (33, 6)
    B, T = 8, 12
    weights = np.eye(n_mice, dtype=np.float32)[owner]
    preds = [(np.abs(rng.normal(size=(B, n, T))) * 2 + 0.05).astype(np.float32) for n in sizes]
    targets = [(np.maximum(rng.normal(size=(B, n, T)), 0) * 6).astype(np.float32) for n in sizes]
    return preds, targets, weights


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("n_mice", [2, 3])
def test_correlation_loss_value_and_dpred(n_mice, reduction):
    """Value: every mouse's term is within 1 fp32 ulp of the checker's (tests/test_gpu_corr.py) and the fp32 additions over mice add
    half an ulp each: (1.5 x mice) ulp of the checker's total.  dpred: the bound of the kernel test, with g = 1."""
    from sensorium_amd import MiceCorrelationLoss
    preds, targets, weights = _loss_case(n_mice, 5 + n_mice)
    pd = [torch.from_numpy(p).to(dev()).requires_grad_(True) for p in preds]
    td = [torch.from_numpy(t).to(dev()) for t in targets]
    loss = MiceCorrelationLoss(reduction=reduction)(pd, (td, torch.from_numpy(weights).to(dev())))
    loss.backward()
    torch.cuda.synchronize()
    want = cr.loss(preds, targets, weights, reduction=reduction)
    ulps = abs(float(loss.detach()) - want) / float(cr.ulp32(want))
    print(f"{n_mice} mice, {reduction}: loss {float(loss.detach()):.7g} vs {want:.9g} ({ulps:.2f} ulp)")
    assert loss.dtype == torch.float32 and loss.dim() == 0 and ulps <= 1.5 * n_mice
    sh = cr.shares(weights)
    for m in range(n_mice):
        d_want, mag = cr.grad_term(preds[m], targets[m], weights[:, m], sh[m], 1.0, cr.EPS, reduction)
        got = pd[m].grad.cpu().numpy().astype(np.float64)
        rho = 1.0 if reduction == "sum" else 1.0 / preds[m].shape[1]
        bound = cr.ulp32(d_want) + min(1.0, sh[m] * rho) * 1e-9 * mag[None, :, None]
        err = np.abs(got - d_want.astype(np.float32).astype(np.float64))
        print(f"  mouse {m}: share {sh[m]}, dpred worst {np.max(err / cr.ulp32(d_want).clip(1e-300)):.2f} ulp")
        assert (err <= bound).all(), m
        assert not got[weights[:, m] == 0].any()
    assert not pd[-1].grad.any() and sh[-1] == 0.0                    # the absent mouse: exactly zero


def test_combined_loss_is_the_weighted_sum():
    """poisson_weight x (the Poisson kernels on the same tensors) + correlation_weight x (the checker): value within 3 fp32 ulp of the
    larger term, dpred within 2 ulp of the larger term per element plus the correlation bound (two fp32 products, one fp32 sum)."""
    from sensorium_amd import MicePoissonCorrelationLoss, MicePoissonLoss
    preds, targets, weights = _loss_case(3, 11)
    pw, cw = 0.5, 8.0
    wd = torch.from_numpy(weights).to(dev())
    td = [torch.from_numpy(t).to(dev()) for t in targets]
    pa = [torch.from_numpy(p).to(dev()).requires_grad_(True) for p in preds]
    pb = [torch.from_numpy(p).to(dev()).requires_grad_(True) for p in preds]
    both = MicePoissonCorrelationLoss(poisson_weight=pw, correlation_weight=cw)(pa, (td, wd))
    both.backward()
    pois = MicePoissonLoss()(pb, (td, wd))
    pois.backward()
    torch.cuda.synchronize()
    cterm = cr.loss(preds, targets, weights)
    want = pw * float(pois.detach()) + cw * cterm
    big = max(abs(pw * float(pois.detach())), abs(cw * cterm))
    print(f"combined {float(both.detach()):.7g} vs {want:.9g} (poisson {float(pois.detach()):.7g}, correlation {cterm:.9g})")
    assert abs(float(both.detach()) - want) <= 3 * float(cr.ulp32(big))
    sh = cr.shares(weights)
    for m in range(3):
        dc, mag = cr.grad_term(preds[m], targets[m], weights[:, m], sh[m], cw)
        dp = pw * pb[m].grad.cpu().numpy().astype(np.float64)
        want_d = dp + dc
        err = np.abs(pa[m].grad.cpu().numpy().astype(np.float64) - want_d)
        bound = 2 * cr.ulp32(np.maximum(np.abs(dp), np.abs(dc))) + cr.ulp32(dc) + cw * sh[m] / preds[m].shape[1] * 1e-9 * mag[None, :, None]
        assert (err <= bound).all(), (m, float(np.max(err - bound)))


# ------------------------------------------------------------------------------------------------------------- 2. the tiny model
def test_tiny_model_gradients_match_the_float64_oracle():
    """fp32, training mode, dense path (weights on the device without a host copy) and row-skipping path (host weights: the
    readouts' backward skips the rows of the other mouse) — both against the oracle at the suite's norm-wise 1e-3, and against each
    other (only fp32 summation order differs: 1e-4 norm-wise is 100 times what 2^-24 sqrt(terms) allows).  The analytically zero
    BatchNorm biases are summation noise in either run (two dense runs differ there as well): they are held to the oracle by the floor
    above and left out of the run-against-run comparison, as gpu_helpers.analytically_zero_grad is there for."""
    x, targets, w = tiny_inputs()
    want_loss, want_preds, grads = oracle_step(x, targets, w)
    runs = {}
    for path in ("dense", "skipping"):
        m = tiny_model(("mice_correlation", {}))
        if path == "dense":
            batch = [x.to(dev()), [[t.to(dev()) for t in targets], w.to(dev())]]
            assert m._active_samples(batch) is None
        else:
            batch = [x, [[t.clone() for t in targets], w.clone()]]
            active = m._active_samples(batch)
            assert active is not None and [a.tolist() for a in active] == [[0, 2], [1, 3]]
        out = m.train_step(batch)
        torch.cuda.synchronize()
        named = dict(m.nn_module.named_parameters())
        for k in range(2):
            assert rel(out["prediction"][k], want_preds[k]) < 1e-3
        worst = worst_grad_error(named, grads)
        print(f"{path}: loss {out['loss']:.7f} (oracle {want_loss:.7f}), worst gradient {worst[0]} {worst[1]:.2e}")
        assert abs(out["loss"] - want_loss) <= 1e-3 * max(1.0, abs(want_loss))
        assert worst[1] < 1e-3, worst
        runs[path] = {k: v.grad.detach().double().cpu() for k, v in named.items()}
    gnorm = math.sqrt(sum(float((g ** 2).sum()) for g in runs["dense"].values()))
    diffs = {k: float((runs["skipping"][k] - g).norm()) / (float(g.norm()) + 1e-4 * gnorm) for k, g in runs["dense"].items()}
    noise = max(v for k, v in diffs.items() if analytically_zero_grad(k))
    diff = max(v for k, v in diffs.items() if not analytically_zero_grad(k))
    print(f"skipping vs dense: {diff:.2e} (analytically zero gradients, not asserted: {noise:.2e})")
    assert diff < 1e-4


def test_val_step_returns_the_loss():
    x, targets, w = tiny_inputs()
    for spec, weights in ((("mice_correlation", {}), (0.0, 1.0)),
                          (("mice_poisson_correlation", {"poisson_weight": 1.0, "correlation_weight": 4.0}), (1.0, 4.0))):
        want, _, _ = oracle_step(x, targets, w, training=False, poisson_weight=weights[0], correlation_weight=weights[1])
        out = tiny_model(spec).val_step([x, [targets, w]])
        print(f"val_step {spec[0]}: loss {out['loss']:.7f} (oracle, eval mode: {want:.7f})")
        assert isinstance(out["loss"], float) and abs(out["loss"] - want) <= 1e-3 * max(1.0, abs(want))


@pytest.mark.parametrize("guarded", [False, True], ids=["fused", "guarded"])
def test_train_step_with_the_combined_loss(guarded):
    x, targets, w = tiny_inputs()
    opt = {"max_grad_norm": 1.0, "skip_nonfinite": True} if guarded else {}
    m = tiny_model(("mice_poisson_correlation", {"poisson_weight": 1.0, "correlation_weight": 4.0}), opt=opt, ema=0.9)
    lo, _, grads = oracle_step(x, targets, w, poisson_weight=1.0, correlation_weight=4.0)
    before = {k: v.detach().clone() for k, v in m.nn_module.named_parameters()}
    out = m.train_step([x, [targets, w]])
    torch.cuda.synchronize()
    worst = worst_grad_error(dict(m.nn_module.named_parameters()), grads)
    print(f"combined step ({'guarded' if guarded else 'fused'}): loss {out['loss']:.6f} (oracle {lo:.6f}), worst gradient {worst}")
    assert abs(out["loss"] - lo) <= 1e-3 * max(1.0, abs(lo)) and worst[1] < 1e-3
    assert m.get_optimizer().guarded == guarded
    if guarded:
        st = m.get_optimizer().guard_stats()
        assert not st["skipped"] and st["nonfinite"] == 0 and math.isfinite(st["norm"])
    moved = sum(int(not torch.equal(before[k], v.detach())) for k, v in m.nn_module.named_parameters())
    assert moved > len(before) // 2
    out2 = m.train_step([x, [targets, w]])
    assert math.isfinite(out2["loss"])


# ------------------------------------------------------------------------------------------------------------------- 3. capture
def test_loss_forward_and_backward_in_a_captured_graph():
    """One torch.cuda.graph around forward + backward; replayed with NEW values in the static inputs — weights and therefore shares
    and counted rows included — it returns the new values' result bit for bit: no host read-back, no scalar baked in."""
    from sensorium_amd import MiceCorrelationLoss
    loss_fn = MiceCorrelationLoss()
    first, second = _loss_case(3, 21), _loss_case(3, 22)
    second[2][:] = np.eye(3, dtype=np.float32)[np.array([2, 1, 2, 0, 1, 2, 2, 2])]        # other owners: mouse 2 present, shares change

    def eager(case):
        pd = [torch.from_numpy(p).to(dev()).requires_grad_(True) for p in case[0]]
        lo = loss_fn(pd, ([torch.from_numpy(t).to(dev()) for t in case[1]], torch.from_numpy(case[2]).to(dev())))
        lo.backward()
        return lo.detach().clone(), [p.grad.clone() for p in pd]

    sp = [torch.from_numpy(p).to(dev()).requires_grad_(True) for p in first[0]]
    st = [torch.from_numpy(t).to(dev()) for t in first[1]]
    sw = torch.from_numpy(first[2]).to(dev())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):                                             # warm-up outside the capture
            grads = torch.autograd.grad(loss_fn(sp, (st, sw)), sp)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_loss = loss_fn(sp, (st, sw))
        s_grads = torch.autograd.grad(s_loss, sp)
    for case in (second, first):
        with torch.no_grad():
            for dst, src in zip(sp, case[0]):
                dst.copy_(torch.from_numpy(src))
            for dst, src in zip(st, case[1]):
                dst.copy_(torch.from_numpy(src))
            sw.copy_(torch.from_numpy(case[2]))
        graph.replay()
        torch.cuda.synchronize()
        want_loss, want_grads = eager(case)
        print(f"replay: loss {float(s_loss.detach()):.7g}, eager {float(want_loss):.7g}")
        assert torch.equal(s_loss, want_loss)
        assert all(torch.equal(a, b) for a, b in zip(s_grads, want_grads))
    assert bool(s_grads[2].any()) is False and bool(eager(second)[1][2].any())            # (first has no row of mouse 2, second has)


# --------------------------------------------------------------------------------------------------------------- 4. fine-tuning
def test_fine_tuning_on_the_correlation_lowers_the_batch_loss():
    """A fixed batch (tiny_inputs, seed 0), the seeded tiny model, dropout and drop-path off, FT_STEPS = 6 AdamW steps at
    lr 2e-3, weight decay 0.05: the batch loss at the last step is below the first by more than FT_MARGIN = 0.03.
    The float64 oracle (oracle.forward + the checker loss + oracle.adamw_step, same seed, run on the CPU) gives
    ORACLE_LOSSES below, 1.0688 -> 0.6972: a drop of 0.3716, more than ten times the margin."""
    x, targets, w = tiny_inputs()
    m = tiny_model(("mice_correlation", {}), opt={"lr": FT_LR, "weight_decay": FT_WD})
    losses = [m.train_step([x, [targets, w]])["loss"] for _ in range(FT_STEPS)]
    print("fine-tuning losses:", " ".join(f"{v:.5f}" for v in losses), "| oracle:", " ".join(f"{v:.5f}" for v in ORACLE_LOSSES))
    assert ORACLE_LOSSES[0] - ORACLE_LOSSES[-1] >= 10 * FT_MARGIN
    assert all(math.isfinite(v) for v in losses)
    assert abs(losses[0] - ORACLE_LOSSES[0]) <= 1e-3
    assert losses[-1] < losses[0] - FT_MARGIN


ORACLE_LOSSES = (1.0688324, 0.9817775, 0.8991518, 0.8237844, 0.7567660, 0.6972361)      # float64 oracle, CPU: a drop of 0.3716


# -------------------------------------------------------------------------------------------------------------- 5. fused metric
def _metric_batches(exact=False):
    """Three uneven validation batches on two mice; the second has no sample of mouse 1.  exact: values k/16 in [0, 4) whose sums,
    sums of squares and of products are exact in float64 in ANY order, with 2 and 1 neurons (a mean over at most two values is
    order-free too): the floats of the unfused path then do not depend on the device's reduction order."""
    rng = np.random.default_rng(77)
    out = []
    for own in ([0, 1, 0], [0, 0, 0, 0, 0], [1, 0]):
        B = len(own)
        if exact:
            mk = lambda n: torch.from_numpy((rng.integers(0, 64, size=(B, n, 5)) / 16.0).astype(np.float32))
            sizes = (2, 1)
        else:
            mk = lambda n: torch.from_numpy((np.abs(rng.normal(size=(B, n, 5))) * 3 + 0.1).astype(np.float32))
            sizes = (70, 33)
        out.append(([mk(sizes[0]), mk(sizes[1])], [mk(sizes[0]), mk(sizes[1])], torch.eye(2)[torch.tensor(own)]))
    return out


def _run_metric(metric, batches):
    for p, t, w in batches:
        metric.update({"prediction": [v.to(dev()) for v in p], "target": ([v.to(dev()) for v in t], w.to(dev()))})
    return metric.compute()


def test_fused_metric_matches_the_concatenation_and_the_unfused_path():
    from sensorium_amd.metrics import CorrelationMetric, corr
    batches = _metric_batches()
    fused, plain = _run_metric(CorrelationMetric(fused=True), batches), _run_metric(CorrelationMetric(), batches)
    assert sorted(fused) == sorted(plain) == [0, 1]
    for k in range(2):
        allp = np.concatenate([b[0][k].numpy() for b in batches]).astype(np.float64)
        allt = np.concatenate([b[1][k].numpy() for b in batches]).astype(np.float64)
        allw = np.concatenate([b[2][:, k].numpy() for b in batches])
        want = float(corr(*cr.select_rows(allp, allt, allw), axis=0).mean())
        print(f"mouse {k}: fused {fused[k]!r}, unfused {plain[k]!r}, corr of the concatenation {want!r}")
        assert abs(fused[k] - want) <= 1e-10 and abs(fused[k] - plain[k]) <= 1e-9
    # a mouse never seen in the epoch is left out, as in the unfused path; reset clears the running moments
    m = CorrelationMetric(fused=True)
    assert sorted(_run_metric(m, batches[1:2])) == [0]
    m.reset()
    assert m.moments == {} and m.compute() == {}


# the parent commit's sensorium_amd/metrics.py on _metric_batches(exact=True), run on an MI355X (every sum it forms is exact, so the
# values do not depend on the reduction order; on the CPU the same code gives -0.18698648291472797 and 0.10736244583103748: the
# element-wise float64 tail differs in the last digits)
PARENT_FLOATS = {0: -0.18698648291472775, 1: 0.10736244583103723}


def test_unfused_metric_gives_the_parent_commits_floats():
    from sensorium_amd.metrics import CorrelationMetric
    got = _run_metric(CorrelationMetric(), _metric_batches(exact=True))
    print("unfused metric:", got)
    assert got == PARENT_FLOATS
    fused = _run_metric(CorrelationMetric(fused=True), _metric_batches(exact=True))
    assert all(abs(fused[k] - PARENT_FLOATS[k]) <= 1e-10 for k in PARENT_FLOATS)

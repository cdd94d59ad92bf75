"""The behaviour modulator at model level: ``DwiseNeuroBehavior`` on the tiny model of
tests/test_gpu_frozen_bn.py with the inputs of tests/test_gpu_model_gaze.py (the planes of one sample made non-constant, so the
plane mean matters).  Ground truth is float64 on the CPU: plane mean -> normalise -> MLP in front of the checker
tests/modulator_reference.py's formula, applied to the oracle's predictions.  Every test prints what it measured before it asserts.
The bounds are those of tests/test_gpu_model_gaze.py for the same model: fp32 1e-3 throughout; bf16 3e-2 on predictions, 1e-1 on
parameter gradients, the measured-and-doubled input-gradient bounds of the frozen and training-mode input gradients."""
import functools
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import gaze_reference as gr  # noqa: E402
from tests.gpu_helpers import dev, rel, synth_inputs  # noqa: E402
from tests.test_gpu_frozen_bn import BF16_DX, INPUT_SCALE, TINY, sd64, tiny_model  # noqa: E402
from tests.test_gpu_model_gaze import SHIFTER, inputs  # noqa: E402
from tests.test_gpu_train_input_grad import BF16_TRAIN_DX  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
# the behaviour planes of the synthetic clips are about (30, 5) +- (10, 5), times INPUT_SCALE
MODULATOR = dict(features=4, hidden_features=8, hidden_layers=1, max_log_gain=1.5, behavior_mean=(0.3, 0.05),
                 behavior_std=(0.1, 0.05), derivative=True)
KW = dict(strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"])


def randomize_heads(model):
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for head in model.modulator.heads:
            head.weight.copy_((torch.randn(head.weight.shape, generator=g) * 0.4).to(head.weight.device))
            head.bias.copy_((torch.randn(head.bias.shape, generator=g) * 0.2).to(head.bias.device))
    return model


def behavior_model(dtype=torch.float32, randomize=True, gaze_shifter=None, **modulator):
    from sensorium_amd import DwiseNeuroBehavior
    base, sd = tiny_model(dtype)
    torch.manual_seed(29)                      # the MLP's default initialisation
    model = DwiseNeuroBehavior(compute_dtype=dtype, **TINY, gaze_shifter=gaze_shifter, modulator=dict(MODULATOR, **modulator))
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith(("modulator.", "shifter.")) for k in res.missing_keys)
    model = model.to(dev())
    return (randomize_heads(model) if randomize else model), base, sd


class Reference:
    """float64: plane mean -> normalise (-> differences) -> MLP -> h; oracle predictions times exp(m tanh(c + h u^T))."""

    def __init__(self, mod, sd, x, training, grads=True, params=None):
        self.mod = mod
        self.p = params if params is not None else {k: v.detach().double().cpu().clone().requires_grad_(True)
                                                    for k, v in mod.named_parameters()}
        self.x = x.double().clone().requires_grad_(True)
        self.sd = sd if params is not None else sd64(sd, grads=grads)
        self.training = training

    def features(self):
        mod = self.mod
        z = (gr.plane_mean(self.x, mod.behavior_channels) - mod.behavior_mean.double().cpu()) / mod.behavior_std.double().cpu()
        if mod.derivative:
            z = torch.cat([z, torch.cat([torch.zeros_like(z[:, :1]), z[:, 1:] - z[:, :-1]], dim=1)], dim=2)
        n_lin = sum(k.startswith("mlp.") for k in self.p) // 2
        for i in range(n_lin):                     # Linear -> Tanh, the last pair included
            z = torch.tanh(z @ self.p[f"mlp.{2 * i}.weight"].t() + self.p[f"mlp.{2 * i}.bias"])
        return z

    def forward(self, index=None):
        h = self.features()
        po = orc.forward(self.sd, self.x, training=self.training, **KW)
        m = self.mod.max_log_gain
        out = []
        for k, y in enumerate(po):
            a = self.p[f"heads.{k}.bias"][None, :, None] + torch.einsum("btk,nk->bnt", h, self.p[f"heads.{k}.weight"])
            out.append(y * torch.exp(m * torch.tanh(a)))
        return out if index is None else out[index]


def grad_report(tag, model, ref, dtype):
    """Worst norm-relative error over the base parameters (with the floor of tests/test_gpu_model.py for the analytically zero
    gradients) and over the modulator's parameters."""
    named = dict(model.named_parameters())
    grads = {k: v.grad for k, v in ref.sd.items() if getattr(v, "grad", None) is not None}
    grads.update({"modulator." + k: v.grad for k, v in ref.p.items()})
    assert set(grads) == set(named)
    gnorm = math.sqrt(sum(float(g.norm()) ** 2 for g in grads.values()))
    worst, worst_mod = ("", 0.0), ("", 0.0)
    for k, g in grads.items():
        assert named[k].grad is not None, k
        if k.startswith("modulator."):
            assert float(g.abs().max()) > 0, f"the reference gradient of {k} is zero"
            err = rel(named[k].grad, g)
            worst_mod = max(worst_mod, (k, err), key=lambda t: t[1])
        else:
            floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm
            err = float((named[k].grad.double().cpu() - g).norm()) / (float(g.norm()) + floor)
            worst = max(worst, (k, err), key=lambda t: t[1])
    print(f"{tag}: worst base parameter gradient {worst[0]} {worst[1]:.3e}; worst modulator gradient {worst_mod[0]} {worst_mod[1]:.3e}")
    return worst[1], worst_mod[1]


# ------------------------------------------------------------------------------------------------ 1. zero heads are the identity
def forward_with_readout_outputs(model, xd):
    """The model's outputs and, through forward hooks, what its readouts returned inside the same forward."""
    seen = []
    hooks = [r.register_forward_hook(lambda mod, args, out: seen.append(out)) for r in model.readouts]
    try:
        with torch.no_grad():
            out = model(xd)
    finally:
        for h in hooks:
            h.remove()
    return out, seen


def check_identity(tag, model, other, xd, training):
    """eval: the outputs are the other model's bit for bit.  train: the product build accumulates the BatchNorm statistics with
    atomics, so two training-mode forwards of ONE plain model already differ in the last bits; there the identity is held bit for
    bit where it is decided — the outputs against what the readouts returned in the same forward — and the other model is matched
    to within what two of its own forwards differ by (printed), bounded by 1e-5 of the norm."""
    model.train(training), other.train(training)
    a, inner = forward_with_readout_outputs(model, xd)
    with torch.no_grad():
        b = other(xd)
        again = other(xd)
    torch.cuda.synchronize()
    same_inner = len(inner) == len(a) and all(torch.equal(p, q) for p, q in zip(a, inner))
    same = all(torch.equal(p, q) for p, q in zip(a, b))
    own = max(rel(p, q) for p, q in zip(again, b))
    err = max(rel(p, q) for p, q in zip(a, b))
    print(f"{tag} training={training}: outputs equal the readouts' bit for bit: {same_inner}; equal the other model's: {same} "
          f"(rel {err:.2e}; two forwards of the other model differ by {own:.2e})")
    assert same_inner
    if training:
        assert err <= 1e-5
    else:
        assert same and own == 0.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_fresh_model_is_the_plain_model(dtype):
    x, _, _ = inputs()
    xd = x.to(dev())
    for training in (False, True):
        model, base, _ = behavior_model(dtype, randomize=False)
        check_identity(f"fresh behaviour model {dtype}", model, base, xd, training)
        with torch.no_grad():
            h = model.modulator.features(xd)
        assert h.shape == (3, 6, 4) and float(h.abs().max()) > 0.01          # the features are not zero: the heads are
        if not training:
            with torch.no_grad():
                assert torch.equal(model(xd, index=1), base(xd)[1])
            for k, v in base.state_dict().items():
                assert torch.equal(v, model.state_dict()[k]), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_fresh_model_with_fresh_shifter_is_the_gaze_model(dtype):
    from sensorium_amd import DwiseNeuroGaze
    x, _, _ = inputs()
    xd = x.to(dev())
    for training in (False, True):
        model, _, sd = behavior_model(dtype, randomize=False, gaze_shifter=dict(SHIFTER))
        torch.manual_seed(23)
        gaze = DwiseNeuroGaze(compute_dtype=dtype, **TINY, gaze_shifter=dict(SHIFTER))
        gaze.load_state_dict(sd, strict=False)
        check_identity(f"fresh behaviour model with a fresh shifter {dtype}", model, gaze.to(dev()), xd, training)


# --------------------------------------------------------------------------------- 2. / 3. gradients against the float64 chain
def _gradient_check(dtype, frozen):
    from sensorium_amd import MicePoissonLoss
    model, _, sd = behavior_model(dtype)
    x, targets, w = inputs()
    ref = Reference(model.modulator, sd, x, training=not frozen)
    po = ref.forward()
    orc.mice_poisson_loss(po, [t.double() for t in targets], w.double()).backward()
    if frozen:
        model.eval().freeze_batchnorm(True)
        before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    else:
        model.train()
    xd = x.to(dev()).requires_grad_()
    preds = model(xd)
    MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    if frozen:
        assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items()), "frozen statistics moved"
    tag = f"behaviour {'frozen' if frozen else 'train'} {dtype}"
    e_h = float((model.modulator.features(xd).detach().double().cpu() - ref.features().detach()).abs().max())
    e_pred = max(rel(p, q) for p, q in zip(preds, po))
    e_x, e_beh = rel(xd.grad, ref.x.grad), rel(xd.grad[:, 1:3], ref.x.grad[:, 1:3])
    gains = [float((p.detach().double().cpu() / q.detach()).min()) for p, q in zip(preds, orc.forward(ref.sd, ref.x, training=not frozen, **KW))]
    print(f"{tag}: |h - ref| {e_h:.2e}; predictions {e_pred:.3e}; x.grad {e_x:.3e}, behaviour planes {e_beh:.3e}; smallest gain {min(gains):.3f}")
    base_err, mod_err = grad_report(tag, model, ref, dtype)
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)
    xt = 1e-3 if dtype == torch.float32 else (BF16_DX if frozen else BF16_TRAIN_DX)["tiny"][1]
    assert min(gains) < 0.9                                    # the heads are really at work
    assert e_h < 1e-5 and e_pred < ft and e_x < xt and e_beh < xt
    assert base_err < gt and mod_err < gt


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_step_gradients_match_the_float64_chain(dtype):
    _gradient_check(dtype, frozen=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_statistics_gradients_match_the_float64_chain(dtype):
    _gradient_check(dtype, frozen=True)


# --------------------------------------------------------------------------------------------------------- 4. MouseModel steps
STEPS, LR, WD, DECAY = 6, 2e-3, 0.05, 0.9


def mouse_model(dtype, sd=None, randomize=False, opt=None, **extra):
    from sensorium_amd.argus_models import MouseModel
    params = {"nn_module": ("dwiseneuro_behavior", dict(TINY, modulator=dict(MODULATOR))), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", dict({"lr": LR, "weight_decay": WD}, **(opt or {}))), "device": str(dev()),
              "amp": dtype == torch.bfloat16, "iter_size": 1, "frame_stack": {"size": 6, "step": 1, "position": "last"}}
    params.update(extra)
    torch.manual_seed(29)
    m = MouseModel(params)
    if sd is not None:
        m.nn_module.load_state_dict(sd, strict=False)
    if randomize:
        randomize_heads(m.nn_module)
    return m


@functools.lru_cache(maxsize=None)
def chain_losses(guarded):
    """STEPS AdamW steps of the float64 chain on the fixed batch, from the state mouse_model(..., randomize=True) starts in:
    the batch loss before each step.  guarded: gradients scaled by min(1, 1 / (norm + 1e-6)) (max_grad_norm = 1)."""
    m = mouse_model(torch.float32, tiny_model()[1], randomize=True)
    mod = m.nn_module.modulator
    x, targets, w = inputs()
    sd = sd64(tiny_model()[1], grads=True)
    p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in mod.named_parameters()}
    leaves = [v for v in sd.values() if getattr(v, "requires_grad", False)] + list(p.values())
    state = [(torch.zeros_like(v), torch.zeros_like(v)) for v in leaves]
    losses = []
    for step in range(1, STEPS + 1):
        for v in leaves:
            v.grad = None
        ref = Reference(mod, sd, x, training=True, params=p)
        loss = orc.mice_poisson_loss(ref.forward(), [t.double() for t in targets], w.double())
        loss.backward()
        losses.append(float(loss.detach()))
        grads = [v.grad if v.grad is not None else torch.zeros_like(v) for v in leaves]
        coef = 1.0
        if guarded:
            norm = math.sqrt(sum(float((g ** 2).sum()) for g in grads))
            coef = min(1.0, 1.0 / (norm + 1e-6))
        with torch.no_grad():
            for i, (v, g) in enumerate(zip(leaves, grads)):
                q, mm, vv = orc.adamw_step(v.detach(), g * coef, state[i][0], state[i][1], step, LR, weight_decay=WD)
                v.copy_(q)
                state[i] = (mm, vv)
    return tuple(losses)


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_mouse_model_train_steps_and_ema(dtype, guarded):
    want = chain_losses(guarded)
    m = mouse_model(dtype, tiny_model()[1], randomize=True,
                    opt=dict(max_grad_norm=1.0, skip_nonfinite=True) if guarded else None)
    m.set_ema(DECAY)
    x, targets, w = inputs()
    batch = (x.to(dev()), ([t.to(dev()) for t in targets], w.to(dev())))
    names = [n for n, _ in m.nn_module.named_parameters() if n.startswith("modulator.heads.")]
    assert len(names) == 4
    params = dict(m.nn_module.named_parameters())
    history = [{n: params[n].detach().double().cpu().clone() for n in names}]
    losses = []
    for _ in range(STEPS):
        losses.append(m.train_step(batch)["loss"])
        history.append({n: params[n].detach().double().cpu().clone() for n in names})
    torch.cuda.synchronize()
    tag = f"behaviour train_step x{STEPS} {dtype} {'guarded' if guarded else 'plain'}"
    print(f"{tag}: losses " + " ".join(f"{v:.5f}" for v in losses) + " | float64 chain " + " ".join(f"{v:.5f}" for v in want))
    tol = 1e-3 if dtype == torch.float32 else 3e-2
    assert want[-1] < want[0] and all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0]
    for got, ref in zip(losses, want):
        assert abs(got - ref) <= tol * max(1.0, abs(ref)), (got, ref)
    assert m.optimizer.folds_ema_of(m.model_ema)
    ema = dict(m.model_ema.ema.named_parameters())
    for n in names:
        moved = float((history[-1][n] - history[0][n]).abs().max())
        e = history[0][n].clone()
        for k in range(1, STEPS + 1):
            e = DECAY * e + (1.0 - DECAY) * history[k][n]
        err = rel(ema[n], e)
        print(f"{tag} {n}: moved by {moved:.3e}; EMA against the float64 replay {err:.3e} (bound 1e-6)")
        assert moved > 0 and err <= 1e-6, n


# ------------------------------------------------------------------------------------------------- 5. checkpoint, hipGraph
def trial(length=40, seed=8):
    xn, _, _ = synth_inputs(np.random.default_rng(seed), 1, length, 9, 11, (1,))
    x = torch.from_numpy(xn)[0] * INPUT_SCALE                      # (5, L, H, W)
    x[1:, :, 1:5, 2:7] *= 1.3                                       # planes not constant over the frame
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_round_trip_and_graph_replay(dtype, tmp_path):
    from sensorium_amd.engine import load_model
    from sensorium_amd.predictors import Predictor
    a = mouse_model(dtype, tiny_model()[1], randomize=True)
    a.save(tmp_path / "behavior.pth")
    c = load_model(tmp_path / "behavior.pth", device=str(dev()))
    assert type(c.nn_module).__name__ == "DwiseNeuroBehavior"
    assert list(c.nn_module.state_dict()) == list(a.nn_module.state_dict())
    for (k, v), u in zip(a.nn_module.state_dict().items(), c.nn_module.state_dict().values()):
        assert torch.equal(v, u), k
    x = trial()                                                     # 35 windows of 6 frames: two full batches of 16 and a ragged one
    mem = Predictor(a, str(dev()), frame_stack_size=6, frame_stack_step=1, windows_per_batch=16, use_graph=False)
    graph = Predictor(str(tmp_path / "behavior.pth"), str(dev()), windows_per_batch=16, use_graph=True)
    assert (graph.frame_stack_size, graph.frame_stack_step) == (6, 1)
    p, first = mem.predict_trial(x, 1), graph.predict_trial(x, 1)
    same = np.array_equal(p, first)
    print(f"behaviour checkpoint {dtype}: prediction {p.shape}; graphs captured {len(graph._graphs)}; the replay from disk equals "
          f"the eager forward in memory: {same}")
    assert p.shape == (10, 40) and np.isfinite(p).all() and len(graph._graphs) == 1 and same
    for net in (graph.model.nn_module, a.nn_module):                # the heads changed in place: the captured graph reads them
        with torch.no_grad():
            net.modulator.heads[1].bias.add_(0.25)
            net.modulator.heads[1].weight.mul_(-1.0)
    second = graph.predict_trial(x, 1)
    assert len(graph._graphs) == 1 and not np.array_equal(first, second)
    assert np.array_equal(second, mem.predict_trial(x, 1))


# -------------------------------------------------------------------------------------------------------------- 6. attribution
@pytest.mark.parametrize("dtype", DTYPES)
def test_attribution_includes_the_path_through_the_modulator(dtype):
    from sensorium_amd import attribution
    model, _, sd = behavior_model(dtype)
    x, _, _ = inputs()
    x = x[:2]
    index, neurons = 1, torch.tensor([0, 3, 4, 9])
    ref = Reference(model.modulator, sd, x, training=False, grads=False)
    ref.forward(index=index)[:, neurons].sum().backward()
    # the same gradient with the features held constant: what reaches the behaviour planes through the core alone
    held = Reference(model.modulator, sd, x, training=False, grads=False)
    h = held.features().detach()
    held.features = lambda: h
    held.forward(index=index)[:, neurons].sum().backward()
    through = ref.x.grad[:, 1:3] - held.x.grad[:, 1:3]
    share = float(through.norm() / ref.x.grad[:, 1:3].norm())
    model.eval()
    g = attribution.input_gradient(model, x.to(dev()), index, neurons.to(dev()))
    torch.cuda.synchronize()
    e, e_beh = rel(g, ref.x.grad), rel(g[:, 1:3], ref.x.grad[:, 1:3])
    print(f"behaviour attribution {dtype}: x.grad rel err {e:.3e}, behaviour planes {e_beh:.3e}; share of the modulator path in "
          f"the behaviour planes' gradient {share:.3f}")
    assert share > 0.01
    tol = 1e-3 if dtype == torch.float32 else BF16_DX["tiny"][1]
    assert e < tol and e_beh < tol


# ------------------------------------------------------------------------------------------------------------ 7. data parallel
@pytest.mark.parametrize("mode", ["dense", "shard"])
def test_one_rank_data_parallel(mode):
    """a fresh child process per mode (nothing may touch the GPU before the process group exists): its start is most of the time"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tests" / "modulator_ddp_worker.py"), mode]
    res = subprocess.run(cmd, cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True, timeout=300)
    print(res.stdout[-600:])
    assert res.returncode == 0 and f"MODULATOR_DDP_OK mode={mode} " in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]

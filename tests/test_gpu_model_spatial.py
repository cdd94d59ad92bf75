"""The retinotopic readout gain at model level: ``DwiseNeuroSpatial`` on the tiny model of
tests/test_gpu_frozen_bn.py with the inputs of tests/test_gpu_model_gaze.py.  Ground truth is float64 on the CPU:
``oracle.core_forward`` -> the projection -> the formula of the checker tests/spatial_reference.py (with the checker's own cell
decision) applied to the oracle's pool, cortex and readout predictions; with a shifter or a modulator, the float64 chains of
tests/test_gpu_model_gaze.py and tests/test_gpu_model_modulator.py around it.  Every test prints what it measured before it
asserts.  The bounds are the standing ones of the modulator's model test: fp32 1e-3 throughout; bf16 3e-2 on predictions, 1e-1 on
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
from tests import spatial_reference as sr  # noqa: E402
from tests.gpu_helpers import dev, rel  # noqa: E402
from tests.test_gpu_frozen_bn import BF16_DX, TINY, sd64, tiny_model  # noqa: E402
from tests.test_gpu_model_gaze import SHIFTER, check_shifter_grads, inputs, randomize_last_layer  # noqa: E402
from tests.test_gpu_model_gaze import Reference as GazeReference  # noqa: E402
from tests.test_gpu_model_modulator import MODULATOR, check_identity, trial  # noqa: E402
from tests.test_gpu_model_modulator import Reference as BehaviorReference  # noqa: E402
from tests.test_gpu_model_modulator import randomize_heads as randomize_modulator_heads  # noqa: E402
from tests.test_gpu_train_input_grad import BF16_TRAIN_DX  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
SPATIAL = dict(features=4, max_log_gain=1.5, init_range=0.8, seed=3)
EXTRA = ("spatial.", "shifter.", "modulator.")


def randomize_heads(model):
    g = torch.Generator().manual_seed(37)
    with torch.no_grad():
        for head in model.spatial.heads:
            head.weight.copy_((torch.randn(head.weight.shape, generator=g) * 0.4).to(head.weight.device))
            head.bias.copy_((torch.randn(head.bias.shape, generator=g) * 0.2).to(head.bias.device))
    return model


def spatial_model(dtype=torch.float32, randomize=True, gaze_shifter=None, modulator=None, **spatial):
    from sensorium_amd import DwiseNeuroSpatial
    base, sd = tiny_model(dtype)
    torch.manual_seed(41)                      # the projection's (and the other branches') default initialisation
    model = DwiseNeuroSpatial(compute_dtype=dtype, **TINY, spatial=dict(SPATIAL, **spatial), gaze_shifter=gaze_shifter,
                              modulator=modulator)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith(EXTRA) for k in res.missing_keys)
    model = model.to(dev())
    if randomize:
        randomize_heads(model)
        if gaze_shifter is not None:
            randomize_last_layer(model)
        if modulator is not None:
            randomize_modulator_heads(model)
    return model, base, sd


def gain64(y, g, pos, weight, bias, m):
    """The checker's formula in differentiable float64 torch, with the checker's cell decision."""
    B, T, Hf, Wf, K = g.shape
    ce = sr.cells(pos.detach().numpy(), Hf, Wf)
    x0 = torch.from_numpy(ce["c"][0] % Wf).double()
    y0 = torch.from_numpy(ce["c"][0] // Wf).double()
    fx = (pos[:, 0].clamp(-1.0, 1.0) + 1.0) / 2.0 * (Wf - 1) - x0
    fy = (pos[:, 1].clamp(-1.0, 1.0) + 1.0) / 2.0 * (Hf - 1) - y0
    assert np.allclose(fx.detach().numpy(), ce["fx"]) and np.allclose(fy.detach().numpy(), ce["fy"])
    w = [(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx]
    gf = g.reshape(B, T, Hf * Wf, K)
    samp = sum(wc[None, None, :, None] * gf[:, :, torch.from_numpy(c)] for wc, c in zip(w, ce["c"]))
    a = bias[None, :, None] + torch.einsum("btnk,nk->bnt", samp, weight)
    return y * torch.exp(m * torch.tanh(a))


class Reference:
    """float64: (gaze chain ->) oracle core -> projection -> pool, cortex, readouts -> spatial gain (-> behaviour gain)."""

    def __init__(self, model, sd, x, training, grads=True, params=None, sd_leaves=None, detach=False):
        self.model, self.training, self.detach = model, training, detach
        self.p = params if params is not None else {k: v.detach().double().cpu().clone().requires_grad_(True)
                                                    for k, v in model.spatial.named_parameters()}
        self.gaze = GazeReference(model, sd, x, training, grads=grads) if hasattr(model, "shifter") else None
        if self.gaze is not None:
            self.x, self.sd = self.gaze.x, self.gaze.sd
        else:
            self.x = x.double().clone().requires_grad_(True)
            self.sd = sd_leaves if sd_leaves is not None else sd64(sd, grads=grads)
        self.beh = None
        if hasattr(model, "modulator"):
            self.beh = BehaviorReference(model.modulator, sd, x, training, grads=False)
            self.beh.x = self.x

    def forward(self, index=None, plain=False):
        xin = self.x if self.gaze is None else self.gaze.xs
        cmap = orc.core_forward(xin.permute(0, 2, 3, 4, 1), self.sd, TINY["spatial_strides"], self.training, None, None)
        feats = cmap.mean(dim=(2, 3))
        for i in range(orc.config_from_state_dict(self.sd)["n_cortex"]):
            feats = orc.cortex_layer(feats, f"cortex.layers.{i}", self.sd, 2, self.training, None, None)
        src = cmap.detach() if self.detach else cmap
        g = src @ self.p["project.weight"].t() if "project.weight" in self.p else src
        h = None if self.beh is None else self.beh.features()
        m = self.model.spatial.max_log_gain
        out = []
        for k, n in enumerate(TINY["readout_outputs"]):
            y = orc.readout(feats, f"readouts.{k}", self.sd, 2, n, 0.07, None)
            if not plain:
                y = gain64(y, g, self.p[f"heads.{k}.pos"], self.p[f"heads.{k}.weight"], self.p[f"heads.{k}.bias"], m)
                if h is not None:
                    q = self.beh.p
                    a = q[f"heads.{k}.bias"][None, :, None] + torch.einsum("btk,nk->bnt", h, q[f"heads.{k}.weight"])
                    y = y * torch.exp(self.model.modulator.max_log_gain * torch.tanh(a))
            out.append(y)
        return out if index is None else out[index]

    def grads(self):
        res = {k: v.grad for k, v in self.sd.items() if getattr(v, "grad", None) is not None}
        res.update({"spatial." + k: v.grad for k, v in self.p.items()})
        if self.gaze is not None:
            res.update({"shifter." + k: v.grad for k, v in self.gaze.p.items()})
        if self.beh is not None:
            res.update({"modulator." + k: v.grad for k, v in self.beh.p.items()})
        return res


def grad_report(tag, model, ref, dtype):
    """Worst norm-relative error over the base parameters (with the floor of tests/test_gpu_model.py for the analytically zero
    gradients) and over the added branches' parameters; every spatial.* reference gradient must be non-zero."""
    named = dict(model.named_parameters())
    grads = ref.grads()
    assert set(grads) == set(named), sorted(set(grads) ^ set(named))
    gnorm = math.sqrt(sum(float(g.norm()) ** 2 for g in grads.values()))
    worst, worst_new = ("", 0.0), ("", 0.0)
    for k, g in grads.items():
        assert named[k].grad is not None, k
        if k.startswith(EXTRA):
            if k.startswith("spatial."):
                assert float(g.abs().max()) > 0, f"the reference gradient of {k} is zero"
            if k.startswith("shifter."):       # sums that cancel: held to sum|terms| by check_shifter_grads in _gradient_check
                assert float(g.abs().max()) > 0, f"the reference gradient of {k} is zero"
                continue
            err = rel(named[k].grad, g)
            worst_new = max(worst_new, (k, err), key=lambda t: t[1])
        else:
            floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm
            err = float((named[k].grad.double().cpu() - g).norm()) / (float(g.norm()) + floor)
            worst = max(worst, (k, err), key=lambda t: t[1])
    print(f"{tag}: worst base parameter gradient {worst[0]} {worst[1]:.3e}; worst added-branch gradient {worst_new[0]} {worst_new[1]:.3e}")
    return worst[1], worst_new[1]


# ------------------------------------------------------------------------------------------------ 1. zero heads are the identity
@pytest.mark.parametrize("dtype", DTYPES)
def test_fresh_model_is_the_plain_model(dtype):
    x, _, _ = inputs()
    xd = x.to(dev())
    for training in (False, True):
        model, base, _ = spatial_model(dtype, randomize=False)
        check_identity(f"fresh spatial model {dtype}", model, base, xd, training)
        for head in model.spatial.heads:
            assert 0.1 < float(head.pos.detach().abs().max()) <= 0.8
        if not training:
            with torch.no_grad():
                assert torch.equal(model(xd, index=1), base(xd)[1])
            for k, v in base.state_dict().items():
                assert torch.equal(v, model.state_dict()[k]), k


# --------------------------------------------------------------------------------- 2. / 3. gradients against the float64 chain
def _gradient_check(dtype, frozen, gaze_shifter=None, modulator=None, **spatial):
    from sensorium_amd import MicePoissonLoss
    model, _, sd = spatial_model(dtype, gaze_shifter=gaze_shifter, modulator=modulator, **spatial)
    x, targets, w = inputs()
    ref = Reference(model, sd, x, training=not frozen, detach=bool(spatial.get("detach_core", False)))
    po = ref.forward()
    orc.mice_poisson_loss(po, [t.double() for t in targets], w.double()).backward()
    if frozen:
        model.eval().freeze_batchnorm(True)
    else:
        model.train()
    xd = x.to(dev()).requires_grad_()
    preds = model(xd)
    MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    tag = f"spatial {'frozen' if frozen else 'train'} {dtype}" + (" composed" if gaze_shifter or modulator else "") + \
          (" detached" if spatial.get("detach_core") else "")
    e_pred = max(rel(p, q) for p, q in zip(preds, po))
    e_x = rel(xd.grad, ref.x.grad)
    with torch.no_grad():
        plain = ref.forward(plain=True)
    gains = [float((q.detach() / r).min()) for q, r in zip(po, plain)]
    print(f"{tag}: predictions {e_pred:.3e}; x.grad {e_x:.3e}; smallest gain {min(gains):.3f}; map {model.spatial._map_size}")
    base_err, new_err = grad_report(tag, model, ref, dtype)
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)
    xt = 1e-3 if dtype == torch.float32 else (BF16_DX if frozen else BF16_TRAIN_DX)["tiny"][1]
    assert min(gains) < 0.9                                    # the heads are really at work
    assert e_pred < ft and e_x < xt
    assert base_err < gt and new_err < gt
    if ref.gaze is not None:                                   # the shifter's gradient now also runs through dG: the gaze test's bound
        check_shifter_grads(tag, model, ref.gaze, xt)
    return model, ref


@pytest.mark.parametrize("dtype", DTYPES)
def test_training_step_gradients_match_the_float64_chain(dtype):
    _gradient_check(dtype, frozen=False)


@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_statistics_gradients_match_the_float64_chain(dtype):
    _gradient_check(dtype, frozen=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_composition_with_shifter_and_modulator(dtype):
    _gradient_check(dtype, frozen=False, gaze_shifter=dict(SHIFTER), modulator=dict(MODULATOR))


def test_sampling_the_core_channels_directly():
    model, ref = _gradient_check(torch.float32, frozen=True, features=None)
    assert model.spatial.project is None and model.spatial.heads[0].weight.shape == (7, 16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_detached_core(dtype):
    """detach_core: the branch's own gradients are those of the attached model (frozen statistics: both forwards are deterministic),
    and the core's gradients are the plain model's multiplied through the gain: the float64 chain with the map detached."""
    from sensorium_amd import MicePoissonLoss
    detached, ref = _gradient_check(dtype, frozen=True, detach_core=True)
    attached, _, _ = spatial_model(dtype)
    attached.eval().freeze_batchnorm(True)
    x, targets, w = inputs()
    MicePoissonLoss()(attached(x.to(dev())), ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    a, d = dict(attached.named_parameters()), dict(detached.named_parameters())
    for k in a:
        if k.startswith("spatial."):
            e = rel(d[k].grad, a[k].grad.double().cpu())
            same = torch.equal(d[k].grad, a[k].grad)
            print(f"detached core {dtype}: {k} against the attached model {e:.3e}; bit for bit: {same}")
            assert same, k
    k = "core.blocks.5.conv_pwl.0.weight"
    assert rel(d[k].grad, a[k].grad.double().cpu()) > 1e-4      # the attached core does see the second consumer


# --------------------------------------------------------------------------------------------------------- 4. MouseModel steps
STEPS, LR, WD, DECAY = 6, 2e-3, 0.05, 0.9


def mouse_model(dtype, sd=None, randomize=False, opt=None, **extra):
    from sensorium_amd.argus_models import MouseModel
    params = {"nn_module": ("dwiseneuro_spatial", dict(TINY, spatial=dict(SPATIAL))), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", dict({"lr": LR, "weight_decay": WD}, **(opt or {}))), "device": str(dev()),
              "amp": dtype == torch.bfloat16, "iter_size": 1, "frame_stack": {"size": 6, "step": 1, "position": "last"}}
    params.update(extra)
    torch.manual_seed(41)
    m = MouseModel(params)
    if sd is not None:
        m.nn_module.load_state_dict(sd, strict=False)
    if randomize:
        randomize_heads(m.nn_module)
    return m


@functools.lru_cache(maxsize=None)
def chain_losses(guarded):
    """STEPS AdamW steps of the float64 chain on the fixed batch, from the state mouse_model(..., randomize=True) starts in: the
    batch loss before each step.  The positions take no weight decay (MouseModel's second group).  guarded: gradients scaled by
    min(1, 1 / (norm + 1e-6)) (max_grad_norm = 1)."""
    m = mouse_model(torch.float32, tiny_model()[1], randomize=True)
    x, targets, w = inputs()
    sd = sd64(tiny_model()[1], grads=True)
    p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in m.nn_module.spatial.named_parameters()}
    leaves = [(v, WD) for v in sd.values() if getattr(v, "requires_grad", False)]
    leaves += [(v, 0.0 if k.endswith(".pos") else WD) for k, v in p.items()]
    state = [(torch.zeros_like(v), torch.zeros_like(v)) for v, _ in leaves]
    losses = []
    for step in range(1, STEPS + 1):
        for v, _ in leaves:
            v.grad = None
        ref = Reference(m.nn_module, None, x, training=True, params=p, sd_leaves=sd)
        loss = orc.mice_poisson_loss(ref.forward(), [t.double() for t in targets], w.double())
        loss.backward()
        losses.append(float(loss.detach()))
        grads = [v.grad if v.grad is not None else torch.zeros_like(v) for v, _ in leaves]
        coef = 1.0
        if guarded:
            norm = math.sqrt(sum(float((g ** 2).sum()) for g in grads))
            coef = min(1.0, 1.0 / (norm + 1e-6))
        with torch.no_grad():
            for i, ((v, wd), g) in enumerate(zip(leaves, grads)):
                q, mm, vv = orc.adamw_step(v.detach(), g * coef, state[i][0], state[i][1], step, LR, weight_decay=wd)
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
    names = [n for n, _ in m.nn_module.named_parameters() if n.startswith("spatial.heads.")]
    assert len(names) == 6
    params = dict(m.nn_module.named_parameters())
    history = [{n: params[n].detach().double().cpu().clone() for n in names}]
    losses = []
    for _ in range(STEPS):
        losses.append(m.train_step(batch)["loss"])
        history.append({n: params[n].detach().double().cpu().clone() for n in names})
    torch.cuda.synchronize()
    groups = m.optimizer.param_groups
    assert len(groups) == 2 and groups[1]["weight_decay"] == 0.0 and groups[0]["weight_decay"] == WD
    assert {id(q) for q in groups[1]["params"]} == {id(h.pos) for h in m.nn_module.spatial.heads}
    tag = f"spatial train_step x{STEPS} {dtype} {'guarded' if guarded else 'plain'}"
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
@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_round_trip_and_graph_replay(dtype, tmp_path):
    from sensorium_amd.engine import load_model
    from sensorium_amd.predictors import Predictor
    a = mouse_model(dtype, tiny_model()[1], randomize=True)
    a.save(tmp_path / "spatial.pth")
    c = load_model(tmp_path / "spatial.pth", device=str(dev()))
    assert type(c.nn_module).__name__ == "DwiseNeuroSpatial"
    assert list(c.nn_module.state_dict()) == list(a.nn_module.state_dict())
    for (k, v), u in zip(a.nn_module.state_dict().items(), c.nn_module.state_dict().values()):
        assert torch.equal(v, u), k
    x = trial()                                                     # 35 windows of 6 frames: two full batches of 16 and a ragged one
    mem = Predictor(a, str(dev()), frame_stack_size=6, frame_stack_step=1, windows_per_batch=16, use_graph=False)
    graph = Predictor(str(tmp_path / "spatial.pth"), str(dev()), windows_per_batch=16, use_graph=True)
    p, first = mem.predict_trial(x, 1), graph.predict_trial(x, 1)
    same = np.array_equal(p, first)
    print(f"spatial checkpoint {dtype}: prediction {p.shape}; graphs captured {len(graph._graphs)}; the replay from disk equals "
          f"the eager forward in memory: {same}")
    assert p.shape == (10, 40) and np.isfinite(p).all() and len(graph._graphs) == 1 and same
    for net in (graph.model.nn_module, a.nn_module):                # the heads changed in place: the captured graph reads them
        with torch.no_grad():
            net.spatial.heads[1].pos.mul_(-1.0)
            net.spatial.heads[1].bias.add_(0.25)
    second = graph.predict_trial(x, 1)
    assert len(graph._graphs) == 1 and not np.array_equal(first, second)
    assert np.array_equal(second, mem.predict_trial(x, 1))


# -------------------------------------------------------------------------------------------------------------- 6. attribution
@pytest.mark.parametrize("dtype", DTYPES)
def test_attribution_input_gradient(dtype):
    from sensorium_amd import attribution
    model, _, sd = spatial_model(dtype)
    x, _, _ = inputs()
    x = x[:2]
    index, neurons = 1, torch.tensor([0, 3, 4, 9])
    ref = Reference(model, sd, x, training=False, grads=False)
    ref.forward(index=index)[:, neurons].sum().backward()
    held = Reference(model, sd, x, training=False, grads=False, detach=True)
    held.forward(index=index)[:, neurons].sum().backward()
    share = float((ref.x.grad - held.x.grad).norm() / ref.x.grad.norm())
    model.eval()
    g = attribution.input_gradient(model, x.to(dev()), index, neurons.to(dev()))
    torch.cuda.synchronize()
    e = rel(g, ref.x.grad)
    print(f"spatial attribution {dtype}: x.grad rel err {e:.3e}; share of the sampled-map path in the input gradient {share:.3f}")
    assert share > 0.01
    assert e < (1e-3 if dtype == torch.float32 else BF16_DX["tiny"][1])


# ------------------------------------------------------------------------------------------------------------ 7. data parallel
@pytest.mark.parametrize("mode", ["dense", "shard"])
def test_one_rank_data_parallel(mode):
    """a fresh child process per mode (nothing may touch the GPU before the process group exists): its start is most of the time"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tests" / "spatial_ddp_worker.py"), mode]
    res = subprocess.run(cmd, cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True, timeout=300)
    print(res.stdout[-600:])
    assert res.returncode == 0 and f"SPATIAL_DDP_OK mode={mode} " in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]

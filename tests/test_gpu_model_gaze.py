"""The gaze shifter at model level: ``DwiseNeuroGaze`` on the tiny model of tests/test_gpu_frozen_bn.py,
inputs ``synth_inputs(..., 3, 6, 9, 11, ...) * INPUT_SCALE`` with the pupil planes of one sample made non-constant (so the plane
mean matters).  Ground truth is float64 on the CPU: the checker tests/gaze_reference.py and a float64 MLP in front of the oracle.
Every test prints what it measured before it asserts.
"""
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
from tests.test_gpu_train_input_grad import BF16_TRAIN_DX  # noqa: E402

DTYPES = [torch.float32, torch.bfloat16]
# the pupil planes of the synthetic clips are about (100, 70) +- 20, times INPUT_SCALE
SHIFTER = dict(hidden_features=16, hidden_layers=1, max_shift=3.0, pupil_mean=(1.0, 0.7), pupil_std=(0.2, 0.2), fill=0.5)
KW = dict(strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"])


def inputs(seed=2, b=3, t=6):
    xn, tn, wn = synth_inputs(np.random.default_rng(seed), b, t, 9, 11, TINY["readout_outputs"])
    x = torch.from_numpy(xn) * INPUT_SCALE
    # sample 1 as CutMix leaves it: a box of all the non-video planes comes from elsewhere, the pupil planes are not constant
    x[1, 1:, :, 2:6, 3:9] = x[0, 1:, :, 2:6, 3:9]
    return x, [torch.from_numpy(v) for v in tn], torch.from_numpy(wn)


def randomize_last_layer(model):
    """Shifts of order one pixel and away from the integers: the last layer's bias puts them at (1.5, -0.5) px and its small
    weights spread them by about a tenth of a pixel."""
    last = model.shifter.mlp[-2]
    g = torch.Generator().manual_seed(17)
    with torch.no_grad():
        last.weight.copy_((torch.randn(last.weight.shape, generator=g) * 0.02).to(last.weight.device))
        ms = model.shifter.max_shift
        last.bias.copy_(torch.tensor([math.atanh(1.5 / ms), math.atanh(-0.5 / ms)]).to(last.bias.device))
    return model


def gaze_model(dtype=torch.float32, randomize=True, **shifter):
    from sensorium_amd import DwiseNeuroGaze
    base, sd = tiny_model(dtype)
    torch.manual_seed(23)                      # the first layer's default initialisation
    model = DwiseNeuroGaze(compute_dtype=dtype, **TINY, gaze_shifter=dict(SHIFTER, **shifter))
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("shifter.") for k in res.missing_keys)
    model = model.to(dev())
    return (randomize_last_layer(model) if randomize else model), base, sd


class Reference:
    """float64: plane mean -> normalise -> MLP -> shifts -> checker resample -> oracle; leaves for every gradient asked of it."""

    def __init__(self, model, sd, x, training, grads=True):
        sh = model.shifter
        self.p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in sh.named_parameters()}
        self.x = x.double().clone().requires_grad_(True)
        self.sd = sd64(sd, grads=grads)
        self.sh = sh
        self.shift = self.shifts_of(self.x)
        self.shift.retain_grad()
        self.xs = gr.resample(self.x, self.shift, sh.video_channel, sh.fill)
        self.xs.retain_grad()
        self.fill, self.vc = sh.fill, sh.video_channel
        self.training = training

    def shifts_of(self, x):
        sh = self.sh
        h = (gr.plane_mean(x, sh.pupil_channels) - sh.pupil_mean.double().cpu()) / sh.pupil_std.double().cpu()
        for i in range(len(self.p) // 2):          # Linear -> Tanh, the last pair included (mlp.0, mlp.2, ...)
            h = torch.tanh(h @ self.p[f"mlp.{2 * i}.weight"].t() + self.p[f"mlp.{2 * i}.bias"])
        return h * sh.max_shift

    def forward(self, **kw):
        return orc.forward(self.sd, self.xs, training=self.training, **KW, **kw)

    def fractions_ok(self):
        fr = (self.shift - self.shift.floor()).detach()
        return float((fr - 0.5).abs().max())

    def shifter_l1(self):
        """sum |terms| of each shifter parameter's gradient (call after backward): g = sum_{frame, k} dshift[frame][k] *
        d shift[frame][k] / d p, and dshift itself a contraction over the frame's pixels of the gradient w.r.t. the shifted input
        with the resample's Jacobian: sum_{frame, k} |d shift / d p| * sum_pixels |dxs * d xs / d shift|."""
        jac = gr.shift_jacobian(self.x.detach(), self.shift.detach(), self.vc, self.fill)        # [B][T][2][H][W]
        a = (self.xs.grad[:, self.vc, :, None].abs() * jac.abs()).sum(dim=(3, 4))                 # [B][T][2]
        l1 = {k: torch.zeros_like(v) for k, v in self.p.items()}
        flat = self.shifts_of(self.x.detach()).reshape(-1)           # the MLP's graph again: backward() has freed the first
        for i in range(flat.numel()):
            gs = torch.autograd.grad(flat[i], list(self.p.values()), retain_graph=True, allow_unused=True)
            for (k, _), g in zip(self.p.items(), gs):
                if g is not None:
                    l1[k] += a.reshape(-1)[i] * g.abs()
        return l1


def check_shifter_grads(tag, model, ref, tol):
    l1 = ref.shifter_l1()
    named = dict(model.shifter.named_parameters())
    for k, p in ref.p.items():
        assert named[k].grad is not None, k
        assert float(p.grad.abs().max()) > 0, f"the reference gradient of {k} is zero"
        err = float(((named[k].grad.double().cpu() - p.grad).abs() / l1[k]).max())
        print(f"{tag} shifter.{k}: |g_ref| {float(p.grad.norm()):.3e} worst |g - g_ref| / sum|terms| {err:.3e} (bound {tol:.0e})")
        assert err < tol, k


def base_grad_worst(model, ref, dtype):
    grads = {k: v.grad for k, v in ref.sd.items() if getattr(v, "grad", None) is not None}
    gnorm = math.sqrt(sum(float(g.norm()) ** 2 for g in grads.values()))
    named = dict(model.named_parameters())
    assert set(grads) == {k for k in named if not k.startswith("shifter.")}
    worst = ("", 0.0)
    for k, g in grads.items():
        assert named[k].grad is not None, k
        floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm        # tests/test_gpu_model.py: analytically-zero gradients
        err = float((named[k].grad.double().cpu() - g).norm()) / (float(g.norm()) + floor)
        worst = max(worst, (k, err), key=lambda t: t[1])
    return worst


# ------------------------------------------------------------------------------------------------ 1. zero shift is the identity
@pytest.mark.parametrize("dtype", DTYPES)
def test_fresh_shifter_is_the_identity(dtype):
    model, base, _ = gaze_model(dtype, randomize=False)
    x, _, _ = inputs()
    xd = x.to(dev())
    model.eval(), base.eval()
    with torch.no_grad():
        shifts = model.shifter.shifts(xd)
        a, b, again = model(xd), base(xd), model(xd)
        one = model(xd, index=1)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(a, b))
    print(f"fresh gaze model {dtype}: max |shift| {float(shifts.abs().max())}; outputs equal the plain model's: {same}")
    assert float(shifts.abs().max()) == 0.0 and shifts.shape == (3, 6, 2)
    assert same and all(torch.equal(p, q) for p, q in zip(a, again)) and torch.equal(one, b[1])


# --------------------------------------------------------------------------------- 2. training-step gradients against the oracle
@pytest.mark.parametrize("dtype", DTYPES)
def test_training_step_gradients_match_oracle(dtype):
    from sensorium_amd import MicePoissonLoss
    model, _, sd = gaze_model(dtype)
    x, targets, w = inputs()
    ref = Reference(model, sd, x, training=True)
    off = ref.fractions_ok()
    print(f"gaze train {dtype}: shifts {ref.shift.detach().min():.3f} ... {ref.shift.detach().max():.3f}, worst |frac - 0.5| {off:.3f}")
    assert off < 0.4
    po = ref.forward()
    orc.mice_poisson_loss(po, [t.double() for t in targets], w.double()).backward()

    model.train()
    xd = x.to(dev()).requires_grad_()
    preds = model(xd)
    MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    e_shift = float((model.shifter.shifts(xd).detach().double().cpu() - ref.shift.detach()).abs().max())
    e_pred = max(rel(p, q) for p, q in zip(preds, po))
    e_x = rel(xd.grad, ref.x.grad)
    worst = base_grad_worst(model, ref, dtype)
    print(f"gaze train {dtype}: |shift - ref| {e_shift:.2e} px; predictions {e_pred:.3e}; x.grad {e_x:.3e}; worst base parameter "
          f"gradient {worst[0]} {worst[1]:.3e}")
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)
    tol = 1e-3 if dtype == torch.float32 else BF16_TRAIN_DX["tiny"][1]
    assert e_shift < 1e-5 and e_pred < ft and worst[1] < gt and e_x < tol
    check_shifter_grads(f"gaze train {dtype}", model, ref, tol)


# ----------------------------------------------------------------------------------------------------------- 3. frozen statistics
@pytest.mark.parametrize("dtype", DTYPES)
def test_frozen_statistics_shifter_gradients(dtype):
    """Fitting the shifter on a trained model: eval(), freeze_batchnorm(True), plain data — against the oracle in eval mode."""
    from sensorium_amd import MicePoissonLoss
    model, _, sd = gaze_model(dtype)
    x, targets, w = inputs()
    ref = Reference(model, sd, x, training=False)
    orc.mice_poisson_loss(ref.forward(), [t.double() for t in targets], w.double()).backward()
    model.eval().freeze_batchnorm(True)
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    preds = model(x.to(dev()))
    MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in before.items()), "frozen statistics moved"
    tol = 1e-3 if dtype == torch.float32 else BF16_DX["tiny"][1]
    check_shifter_grads(f"gaze frozen {dtype}", model, ref, tol)
    worst = base_grad_worst(model, ref, dtype)
    print(f"gaze frozen {dtype}: worst base parameter gradient {worst[0]} {worst[1]:.3e}")
    assert worst[1] < (1e-3 if dtype == torch.float32 else 1e-1)


# ------------------------------------------------------------------------------------------------------------------ 4. mode rule
@pytest.mark.parametrize("dtype", DTYPES)
def test_eval_mode_is_decided_from_the_callers_input(dtype):
    model, _, _ = gaze_model(dtype)
    x, _, _ = inputs()
    xd = x.to(dev())
    model.eval()
    with torch.no_grad():
        ref = model(xd)
    assert all(p.requires_grad for p in model.shifter.parameters())
    plain = model(xd)                           # grad enabled, plain data, a trainable shifter: still the eval kernels
    same = all(torch.equal(a, b) for a, b in zip(plain, ref))
    print(f"gaze mode rule {dtype}: grad-enabled eval forward equals the no_grad forward bit for bit: {same}")
    assert same
    with pytest.raises(RuntimeError, match="backward through eval-mode BatchNorm is not built"):
        sum(p.sum() for p in plain).backward()
    # the caller's input requires grad: frozen statistics, and a backward exists (through the shifter too)
    xg = xd.clone().requires_grad_()
    sum(p.sum() for p in model(xg)).backward()
    assert xg.grad is not None and model.shifter.mlp[0].weight.grad is not None


# --------------------------------------------------------------------------------------------------------- 5. MouseModel steps
def mouse_model(dtype, sd=None, randomize=False, opt=None, **extra):
    from sensorium_amd.argus_models import MouseModel
    params = {"nn_module": ("dwiseneuro_gaze", dict(TINY, gaze_shifter=dict(SHIFTER))), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", dict({"lr": 1e-3, "weight_decay": 0.05}, **(opt or {}))), "device": str(dev()),
              "amp": dtype == torch.bfloat16, "iter_size": 1, "frame_stack": {"size": 6, "step": 1, "position": "last"}}
    params.update(extra)
    m = MouseModel(params)
    if sd is not None:
        m.nn_module.load_state_dict(sd, strict=False)
    if randomize:
        randomize_last_layer(m.nn_module)
    return m


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "guarded"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_mouse_model_train_steps_and_ema(dtype, guarded):
    decay = 0.9
    sd = tiny_model()[1]
    # the last layer randomised: non-zero shifts, so every one of the four tensors receives a gradient in the first step
    m = mouse_model(dtype, sd, randomize=True, opt=dict(max_grad_norm=1.0, skip_nonfinite=True, weight_decay=0.0) if guarded
                    else dict(weight_decay=0.0))
    m.set_ema(decay)
    x, targets, w = inputs()
    batch = (x.to(dev()), ([t.to(dev()) for t in targets], w.to(dev())))
    names = [n for n, _ in m.nn_module.named_parameters() if n.startswith("shifter.")]
    assert len(names) == 4
    params = dict(m.nn_module.named_parameters())
    history = [{n: params[n].detach().double().cpu().clone() for n in names}]
    for _ in range(3):
        out = m.train_step(batch)
        assert math.isfinite(out["loss"])
        history.append({n: params[n].detach().double().cpu().clone() for n in names})
    torch.cuda.synchronize()
    assert m.optimizer.folds_ema_of(m.model_ema)
    ema = dict(m.model_ema.ema.named_parameters())
    for n in names:
        moved = float((history[-1][n] - history[0][n]).abs().max())
        e = history[0][n].clone()
        for k in range(1, 4):
            e = decay * e + (1.0 - decay) * history[k][n]
        err = rel(ema[n], e)
        print(f"gaze train_step x3 {dtype} {'guarded' if guarded else 'plain'} {n}: moved by {moved:.3e}; EMA against the float64 "
              f"replay {err:.3e} (bound 1e-6)")
        assert moved > 0 and float(e.abs().max()) > 0           # weight_decay is 0: a parameter moves only through its gradient
        assert err <= 1e-6, n


# ------------------------------------------------------------------------------------------------- 6. / 7. checkpoint, hipGraph
def trial(length=40, seed=8):
    xn, _, _ = synth_inputs(np.random.default_rng(seed), 1, length, 9, 11, (1,))
    x = torch.from_numpy(xn)[0] * INPUT_SCALE                      # (5, L, H, W)
    x[3:, :, 1:5, 2:7] *= 1.3                                       # pupil planes not constant over the frame
    return x


@pytest.mark.parametrize("dtype", DTYPES)
def test_checkpoint_round_trip_and_predictor(dtype, tmp_path):
    from sensorium_amd.engine import load_model
    from sensorium_amd.predictors import Predictor
    sd = tiny_model()[1]
    a = mouse_model(dtype, sd, randomize=True)
    a.save(tmp_path / "gaze.pth")
    c = load_model(tmp_path / "gaze.pth", device=str(dev()))
    assert type(c.nn_module).__name__ == "DwiseNeuroGaze"
    assert list(c.nn_module.state_dict()) == list(a.nn_module.state_dict())
    for (k, v), u in zip(a.nn_module.state_dict().items(), c.nn_module.state_dict().values()):
        assert torch.equal(v, u), k
    x = trial()
    mem = Predictor(a, str(dev()), frame_stack_size=6, frame_stack_step=1, windows_per_batch=16, use_graph=False)
    disk = Predictor(str(tmp_path / "gaze.pth"), str(dev()), windows_per_batch=16, use_graph=False)
    assert (disk.frame_stack_size, disk.frame_stack_step) == (6, 1)
    p, q = mem.predict_trial(x, 1), disk.predict_trial(x, 1)
    with torch.no_grad():
        s = a.nn_module.shifter.shifts(x[None].to(dev()))
    print(f"gaze checkpoint {dtype}: prediction {p.shape}, shifts {float(s.min()):.3f} ... {float(s.max()):.3f}; from disk equals "
          f"in memory: {np.array_equal(p, q)}")
    assert p.shape == (10, 40) and np.isfinite(p).all() and float(s.abs().max()) > 0.1
    assert np.array_equal(p, q)


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_replay_computes_the_shift_on_the_device(dtype):
    from sensorium_amd.predictors import Predictor
    model = mouse_model(dtype, tiny_model()[1], randomize=True)
    x = trial()                                                     # 35 windows of 6 frames: two full batches of 16 and a ragged one
    graph = Predictor(model, str(dev()), frame_stack_size=6, frame_stack_step=1, windows_per_batch=16, use_graph=True)
    plain = Predictor(model, str(dev()), frame_stack_size=6, frame_stack_step=1, windows_per_batch=16, use_graph=False)
    first = graph.predict_trial(x, 1)
    same = np.array_equal(first, plain.predict_trial(x, 1))
    print(f"gaze hipGraph {dtype}: graphs captured {len(graph._graphs)}; replay equals the eager forward: {same}")
    assert len(graph._graphs) == 1 and same
    with torch.no_grad():
        model.nn_module.shifter.mlp[-2].bias.add_(0.2)
    second = graph.predict_trial(x, 1)                              # a replay of the graph captured before the change
    assert len(graph._graphs) == 1 and not np.array_equal(first, second)
    assert np.array_equal(second, plain.predict_trial(x, 1))


# -------------------------------------------------------------------------------------------------------------- 8. attribution
@pytest.mark.parametrize("dtype", DTYPES)
def test_attribution_includes_the_path_through_the_shifter(dtype):
    from sensorium_amd import attribution
    model, _, sd = gaze_model(dtype)
    x, _, _ = inputs()
    x = x[:2]
    index, neurons = 1, torch.tensor([0, 3, 4, 9])
    ref = Reference(model, sd, x, training=False, grads=False)
    ref.forward(index=index)[:, neurons].sum().backward()
    # the pupil planes' gradient without the shifter path: the shifted input's gradient on those channels alone
    direct = ref.xs.grad[:, 3:5]
    through = ref.x.grad[:, 3:5] - direct
    share = float(through.norm() / ref.x.grad[:, 3:5].norm())
    model.eval()
    g = attribution.input_gradient(model, x.to(dev()), index, neurons.to(dev()))
    torch.cuda.synchronize()
    e, e_pupil = rel(g, ref.x.grad), rel(g[:, 3:5], ref.x.grad[:, 3:5])
    print(f"gaze attribution {dtype}: x.grad rel err {e:.3e}, pupil planes {e_pupil:.3e}; share of the shifter path in the pupil "
          f"planes' gradient {share:.3f}")
    assert share > 0.01
    tol = 1e-3 if dtype == torch.float32 else BF16_DX["tiny"][1]
    assert e < tol and e_pupil < tol


# ------------------------------------------------------------------------------------------------------------ 9. data parallel
@pytest.mark.parametrize("mode", ["dense", "shard"])
def test_one_rank_data_parallel(mode):
    """a fresh child process per mode (nothing may touch the GPU before the process group exists): its start is most of the time"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tests" / "gaze_ddp_worker.py"), mode]
    res = subprocess.run(cmd, cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True, timeout=300)
    print(res.stdout[-600:])
    assert res.returncode == 0 and f"GAZE_DDP_OK mode={mode} " in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]

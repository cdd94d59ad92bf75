"""Learnable Softplus beta at module level: the tiny two-readout model at B = 2, T = 8.

Training-step gradients (every parameter and both dbeta) against oracle.forward in float64 with each readout's beta a leaf, to the
bounds of tests/test_gpu_model.py; the "log" form; forward(x, index); recovery of a teacher's beta by 200 optimizer steps, plain and
guarded; the EMA copy against the float64 lerp recursion; eval through a captured graph with beta changed in place between two
replays; a checkpoint round trip; and one-rank data parallelism, dense / bf16 exchange / sharded (tests/lsp_ddp_worker.py).
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

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests.gpu_helpers import analytically_zero_grad, dev, rel  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
OUTPUTS = (7, 10)
TINY = dict(readout_outputs=OUTPUTS, in_channels=5, core_features=(8, 8, 16), spatial_strides=(2, 1, 2), spatial_kernel=3,
            temporal_kernel=5, expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), groups=2, softplus_beta=0.07,
            drop_rate=0.0, drop_path_rate=0.0)
BETAS = (0.07, 0.11)            # one per readout: a gradient routed to the wrong gate would show
B, T, H, W = 2, 8, 12, 16


@pytest.fixture(scope="module")
def sd():
    return orc.make_state_dict(readout_outputs=OUTPUTS, core_features=(8, 8, 16), expansion_ratio=3, se_reduce_ratio=4,
                               cortex_features=(32, 64), seed=1, randomize_bn=True)


@pytest.fixture(scope="module")
def batch():
    from sensorium_amd.synthetic import make_batch
    return make_batch(B, T, H, W, OUTPUTS, seed=11)


def build(sd, form="beta", betas=BETAS, **over):
    from sensorium_amd import DwiseNeuro
    model = DwiseNeuro(**dict(TINY, **over), learnable_softplus=True, softplus_param=form)
    res = model.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(".gate." in k for k in res.missing_keys) and len(res.missing_keys) == 2
    with torch.no_grad():
        for r, b in zip(model.readouts, betas):
            next(r.gate.parameters()).fill_(b if form == "beta" else math.log(b))
    return model.to(dev())


def gate_params(model):
    return model.softplus_parameters()


@pytest.fixture(scope="module")
def oracle_grads(sd, batch):
    """float64 autograd through oracle.forward in training mode, readout m with beta_m a float64 leaf; computed once"""
    x, (targets, w) = batch
    sdo = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and "inv_freq" not in k
               else (v.double() if v.is_floating_point() else v)) for k, v in sd.items()}
    betas = [torch.tensor(float(np.float32(b)), dtype=torch.float64, requires_grad=True) for b in BETAS]
    preds = [orc.forward(sdo, x.double(), strides=TINY["spatial_strides"], readout_outputs=OUTPUTS, training=True,
                         softplus_beta=betas[m], index=m) for m in range(2)]
    loss = orc.mice_poisson_loss(preds, [t.double() for t in targets], w.double())
    loss.backward()
    grads = {k: v.grad for k, v in sdo.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None}
    return dict(preds=[p.detach() for p in preds], loss=float(loss.detach()), grads=grads, dbeta=[float(b.grad.detach()) for b in betas])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_train_step_gradients_match_oracle(sd, batch, oracle_grads, dtype):
    from sensorium_amd import MicePoissonLoss
    x, (targets, w) = batch
    model = build(sd, compute_dtype=dtype).train()
    preds = model(x.to(dev()))
    loss = MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev())))
    loss.backward()
    torch.cuda.synchronize()
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)            # tests/test_gpu_model.py
    for m in range(2):
        assert rel(preds[m], oracle_grads["preds"][m]) < ft
    grads = oracle_grads["grads"]
    gnorm = math.sqrt(sum(float((g ** 2).sum()) for g in grads.values()) + sum(g * g for g in oracle_grads["dbeta"]))
    floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm
    named = dict(model.named_parameters())
    worst = ("", 0.0)
    for k, g in grads.items():
        mine = named[k].grad
        assert mine is not None, k
        err = float((mine.double().cpu() - g).norm()) / (float(g.norm()) + floor)
        worst = max(worst, (k, err), key=lambda t: t[1])
    assert worst[1] < gt, worst
    for m, p in enumerate(gate_params(model)):
        ref = oracle_grads["dbeta"][m]
        err = abs(float(p.grad) - ref) / (abs(ref) + floor)
        print(f"LSPFIG model {str(dtype).split('.')[-1]} dbeta[{m}] {float(p.grad):.6e} ref {ref:.6e} err {err:.3e} "
              f"|dbeta|/gnorm {abs(ref) / gnorm:.3e}")
        assert p.grad.dim() == 0 and err < gt, (m, float(p.grad), ref)


def test_log_form_gradient_is_beta_times_the_beta_form():
    """Same features, same dout, the readout alone (its forward and the dbeta reduction have no atomics: the two runs see the same
    bits): d/d log(beta) = beta * d/d beta, one fp32 product on top — two roundings, 2^-23."""
    from sensorium_amd.dwiseneuro import Readout
    torch.manual_seed(5)
    x = torch.randn(B, T, 64, device=dev())
    dout = torch.randn(B, 10, T, device=dev())
    g = {}
    for form in ("beta", "log"):
        torch.manual_seed(6)
        ro = Readout(64, 10, groups=2, softplus_beta=0.07, learnable_softplus=True, softplus_param=form).to(dev()).train()
        with torch.no_grad():
            ro.layer[1].weight.mul_(20.0)
        ro(x).backward(dout)
        g[form] = float(next(ro.gate.parameters()).grad)
        beta = float(ro.beta())
    assert g["beta"] != 0.0 and abs(g["log"] - beta * g["beta"]) <= 2.0 ** -22 * abs(g["log"]), g


@pytest.mark.parametrize("guarded", [False, True])
def test_index_forward_leaves_the_other_gate_alone(sd, batch, guarded):
    from sensorium_amd.optim import FusedAdamWEma
    x, _ = batch
    model = build(sd).train()
    kw = dict(max_grad_norm=1.0) if guarded else {}
    opt = FusedAdamWEma(model.parameters(), lr=1e-3, weight_decay=0.0, **kw)
    model(x.to(dev()), index=1).sum().backward()
    g0, g1 = gate_params(model)
    assert g0.grad is None and model.readouts[0].layer[1].weight.grad is None and g1.grad is not None
    opt.step()
    torch.cuda.synchronize()
    assert float(g0.detach()) == float(np.float32(BETAS[0])) and not opt.state[g0]           # skipped like its weights
    assert float(g1.detach()) != float(np.float32(BETAS[1])) and int(opt.state[g1]["step"]) == 1


BETA_STAR, BETA_0, STEPS, DECAY = 0.07, 0.3, 200, 0.99


def _recover(sd, batch, form, guarded):
    """200 steps on the gate parameters alone against the teacher's own eval-mode predictions; returns the beta trajectory
    [steps + 1][2] (one read-back at the end), the parameter trajectory and the EMA copies."""
    from sensorium_amd import MicePoissonLoss
    from sensorium_amd.optim import FusedAdamWEma
    x, (_, w) = batch
    x, w = x.to(dev()), w.to(dev())
    teacher = build(sd, betas=(BETA_STAR, BETA_STAR)).eval()
    with torch.no_grad():
        targets = [p.clone() for p in teacher(x)]
    student = build(sd, form=form, betas=(BETA_0, BETA_0)).eval().freeze_batchnorm()
    for p in student.parameters():
        p.requires_grad_(False)
    gates = gate_params(student)
    for p in gates:
        p.requires_grad_(True)
    emas = [p.detach().clone() for p in gates]
    kw = dict(max_grad_norm=1.0) if guarded else {}
    opt = FusedAdamWEma(gates, lr=1e-2, weight_decay=0.0, ema_params=emas, ema_decay=DECAY, **kw)
    loss_fn = MicePoissonLoss()
    traj = [torch.stack([r.beta() for r in student.readouts])]
    ptraj = [torch.stack([p.detach().clone() for p in gates])]
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        loss_fn(student(x), (targets, w)).backward()
        opt.step()
        traj.append(torch.stack([r.beta() for r in student.readouts]))
        ptraj.append(torch.stack([p.detach().clone() for p in gates]))
    return torch.stack(traj).cpu().double(), torch.stack(ptraj).cpu().double(), torch.stack(emas).cpu().double()


def test_recovers_the_teachers_beta_and_ema_follows(sd, batch):
    traj, ptraj, emas = _recover(sd, batch, "beta", False)
    ratio = (traj[-1] - BETA_STAR).abs() / abs(BETA_0 - BETA_STAR)
    print(f"LSPFIG recovery plain ratio {ratio.tolist()} min beta {float(traj.min()):.4f}")
    assert bool((traj > 0).all()), "beta went non-positive on the way"
    assert bool((ratio < 0.05).all()), ratio
    # the fused EMA lerp of the 0-d parameter: e <- d e + (1 - d) p after every step, in float64 over the fp32 trajectory.  Each
    # fp32 step rounds at most twice (2^-24 of |e| each) and the recursion forgets errors at rate d: 2 * 2^-24 / (1 - d)
    e = ptraj[0].clone()
    for k in range(1, STEPS + 1):
        e = DECAY * e + (1.0 - DECAY) * ptraj[k]
    err = ((emas - e).abs() / e.abs()).max()
    assert float(err) <= 2 * 2.0 ** -24 / (1.0 - DECAY), float(err)


def test_guarded_log_form_shrinks_the_error(sd, batch):
    traj, _, _ = _recover(sd, batch, "log", True)
    ratio = (traj[-1] - BETA_STAR).abs() / abs(BETA_0 - BETA_STAR)
    print(f"LSPFIG recovery guarded-log ratio {ratio.tolist()}")
    assert bool((traj > 0).all()) and bool((ratio < 1.0).all()), ratio


def _mouse_model(sd, form="beta", **extra):
    from sensorium_amd.argus_models import MouseModel
    params = {"nn_module": ("dwiseneuro", dict(TINY, learnable_softplus=True, softplus_param=form)), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", {"lr": 1e-3, "weight_decay": 0.05}), "device": str(dev()), "amp": False, "iter_size": 1}
    params.update(extra)
    m = MouseModel(params)
    m.nn_module.load_state_dict(sd, strict=False)
    return m


def test_graph_replay_reads_beta_from_device_memory(sd):
    from sensorium_amd.predictors import Predictor
    model = _mouse_model(sd)
    pred = Predictor(model, str(dev()), frame_stack_size=4, frame_stack_step=1, windows_per_batch=2, use_graph=True)
    rng = np.random.default_rng(3)
    inputs = torch.from_numpy((rng.normal(size=(5, 5, H, W)) * 30 + 60).astype(np.float32))      # 5 frames: one batch of 2 windows
    first = pred.predict_trial(inputs, 1)
    assert len(pred._graphs) == 1
    with torch.no_grad():
        for p in gate_params(model.nn_module):
            p.fill_(0.2)
    second = pred.predict_trial(inputs, 1)                       # a replay of the graph captured with beta = 0.07
    assert len(pred._graphs) == 1 and not np.array_equal(first, second)
    plain = Predictor(model, str(dev()), frame_stack_size=4, frame_stack_step=1, windows_per_batch=2, use_graph=False)
    assert np.array_equal(second, plain.predict_trial(inputs, 1))


def test_checkpoint_round_trip(sd, batch, tmp_path):
    import sensorium_amd._lib as L
    from sensorium_amd.engine import load_model
    x, (targets, w) = batch
    b = (x.to(dev()), ([t.to(dev()) for t in targets], w.to(dev())))
    # the ordered-reduction build (DWN_DETERMINISTIC=1) makes the two runs the same bits: there the parameters must be EQUAL; with
    # the product build the runs differ by the arrival order of float atomics
    a = _mouse_model(sd)
    a.train_step(b)
    a.save(tmp_path / "lsp.pth", optimizer_state=True)
    c = load_model(tmp_path / "lsp.pth", device=str(dev()))
    assert [n for n, _ in c.nn_module.named_parameters()] == [n for n, _ in a.nn_module.named_parameters()]
    for (n, p), q in zip(a.nn_module.named_parameters(), c.nn_module.parameters()):
        assert torch.equal(p, q), n
    assert len(c.get_optimizer().param_groups) == 2 and c.optimizer.param_groups[1]["weight_decay"] == 0.0
    a.train_step(b)
    c.train_step(b)
    for (n, p), q in zip(a.nn_module.named_parameters(), c.nn_module.parameters()):
        if L.DETERMINISTIC:
            assert torch.equal(p, q), n
            continue
        # Adam's second step moves a parameter by about lr whatever its gradient's size: lr * 1e-2 = 1e-5 absolute (the bound
        # tests/ddp_gpu_worker.py applies to the parameters after a step) where the gradient is not summation noise
        if ".gate." in n:
            assert abs(float(p.detach()) - float(q.detach())) <= 1e-5, n
            assert float(p.detach()) != float(np.float32(0.07))
        elif not analytically_zero_grad(n):
            assert float(((p - q).abs() > 1e-5).float().mean()) < 1e-3, n


@pytest.mark.parametrize("mode", ["dense", "bf16comm", "shard", "log"])
def test_one_rank_data_parallel(mode):
    """a fresh child process per mode (nothing may touch the GPU before the process group exists): its start is most of the time"""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tests" / "lsp_ddp_worker.py"), mode]
    res = subprocess.run(cmd, cwd=str(ROOT), env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and f"LSP_DDP_OK mode={mode} " in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]

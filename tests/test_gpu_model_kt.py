"""DwiseNeuro(temporal_kernel=7 / 9) through the public interface against the CPU oracle (the oracle at these sizes is pinned to the
reference module by tests/test_temporal_kernel_cpu.py): load_state_dict(strict=True) of (kt, 1, 1) temporal weights, eval forward,
training forward + Poisson loss + backward with every parameter gradient, x.grad in eval mode (frozen BatchNorm) and in training
mode, one FusedAdamWEma step, and Predictor.predict_trial under a captured hipGraph — the tests of tests/test_gpu_model_ks.py.

Model: the tiny model of tests/golden/temporal_kernel_7_9.npz: core_features (8, 16), strides (2, 1), spatial_kernel 3, one readout;
inputs (2, 5, T, 9, 11) at T = 3 (shorter than the padding of either size) and T = 11.  Bounds are the ones
tests/test_gpu_model_ks.py takes from the existing tiny-model tests (tests/test_gpu_model.py, test_gpu_frozen_bn.py,
test_gpu_train_input_grad.py, test_gpu_step.py, gpu_helpers.ADAMW_BOUND)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests.gpu_helpers import ADAMW_BOUND, dev, rel, synth_inputs  # noqa: E402

N_OUT = 9
INPUT_SCALE = 0.01            # tests/test_gpu_frozen_bn.py: inputs of order one keep the input-gradient cases well conditioned


def model_kw(kt):
    return dict(readout_outputs=(N_OUT,), in_channels=5, core_features=(8, 16), spatial_strides=(2, 1), spatial_kernel=3,
                temporal_kernel=kt, expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), groups=2, softplus_beta=0.07,
                drop_rate=0.0, drop_path_rate=0.0)


ORC_KW = dict(strides=(2, 1), readout_outputs=(N_OUT,))


def state_dict(kt, seed=3):
    return orc.make_state_dict(readout_outputs=(N_OUT,), core_features=(8, 16), spatial_kernel=3, temporal_kernel=kt,
                               expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), seed=seed, randomize_bn=True)


def build(kt, dtype):
    from sensorium_amd import DwiseNeuro
    sd = state_dict(kt)
    assert sd["core.blocks.1.temp_covn_dw.0.weight"].shape[2:] == (kt, 1, 1)
    model = DwiseNeuro(compute_dtype=dtype, **model_kw(kt))
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model.to(dev()), sd


def sd64(sd, grads=False):
    out = {}
    for k, v in sd.items():
        if v.is_floating_point():
            v = v.double()
            if grads and "running" not in k and "inv_freq" not in k:
                v = v.clone().requires_grad_(True)
        out[k] = v
    return out


def batch(T, scale=1.0, seed=2):
    xn, tn, wn = synth_inputs(np.random.default_rng(seed), 2, T, 9, 11, (N_OUT,))
    return torch.from_numpy(xn) * scale, [torch.from_numpy(t) for t in tn], torch.from_numpy(wn)


PARAMS = [pytest.param(kt, T, dtype, id=f"kt{kt}-T{T}-{str(dtype)[6:]}") for kt in (7, 9) for T in (3, 11)
          for dtype in (torch.float32, torch.bfloat16)]


@pytest.mark.parametrize("kt,T,dtype", PARAMS)
def test_eval_forward(kt, T, dtype):
    model, sd = build(kt, dtype)
    x, _, _ = batch(T)
    assert x.shape == (2, 5, T, 9, 11)
    ref = orc.forward(sd64(sd), x.double(), training=False, **ORC_KW)
    model.eval()
    with torch.no_grad():
        preds = model(x.to(dev()))
        again = model(x.to(dev()))
    e = rel(preds[0], ref[0])
    print(f"eval forward kt{kt} T{T} {dtype}: rel err {e:.3e}")
    assert e < (1e-3 if dtype == torch.float32 else 3e-2)
    assert torch.equal(again[0], preds[0])               # the eval forward is exact from call to call


def _param_grad_worst(model, grads, dtype):
    gnorm = math.sqrt(sum(float(g.norm()) ** 2 for g in grads.values()))
    named = dict(model.named_parameters())
    assert set(grads) == set(named)
    worst = ("", 0.0)
    for k, g in grads.items():
        mine = named[k].grad
        assert mine is not None, k
        floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm          # tests/test_gpu_model.py: analytically-zero gradients
        err = float((mine.double().cpu() - g).norm()) / (float(g.norm()) + floor)
        if err > worst[1]:
            worst = (k, err)
    return worst


def _train_reference(sd, x, targets, w):
    ref_sd = sd64(sd, grads=True)
    x64 = x.double().requires_grad_(True)
    new_stats = {}
    po = orc.forward(ref_sd, x64, training=True, new_stats=new_stats, **ORC_KW)
    lo = orc.mice_poisson_loss(po, [t.double() for t in targets], w.double())
    lo.backward()
    grads = {k: v.grad for k, v in ref_sd.items() if getattr(v, "grad", None) is not None}
    return po, lo.detach(), grads, x64.grad, new_stats


@pytest.mark.parametrize("kt,T,dtype", PARAMS)
def test_train_step_and_adamw(kt, T, dtype):
    """Training forward, Poisson loss, backward: predictions, loss, every parameter gradient and the running statistics against the
    oracle; then one FusedAdamWEma step on those gradients against the oracle's AdamW / EMA restatement."""
    from sensorium_amd import MicePoissonLoss
    from sensorium_amd.optim import FusedAdamWEma
    model, sd = build(kt, dtype)
    x, targets, w = batch(T)
    po, lo, grads, _, new_stats = _train_reference(sd, x, targets, w)
    model.train()
    preds = model(x.to(dev()))
    loss = MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev())))
    loss.backward()
    torch.cuda.synchronize()
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)
    e_pred = rel(preds[0], po[0])
    worst = _param_grad_worst(model, grads, dtype)
    print(f"train step kt{kt} T{T} {dtype}: predictions {e_pred:.3e}; loss {float(loss):.6f} (oracle {float(lo):.6f}); worst gradient "
          f"{worst[0]} {worst[1]:.3e}")
    assert e_pred < ft
    scale = float(po[0].detach().abs().sum()) / x.shape[0]
    floor = (1e-3 if dtype == torch.float32 else 1e-2) * scale                # tests/test_gpu_model.py: the loss is a cancelling sum
    assert abs(float(loss.detach()) - float(lo)) <= ft * max(abs(float(lo)), floor)
    assert worst[1] < gt, worst
    msd = model.state_dict()
    for k, v in new_stats.items():
        if v.is_floating_point():
            assert rel(msd[k], v) < (1e-4 if dtype == torch.float32 else 3e-2), k
        else:
            assert int(msd[k]) == int(v), k
    # ---- one fused AdamW + EMA step on the gradients just computed
    params = [p for p in model.parameters()]
    emas = [p.detach().clone() + 0.01 for p in params]
    ema0 = [e.clone() for e in emas]
    p0 = [p.detach().clone() for p in params]
    opt = FusedAdamWEma(params, lr=2.4e-3, weight_decay=0.05, ema_params=emas, ema_decay=0.99)
    opt.step()
    torch.cuda.synchronize()
    for p, q0, e, e0 in zip(params, p0, emas, ema0):
        g = p.grad.double().cpu()
        want, _, _ = orc.adamw_step(q0.double().cpu(), g, torch.zeros_like(g), torch.zeros_like(g), 1, 2.4e-3, weight_decay=0.05)
        assert rel(p.detach(), want) < ADAMW_BOUND
        assert rel(e, orc.ema_update(e0.double().cpu(), want, 0.99)) < ADAMW_BOUND


@pytest.mark.parametrize("kt,T,dtype", PARAMS)
def test_eval_mode_input_gradient(kt, T, dtype):
    """model.eval(); x.requires_grad_(): frozen BatchNorm statistics, x.grad against the oracle's eval-mode autograd."""
    model, sd = build(kt, dtype)
    x, _, _ = batch(T, INPUT_SCALE)
    neurons = torch.tensor([0, 3, 4, 8])
    x64 = x.double().requires_grad_(True)
    orc.forward(sd64(sd), x64, index=0, training=False, **ORC_KW)[:, neurons].sum().backward()
    model.eval()
    before = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    xd = x.to(dev()).requires_grad_()
    model(xd, index=0)[:, neurons.to(dev())].sum().backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape
    assert float(x64.grad.abs().max()) > 0
    e = rel(xd.grad, x64.grad)
    print(f"eval-mode input gradient kt{kt} T{T} {dtype}: rel err {e:.3e}")
    for k, v in before.items():
        assert torch.equal(model.state_dict()[k], v), k
    assert e < (1e-3 if dtype == torch.float32 else 3e-2)        # tests/test_gpu_frozen_bn.py, tiny model


@pytest.mark.parametrize("kt,T,dtype", PARAMS)
def test_train_mode_input_gradient(kt, T, dtype):
    from sensorium_amd import MicePoissonLoss
    model, sd = build(kt, dtype)
    x, targets, w = batch(T, INPUT_SCALE)
    _, _, grads, g_ref, _ = _train_reference(sd, x, targets, w)
    model.train()
    xd = x.to(dev()).requires_grad_()
    MicePoissonLoss()(model(xd), ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape
    assert float(g_ref.abs().max()) > 0
    e = rel(xd.grad, g_ref)
    worst = _param_grad_worst(model, grads, dtype)
    print(f"train-mode input gradient kt{kt} T{T} {dtype}: rel err {e:.3e}; worst parameter gradient {worst[0]} {worst[1]:.3e}")
    assert worst[1] < (1e-3 if dtype == torch.float32 else 1e-1), worst
    assert e < (1e-3 if dtype == torch.float32 else 5e-2)        # tests/test_gpu_train_input_grad.py, tiny model


@pytest.mark.parametrize("kt", [7, 9])
def test_predict_trial_under_hipgraph(kt):
    """Sliding-window prediction of a 40-frame clip with the eval forward captured into a hipGraph, against the oracle's loop."""
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.predictors import Predictor
    sd = state_dict(kt)
    params = {"nn_module": ("dwiseneuro", model_kw(kt)), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", {"lr": 2.4e-3, "weight_decay": 0.05}), "device": "cuda:0", "amp": False, "iter_size": 1}
    model = MouseModel(params)
    model.nn_module.load_state_dict(sd, strict=True)
    xn, _, _ = synth_inputs(np.random.default_rng(5), 1, 40, 9, 11, (N_OUT,))
    inputs = torch.from_numpy(xn[0])                                # (C, L, H, W), L = 40
    size, step = 8, 2
    ref_sd = sd64(sd)
    with torch.no_grad():
        want = orc.predict_trial(lambda win: orc.forward(ref_sd, win.double(), index=0, **ORC_KW)[0], inputs, N_OUT,
                                 size=size, step=step)
    pred = Predictor(model, frame_stack_size=size, frame_stack_step=step, windows_per_batch=4, use_graph=True)
    out = pred.predict_trial(inputs, 0)
    assert out.shape == want.shape and out.dtype == np.float32
    e = rel(torch.from_numpy(out), torch.from_numpy(want))
    print(f"predict_trial kt{kt}: rel err {e:.3e}")
    assert e < 1e-3
    assert np.array_equal(pred.predict_trial(inputs, mouse_index=0), out)

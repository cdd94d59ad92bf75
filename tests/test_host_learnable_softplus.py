"""CPU tests of the host side of the learnable Softplus beta: off, the module tree and the state_dict are
exactly the reference's; on, every readout holds one 0-d gate parameter; MouseModel gives those parameters a group without weight
decay and keeps the EMA copies in the optimizer's order; the C-ABI struct grew by two pointers under the same ABI version and the
backward entry refuses half a pair before it touches a device.  No kernel runs here."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
TINY = dict(readout_outputs=(7, 10), core_features=(8, 8, 16), spatial_strides=(2, 1, 2), expansion_ratio=3, se_reduce_ratio=4,
            cortex_features=(32, 64))
PTR = 256            # never dereferenced on the host


def _ref_keys(golden_dir):
    z = np.load(golden_dir / "tiny_model_eval.npz")
    return z, [k[3:] for k in z.files if k.startswith("sd:")]


def test_off_is_the_reference_module(golden_dir):
    from sensorium_amd import DwiseNeuro
    z, ref_keys = _ref_keys(golden_dir)
    plain = DwiseNeuro(**TINY)
    off = DwiseNeuro(**TINY, learnable_softplus=False, softplus_param="beta")
    assert list(off.state_dict().keys()) == ref_keys == list(plain.state_dict().keys())
    assert [n for n, _ in off.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert repr(off) == repr(plain) and isinstance(off.readouts[0].gate, torch.nn.Softplus)
    assert off.softplus_parameters() == []
    res = off.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # the new arguments come last: positional calls keep their meaning
    import inspect
    names = list(inspect.signature(DwiseNeuro.__init__).parameters)
    assert names[-3:] == ["compute_dtype", "learnable_softplus", "softplus_param"]


@pytest.mark.parametrize("form,leaf", [("beta", "beta"), ("log", "log_beta")])
def test_on_adds_one_scalar_per_readout(golden_dir, form, leaf):
    from sensorium_amd import DwiseNeuro
    z, ref_keys = _ref_keys(golden_dir)
    model = DwiseNeuro(**TINY, softplus_beta=0.07, learnable_softplus=True, softplus_param=form)
    gate_keys = [f"readouts.{k}.gate.{leaf}" for k in range(2)]
    keys = list(model.state_dict().keys())
    assert [k for k in keys if k not in gate_keys] == ref_keys and [k for k in keys if k in gate_keys] == gate_keys
    want = np.float32(0.07) if form == "beta" else np.float32(math.log(0.07))
    for k, p in zip(range(2), model.softplus_parameters()):
        assert p is dict(model.named_parameters())[gate_keys[k]]
        assert p.dim() == 0 and p.dtype == torch.float32 and p.requires_grad and float(p.detach()) == float(want)
        r = model.readouts[k]
        assert r.softplus_beta == 0.07                                   # stays the construction value
        assert r.beta().dim() == 0 and not r.beta().requires_grad
        assert abs(float(r.beta()) - 0.07) <= 1e-7 * 0.07 * (1 if form == "beta" else 4)
    # a fixed-beta checkpoint: only the gate keys are missing, and beta keeps its initial value
    res = model.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}, strict=False)
    assert sorted(res.missing_keys) == sorted(gate_keys) and not res.unexpected_keys
    assert all(float(p.detach()) == float(want) for p in model.softplus_parameters())
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}, strict=True)
    for on in (True, False):                       # validated with the feature off as well
        with pytest.raises(ValueError):
            DwiseNeuro(**TINY, learnable_softplus=on, softplus_param="sqrt")


def _mouse_model(extra=None, **kw):
    from sensorium_amd.argus_models import MouseModel
    params = {"nn_module": ("dwiseneuro", dict(TINY, **kw)), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", {"lr": 3e-4, "weight_decay": 0.05, "betas": (0.8, 0.99)}), "device": "cpu"}
    params.update(extra or {})
    return MouseModel(params)


def test_mouse_model_param_groups():
    m = _mouse_model(learnable_softplus=True)
    groups = m.get_optimizer().param_groups
    assert len(groups) == 2
    gate = m.nn_module.softplus_parameters()
    assert [id(p) for p in groups[1]["params"]] == [id(p) for p in gate] and len(gate) == 2
    assert not {id(p) for p in groups[0]["params"]} & {id(p) for p in gate}
    assert len(groups[0]["params"]) + 2 == len(list(m.nn_module.parameters()))
    assert groups[1]["weight_decay"] == 0.0 and groups[0]["weight_decay"] == 0.05
    assert groups[1]["lr"] == groups[0]["lr"] == 3e-4 and tuple(groups[1]["betas"]) == tuple(groups[0]["betas"]) == (0.8, 0.99)
    # set_lr / get_lr and a per-iteration scheduler see two groups
    m.set_lr(1e-3)
    assert m.get_lr() == [1e-3, 1e-3]
    sched = torch.optim.lr_scheduler.LambdaLR(m.optimizer, lambda it: 0.5)
    assert [g["lr"] for g in m.optimizer.param_groups] == [5e-4, 5e-4] and sched.get_last_lr() == [5e-4, 5e-4]
    # the override is merged over the defaults
    m2 = _mouse_model({"softplus_optimizer": {"lr": 1e-2}}, learnable_softplus=True, softplus_param="log")
    g2 = m2.get_optimizer().param_groups
    assert g2[1]["lr"] == 1e-2 and g2[1]["weight_decay"] == 0.0 and g2[0]["lr"] == 3e-4
    # off: one group, every parameter, as before
    m3 = _mouse_model()
    g3 = m3.get_optimizer().param_groups
    assert len(g3) == 1 and [id(p) for p in g3[0]["params"]] == [id(p) for p in m3.nn_module.parameters()]


def test_ema_copies_follow_the_optimizer_order():
    m = _mouse_model(learnable_softplus=True)
    m.set_ema(0.99)
    opt = m.get_optimizer()
    ema_names = {id(p): n for n, p in m.model_ema.ema.named_parameters()}
    names = {id(p): n for n, p in m.nn_module.named_parameters()}
    flat = [p for g in opt.param_groups for p in g["params"]]
    assert len(opt._ema_of) == len(flat)
    for p in flat:
        assert ema_names[id(opt._ema_of[id(p)])] == names[id(p)]
    assert names[id(flat[-1])] == "readouts.1.gate.beta"
    assert opt.folds_ema_of(m.model_ema)


def test_abi_struct_and_header():
    import sensorium_amd._lib as L
    assert L.lib.dwn_abi_version() == 7
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header)
    assert L.lib.dwn_sizeof(b"dwn_readout_args") == C.sizeof(L.ReadoutArgs)
    assert L.lib.dwn_sizeof(b"dwn_gemm_nn_args") == C.sizeof(L.GemmNNArgs)
    # appended behind the last field there was; zero-initialised by ctypes, so an existing caller passes two nulls
    assert L.ReadoutArgs.beta_dev.offset > L.ReadoutArgs.f32_products.offset and L.ReadoutArgs.dbeta.offset == L.ReadoutArgs.beta_dev.offset + 8
    assert C.sizeof(L.ReadoutArgs) == L.ReadoutArgs.dbeta.offset + 8
    assert L.GemmNNArgs.sp_beta_dev.offset > L.GemmNNArgs.variant.offset
    a = L.ReadoutArgs()
    assert a.beta_dev is None and a.dbeta is None
    assert re.search(r"const float\* beta_dev; float\* dbeta;", header) and "const float* sp_beta_dev;" in header


def test_backward_refuses_half_a_pair_and_workspace_accounts_for_the_partials():
    import sensorium_amd._lib as L
    a = L.ReadoutArgs()
    a.dtype = L.DWN_F32; a.B = 3; a.T = 5; a.Cin = 16; a.groups = 2; a.n_out = 130
    base = L.lib.dwn_readout_workspace_bytes(C.byref(a), 1)
    fwd = L.lib.dwn_readout_workspace_bytes(C.byref(a), 0)
    a.beta_dev = PTR
    # Rp = 128 per group: 4 tiles of 64 neurons x 3 samples = 12 float64 partials, carved on a 256-byte boundary
    assert L.lib.dwn_readout_workspace_bytes(C.byref(a), 1) == (base - 256 + 255) // 256 * 256 + 12 * 8 + 256
    assert L.lib.dwn_readout_workspace_bytes(C.byref(a), 0) == fwd               # the forward needs none
    for beta_dev, dbeta in ((PTR, None), (None, PTR)):
        a.beta_dev, a.dbeta = beta_dev, dbeta
        assert L.lib.dwn_readout_backward(C.byref(a), 10 ** 6, None) == -2       # (a device index no machine has: never entered)
        assert b"beta_dev and dbeta" in L.lib.dwn_last_error()

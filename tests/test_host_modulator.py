"""CPU tests of the host side of the behaviour modulator: DwiseNeuro and DwiseNeuroGaze are untouched,
DwiseNeuroBehavior appends ``shifter.*`` (when asked) and ``modulator.*`` behind the reference keys and starts as the identity,
MouseModel builds it with its optimizer and EMA copies, the three C-ABI entries are declared, exported and bound, and every
argument check answers before a device is entered.  No kernel runs here."""
import ctypes as C
import inspect
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
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)


def _ref_keys(golden_dir):
    z = np.load(golden_dir / "tiny_model_eval.npz")
    return z, [k[3:] for k in z.files if k.startswith("sd:")]


def test_base_classes_are_untouched(golden_dir):
    from sensorium_amd import DwiseNeuro, DwiseNeuroGaze
    _, ref_keys = _ref_keys(golden_dir)
    names = list(inspect.signature(DwiseNeuro.__init__).parameters)
    assert names[-3:] == ["compute_dtype", "learnable_softplus", "softplus_param"]
    assert "modulator" not in names and "gaze_shifter" not in names
    plain = DwiseNeuro(**TINY)
    assert list(plain.state_dict().keys()) == ref_keys
    assert "modulator" not in repr(plain) and not hasattr(plain, "modulator") and not hasattr(plain, "shifter")
    assert list(inspect.signature(DwiseNeuroGaze.__init__).parameters) == ["self", "args", "gaze_shifter", "kwargs"]
    gaze = DwiseNeuroGaze(**TINY)
    keys = list(gaze.state_dict().keys())
    assert keys[:len(ref_keys)] == ref_keys and all(k.startswith("shifter.") for k in keys[len(ref_keys):])
    assert "modulator" not in repr(gaze) and not hasattr(gaze, "modulator")


@pytest.mark.parametrize("with_shifter", [False, True])
def test_behavior_model_keys_and_initial_state(golden_dir, with_shifter):
    from sensorium_amd import BehaviorModulator, DwiseNeuro, DwiseNeuroBehavior, GazeShifter
    z, ref_keys = _ref_keys(golden_dir)
    model = DwiseNeuroBehavior(**TINY, gaze_shifter=dict(max_shift=4.0) if with_shifter else None)
    assert isinstance(model, DwiseNeuro) and isinstance(model.modulator, BehaviorModulator)
    assert hasattr(model, "shifter") == with_shifter and (not with_shifter or isinstance(model.shifter, GazeShifter))
    keys = list(model.state_dict().keys())
    extra = keys[len(ref_keys):]
    assert keys[:len(ref_keys)] == ref_keys
    n_shift = sum(k.startswith("shifter.") for k in extra)
    assert (n_shift > 0) == with_shifter
    assert all(k.startswith("shifter.") for k in extra[:n_shift]) and all(k.startswith("modulator.") for k in extra[n_shift:])
    assert extra[n_shift:] == ["modulator.behavior_mean", "modulator.behavior_std", "modulator.mlp.0.weight", "modulator.mlp.0.bias",
                               "modulator.mlp.2.weight", "modulator.mlp.2.bias", "modulator.heads.0.weight",
                               "modulator.heads.0.bias", "modulator.heads.1.weight", "modulator.heads.1.bias"]
    # parameters: the base's in its order, then the shifter's, then the modulator's
    pnames = [n for n, _ in model.named_parameters()]
    base_pnames = [n for n, _ in DwiseNeuro(**TINY).named_parameters()]
    rest = pnames[len(base_pnames):]
    assert pnames[:len(base_pnames)] == base_pnames
    n_sp = 4 if with_shifter else 0
    assert all(n.startswith("shifter.mlp.") for n in rest[:n_sp]) and all(n.startswith("modulator.") for n in rest[n_sp:])
    assert len(rest) == n_sp + 8
    # a reference checkpoint: exactly the new keys are missing
    ref_sd = {k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}
    res = model.load_state_dict(ref_sd, strict=False)
    assert sorted(res.missing_keys) == sorted(extra) and not res.unexpected_keys
    with pytest.raises(RuntimeError):
        model.load_state_dict(ref_sd, strict=True)
    # the heads are zero: the gain is exactly 1
    assert len(model.modulator.heads) == 2
    for head, n in zip(model.modulator.heads, TINY["readout_outputs"]):
        assert head.weight.shape == (n, 8) and head.bias.shape == (n,)
        assert head.weight.dtype == head.bias.dtype == torch.float32
        assert not bool(head.weight.any()) and not bool(head.bias.any())
    assert isinstance(model.modulator.mlp[-1], torch.nn.Tanh)


def test_modulator_arguments():
    from sensorium_amd import BehaviorModulator, DwiseNeuroBehavior
    sig = inspect.signature(BehaviorModulator.__init__).parameters
    assert list(sig)[1:] == ["readout_outputs", "features", "hidden_features", "hidden_layers", "max_log_gain", "behavior_channels",
                             "derivative", "behavior_mean", "behavior_std"]
    d = {k: p.default for k, p in sig.items() if k not in ("self", "readout_outputs")}
    assert d == dict(features=8, hidden_features=16, hidden_layers=1, max_log_gain=2.0, behavior_channels=(1, 2), derivative=False,
                     behavior_mean=(0., 0.), behavior_std=(1., 1.))
    assert list(inspect.signature(DwiseNeuroBehavior.__init__).parameters) == ["self", "args", "gaze_shifter", "modulator", "kwargs"]
    m = BehaviorModulator((3, 5), features=4, hidden_features=6, hidden_layers=2, max_log_gain=1.5, derivative=True,
                          behavior_mean=(0.5, -1.0), behavior_std=(2.0, 4.0))
    lin = [q for q in m.mlp if isinstance(q, torch.nn.Linear)]
    assert [(q.in_features, q.out_features) for q in lin] == [(4, 6), (6, 6), (6, 4)]      # derivative: 2 traces + 2 differences
    assert m.state_dict()["behavior_mean"].tolist() == [0.5, -1.0] and m.state_dict()["behavior_std"].tolist() == [2.0, 4.0]
    assert m.max_log_gain == 1.5 and [tuple(h.weight.shape) for h in m.heads] == [(3, 4), (5, 4)]
    lin_model = BehaviorModulator((3,), features=None, hidden_layers=0)               # the pure linear gain model
    assert lin_model.mlp is None and tuple(lin_model.heads[0].weight.shape) == (3, 2)
    assert list(lin_model.state_dict()) == ["behavior_mean", "behavior_std", "heads.0.weight", "heads.0.bias"]
    assert tuple(BehaviorModulator((3,), features=None, hidden_layers=0, derivative=True).heads[0].weight.shape) == (3, 4)
    net = DwiseNeuroBehavior(**TINY, modulator=dict(features=None, hidden_layers=0, max_log_gain=1.0))
    assert net.modulator.max_log_gain == 1.0 and not hasattr(net, "shifter")
    for bad in (dict(behavior_mean=(0.0,)), dict(behavior_std=(1.0, 1.0, 1.0)), dict(hidden_layers=-1), dict(hidden_features=0),
                dict(features=None), dict(features=33), dict(features=0), dict(max_log_gain=0.0), dict(max_log_gain=-1.0),
                dict(max_log_gain=math.inf), dict(max_log_gain=math.nan), dict(behavior_channels=())):
        with pytest.raises(ValueError):
            BehaviorModulator((3, 5), **bad)
    with pytest.raises(ValueError):
        BehaviorModulator(())
    with pytest.raises(ValueError):
        BehaviorModulator((3, 0))


def test_mouse_model_builds_optimizer_and_ema():
    from sensorium_amd import DwiseNeuroBehavior
    from sensorium_amd.argus_models import MouseModel
    assert MouseModel.nn_module["dwiseneuro_behavior"] is DwiseNeuroBehavior
    params = {"nn_module": ("dwiseneuro_behavior", dict(TINY, gaze_shifter=dict(max_shift=4.0), modulator=dict(max_log_gain=1.5))),
              "loss": ("mice_poisson", {}), "optimizer": ("AdamW", {"lr": 3e-4, "weight_decay": 0.05}), "device": "cpu"}
    m = MouseModel(params)
    assert isinstance(m.nn_module, DwiseNeuroBehavior) and m.nn_module.modulator.max_log_gain == 1.5
    m.set_ema(0.99)
    opt = m.get_optimizer()
    assert len(opt.param_groups) == 1                                     # the ordinary group: weight decay pulls the gain to 1
    flat = [p for g in opt.param_groups for p in g["params"]]
    assert [id(p) for p in flat] == [id(p) for p in m.nn_module.parameters()]
    names = {id(p): n for n, p in m.nn_module.named_parameters()}
    ema_names = {id(p): n for n, p in m.model_ema.ema.named_parameters()}
    assert len(opt._ema_of) == len(flat)
    for p in flat:
        assert ema_names[id(opt._ema_of[id(p)])] == names[id(p)]
    assert names[id(flat[-1])] == "modulator.heads.1.bias" and opt.folds_ema_of(m.model_ema)
    assert isinstance(m.model_ema.ema, DwiseNeuroBehavior)


def test_symbols_struct_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, rtype, nargs in (("dwn_modulator_ws_bytes", "size_t", 1), ("dwn_modulator_forward", "int", 3),
                               ("dwn_modulator_backward", "int", 3)):
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        restype, argtypes = L.SYMBOLS[name]
        assert restype is (C.c_size_t if rtype == "size_t" else C.c_int) and len(argtypes) == nargs
        decl = re.search(r"%s %s\(([^;]*)\);" % (rtype, name), header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert L._STRUCTS["dwn_modulator_args"] is L.ModulatorArgs
    assert L.lib.dwn_sizeof(b"dwn_modulator_args") == C.sizeof(L.ModulatorArgs) == 120
    fields = re.search(r"typedef struct dwn_modulator_args \{(.*?)\} dwn_modulator_args;", header, re.S).group(1)
    for f, _ in L.ModulatorArgs._fields_:
        assert re.search(r"\b%s\b" % f, fields), f
    assert "dwn_modulator.hip" in L.HASH_SRCS and "dwn_modulator.hip" in (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n in ("dwn_modulator_ws_bytes", "dwn_modulator_forward", "dwn_modulator_backward")), doc


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.ModulatorArgs()
    a.B, a.N, a.T, a.K, a.max_log_gain = 3, 200, 5, 8, 2.0
    a.y = a.h = a.u = a.c = a.dout = a.dy = a.dh = a.du = a.dc = PTR
    a.out = a.ws = 2 * PTR
    a.ws_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    fwd, bwd, wsb = lib.dwn_modulator_forward, lib.dwn_modulator_backward, lib.dwn_modulator_ws_bytes
    assert fwd(None, NO_DEVICE, None) == -1 and bwd(None, NO_DEVICE, None) == -1 and wsb(None) == 0
    for f in (fwd, bwd):
        for field in ("B", "N", "T"):
            for bad in (0, -3):
                assert f(C.byref(_args(**{field: bad})), NO_DEVICE, None) == -2, field
                assert b"must be positive" in err()
        for k in (0, 33, -1):
            assert f(C.byref(_args(K=k)), NO_DEVICE, None) == -2 and b"K outside [1, 32]" in err()
        for m in (0.0, -1.0, math.nan, math.inf):
            assert f(C.byref(_args(max_log_gain=m)), NO_DEVICE, None) == -2 and b"max_log_gain" in err()
    assert wsb(C.byref(_args(K=0))) == 0 and wsb(C.byref(_args(max_log_gain=0.0))) == 0
    for field in ("y", "h", "u", "c", "out"):
        assert fwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert fwd(C.byref(_args(out=PTR)), NO_DEVICE, None) == -2 and b"alias" in err()
    for field in ("y", "h", "u", "c", "dout", "ws"):
        assert bwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert bwd(C.byref(_args(dy=None, dh=None, du=None, dc=None)), NO_DEVICE, None) == -1 and b"all null" in err()
    # the workspace: its size depends on the geometry alone (any subset of outputs fits), is a whole number of doubles, and holds
    # at least one float64 partial per reduced output
    need = wsb(C.byref(_args()))
    assert need % 8 == 0 and need >= 8 * (200 * 8 + 200 + 3 * 5 * 8)
    assert need == wsb(C.byref(_args(dy=None, dh=None, out=None, ws=None, ws_bytes=0)))
    assert bwd(C.byref(_args(ws_bytes=need - 1)), NO_DEVICE, None) == -2 and b"workspace" in err()
    assert bwd(C.byref(_args(ws_bytes=0)), NO_DEVICE, None) == -2
    assert bwd(C.byref(_args(ws=2 * PTR + 4)), NO_DEVICE, None) == -2 and b"aligned" in err()
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert fwd(C.byref(_args()), NO_DEVICE, None) > 0
    assert bwd(C.byref(_args(ws_bytes=need)), NO_DEVICE, None) > 0
    assert bwd(C.byref(_args(dy=None, dh=None, du=None)), NO_DEVICE, None) > 0
    assert fwd(C.byref(_args(K=1)), NO_DEVICE, None) > 0 and fwd(C.byref(_args(K=32)), NO_DEVICE, None) > 0


def test_functions_refuse_cpu_tensors():
    from sensorium_amd import BehaviorModulator, ops
    y, h, u, c = torch.zeros(1, 3, 2), torch.zeros(1, 2, 4), torch.zeros(3, 4), torch.zeros(3)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.ModulatorFn.apply(y, h, u, c, 2.0)
    mod = BehaviorModulator((3,), features=4)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        mod(y, h, 0)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        mod.features(torch.zeros(1, 5, 2, 4, 6))

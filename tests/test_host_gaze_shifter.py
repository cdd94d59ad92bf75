"""CPU tests of the host side of the gaze shifter: DwiseNeuro itself is untouched, DwiseNeuroGaze appends
``shifter.*`` behind the reference keys and starts as the identity, MouseModel builds it with its optimizer and EMA copies, the
three C-ABI entries are declared, exported and bound, and every argument check answers before a device is entered.  No kernel runs
here."""
import ctypes as C
import inspect
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


def test_base_class_is_untouched(golden_dir):
    from sensorium_amd import DwiseNeuro
    _, ref_keys = _ref_keys(golden_dir)
    names = list(inspect.signature(DwiseNeuro.__init__).parameters)
    assert names[-3:] == ["compute_dtype", "learnable_softplus", "softplus_param"] and "gaze_shifter" not in names
    plain = DwiseNeuro(**TINY)
    assert list(plain.state_dict().keys()) == ref_keys
    assert "shifter" not in repr(plain) and not hasattr(plain, "shifter")
    assert list(inspect.signature(DwiseNeuro.trunk).parameters) == ["self", "x", "mode_from"]
    assert inspect.signature(DwiseNeuro.trunk).parameters["mode_from"].default is None


def test_gaze_model_keys_and_initial_state(golden_dir):
    from sensorium_amd import DwiseNeuro, DwiseNeuroGaze, GazeShifter
    z, ref_keys = _ref_keys(golden_dir)
    model = DwiseNeuroGaze(**TINY)
    assert isinstance(model, DwiseNeuro) and isinstance(model.shifter, GazeShifter)
    keys = list(model.state_dict().keys())
    extra = keys[len(ref_keys):]
    assert keys[:len(ref_keys)] == ref_keys and extra and all(k.startswith("shifter.") for k in extra)
    assert "shifter.pupil_mean" in extra and "shifter.pupil_std" in extra
    # parameters: the base's, in its order, then the shifter's (registered last: the last gradient bucket under data parallelism)
    pnames = [n for n, _ in model.named_parameters()]
    base_pnames = [n for n, _ in DwiseNeuro(**TINY).named_parameters()]
    assert pnames[:len(base_pnames)] == base_pnames and all(n.startswith("shifter.mlp.") for n in pnames[len(base_pnames):])
    assert len(pnames) == len(base_pnames) + 4                      # Linear(2, 16), Linear(16, 2): weight and bias each
    # a reference checkpoint: only shifter.* is missing
    res = model.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}, strict=False)
    assert sorted(res.missing_keys) == sorted(extra) and not res.unexpected_keys
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}, strict=True)
    last = [m for m in model.shifter.mlp if isinstance(m, torch.nn.Linear)][-1]
    assert last.out_features == 2 and not bool(last.weight.any()) and not bool(last.bias.any())
    assert isinstance(model.shifter.mlp[-1], torch.nn.Tanh)


def test_shifter_arguments():
    from sensorium_amd import DwiseNeuroGaze, GazeShifter
    names = list(inspect.signature(GazeShifter.__init__).parameters)[1:]
    assert names == ["hidden_features", "hidden_layers", "max_shift", "pupil_channels", "video_channel", "fill", "pupil_mean",
                     "pupil_std"]
    d = {k: p.default for k, p in inspect.signature(GazeShifter.__init__).parameters.items() if k != "self"}
    assert d == dict(hidden_features=16, hidden_layers=1, max_shift=8.0, pupil_channels=(3, 4), video_channel=0, fill=0.0,
                     pupil_mean=(0., 0.), pupil_std=(1., 1.))
    s = GazeShifter(hidden_features=5, hidden_layers=2, max_shift=3.0, pupil_mean=(0.5, -1.0), pupil_std=(2.0, 4.0), fill=1.5)
    lin = [m for m in s.mlp if isinstance(m, torch.nn.Linear)]
    assert [(m.in_features, m.out_features) for m in lin] == [(2, 5), (5, 5), (5, 2)]
    assert s.state_dict()["pupil_mean"].tolist() == [0.5, -1.0] and s.state_dict()["pupil_std"].tolist() == [2.0, 4.0]
    assert s.max_shift == 3.0 and s.fill == 1.5
    m = DwiseNeuroGaze(**TINY, gaze_shifter=dict(hidden_layers=0, max_shift=2.0))
    assert [k for k in m.state_dict() if k.startswith("shifter.")] == ["shifter.pupil_mean", "shifter.pupil_std",
                                                                       "shifter.mlp.0.weight", "shifter.mlp.0.bias"]
    assert list(inspect.signature(DwiseNeuroGaze.__init__).parameters) == ["self", "args", "gaze_shifter", "kwargs"]
    with pytest.raises(ValueError):
        GazeShifter(pupil_mean=(0.0,))


def test_mouse_model_builds_optimizer_and_ema():
    from sensorium_amd import DwiseNeuroGaze
    from sensorium_amd.argus_models import MouseModel
    assert MouseModel.nn_module["dwiseneuro_gaze"] is DwiseNeuroGaze
    params = {"nn_module": ("dwiseneuro_gaze", dict(TINY, gaze_shifter=dict(max_shift=4.0))), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", {"lr": 3e-4, "weight_decay": 0.05}), "device": "cpu"}
    m = MouseModel(params)
    assert isinstance(m.nn_module, DwiseNeuroGaze) and m.nn_module.shifter.max_shift == 4.0
    m.set_ema(0.99)
    opt = m.get_optimizer()
    assert len(opt.param_groups) == 1                                     # no separate group for the shifter
    flat = [p for g in opt.param_groups for p in g["params"]]
    assert [id(p) for p in flat] == [id(p) for p in m.nn_module.parameters()]
    names = {id(p): n for n, p in m.nn_module.named_parameters()}
    ema_names = {id(p): n for n, p in m.model_ema.ema.named_parameters()}
    assert len(opt._ema_of) == len(flat)
    for p in flat:
        assert ema_names[id(opt._ema_of[id(p)])] == names[id(p)]
    assert names[id(flat[-1])].startswith("shifter.mlp.") and opt.folds_ema_of(m.model_ema)
    assert isinstance(m.model_ema.ema, DwiseNeuroGaze)


def test_symbols_struct_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, nargs in (("dwn_gaze_shift_forward", 3), ("dwn_gaze_shift_backward", 3), ("dwn_plane_mean", 11)):
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        restype, argtypes = L.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == nargs
        decl = re.search(r"int %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert L._STRUCTS["dwn_gaze_args"] is L.GazeArgs
    assert L.lib.dwn_sizeof(b"dwn_gaze_args") == C.sizeof(L.GazeArgs) == 80
    fields = re.search(r"typedef struct dwn_gaze_args \{(.*?)\} dwn_gaze_args;", header, re.S).group(1)
    for f, _ in L.GazeArgs._fields_:
        assert re.search(r"\b%s\b" % f, fields), f
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n in ("dwn_gaze_shift_forward", "dwn_gaze_shift_backward", "dwn_plane_mean")), doc


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.GazeArgs()
    a.B, a.Cin, a.T, a.H, a.W, a.video_channel, a.fill = 2, 5, 3, 5, 7, 0, 0.0
    a.x = a.shift = a.out = a.dout = a.dx = a.dshift = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    fwd, bwd = lib.dwn_gaze_shift_forward, lib.dwn_gaze_shift_backward
    assert fwd(None, NO_DEVICE, None) == -1 and bwd(None, NO_DEVICE, None) == -1
    for f in (fwd, bwd):
        for field in ("B", "Cin", "T", "H", "W"):
            for bad in (0, -3):
                assert f(C.byref(_args(**{field: bad})), NO_DEVICE, None) == -2, field
                assert b"must be positive" in err()
        for vc in (-1, 5):
            assert f(C.byref(_args(video_channel=vc)), NO_DEVICE, None) == -2
            assert b"video_channel" in err()
        assert f(C.byref(_args(H=1 << 16, W=1 << 15)), NO_DEVICE, None) == -2
    for field in ("x", "shift", "out"):
        assert fwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    for field in ("shift", "dout"):
        assert bwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert bwd(C.byref(_args(dx=None, dshift=None)), NO_DEVICE, None) == -1
    assert b"both null" in err()
    assert bwd(C.byref(_args(x=None)), NO_DEVICE, None) == -1 and b"dshift needs x" in err()
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert fwd(C.byref(_args()), NO_DEVICE, None) > 0
    assert bwd(C.byref(_args(dx=None)), NO_DEVICE, None) > 0 and bwd(C.byref(_args(x=None, dshift=None)), NO_DEVICE, None) > 0

    pm = lib.dwn_plane_mean
    assert pm(None, 2, 5, 3, 5, 7, 3, 2, PTR, NO_DEVICE, None) == -1 and pm(PTR, 2, 5, 3, 5, 7, 3, 2, None, NO_DEVICE, None) == -1
    for i in range(5):
        dims = [2, 5, 3, 5, 7]
        dims[i] = 0
        assert pm(PTR, *dims, 0, 1, PTR, NO_DEVICE, None) == -2 and b"must be positive" in err()
    for c0, nc in ((-1, 1), (5, 1), (3, 3), (0, 0), (4, 2), (0, 6)):
        assert pm(PTR, 2, 5, 3, 5, 7, c0, nc, PTR, NO_DEVICE, None) == -2, (c0, nc)
        assert b"outside [0, Cin)" in err()
    assert pm(PTR, 2, 5, 3, 5, 7, 3, 2, PTR, NO_DEVICE, None) > 0


def test_functions_refuse_cpu_tensors():
    from sensorium_amd import GazeShifter, ops
    x, s = torch.zeros(1, 5, 2, 4, 6), torch.zeros(1, 2, 2)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.GazeShiftFn.apply(x, s, 0, 0.0)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.PlaneMeanFn.apply(x, 3, 2)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        GazeShifter()(x)

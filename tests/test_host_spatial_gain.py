"""CPU tests of the host side of the retinotopic readout gain: DwiseNeuro is untouched, DwiseNeuroSpatial
appends ``shifter.*`` (when asked), ``spatial.*`` and ``modulator.*`` (when asked) behind the reference keys and starts as the
identity, MouseModel builds it with the positions in the no-weight-decay group, ``positions()`` speaks three units (and a delta image
through the oracle's strided depth-wise convolution shows where a cell sits), the three C-ABI entries are declared, exported and
bound, and every argument check answers before a device is entered.  No kernel runs here."""
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
HEAD_KEYS = ["spatial.project.weight", "spatial.heads.0.pos", "spatial.heads.0.weight", "spatial.heads.0.bias",
             "spatial.heads.1.pos", "spatial.heads.1.weight", "spatial.heads.1.bias"]


def _ref_keys(golden_dir):
    z = np.load(golden_dir / "tiny_model_eval.npz")
    return z, [k[3:] for k in z.files if k.startswith("sd:")]


def test_base_class_is_untouched(golden_dir):
    from sensorium_amd import DwiseNeuro
    _, ref_keys = _ref_keys(golden_dir)
    plain = DwiseNeuro(**TINY)
    assert list(plain.state_dict().keys()) == ref_keys
    assert not hasattr(plain, "spatial") and "spatial" not in repr(plain).replace("spatial_", "").replace("spat_", "")
    assert list(inspect.signature(DwiseNeuro.trunk).parameters) == ["self", "x", "mode_from"]
    sig = inspect.signature(DwiseNeuro.trunk_with_map).parameters
    assert list(sig) == ["self", "x", "mode_from"] and sig["mode_from"].default is None


@pytest.mark.parametrize("with_shifter,with_modulator", [(False, False), (True, False), (False, True), (True, True)])
def test_spatial_model_keys_and_initial_state(golden_dir, with_shifter, with_modulator):
    from sensorium_amd import BehaviorModulator, DwiseNeuro, DwiseNeuroSpatial, GazeShifter, SpatialGain
    z, ref_keys = _ref_keys(golden_dir)
    model = DwiseNeuroSpatial(**TINY, gaze_shifter=dict(max_shift=4.0) if with_shifter else None,
                              modulator=dict(features=4) if with_modulator else None)
    assert isinstance(model, DwiseNeuro) and isinstance(model.spatial, SpatialGain)
    assert hasattr(model, "shifter") == with_shifter and (not with_shifter or isinstance(model.shifter, GazeShifter))
    assert hasattr(model, "modulator") == with_modulator and (not with_modulator or isinstance(model.modulator, BehaviorModulator))
    keys = list(model.state_dict().keys())
    extra = keys[len(ref_keys):]
    assert keys[:len(ref_keys)] == ref_keys
    order = [k.split(".")[0] for k in extra]
    want = (["shifter"] if with_shifter else []) + ["spatial"] + (["modulator"] if with_modulator else [])
    assert [k for i, k in enumerate(order) if i == 0 or order[i - 1] != k] == want          # one run of each, in this order
    assert [k for k in extra if k.startswith("spatial.")] == HEAD_KEYS
    # parameters: the base's in its order, then the branches' in the same order as the keys
    pnames = [n for n, _ in model.named_parameters()]
    base_pnames = [n for n, _ in DwiseNeuro(**TINY).named_parameters()]
    rest = [n.split(".")[0] for n in pnames[len(base_pnames):]]
    assert pnames[:len(base_pnames)] == base_pnames
    assert [k for i, k in enumerate(rest) if i == 0 or rest[i - 1] != k] == want
    # a reference checkpoint: exactly the new keys are missing
    ref_sd = {k: torch.from_numpy(z["sd:" + k]) for k in ref_keys}
    res = model.load_state_dict(ref_sd, strict=False)
    assert sorted(res.missing_keys) == sorted(extra) and not res.unexpected_keys
    with pytest.raises(RuntimeError):
        model.load_state_dict(ref_sd, strict=True)
    # zero heads: the gain is exactly 1; positions uniform in [-0.5, 0.5]^2 from the seed
    assert model.spatial.project.weight.shape == (16, 16) and model.spatial.project.bias is None
    assert model.total_stride == 4 and model.spatial.stride == 4
    for head, n in zip(model.spatial.heads, TINY["readout_outputs"]):
        assert head.pos.shape == (n, 2) and head.weight.shape == (n, 16) and head.bias.shape == (n,)
        assert head.pos.dtype == head.weight.dtype == head.bias.dtype == torch.float32
        assert not bool(head.weight.any()) and not bool(head.bias.any())
        assert 0.2 < float(head.pos.detach().abs().max()) <= 0.5
    again = DwiseNeuroSpatial(**TINY)
    assert all(torch.equal(a.pos, b.pos) for a, b in zip(again.spatial.heads, model.spatial.heads))
    other = DwiseNeuroSpatial(**TINY, spatial=dict(seed=1))
    assert not torch.equal(other.spatial.heads[0].pos, model.spatial.heads[0].pos)


def test_spatial_gain_arguments():
    from sensorium_amd import DwiseNeuroSpatial, SpatialGain
    sig = inspect.signature(SpatialGain.__init__).parameters
    assert list(sig)[1:8] == ["readout_outputs", "in_features", "features", "max_log_gain", "init_range", "seed", "detach_core"]
    d = {k: p.default for k, p in sig.items() if k in ("features", "max_log_gain", "init_range", "seed", "detach_core")}
    assert d == dict(features=16, max_log_gain=1.0, init_range=0.5, seed=0, detach_core=False)
    assert list(inspect.signature(DwiseNeuroSpatial.__init__).parameters) == ["self", "args", "spatial", "gaze_shifter", "modulator",
                                                                             "kwargs"]
    direct = SpatialGain((3, 5), 12, features=None, max_log_gain=1.5, init_range=1.0)
    assert direct.project is None and [tuple(h.weight.shape) for h in direct.heads] == [(3, 12), (5, 12)]
    assert list(direct.state_dict()) == ["heads.0.pos", "heads.0.weight", "heads.0.bias", "heads.1.pos", "heads.1.weight",
                                         "heads.1.bias"]
    net = DwiseNeuroSpatial(**TINY, spatial=dict(features=4, detach_core=True))
    assert net.spatial.detach_core and net.spatial.project.weight.shape == (4, 16) and not hasattr(net, "shifter")
    assert [id(p) for p in net.position_parameters()] == [id(h.pos) for h in net.spatial.heads]
    for bad in (dict(features=0), dict(features=65), dict(max_log_gain=0.0), dict(max_log_gain=-1.0), dict(max_log_gain=math.inf),
                dict(max_log_gain=math.nan), dict(init_range=-0.1), dict(init_range=1.5)):
        with pytest.raises(ValueError):
            SpatialGain((3, 5), 16, **bad)
    with pytest.raises(ValueError):
        SpatialGain((3, 5), 65, features=None)
    with pytest.raises(ValueError):
        SpatialGain((), 16)
    with pytest.raises(ValueError):
        SpatialGain((3, 0), 16)


def test_mouse_model_parameter_groups_and_ema():
    from sensorium_amd import DwiseNeuroSpatial
    from sensorium_amd.argus_models import MouseModel
    assert MouseModel.nn_module["dwiseneuro_spatial"] is DwiseNeuroSpatial
    params = {"nn_module": ("dwiseneuro_spatial", dict(TINY, learnable_softplus=True, spatial=dict(features=4),
                                                       modulator=dict(max_log_gain=1.5))),
              "loss": ("mice_poisson", {}), "optimizer": ("AdamW", {"lr": 3e-4, "weight_decay": 0.05}), "device": "cpu"}
    m = MouseModel(params)
    assert isinstance(m.nn_module, DwiseNeuroSpatial)
    m.set_ema(0.99)
    opt = m.get_optimizer()
    names = {id(p): n for n, p in m.nn_module.named_parameters()}
    assert len(opt.param_groups) == 2 and opt.param_groups[0]["weight_decay"] == 0.05 and opt.param_groups[1]["weight_decay"] == 0.0
    assert sorted(names[id(p)] for p in opt.param_groups[1]["params"]) == sorted(
        ["readouts.0.gate.beta", "readouts.1.gate.beta", "spatial.heads.0.pos", "spatial.heads.1.pos"])
    flat = [p for g in opt.param_groups for p in g["params"]]
    assert sorted(id(p) for p in flat) == sorted(id(p) for p in m.nn_module.parameters())
    decayed = {names[id(p)] for p in opt.param_groups[0]["params"]}
    assert {"spatial.project.weight", "spatial.heads.0.weight", "spatial.heads.1.bias", "modulator.heads.0.weight"} <= decayed
    ema_names = {id(p): n for n, p in m.model_ema.ema.named_parameters()}
    for p in flat:
        assert ema_names[id(opt._ema_of[id(p)])] == names[id(p)]
    assert isinstance(m.model_ema.ema, DwiseNeuroSpatial) and opt.folds_ema_of(m.model_ema)
    # without the gate parameters the positions alone make the second group
    plain = MouseModel(dict(params, nn_module=("dwiseneuro_spatial", dict(TINY))))
    groups = plain.get_optimizer().param_groups
    assert len(groups) == 2 and [tuple(p.shape) for p in groups[1]["params"]] == [(7, 2), (10, 2)]


def test_positions_in_three_units():
    from sensorium_amd import DwiseNeuroSpatial
    net = DwiseNeuroSpatial(**TINY)
    assert net.map_size(9, 11) == (3, 3) and net.map_size(64, 64) == (16, 16)
    with torch.no_grad():
        net.spatial.heads[0].pos[:4] = torch.tensor([[-1.0, -1.0], [1.0, 1.0], [0.0, 0.5], [1.5, -7.0]])
    with pytest.raises(RuntimeError):
        net.positions(0, "cells")                                  # no forward yet and no size given
    norm = net.positions(0)
    assert norm.shape == (7, 2) and norm[:4].tolist() == [[-1.0, -1.0], [1.0, 1.0], [0.0, 0.5], [1.0, -1.0]]     # clamped
    assert not norm.requires_grad
    cells = net.positions(0, "cells", input_size=(33, 65))         # map 9 x 17: x in [0, 16], y in [0, 8]
    assert net.map_size(33, 65) == (9, 17)
    assert cells[:4].tolist() == [[0.0, 0.0], [16.0, 8.0], [8.0, 6.0], [16.0, 0.0]]
    pixels = net.positions(0, "input", input_size=(33, 65))
    assert pixels[:4].tolist() == [[0.0, 0.0], [64.0, 32.0], [32.0, 24.0], [64.0, 0.0]]
    assert torch.equal(net.spatial.positions(0, "cells", map_size=(9, 17)), cells)
    with pytest.raises(ValueError):
        net.positions(0, "pixels")


@pytest.mark.parametrize("k,stride", [(3, 2), (5, 2), (7, 2), (3, 4)])
def test_cell_j_sits_at_input_pixel_j_times_stride(k, stride):
    """A delta image through the oracle's strided depth-wise convolution with a kernel that is itself a centred delta: output cell j
    answers to input pixel j * stride exactly, with no half-pixel term (padding k // 2 centres tap k // 2 of output j on it).  Two
    such layers compose to j * s1 * s2: the statement ``positions(units="input")`` makes."""
    from oracle import dwiseneuro_oracle as orc
    h, w = 13, 17
    weight = torch.zeros(1, 1, 1, k, k, dtype=torch.float64)
    weight[0, 0, 0, k // 2, k // 2] = 1.0
    for jy, jx in ((0, 0), (2, 3), ((h - 1) // stride, (w - 1) // stride)):
        x = torch.zeros(1, 1, h, w, 1, dtype=torch.float64)
        x[0, 0, jy * stride, jx * stride, 0] = 1.0
        y = orc.dw_spatial(x, weight, stride)
        assert y.shape[2:4] == ((h - 1) // stride + 1, (w - 1) // stride + 1)
        assert float(y[0, 0, jy, jx, 0]) == 1.0 and float(y.sum()) == 1.0
        if stride == 2:                                             # a pixel between two cells reaches neither through the centre tap
            x = torch.zeros(1, 1, h, w, 1, dtype=torch.float64)
            x[0, 0, 1, 1, 0] = 1.0
            assert float(orc.dw_spatial(x, weight, stride).sum()) == 0.0
    x = torch.zeros(1, 1, h, w, 1, dtype=torch.float64)
    x[0, 0, 8, 12, 0] = 1.0                                         # two layers of stride 2: cell (2, 3) of the second map
    y = orc.dw_spatial(orc.dw_spatial(x, weight, 2), weight, 2)
    assert float(y[0, 0, 2, 3, 0]) == 1.0 and float(y.sum()) == 1.0


def test_symbols_struct_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, rtype, nargs in (("dwn_spatial_gain_ws_bytes", "size_t", 1), ("dwn_spatial_gain_forward", "int", 3),
                               ("dwn_spatial_gain_backward", "int", 3)):
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        restype, argtypes = L.SYMBOLS[name]
        assert restype is (C.c_size_t if rtype == "size_t" else C.c_int) and len(argtypes) == nargs
        decl = re.search(r"%s %s\(([^;]*)\);" % (rtype, name), header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    order = [list(L.SYMBOLS).index(n) for n in ("dwn_modulator_backward", "dwn_spatial_gain_ws_bytes", "dwn_spatial_gain_forward",
                                                "dwn_spatial_gain_backward")]
    assert order == sorted(order)                                   # appended behind the earlier entries, in the header's order
    assert L._STRUCTS["dwn_spatial_gain_args"] is L.SpatialGainArgs
    assert L.lib.dwn_sizeof(b"dwn_spatial_gain_args") == C.sizeof(L.SpatialGainArgs) == 144
    fields = re.search(r"typedef struct dwn_spatial_gain_args \{(.*?)\} dwn_spatial_gain_args;", header, re.S).group(1)
    for f, _ in L.SpatialGainArgs._fields_:
        assert re.search(r"\b%s\b" % f, fields), f
    makefile = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    for src in ("dwn_spatial.hip", "dwn_gain.h"):
        assert src in L.HASH_SRCS and src in makefile
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n in ("dwn_spatial_gain_ws_bytes", "dwn_spatial_gain_forward", "dwn_spatial_gain_backward")), doc


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.SpatialGainArgs()
    a.B, a.N, a.T, a.Hf, a.Wf, a.K, a.g_dtype, a.max_log_gain = 3, 200, 5, 8, 8, 16, L.DWN_BF16, 1.0
    a.y = a.g = a.pos = a.weight = a.bias = a.dout = a.dy = a.dg = a.dpos = a.dweight = a.dbias = PTR
    a.out = a.ws = 2 * PTR
    a.ws_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    fwd, bwd, wsb = lib.dwn_spatial_gain_forward, lib.dwn_spatial_gain_backward, lib.dwn_spatial_gain_ws_bytes
    assert fwd(None, NO_DEVICE, None) == -1 and bwd(None, NO_DEVICE, None) == -1 and wsb(None) == 0
    for f in (fwd, bwd):
        for field in ("B", "N", "T", "Hf", "Wf"):
            for bad in (0, -3):
                assert f(C.byref(_args(**{field: bad})), NO_DEVICE, None) == -2, field
                assert b"must be positive" in err()
        for k in (0, 65, -1):
            assert f(C.byref(_args(K=k)), NO_DEVICE, None) == -2 and b"K outside [1, 64]" in err()
        for hf, wf in ((16, 17), (257, 1), (1, 257)):
            assert f(C.byref(_args(Hf=hf, Wf=wf)), NO_DEVICE, None) == -2 and b"above 256" in err()
        for dt in (2, -1):
            assert f(C.byref(_args(g_dtype=dt)), NO_DEVICE, None) == -2 and b"g_dtype" in err()
        for m in (0.0, -1.0, math.nan, math.inf):
            assert f(C.byref(_args(max_log_gain=m)), NO_DEVICE, None) == -2 and b"max_log_gain" in err()
    assert wsb(C.byref(_args(K=0))) == 0 and wsb(C.byref(_args(max_log_gain=0.0))) == 0 and wsb(C.byref(_args(Hf=32, Wf=32))) == 0
    for field in ("y", "g", "pos", "weight", "bias", "out"):
        assert fwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert fwd(C.byref(_args(out=PTR)), NO_DEVICE, None) == -2 and b"alias" in err()
    for field in ("y", "g", "pos", "weight", "bias", "dout", "ws"):
        assert bwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert bwd(C.byref(_args(dy=None, dg=None, dpos=None, dweight=None, dbias=None)), NO_DEVICE, None) == -1 and b"all null" in err()
    # the workspace: its size depends on the sizes B, N, T, Hf * Wf, K alone (not on the dtype, the pointers or the outputs asked
    # for), is a multiple of 16 bytes and holds a float64 partial per reduced output, the per-neuron table, a bucket of up to N
    # (neuron, weight) pairs per cell and s as [B][N][T] fp32
    need = wsb(C.byref(_args()))
    assert need % 16 == 0 and need >= 8 * (200 * 16 + 3 * 200) + 200 * 40 + 64 * 200 * 8 + 4 * 3 * 200 * 5
    assert need == wsb(C.byref(_args(dy=None, dg=None, out=None, ws=None, ws_bytes=0, g=PTR + 4)))
    assert need == wsb(C.byref(_args(Hf=4, Wf=16, g_dtype=L.DWN_F32)))
    for field, v in (("B", 4), ("N", 201), ("T", 40), ("K", 17), ("Hf", 9)):
        assert wsb(C.byref(_args(**{field: v}))) > need, field
    assert bwd(C.byref(_args(ws_bytes=need - 1)), NO_DEVICE, None) == -2 and b"workspace" in err()
    assert bwd(C.byref(_args(ws_bytes=0)), NO_DEVICE, None) == -2
    assert bwd(C.byref(_args(ws=2 * PTR + 8)), NO_DEVICE, None) == -2 and b"aligned" in err()
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert fwd(C.byref(_args()), NO_DEVICE, None) > 0
    assert bwd(C.byref(_args(ws_bytes=need)), NO_DEVICE, None) > 0
    assert bwd(C.byref(_args(dy=None, dpos=None, dweight=None, dbias=None)), NO_DEVICE, None) > 0
    assert fwd(C.byref(_args(K=1, Hf=1, Wf=1)), NO_DEVICE, None) > 0 and fwd(C.byref(_args(K=64, Hf=16, Wf=16)), NO_DEVICE, None) > 0


def test_functions_refuse_cpu_tensors():
    from sensorium_amd import SpatialGain, ops
    y, g = torch.zeros(1, 3, 2), torch.zeros(1, 2, 2, 2, 4)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.SpatialGainFn.apply(y, g, torch.zeros(3, 2), torch.zeros(3, 4), torch.zeros(3), 1.0)
    mod = SpatialGain((3,), 4, features=None)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        mod(y, g, 0)
    assert mod.project_map(g) is g and mod._map_size == (2, 2)

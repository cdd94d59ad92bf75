"""CPU tests of the frozen-statistics BatchNorm mode's host side (include/dwn.h DWN_BN_FROZEN, dwn_stem_input_grad): the library
loads without a GPU, ABI 7, the new entry is exported and its struct agrees between header and ctypes, the workspace functions take
mode 2, and the mode checks of the backward entries answer before anything touches a device."""
import ctypes as C
import re
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]


def _block(L, training, dtype):
    a = L.BlockArgs(); a.dtype = dtype; a.B = 2; a.T = 4; a.Hin = 8; a.Win = 16; a.Hout = 8; a.Wout = 16
    a.Cin = 64; a.Cmid = 448; a.Cout = 64; a.stride = 1; a.ks = 3; a.kt = 5; a.se_r = 14; a.training = training
    return a


def test_abi_and_new_entry():
    import sensorium_amd._lib as L
    assert L.lib.dwn_abi_version() == 7
    assert hasattr(L.lib, "dwn_stem_input_grad") and "dwn_stem_input_grad" in L.SYMBOLS
    assert L.lib.dwn_sizeof(b"dwn_stem_input_grad_args") == C.sizeof(L.StemInputGradArgs)
    header = (ROOT / "include" / "dwn.h").read_text()
    for name, value in (("DWN_BN_EVAL", L.BN_EVAL), ("DWN_BN_TRAIN", L.BN_TRAIN), ("DWN_BN_FROZEN", L.BN_FROZEN)):
        assert int(re.search(rf"#define {name} (\d+)", header).group(1)) == value
    # the header's struct, field by field, against the ctypes mirror
    body = re.search(r"typedef struct dwn_stem_input_grad_args \{(.*?)\} dwn_stem_input_grad_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n.strip(" *") for decl in body.split(";") if decl.strip()
              for n in re.sub(r"^\s*(const\s+)?(long long|int|float|void|double)\b", "", decl.strip()).split(",")]
    assert fields == [f[0] for f in L.StemInputGradArgs._fields_]
    assert "dwn_stem_input_grad_args" in L._STRUCTS


def test_workspace_functions_accept_frozen_mode():
    import sensorium_amd._lib as L
    for dtype in (L.DWN_F32, L.DWN_BF16):
        for y1_mode in (0, 1, 2):
            sizes = {}
            for training in (L.BN_TRAIN, L.BN_FROZEN):
                a = _block(L, training, dtype); a.y1_mode = y1_mode
                sizes[training] = (L.lib.dwn_block_workspace_bytes(C.byref(a), 0), L.lib.dwn_block_workspace_bytes(C.byref(a), 1),
                                   L.lib.dwn_block_forward_writes(C.byref(a)))
            assert sizes[L.BN_FROZEN] == sizes[L.BN_TRAIN] and min(sizes[L.BN_FROZEN][:2]) > 0
        c = L.CortexArgs(); c.dtype = dtype; c.B = 2; c.T = 4; c.Cin = 64; c.C = 128; c.groups = 2
        got = []
        for training in (L.BN_TRAIN, L.BN_FROZEN):
            c.training = training
            got.append((L.lib.dwn_cortex_workspace_bytes(C.byref(c), 0), L.lib.dwn_cortex_workspace_bytes(C.byref(c), 1)))
        assert got[0] == got[1] and min(got[1]) > 0
        s = L.StemArgs(); s.dtype = dtype; s.training = L.BN_FROZEN; s.B = 2; s.Cin = 5; s.C0 = 64; s.S = 128
        assert L.lib.dwn_stem_workspace_bytes(C.byref(s)) > 0


def test_mode_checks_answer_without_a_device():
    """mode 0 keeps its -7; mode 2 passes the mode check (what follows needs a device: on a host without one the call comes back
    with the runtime's error, on a GPU box with a workspace error — never with -7)."""
    import sensorium_amd._lib as L
    a = _block(L, L.BN_EVAL, L.DWN_BF16)
    assert L.lib.dwn_block_backward(C.byref(a), 0, None) == -7
    assert b"frozen" in L.lib.dwn_last_error()
    a.training = L.BN_FROZEN
    rc = L.lib.dwn_block_backward(C.byref(a), 0, None)
    assert rc != 0 and rc != -7 and L.lib.dwn_last_error()
    c = L.CortexArgs(); c.dtype = L.DWN_BF16; c.training = L.BN_EVAL; c.B = 2; c.T = 4; c.Cin = 64; c.C = 128; c.groups = 2
    assert L.lib.dwn_cortex_backward(C.byref(c), 0, None) == -7
    c.training = L.BN_FROZEN
    rc = L.lib.dwn_cortex_backward(C.byref(c), 0, None)
    assert rc != 0 and rc != -7
    # the new entry: null pointers, a bad width, the modes that are not built — all before the device is touched
    g = L.StemInputGradArgs(); g.dtype = L.DWN_BF16; g.training = L.BN_FROZEN; g.B = 2; g.Cin = 5; g.C0 = 64; g.S = 128
    assert L.lib.dwn_stem_input_grad(C.byref(g), 0, None) == -1
    g.w = g.coef = g.dout = g.dx = 256          # never dereferenced on the host
    g.C0 = 60
    assert L.lib.dwn_stem_input_grad(C.byref(g), 0, None) == -2
    g.C0 = 64
    for mode in (L.BN_EVAL, L.BN_TRAIN):
        g.training = mode
        assert L.lib.dwn_stem_input_grad(C.byref(g), 0, None) == -7


def test_mode_selection_is_host_logic():
    """ops.bn_mode / wants_frozen: eval + grad enabled + (input requires grad or the switch); the model's scope overrides."""
    from sensorium_amd import _lib as L, ops
    x = torch.zeros(2)
    xg = torch.zeros(2, requires_grad=True)
    assert ops.bn_mode(True, xg) == L.BN_TRAIN
    assert ops.bn_mode(False, x) == L.BN_EVAL and ops.bn_mode(False, xg) == L.BN_FROZEN
    with torch.no_grad():
        assert ops.bn_mode(False, xg) == L.BN_EVAL and not ops.wants_frozen(xg, True)
    assert ops.wants_frozen(x, True) and not ops.wants_frozen(x, False)
    with ops.bn_mode_scope(L.BN_EVAL):
        assert ops.bn_mode(False, xg) == L.BN_EVAL and ops.bn_mode(True, xg) == L.BN_TRAIN
        with ops.bn_mode_scope(L.BN_FROZEN):
            assert ops.bn_mode(False, x) == L.BN_FROZEN
        assert ops.bn_mode(False, xg) == L.BN_EVAL
    assert ops.bn_mode(False, xg) == L.BN_FROZEN

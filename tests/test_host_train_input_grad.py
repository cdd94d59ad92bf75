"""CPU tests of the host side of the training-mode input gradient (include/dwn.h dwn_stem_backward_input): the entry is exported
with a ctypes prototype, the header declares it, the ABI is still 7, its argument checks answer before anything touches a device,
and the old entry still refuses batch statistics."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _stem(L, training):
    a = L.StemArgs(); a.dtype = L.DWN_BF16; a.training = training; a.B = 2; a.Cin = 5; a.C0 = 64; a.S = 128
    return a


def test_symbol_prototype_and_header():
    import sensorium_amd._lib as L
    assert L.lib.dwn_abi_version() == 7
    assert hasattr(L.lib, "dwn_stem_backward_input") and "dwn_stem_backward_input" in L.SYMBOLS
    restype, argtypes = L.SYMBOLS["dwn_stem_backward_input"]
    assert restype is C.c_int and len(argtypes) == 4 and argtypes[0] is C.POINTER(L.StemArgs)
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"int dwn_stem_backward_input\(const dwn_stem_args\* a, float\* dx, int device, void\* stream\);", header)
    # the struct the entry takes did not change: additive, ABI 7
    assert L.lib.dwn_sizeof(b"dwn_stem_args") == C.sizeof(L.StemArgs)
    # the sentences that said "not built" are gone from the three places that carried them
    assert "that are not built" not in header
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        assert "dwn_stem_backward_input" in (ROOT / doc).read_text(), doc


def test_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    a = _stem(L, L.BN_TRAIN)
    a.x = a.w = a.dout = a.dw = a.ws = a.xmom = 256; a.bn.coef = 256          # never dereferenced on the host
    a.ws_bytes = 1 << 20
    assert L.lib.dwn_stem_backward_input(C.byref(a), None, 0, None) == -1     # null dx
    assert b"stem_backward_input" in L.lib.dwn_last_error()
    for mode in (L.BN_EVAL, L.BN_FROZEN):       # mode 0 like every backward; mode 2 lives on the two older calls
        a.training = mode
        assert L.lib.dwn_stem_backward_input(C.byref(a), 256, 0, None) == -7
    a.training = L.BN_TRAIN
    a.xmom = None
    assert L.lib.dwn_stem_backward_input(C.byref(a), 256, 0, None) == -1      # the forward's moments are required
    a.xmom = 256
    a.C0 = 60
    assert L.lib.dwn_stem_backward_input(C.byref(a), 256, 0, None) == -2
    a.C0 = 256
    assert L.lib.dwn_stem_backward_input(C.byref(a), 256, 0, None) == -4
    a.C0 = 64; a.Cin = 9
    assert L.lib.dwn_stem_backward_input(C.byref(a), 256, 0, None) == -4


def test_old_entry_keeps_its_contract_and_the_workspace_did_not_grow():
    import sensorium_amd._lib as L
    g = L.StemInputGradArgs(); g.dtype = L.DWN_BF16; g.training = L.BN_TRAIN; g.B = 2; g.Cin = 5; g.C0 = 64; g.S = 128
    g.w = g.coef = g.dout = g.dx = 256
    assert L.lib.dwn_stem_input_grad(C.byref(g), 0, None) == -7
    # Q, q0 and the input means live in the workspace's moment slot: DWN_NREP x (72 moments + C0 x 9 sums) doubles + alignment
    a = _stem(L, L.BN_TRAIN)
    assert L.lib.dwn_stem_workspace_bytes(C.byref(a)) == 32 * 72 * 8 + 256 + 32 * 64 * 9 * 8 + 1024

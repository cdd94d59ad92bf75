"""CPU tests of the host side of temporal_kernel 7 and 9 (include/dwn.h: dwn_dw_temporal_wide_fwd / _bwd and the block entries): the
two entries are exported and declared, ABI 7 as before, the block's workspace and write-set functions answer for the new sizes as
they do for 5, the block check names the built set, and every refusal of the new entries comes back before a device is touched
(this file runs on a host without one)."""
import ctypes as C

import pytest


def _block(L, training, dtype, kt):
    a = L.BlockArgs(); a.dtype = dtype; a.B = 2; a.T = 4; a.Hin = 8; a.Win = 16; a.Hout = 8; a.Wout = 16
    a.Cin = 64; a.Cmid = 448; a.Cout = 64; a.stride = 1; a.ks = 3; a.kt = kt; a.se_r = 14; a.training = training
    return a


def test_abi_and_new_entries():
    import sensorium_amd._lib as L
    assert L.lib.dwn_abi_version() == 7
    for name in ("dwn_dw_temporal_wide_fwd", "dwn_dw_temporal_wide_bwd"):
        assert hasattr(L.lib, name) and name in L.SYMBOLS
    assert L.SYMBOLS["dwn_dw_temporal_wide_fwd"] == L.SYMBOLS["dwn_dw_temporal_fwd"]
    assert L.SYMBOLS["dwn_dw_temporal_wide_bwd"] == L.SYMBOLS["dwn_dw_temporal_bwd"]


def test_block_sizes_answer_for_7_and_9_as_for_5():
    import sensorium_amd._lib as L
    for dtype in (L.DWN_F32, L.DWN_BF16):
        for kt in (5, 7, 9):
            sizes = {}
            for training in (L.BN_TRAIN, L.BN_FROZEN):
                a = _block(L, training, dtype, kt)
                sizes[training] = (L.lib.dwn_block_workspace_bytes(C.byref(a), 0), L.lib.dwn_block_workspace_bytes(C.byref(a), 1),
                                   L.lib.dwn_block_forward_writes(C.byref(a)))
            assert sizes[L.BN_FROZEN] == sizes[L.BN_TRAIN] and min(sizes[L.BN_FROZEN]) > 0, (kt, sizes)


@pytest.mark.parametrize("kt", [0, 1, 2, 4, 6, 8, 11])
def test_block_check_refuses_the_rest_and_names_the_built_set(kt):
    import sensorium_amd._lib as L
    for training in (L.BN_TRAIN, L.BN_FROZEN):          # dwn_block_backward runs the block check before it enters the device
        a = _block(L, training, L.DWN_BF16, kt)
        assert L.lib.dwn_block_backward(C.byref(a), 0, None) == -4
        msg = L.lib.dwn_last_error().decode()
        assert "temporal_kernel" in msg and all(f"{k}" in msg for k in (3, 5, 7, 9)), msg


@pytest.mark.parametrize("kt", [7, 9])
def test_block_check_accepts_7_and_9(kt):
    """Past the check the call needs a device and a workspace: whatever it answers on this host, it is not the size refusal."""
    import sensorium_amd._lib as L
    a = _block(L, L.BN_TRAIN, L.DWN_BF16, kt)
    assert L.lib.dwn_block_backward(C.byref(a), 0, None) not in (0, -4)


def test_wide_entries_refuse_before_the_device():
    """Pointers are null and the device index is one no machine has: an entry that got as far as either would not answer these codes."""
    import sensorium_amd._lib as L
    nodev = 1 << 20
    for dt in (L.DWN_BF16, L.DWN_F32):
        f = L.DwTemporalFwdArgs(); f.B = 2; f.T = 6; f.HW = 9; f.C = 64
        b = L.DwTemporalBwdArgs(); b.B = 2; b.T = 6; b.HW = 9; b.C = 64; b.dy_kind = L.LD_PLAIN
        for kt in (3, 5, 11):
            f.kt = b.kt = kt
            assert L.lib.dwn_dw_temporal_wide_fwd(C.byref(f), dt, nodev, None) == -4
            assert b"7 or 9" in L.lib.dwn_last_error()
            assert L.lib.dwn_dw_temporal_wide_bwd(C.byref(b), dt, nodev, None) == -4
        for kt in (7, 9):
            f.kt = b.kt = kt
            f.C = b.C = 12
            assert L.lib.dwn_dw_temporal_wide_fwd(C.byref(f), dt, nodev, None) == -2
            assert L.lib.dwn_dw_temporal_wide_bwd(C.byref(b), dt, nodev, None) == -2
            f.C = b.C = 64
            for kind in (L.LD_AFFINE2, L.LD_DY3):
                b.dy_kind = kind
                assert L.lib.dwn_dw_temporal_wide_bwd(C.byref(b), dt, nodev, None) == -3
                msg = L.lib.dwn_last_error().decode()
                assert "3 and 5 only" in msg and "stored-y3" in msg, msg
            b.dy_kind = L.LD_PLAIN

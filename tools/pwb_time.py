#!/usr/bin/env python3
"""Time dwn_pw_backward (conv_pw data + weight gradient without y1: Bp / Gram prep, the product kernels, the fold) at the
benchmark's block shapes: the one-pass kernels of the 64- and 128-channel blocks and the two-GEMM path of the others.
--res folds the shortcut branch's gradient in where the one-pass kernel is built, in the form the block of that shape uses:
the identity map with res_C = Cin or 2 Cin, or (block 4: 18 x 32 planes, stride 2) the gathered form.  --c128: the 128-channel
shapes only (a short run for a counter pass)."""
import ctypes as C
import sys
import torch
sys.path.insert(0, ".")
import sensorium_amd._lib as L  # noqa: E402

with_res = "--res" in sys.argv          # fold a shortcut branch's gradient in (dwn_pw_bwd_args.res)
bf = torch.bfloat16
# M, E, Cin, shortcut form under --res: ("id", res_C / Cin) or ("gather", Hin, Win)
SHAPES = ((2359296, 448, 64, ("id", 1)), (589824, 448, 64, ("id", 1)),
          (589824, 896, 128, ("gather", 18, 32)),       # block 4
          (147456, 896, 128, ("id", 1)),                # block 5
          (147456, 896, 128, ("id", 2)),                # block 6
          (147456, 1792, 256, None), (40960, 1792, 256, None))
for M, E, Cin, form in SHAPES:
    if "--c128" in sys.argv and Cin != 128:
        continue
    dh1 = torch.randn(M, E, device="cuda").to(bf)
    a0 = torch.randn(M, Cin, device="cuda").to(bf)
    w1 = torch.randn(E, Cin, device="cuda") * 0.1
    abc = torch.randn(3, E, device="cuda")
    da0 = torch.empty(M, Cin, device="cuda", dtype=bf)
    dw = torch.zeros(E, Cin, device="cuda")
    nws = L.lib.dwn_pw_backward_workspace_bytes(E, Cin, L.DWN_BF16)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    a = L.PwBwdArgs()
    a.dh1, a.a0, a.w_pw, a.abc = dh1.data_ptr(), a0.data_ptr(), w1.data_ptr(), abc.data_ptr()
    a.da0, a.dw, a.M, a.E, a.Cin, a.ws, a.ws_bytes = da0.data_ptr(), dw.data_ptr(), M, E, Cin, ws.data_ptr(), nws
    fused = L.lib.dwn_pw_bwd_fused_supported(L.DWN_BF16, M, E, Cin)
    extra = 0                           # bytes of the shortcut's operand
    if with_res and fused and form:
        if form[0] == "id":
            rc, rows = form[1] * Cin, M
        else:
            _, Hin, Win = form
            Hout, Wout = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
            rc, rows = Cin, M // (Hin * Win) * Hout * Wout
            hinv = torch.full((Hin,), -1, dtype=torch.int32); hinv[::2] = torch.arange(Hout, dtype=torch.int32)
            winv = torch.full((Win,), -1, dtype=torch.int32); winv[::2] = torch.arange(Wout, dtype=torch.int32)
            hinv, winv = hinv.cuda(), winv.cuda()
            a.res_hinv, a.res_winv = hinv.data_ptr(), winv.data_ptr()
            a.res_Hin, a.res_Win, a.res_Hout, a.res_Wout = Hin, Win, Hout, Wout
        res = torch.randn(rows, rc, device="cuda").to(bf)
        rabc = torch.randn(3, rc, device="cuda")
        a.res, a.res_abc, a.res_C = res.data_ptr(), rabc.data_ptr(), rc
        extra = rows * rc * 2
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(3):
        L.check(L.lib.dwn_pw_backward(C.byref(a), L.DWN_BF16, 0, st), "pw_backward")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        L.lib.dwn_pw_backward(C.byref(a), L.DWN_BF16, 0, st)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 100
    by = M * ((1 if fused else 2) * E + (2 if fused else 3) * Cin) * 2 + extra
    print(f"M={M} E={E} Cin={Cin} one_pass={fused} res={form if with_res and fused else None} {us:.1f} us  "
          f"{by / us / 1e3:.0f} GB/s of the bytes the path has to move", flush=True)

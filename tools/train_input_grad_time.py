#!/usr/bin/env python3
"""Timing of the training-mode input gradient, HIP events, same box, alternating legs.

  stem  B=32, T=32, 36x64 (2 359 296 rows x 64 bf16): dwn_stem_backward_input against dwn_stem_backward (the difference is the
        dx pass plus its one-workgroup finaliser) and against dwn_stem_input_grad (the frozen variant of the same kernel on the
        same dout), alternating calls.  Under `rocprofv3 --kernel-trace --stats` the same leg gives the two instantiations' own
        kernel times.
  step  forward + loss + backward of the metric shape (B=32, T=32, 36x64, bf16, expansion 7, one readout) in training mode with
        and without x.requires_grad, alternating rounds.

python tools/train_input_grad_time.py [stem] [step] [--iters 6] [--rounds 4]
One process per leg and a time limit on each are the caller's: e.g. `timeout -k 10 300 python tools/train_input_grad_time.py stem`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from sensorium_amd import _lib as L
from sensorium_amd.argus_models import MouseModel
from sensorium_amd.synthetic import make_batch

dev = torch.device("cuda", 0)


def timed(fn, n):
    """n calls of fn, one HIP event pair each: list of ms"""
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def summary(ms):
    s = sorted(ms)
    return dict(median_ms=round(statistics.median(s), 4), min_ms=round(s[0], 4), max_ms=round(s[-1], 4), n=len(s))


def run_stem(args):
    B, T, H, W, Cin, C0 = 32, 32, 36, 64, 5, 64
    S = T * H * W
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, Cin, S, generator=g) * 255).to(dev)
    w = (torch.randn(C0, Cin, generator=g) * 0.02).to(dev)
    dout = torch.randn(B * S, C0, generator=g).to(torch.bfloat16).to(dev)
    out = torch.empty(B * S, C0, dtype=torch.bfloat16, device=dev)
    dx = torch.empty(B, Cin, S, device=dev)
    gamma, beta, rm, rv = (torch.ones(C0, device=dev) for _ in range(4))
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    coef = torch.empty(4 * C0, device=dev)
    xmom, dw, dgamma, dbeta = torch.zeros(72, dtype=torch.float64, device=dev), torch.empty(C0, Cin, device=dev), torch.empty(C0, device=dev), torch.empty(C0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    a = L.StemArgs()
    a.dtype = L.DWN_BF16; a.training = L.BN_TRAIN; a.B = B; a.Cin = Cin; a.C0 = C0; a.S = S; a.eps = 1e-5; a.momentum = 0.1
    a.x = x.data_ptr(); a.w = w.data_ptr(); a.xmom = xmom.data_ptr(); a.dout = dout.data_ptr(); a.dw = dw.data_ptr(); a.out = out.data_ptr()
    a.bn.gamma = gamma.data_ptr(); a.bn.beta = beta.data_ptr(); a.bn.running_mean = rm.data_ptr(); a.bn.running_var = rv.data_ptr()
    a.bn.num_batches_tracked = nbt.data_ptr(); a.bn.coef = coef.data_ptr(); a.bn.dgamma = dgamma.data_ptr(); a.bn.dbeta = dbeta.data_ptr()
    ws = torch.empty(L.lib.dwn_stem_workspace_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_stem_forward(C.byref(a), 0, stream), "dwn_stem_forward")      # real moments and coefficients
    gi = L.StemInputGradArgs()
    gi.dtype = L.DWN_BF16; gi.training = L.BN_FROZEN; gi.B = B; gi.Cin = Cin; gi.C0 = C0; gi.S = S
    gi.w = w.data_ptr(); gi.coef = coef.data_ptr(); gi.dout = dout.data_ptr(); gi.dx = dx.data_ptr()

    def bwd():
        L.check(L.lib.dwn_stem_backward(C.byref(a), 0, stream), "dwn_stem_backward")

    def bwd_dx():
        L.check(L.lib.dwn_stem_backward_input(C.byref(a), dx.data_ptr(), 0, stream), "dwn_stem_backward_input")

    def frozen():
        L.check(L.lib.dwn_stem_input_grad(C.byref(gi), 0, stream), "dwn_stem_input_grad")

    for _ in range(5):
        bwd(); bwd_dx(); frozen()
    torch.cuda.synchronize()
    t_b, t_d, t_f = [], [], []
    for _ in range(30):
        t_b += timed(bwd, 1)
        t_d += timed(bwd_dx, 1)
        t_f += timed(frozen, 1)
    rows = B * S
    mb, md, mf = (statistics.median(t) for t in (t_b, t_d, t_f))
    nbytes = rows * C0 * 2 + 2 * rows * Cin * 4
    print(json.dumps({"what": f"stem, {rows} rows x {C0} bf16", "stem_backward": summary(t_b), "stem_backward_input": summary(t_d),
                      "stem_input_grad_frozen": summary(t_f), "dx_pass_plus_finaliser_ms": round(md - mb, 4),
                      "ratio_to_frozen_pass": round((md - mb) / mf, 3), "byte_ratio": round(nbytes / (rows * C0 * 2 + rows * Cin * 4), 3),
                      "dx_pass_GBps_at_that_time": round(nbytes / (md - mb) / 1e6, 1)}), flush=True)


def run_step(args):
    params = bench.model_params(7)
    params["device"] = "cuda:0"
    torch.manual_seed(0)
    model = MouseModel(params)
    net = model.nn_module.train()
    inp, tgt = make_batch(32, 32, 36, 64, (bench.NUM_NEURONS_MOUSE0,), seed=1, device=dev)
    inputs = {"plain": inp, "x_requires_grad": inp.clone().requires_grad_()}

    def fwd_bwd(x):
        net.zero_grad(set_to_none=True)
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model.loss(net(x), tgt)
        loss.backward()

    ms = {m: [] for m in inputs}
    for _ in range(args.rounds):
        for m, x in inputs.items():
            for _ in range(2):
                fwd_bwd(x)
            torch.cuda.synchronize()
            ms[m] += timed(lambda: fwd_bwd(x), args.iters)
    out = {m: dict(summary(v), clips_per_s=round(32e3 / statistics.median(v), 2)) for m, v in ms.items()}
    diff = statistics.median(ms["x_requires_grad"]) - statistics.median(ms["plain"])
    print(json.dumps({"what": "fwd+bwd B=32 T=32 36x64 bf16, training mode", **out, "difference_ms": round(diff, 4)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["stem", "step"])
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    for what in args.what:
        {"stem": run_stem, "step": run_step}[what](args)

#!/usr/bin/env python3
"""Timing of the frozen-statistics BatchNorm mode, HIP events, same box, alternating with the comparison:

  step  forward + loss + backward of the metric shape (B=32, T=32, 36x64, bf16, expansion 7, one readout) in training mode and in
        frozen mode (model.eval().freeze_batchnorm()), in alternating rounds.  With DWN_LIB_PATH set to an older build of the
        library pass --modes train: that is the parent's figure on the same box.
  stem  dwn_stem_input_grad against dwn_stem_backward (whose accumulation pass streams the same dout once), alternating calls.
  mei   ms per ascent step of attribution.most_exciting_input on the full-width model (launch-bound sizes, no bar).

python tools/frozen_time.py [step] [stem] [mei] [--modes train,frozen] [--iters 6] [--rounds 4]
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


def lib_name():
    p = os.environ.get("DWN_LIB_PATH")
    return os.path.relpath(p, os.path.dirname(os.path.dirname(os.path.abspath(__file__)))) if p else "tree"


def summary(ms):
    s = sorted(ms)
    return dict(median_ms=round(statistics.median(s), 4), min_ms=round(s[0], 4), max_ms=round(s[-1], 4), n=len(s))


def run_step(args):
    params = bench.model_params(7)
    params["device"] = "cuda:0"
    torch.manual_seed(0)
    model = MouseModel(params)
    net = model.nn_module
    inp, tgt = make_batch(32, 32, 36, 64, (bench.NUM_NEURONS_MOUSE0,), seed=1, device=dev)

    def fwd_bwd():
        net.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model.loss(net(inp), tgt)
        loss.backward()

    def set_mode(mode):
        if mode == "train":
            net.train()
        else:
            net.eval().freeze_batchnorm()

    modes = args.modes.split(",")
    ms = {m: [] for m in modes}
    for _ in range(args.rounds):
        for m in modes:
            set_mode(m)
            for _ in range(2):
                fwd_bwd()
            torch.cuda.synchronize()
            ms[m] += timed(fwd_bwd, args.iters)
    out = {m: dict(summary(v), clips_per_s=round(32e3 / statistics.median(v), 2)) for m, v in ms.items()}
    print(json.dumps({"what": "fwd+bwd B=32 T=32 36x64 bf16", "lib": lib_name(), **out}), flush=True)


def run_stem(args):
    B, T, H, W, Cin, C0 = 32, 32, 36, 64, 5, 64
    S = T * H * W
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(B, Cin, S, generator=g) * 255).to(dev)
    w = (torch.randn(C0, Cin, generator=g) * 0.1).to(dev)
    coef = torch.cat([torch.rand(C0, generator=g) + 0.5, torch.randn(3 * C0, generator=g)]).to(dev)
    dout = torch.randn(B * S, C0, generator=g).to(torch.bfloat16).to(dev)
    dx = torch.empty(B, Cin, S, device=dev)
    gamma, beta, rm, rv = (torch.ones(C0, device=dev) for _ in range(4))
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    xmom, dw, dgamma, dbeta = torch.zeros(72, dtype=torch.float64, device=dev), torch.empty(C0, Cin, device=dev), torch.empty(C0, device=dev), torch.empty(C0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    a = L.StemArgs()
    a.dtype = L.DWN_BF16; a.training = L.BN_TRAIN; a.B = B; a.Cin = Cin; a.C0 = C0; a.S = S; a.eps = 1e-5; a.momentum = 0.1
    a.x = x.data_ptr(); a.w = w.data_ptr(); a.xmom = xmom.data_ptr(); a.dout = dout.data_ptr(); a.dw = dw.data_ptr()
    a.bn.gamma = gamma.data_ptr(); a.bn.beta = beta.data_ptr(); a.bn.running_mean = rm.data_ptr(); a.bn.running_var = rv.data_ptr()
    a.bn.num_batches_tracked = nbt.data_ptr(); a.bn.coef = coef.data_ptr(); a.bn.dgamma = dgamma.data_ptr(); a.bn.dbeta = dbeta.data_ptr()
    ws = torch.empty(L.lib.dwn_stem_workspace_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    gi = L.StemInputGradArgs()
    gi.dtype = L.DWN_BF16; gi.training = L.BN_FROZEN; gi.B = B; gi.Cin = Cin; gi.C0 = C0; gi.S = S
    gi.w = w.data_ptr(); gi.coef = coef.data_ptr(); gi.dout = dout.data_ptr(); gi.dx = dx.data_ptr()

    def bwd():
        L.check(L.lib.dwn_stem_backward(C.byref(a), 0, stream), "dwn_stem_backward")

    def ig():
        L.check(L.lib.dwn_stem_input_grad(C.byref(gi), 0, stream), "dwn_stem_input_grad")

    for _ in range(5):
        bwd(); ig()
    torch.cuda.synchronize()
    t_b, t_i = [], []
    for _ in range(30):
        t_b += timed(bwd, 1)
        t_i += timed(ig, 1)
    rows = B * S
    nbytes = rows * C0 * 2 + rows * Cin * 4
    mi = statistics.median(t_i)
    print(json.dumps({"what": f"stem dout pass, {rows} rows x {C0} bf16", "stem_backward": summary(t_b), "stem_input_grad": summary(t_i),
                      "ratio": round(mi / statistics.median(t_b), 3), "input_grad_GBps": round(nbytes / mi / 1e6, 1),
                      "fraction_of_8TBps": round(nbytes / mi / 1e6 / 8000, 3)}), flush=True)


def run_mei(args):
    from sensorium_amd import DwiseNeuro, attribution
    torch.manual_seed(0)
    net = DwiseNeuro(readout_outputs=(bench.NUM_NEURONS_MOUSE0,), expansion_ratio=7).to(dev).eval()
    neurons = list(range(0, 320, 10))
    out = {}
    for B in (1, 4, 16):
        init = torch.rand(B, 5, 16, 64, 64, device=dev) * 255

        def ascent(steps):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                attribution.most_exciting_input(net, 0, neurons, steps=steps, lr=1.0, init=init)
        ascent(3)
        torch.cuda.synchronize()
        ms = timed(lambda: ascent(10), 3)
        out[f"B={B}"] = round(statistics.median(ms) / 11, 3)       # 10 steps + the closing forward
    print(json.dumps({"what": "most_exciting_input, full width, T=16 64x64 bf16: ms per ascent step", **out}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["step", "stem", "mei"])
    ap.add_argument("--modes", default="train,frozen")
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    for what in args.what:
        {"step": run_step, "stem": run_stem, "mei": run_mei}[what](args)

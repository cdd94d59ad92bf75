#!/usr/bin/env python3
"""Timing of the depth-wise spatial kernels of size 5 and 7, HIP events, one process:

  kernels  dwn_dw_spatial_fwd / dwn_dw_spatial_bwd alone on the shapes of blocks 0, 4 and 7 of the benchmarked model (B = 32,
           T = 32: 1024 planes), bf16 and fp32, k = 3 with impl = 1 (the generic / pair kernels: the like-for-like baseline), k = 5
           and k = 7, in alternating rounds; the ratio to k = 3 beside the tap ratio (25/9, 49/9).
  step     forward + loss + backward + optimizer step of the benchmark model built with spatial_kernel = 3 and 5, alternating.

python tools/spatial_kernel_time.py [kernels] [step] [--iters 5] [--rounds 3] [--out profiles/spatial_kernel_time.txt]
Lines are printed and appended to --out."""
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
BLOCKS = {"block0": (36, 64, 448, 2), "block4": (18, 32, 896, 2), "block7": (9, 16, 1792, 2)}       # Hin, Win, E, stride
PLANES = 32 * 32


def timed(fn, n):
    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    with open(out, "a") as f:
        f.write(line + "\n")


def desc(p, ld, **kw):
    d = L.LoadDesc()
    d.p = p.data_ptr(); d.ld = ld; d.rows_per_sample = 1
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def run_kernels(args):
    stream = torch.cuda.current_stream().cuda_stream
    for name, (Hin, Win, E, stride) in BLOCKS.items():
        Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
        Min, Mout = PLANES * Hin * Win, PLANES * Hout * Wout
        for dtype, dt in ((torch.bfloat16, L.DWN_BF16), (torch.float32, L.DWN_F32)):
            g = torch.Generator(device=dev); g.manual_seed(0)
            y1 = torch.randn(Min, E, device=dev, generator=g).to(dtype)
            dh2 = torch.randn(Mout, E, device=dev, generator=g).to(dtype)
            y2 = torch.empty(Mout, E, device=dev, dtype=dtype)
            dh1 = torch.empty(Min, E, device=dev, dtype=dtype)
            coef = torch.cat([torch.rand(E, device=dev) + 0.5, torch.randn(E, device=dev) * 0.3, torch.randn(E, device=dev) * 0.2,
                              torch.rand(E, device=dev) + 0.5])
            abc = torch.randn(3 * E, device=dev) * 0.5
            st = torch.zeros(32 * 2 * E, dtype=torch.float64, device=dev)
            calls = {}
            keep = []
            for ks in (3, 5, 7):
                w = torch.randn(ks * ks, E, device=dev) / ks
                dw = torch.zeros(E, ks * ks, device=dev)
                f = L.DwSpatialFwdArgs()
                f.inp = desc(y1, E, v1=coef, v2=coef[E:], act=1)
                f.w = w.data_ptr(); f.out = y2.data_ptr(); f.planes = PLANES; f.Hin = Hin; f.Win = Win; f.Hout = Hout; f.Wout = Wout
                f.C = E; f.stride = stride; f.ks = ks; f.stats = st.data_ptr(); f.impl = 1
                b = L.DwSpatialBwdArgs()
                b.dy = desc(dh2, E, q=y2, v1=abc, v2=abc[E:], v3=abc[2 * E:])
                b.y1 = desc(y1, E, v1=coef, v2=coef[E:], v3=coef[2 * E:], v4=coef[3 * E:])
                b.w = w.data_ptr(); b.dh1 = dh1.data_ptr(); b.dw = dw.data_ptr(); b.planes = PLANES; b.Hin = Hin; b.Win = Win
                b.Hout = Hout; b.Wout = Wout; b.C = E; b.stride = stride; b.ks = ks; b.stats = st.data_ptr(); b.impl = 1
                keep += [w, dw, f, b]
                calls[("fwd", ks)] = (lambda f=f: L.check(L.lib.dwn_dw_spatial_fwd(C.byref(f), dt, 0, stream), "dwn_dw_spatial_fwd"))
                calls[("bwd", ks)] = (lambda b=b: L.check(L.lib.dwn_dw_spatial_bwd(C.byref(b), dt, 0, stream), "dwn_dw_spatial_bwd"))
            ms = {k: [] for k in calls}
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k, fn in calls.items():
                    ms[k] += timed(fn, args.iters)
            for direction in ("fwd", "bwd"):
                med = {ks: statistics.median(ms[(direction, ks)]) for ks in (3, 5, 7)}
                emit(args.out, {"what": f"dwn_dw_spatial_{direction} {name} planes={PLANES} {Hin}x{Win} E={E} stride={stride} "
                                        f"{str(dtype)[6:]}",
                                "k3_impl1_ms": round(med[3], 4), "k5_ms": round(med[5], 4), "k7_ms": round(med[7], 4),
                                "k5_over_k3": round(med[5] / med[3], 2), "k7_over_k3": round(med[7] / med[3], 2),
                                "tap_ratio_k5": round(25 / 9, 2), "tap_ratio_k7": round(49 / 9, 2),
                                "min_ms": {str(ks): round(min(ms[(direction, ks)]), 4) for ks in (3, 5, 7)},
                                "n": len(ms[(direction, 3)])})
            del y1, dh2, y2, dh1, keep, calls
            torch.cuda.empty_cache()


def run_step(args):
    batch = make_batch(32, 32, 36, 64, (bench.NUM_NEURONS_MOUSE0,), seed=1, device=dev)
    models = {}
    for ks in (3, 5):
        params = bench.model_params(7)
        params["device"] = "cuda:0"
        params["nn_module"][1]["spatial_kernel"] = ks
        torch.manual_seed(0)
        models[ks] = MouseModel(params)
    ms = {ks: [] for ks in models}
    for _ in range(args.rounds):
        for ks, model in models.items():
            for _ in range(2):
                model.train_step(batch, sync_loss=False)
            torch.cuda.synchronize()
            ms[ks] += timed(lambda: model.train_step(batch, sync_loss=False), args.iters)
    med = {ks: statistics.median(v) for ks, v in ms.items()}
    emit(args.out, {"what": "training step B=32 T=32 36x64 bf16 expansion 7, one readout (the benchmark model)",
                    "k3_ms": round(med[3], 3), "k5_ms": round(med[5], 3), "k5_over_k3": round(med[5] / med[3], 3),
                    "min_ms": {str(ks): round(min(v), 3) for ks, v in ms.items()}, "n": len(ms[3])})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "step"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spatial_kernel_time.txt"))
    args = ap.parse_args()
    for what in args.what:
        {"kernels": run_kernels, "step": run_step}[what](args)

#!/usr/bin/env python3
"""Timing of the depth-wise temporal kernels of size 7 and 9, HIP events, one process:

  kernels  the temporal forward and the y3-recomputing backward (DWN_LD_PLAIN) alone at one geometry per block width of the
           benchmarked model, (B, T, HW, C) = (32, 32, 576, 448), (32, 32, 144, 896), (32, 32, 40, 1792), bf16 and fp32: kt = 5
           (dwn_dw_temporal_fwd / _bwd, the baseline), kt = 7 and kt = 9 (dwn_dw_temporal_wide_fwd / _bwd) in alternating rounds; the
           ratio to kt = 5 beside the tap ratio (7/5, 9/5).  The bytes moved are the same at every kt.
  step     forward + loss + backward + optimizer step of the benchmark model built with temporal_kernel = 5, 7 and 9, alternating.

python tools/temporal_kernel_time.py [kernels] [step] [--iters 5] [--rounds 3] [--out profiles/temporal_kernel_time.txt]
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
GEOMS = {"blocks0-3": (32, 32, 576, 448), "blocks4-6": (32, 32, 144, 896), "blocks7-8": (32, 32, 40, 1792)}      # B, T, HW, C
KTS = (5, 7, 9)


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
    for name, (B, T, HW, E) in GEOMS.items():
        M = B * T * HW
        for dtype, dt in ((torch.bfloat16, L.DWN_BF16), (torch.float32, L.DWN_F32)):
            g = torch.Generator(device=dev); g.manual_seed(0)
            y2 = torch.randn(M, E, device=dev, generator=g).to(dtype)
            dh3 = torch.randn(M, E, device=dev, generator=g).to(dtype)
            out = torch.empty(M, E, device=dev, dtype=dtype)
            coef = torch.cat([torch.rand(E, device=dev) + 0.5, torch.randn(E, device=dev) * 0.3, torch.randn(E, device=dev) * 0.2,
                              torch.rand(E, device=dev) + 0.5])
            abc = torch.randn(3 * E, device=dev) * 0.5
            st = torch.zeros(32 * 2 * E, dtype=torch.float64, device=dev)
            calls, keep = {}, []
            for kt in KTS:
                w = torch.randn(kt, E, device=dev) / kt ** 0.5
                dw = torch.zeros(E, kt, device=dev)
                f = L.DwTemporalFwdArgs()
                f.inp = desc(y2, E, v1=coef, v2=coef[E:], act=1)
                f.w = w.data_ptr(); f.out = out.data_ptr(); f.B = B; f.T = T; f.HW = HW; f.C = E; f.kt = kt; f.stats = st.data_ptr()
                b = L.DwTemporalBwdArgs()
                b.dy = desc(dh3, E, v1=abc, v2=abc[E:], v3=abc[2 * E:]); b.dy_kind = L.LD_PLAIN
                b.y2 = desc(y2, E, v1=coef, v2=coef[E:], v3=coef[2 * E:], v4=coef[3 * E:])
                b.w = w.data_ptr(); b.dh2 = out.data_ptr(); b.dw = dw.data_ptr(); b.B = B; b.T = T; b.HW = HW; b.C = E; b.kt = kt
                b.stats = st.data_ptr()
                keep += [w, dw, f, b]
                fwd = L.lib.dwn_dw_temporal_fwd if kt <= 5 else L.lib.dwn_dw_temporal_wide_fwd
                bwd = L.lib.dwn_dw_temporal_bwd if kt <= 5 else L.lib.dwn_dw_temporal_wide_bwd
                calls[("fwd", kt)] = (lambda f=f, fwd=fwd: L.check(fwd(C.byref(f), dt, 0, stream), "temporal forward"))
                calls[("bwd", kt)] = (lambda b=b, bwd=bwd: L.check(bwd(C.byref(b), dt, 0, stream), "temporal backward"))
            ms = {k: [] for k in calls}
            for fn in calls.values():
                fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for k, fn in calls.items():
                    ms[k] += timed(fn, args.iters)
            for direction in ("fwd", "bwd"):
                med = {kt: statistics.median(ms[(direction, kt)]) for kt in KTS}
                emit(args.out, {"what": f"dw_temporal_{direction} {name} B={B} T={T} HW={HW} C={E} {str(dtype)[6:]}",
                                "kt5_ms": round(med[5], 4), "kt7_ms": round(med[7], 4), "kt9_ms": round(med[9], 4),
                                "kt7_over_kt5": round(med[7] / med[5], 2), "kt9_over_kt5": round(med[9] / med[5], 2),
                                "tap_ratio_kt7": 1.4, "tap_ratio_kt9": 1.8,
                                "min_ms": {str(kt): round(min(ms[(direction, kt)]), 4) for kt in KTS}, "n": len(ms[(direction, 5)])})
            del y2, dh3, out, keep, calls
            torch.cuda.empty_cache()


def run_step(args):
    batch = make_batch(32, 32, 36, 64, (bench.NUM_NEURONS_MOUSE0,), seed=1, device=dev)
    models = {}
    for kt in KTS:
        params = bench.model_params(7)
        params["device"] = "cuda:0"
        params["nn_module"][1]["temporal_kernel"] = kt
        torch.manual_seed(0)
        models[kt] = MouseModel(params)
    ms = {kt: [] for kt in models}
    for _ in range(args.rounds):
        for kt, model in models.items():
            for _ in range(2):
                model.train_step(batch, sync_loss=False)
            torch.cuda.synchronize()
            ms[kt] += timed(lambda: model.train_step(batch, sync_loss=False), args.iters)
    med = {kt: statistics.median(v) for kt, v in ms.items()}
    emit(args.out, {"what": "training step B=32 T=32 36x64 bf16 expansion 7, one readout (the benchmark model)",
                    "kt5_ms": round(med[5], 3), "kt7_ms": round(med[7], 3), "kt9_ms": round(med[9], 3),
                    "kt7_over_kt5": round(med[7] / med[5], 3), "kt9_over_kt5": round(med[9] / med[5], 3),
                    "min_ms": {str(kt): round(min(v), 3) for kt, v in ms.items()}, "n": len(ms[5])})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "step"])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "temporal_kernel_time.txt"))
    args = ap.parse_args()
    for what in args.what:
        {"kernels": run_kernels, "step": run_step}[what](args)

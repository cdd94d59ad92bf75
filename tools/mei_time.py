#!/usr/bin/env python3
"""Timing of the regularised-MEI kernels and of one regularised ascent step, HIP events, same process,
alternating with the comparison:

  kernels  dwn_blur3d at the two production blocks (1 x 16 x 64 x 64 and 2 x 32 x 36 x 64, radii (2, 6, 6)) against clone() of the
           same channel block; dwn_clip_moments against dwn_plane_mean of the same channel; dwn_mei_update (both modes) against
           clone().
  step     ms per ascent step of attribution.most_exciting_input on the full-width model (bf16, T = 16, 64 x 64, B = 1, 4, 16):
           the plain loop, the regularised loop eager, the regularised loop replayed from a captured graph.

python tools/mei_time.py [kernels] [step] [--reps 200] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from sensorium_amd import ops

dev = torch.device("cuda", 0)


def timed_alternating(fns, reps):
    """reps rounds over the callables, one HIP event pair per call: {name: median microseconds}"""
    for fn in fns.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    evs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs[k].append((a, b))
    torch.cuda.synchronize()
    return {k: round(statistics.median(a.elapsed_time(b) for a, b in v) * 1e3, 2) for k, v in evs.items()}


def run_kernels(args):
    for shape in ((1, 5, 16, 64, 64), (2, 5, 32, 36, 64)):
        B, C, T, H, W = shape
        g = torch.randn(shape, device=dev)
        x = torch.rand(shape, device=dev) * 255
        block = torch.randn(B, 1, T, H, W, device=dev)
        table, radii = ops.blur_taps_table([ops.gaussian_taps(s, r) for s, r in zip((0.7, 2.0, 2.0), (2, 6, 6))], dev)
        out = torch.empty(B, 1, T, H, W, device=dev)
        ws = torch.empty(out.numel(), device=dev)
        stat = torch.zeros(B, 4, dtype=torch.float64, device=dev)
        mws = torch.empty(ops.clip_moments_ws(shape), dtype=torch.float64, device=dev)
        lr = torch.ones(1, device=dev)
        ops.clip_moments(out, out=stat, ws=mws)
        fns = {
            "clone_channel_block": lambda: block.clone(),
            "blur3d": lambda: ops.blur3d(g, table, radii, out=out, ws=ws),
            "plane_mean": lambda: ops.PlaneMeanFn.apply(x, 0, 1),
            "clip_moments": lambda: ops.clip_moments(x, out=stat, ws=mws),
            "mei_update_step": lambda: ops.mei_update(x, stat, "step", g=block, lr=lr),
            "mei_update_project": lambda: ops.mei_update(x, stat, "project", mean=127.5, contrast=30.0),
        }
        ops.blur3d(g, table, radii, out=out, ws=ws)
        ops.clip_moments(out, out=stat, ws=mws)
        us = timed_alternating(fns, args.reps)
        nbytes = block.numel() * 4 * 2
        print(json.dumps({"what": "kernels, median us per call (HIP events, alternating)", "shape": list(shape), "radii": list(radii),
                          "clone_bytes": nbytes, **us, "blur_over_clone": round(us["blur3d"] / us["clone_channel_block"], 2),
                          "moments_over_plane_mean": round(us["clip_moments"] / us["plane_mean"], 2),
                          "step_over_clone": round(us["mei_update_step"] / us["clone_channel_block"], 2),
                          "project_over_clone": round(us["mei_update_project"] / us["clone_channel_block"], 2)}), flush=True)


def run_step(args):
    from sensorium_amd import DwiseNeuro, attribution
    torch.manual_seed(0)
    net = DwiseNeuro(readout_outputs=(bench.NUM_NEURONS_MOUSE0,), expansion_ratio=7).to(dev).eval()
    neurons = list(range(0, 320, 10))
    reg = dict(blur_sigma=(0.7, 2.0, 2.0), mean=127.5, contrast=30.0)
    for B in (1, 4, 16):
        init = torch.rand(B, 5, 16, 64, 64, device=dev) * 255

        def ascent(steps, **kw):
            with torch.autocast("cuda", dtype=torch.bfloat16):
                attribution.most_exciting_input(net, 0, neurons, steps=steps, lr=1.0, init=init, **kw)

        def ms_per_step(**kw):
            # (t(2 n) - t(n)) / n: the start-up of a call (buffers, the capture) and the closing forward drop out
            out = []
            for _ in range(3):
                t = []
                for n in (args.steps, 2 * args.steps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    ascent(n, **kw)
                    b.record()
                    torch.cuda.synchronize()
                    t.append(a.elapsed_time(b))
                out.append((t[1] - t[0]) / args.steps)
            return round(statistics.median(out), 3)
        for kw in (dict(), reg, dict(reg, use_graph=True)):
            ascent(3, **kw)
        torch.cuda.synchronize()
        res = {}
        for _ in range(2):                                   # alternating rounds; the last round is reported, the first shown
            res = {"plain": ms_per_step(), "regularised_eager": ms_per_step(**reg), "regularised_graph": ms_per_step(**reg, use_graph=True)}
            print(json.dumps({"what": "ms per ascent step, full width, bf16, T=16 64x64", "B": B, **res,
                              "eager_minus_plain_us": round((res["regularised_eager"] - res["plain"]) * 1e3, 1),
                              "graph_over_eager": round(res["regularised_graph"] / res["regularised_eager"], 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["kernels", "step"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    for what in args.what:
        {"kernels": run_kernels, "step": run_step}[what](args)

#!/usr/bin/env python3
"""What the drifting-Gabor stimulus costs, HIP events, one box; writes profiles/gabor_stimulus_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  dwn_gabor_forward against x.clone() of the same tensor (the bytes are the same) and dwn_gabor_backward against the dshift
           pass of dwn_gaze_shift_backward at the same shape (the nearest existing kernel: one plane family read, a float64
           fixed-order reduction per frame), taking turns in one process; at the metric shape (32 x 5 x 32 x 36 x 64) and at the
           inference window (1 x 5 x 16 x 64 x 64, the 36-row screen), both envelopes.
  ascent   one attribution.optimal_gabor step (8 starts) against one attribution.most_exciting_input step on the full-width model
           (7863 neurons, 16 x 64 x 64), each taken as (time of 5 steps - time of 1 step) / 4, taking turns in one process.
  step     the DEFAULT training step (plain ``dwiseneuro``: metric configuration, B=32 T=32 36x64 bf16, expansion 7, one readout,
           EMA) with this build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH),
           alternating parent / this / ...; reported: every process's median, the parent's own spread, whether this build lies in it.

There is no fallback: without a GPU the tool refuses to run.

python tools/gabor_stimulus_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 8]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# name -> (B, Cin, T, H, W), window
SHAPES = {"metric": ((32, 5, 32, 36, 64), None), "inference": ((1, 5, 16, 64, 64), (14, 0, 36, 64))}


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gabor_stimulus_time: no GPU; this tool measures HIP kernels and has no fallback")


def median(ms):
    return round(statistics.median(ms), 4)


def timed(fn, n):
    import torch
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        out.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in out]


def leg_kernels(args):
    import torch
    import sensorium_amd._lib as L
    from sensorium_amd.stimuli import DriftingGabor
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, (shape, window) in SHAPES.items():
        B, Cin, T, H, W = shape
        torch.manual_seed(0)
        x = torch.rand(shape, device=dev) * 255
        dout = torch.randn(shape, device=dev)
        g = DriftingGabor(B, T, (H, W), window=window, init=dict(theta=torch.linspace(0, 3, B))).to(dev)
        params = g.params.detach().contiguous()
        out, dparams = torch.empty_like(x), torch.empty_like(params)
        shift = (torch.rand(B, T, 2, device=dev) * 2 - 1) * 4
        dshift = torch.empty_like(shift)
        ga = L.GazeArgs()
        ga.B, ga.Cin, ga.T, ga.H, ga.W, ga.video_channel, ga.fill = B, Cin, T, H, W, 0, 0.0
        ga.x, ga.shift, ga.dout, ga.dshift = x.data_ptr(), shift.data_ptr(), dout.data_ptr(), dshift.data_ptr()
        legs = {"clone": lambda: x.clone(),
                "gaze_dshift": lambda: L.check(L.lib.dwn_gaze_shift_backward(C.byref(ga), 0, stream), "dwn_gaze_shift_backward")}
        keep = []
        for env, code in (("gaussian", L.GABOR_GAUSSIAN), ("none", L.GABOR_NONE)):
            a = L.GaborArgs()
            a.B, a.Cin, a.T, a.H, a.W, a.video_channel, a.envelope = B, Cin, T, H, W, 0, code
            a.clamp, a.lo, a.hi, a.background = 1, 0.0, 255.0, 127.5
            if window:
                a.y0, a.x0, a.wh, a.ww = window
            need = L.lib.dwn_gabor_workspace_bytes(C.byref(a))
            ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
            a.x, a.params, a.out, a.dout, a.dparams, a.ws, a.ws_bytes = (x.data_ptr(), params.data_ptr(), out.data_ptr(),
                                                                         dout.data_ptr(), dparams.data_ptr(), ws.data_ptr(), need)
            keep.append((a, ws))
            legs["forward_" + env] = lambda a=a: L.check(L.lib.dwn_gabor_forward(C.byref(a), 0, stream), "dwn_gabor_forward")
            legs["backward_" + env] = lambda a=a: L.check(L.lib.dwn_gabor_backward(C.byref(a), 0, stream), "dwn_gabor_backward")
        ms = {k: [] for k in legs}
        for fn in legs.values():
            timed(fn, 3)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k] += timed(fn, args.iters)
        us = {k: round(1e3 * statistics.median(v), 1) for k, v in ms.items()}
        nbytes = x.numel() * 4
        print(json.dumps({"leg": "kernels", "shape": name, "dims": shape, "window": window, "tensor_MB": round(nbytes / 1e6, 2),
                          "median_us": us,
                          "forward_over_clone": {e: round(us["forward_" + e] / us["clone"], 3) for e in ("gaussian", "none")},
                          "backward_over_gaze_dshift": {e: round(us["backward_" + e] / us["gaze_dshift"], 3) for e in ("gaussian", "none")},
                          "video_Mpixels": round(B * T * (window[2] * window[3] if window else H * W) / 1e6, 3),
                          "n": len(ms["clone"])}), flush=True)
        del x, dout, out
        torch.cuda.empty_cache()


def leg_ascent(args):
    import torch
    from sensorium_amd import DwiseNeuro, attribution
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = DwiseNeuro(readout_outputs=(7863,), expansion_ratio=6, drop_rate=0.0, drop_path_rate=0.0).to(dev).eval()
    neurons = list(range(0, 7863, 256))
    starts = dict(theta=torch.linspace(0, 2.7, 8))

    def gabor(steps):
        attribution.optimal_gabor(model, 0, neurons, starts=starts, steps=steps, lr=0.05, shape=(16, 64, 64), window=(14, 0, 36, 64))

    def mei(steps):
        attribution.most_exciting_input(model, 0, neurons, shape=(16, 64, 64), steps=steps, lr=1.0)

    def gabor1(steps):
        attribution.optimal_gabor(model, 0, neurons, starts=dict(theta=torch.zeros(1)), steps=steps, lr=0.05, shape=(16, 64, 64),
                                  window=(14, 0, 36, 64))

    legs = {"optimal_gabor_8_starts": gabor, "optimal_gabor_1_start": gabor1, "most_exciting_input": mei}
    ms = {(k, s): [] for k in legs for s in (1, 5)}
    for fn in legs.values():
        timed(lambda: fn(1), 2)
    for _ in range(args.rounds):
        for k, fn in legs.items():
            for s in (1, 5):
                ms[(k, s)] += timed(lambda: fn(s), max(args.iters // 4, 2))
    per_step = {k: round((statistics.median(ms[(k, 5)]) - statistics.median(ms[(k, 1)])) / 4, 4) for k in legs}
    print(json.dumps({"leg": "ascent", "per_step_ms": per_step,
                      "gabor_1_start_over_mei": round(per_step["optimal_gabor_1_start"] / per_step["most_exciting_input"], 3),
                      "gabor_8_starts_over_mei": round(per_step["optimal_gabor_8_starts"] / per_step["most_exciting_input"], 3),
                      "n": len(ms[("most_exciting_input", 1)])}), flush=True)


def make_model():
    import torch
    import bench
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    readouts = bench.NUM_NEURONS_ALL[:1]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    torch.manual_seed(0)
    model = MouseModel(params)
    model.set_ema(0.999)
    return model, make_batch(32, 32, 36, 64, readouts, seed=1, device=torch.device("cuda", 0))


def leg_step(args):
    model, batch = make_model()
    timed(lambda: model.train_step(batch, sync_loss=False), 3)
    ms = timed(lambda: model.train_step(batch, sync_loss=False), args.iters)
    print(json.dumps({"leg": "step", "lib": os.environ.get("DWN_LIB_PATH", "this build"), "median_ms": median(ms),
                      "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}), flush=True)


def child(leg, args, lib=None, limit=300):
    env = dict(os.environ)
    env.pop("DWN_LIB_PATH", None)
    if lib:
        env["DWN_LIB_PATH"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds", str(args.rounds),
           "--iters", str(args.iters)]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit(f"leg {leg} ({lib or 'this build'}) ended with status {res.returncode}: nothing more is started")
    rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    print(f"# {leg} ({lib or 'this build'}): {rows}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "kernels", "ascent", "step"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gabor_stimulus_time.txt"))
    args = ap.parse_args()
    require_gpu()
    if args.leg != "all":
        {"kernels": leg_kernels, "ascent": leg_ascent, "step": leg_step}[args.leg](args)
        return
    lines = ["drifting-Gabor stimulus: measured times (tools/gabor_stimulus_time.py; HIP events, one MI355X, one box)", ""]
    for r in child("kernels", args):
        lines.append(f"{r['shape']} shape {tuple(r['dims'])} window {r['window']} ({r['tensor_MB']} MB, {r['video_Mpixels']} M rendered "
                     f"pixels): median us {r['median_us']}; forward / clone {r['forward_over_clone']}, backward / gaze dshift "
                     f"{r['backward_over_gaze_dshift']}; n = {r['n']} per leg")
    lines.append("")
    for r in child("ascent", args, limit=500):
        lines.append(f"one ascent step on the full-width model, ms: {r['per_step_ms']}; optimal_gabor / most_exciting_input "
                     f"{r['gabor_1_start_over_mei']} (1 start), {r['gabor_8_starts_over_mei']} (8 starts in one batch); n = {r['n']} per point")
    lines.append("")
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        for _ in range(args.rounds):
            runs["parent"] += child("step", args, lib=args.parent_lib)
            runs["this"] += child("step", args)
        pm, tm = [r["median_ms"] for r in runs["parent"]], [r["median_ms"] for r in runs["this"]]
        lo, hi = min(pm), max(pm)
        lines += ["default training step (plain dwiseneuro), parent commit's library against this build's, alternating processes:",
                  f"  parent medians ms/step: {pm}   own run-to-run spread {lo} .. {hi}",
                  f"  this   medians ms/step: {tm}",
                  f"  this build inside the parent's spread: {[lo <= t <= hi for t in tm]}; "
                  f"median of medians: parent {median(pm)}, this {median(tm)}", ""]
    else:
        lines += ["default-step A/B against the parent commit: not run (no --parent-lib)", ""]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

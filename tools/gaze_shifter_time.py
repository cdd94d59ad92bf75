#!/usr/bin/env python3
"""What the gaze shifter costs, HIP events, one box; writes profiles/gaze_shifter_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  dwn_gaze_shift_forward / _backward (dx + dshift) / dwn_plane_mean at the metric shape (32 x 5 x 32 x 36 x 64) and the
           inference shape (90 x 5 x 16 x 64 x 64) against x.clone() of the same tensor, taking turns in one process.  The clone
           moves the same bytes as the forward; the backward also reads the two resampled-channel planes for dshift.
  step     the DEFAULT training step (plain ``dwiseneuro``: metric configuration, B=32 T=32 36x64 bf16, expansion 7, one readout,
           EMA) with this build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH),
           alternating parent / this / ...; reported: every process's median, the parent's own spread, whether this build lies in it.
  gaze     the ``dwiseneuro_gaze`` step against the ``dwiseneuro`` step, two models in one process taking turns.

There is no fallback: without a GPU the tool refuses to run.

python tools/gaze_shifter_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 8]
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
SHAPES = {"metric": (32, 5, 32, 36, 64), "inference": (90, 5, 16, 64, 64)}


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gaze_shifter_time: no GPU; this tool measures HIP kernels and has no fallback")


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
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for name, shape in SHAPES.items():
        B, Cin, T, H, W = shape
        torch.manual_seed(0)
        x = torch.rand(shape, device=dev) * 255
        dout = torch.randn(shape, device=dev)
        shift = (torch.rand(B, T, 2, device=dev) * 2 - 1) * 4
        out, dx = torch.empty_like(x), torch.empty_like(x)
        dshift, mean = torch.empty_like(shift), torch.empty(B, T, 2, device=dev)
        a = L.GazeArgs()
        a.B, a.Cin, a.T, a.H, a.W, a.video_channel, a.fill = B, Cin, T, H, W, 0, 0.0
        a.x, a.shift, a.out, a.dout, a.dx, a.dshift = (t.data_ptr() for t in (x, shift, out, dout, dx, dshift))
        legs = {
            "clone": lambda: x.clone(),
            "forward": lambda: L.check(L.lib.dwn_gaze_shift_forward(C.byref(a), 0, stream), "dwn_gaze_shift_forward"),
            "backward": lambda: L.check(L.lib.dwn_gaze_shift_backward(C.byref(a), 0, stream), "dwn_gaze_shift_backward"),
            "plane_mean": lambda: L.check(L.lib.dwn_plane_mean(x.data_ptr(), B, Cin, T, H, W, 3, 2, mean.data_ptr(), 0, stream),
                                          "dwn_plane_mean"),
        }
        ms = {k: [] for k in legs}
        for fn in legs.values():
            timed(fn, 3)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k] += timed(fn, args.iters)
        us = {k: round(1e3 * statistics.median(v), 1) for k, v in ms.items()}
        nbytes = x.numel() * 4
        print(json.dumps({"leg": "kernels", "shape": name, "dims": shape, "tensor_MB": round(nbytes / 1e6, 1), "median_us": us,
                          "forward_over_clone": round(us["forward"] / us["clone"], 3),
                          "backward_over_clone": round(us["backward"] / us["clone"], 3),
                          "clone_GBps_read_plus_write": round(2 * nbytes / us["clone"] / 1e3, 1), "n": len(ms["clone"])}), flush=True)
        del x, dout, out, dx
        torch.cuda.empty_cache()


def make_model(gaze):
    import torch
    import bench
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    readouts = bench.NUM_NEURONS_ALL[:1]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    if gaze:
        name, kw = params["nn_module"]
        params["nn_module"] = ("dwiseneuro_gaze", dict(kw, gaze_shifter=dict(pupil_mean=(100.0, 70.0), pupil_std=(20.0, 20.0))))
    torch.manual_seed(0)
    model = MouseModel(params)
    model.set_ema(0.999)
    return model, make_batch(32, 32, 36, 64, readouts, seed=1, device=torch.device("cuda", 0))


def leg_step(args):
    model, batch = make_model(False)
    timed(lambda: model.train_step(batch, sync_loss=False), 3)
    ms = timed(lambda: model.train_step(batch, sync_loss=False), args.iters)
    print(json.dumps({"leg": "step", "lib": os.environ.get("DWN_LIB_PATH", "this build"), "median_ms": median(ms),
                      "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}), flush=True)


def leg_gaze(args):
    models = {"plain": make_model(False), "gaze": make_model(True)}
    ms = {k: [] for k in models}
    for m, b in models.values():
        timed(lambda: m.train_step(b, sync_loss=False), 3)
    for _ in range(args.rounds):
        for k, (m, b) in models.items():
            ms[k] += timed(lambda: m.train_step(b, sync_loss=False), args.iters)
    print(json.dumps({"leg": "gaze", "plain_median_ms": median(ms["plain"]), "gaze_median_ms": median(ms["gaze"]),
                      "gaze_minus_plain_us": round(1e3 * (statistics.median(ms["gaze"]) - statistics.median(ms["plain"])), 1),
                      "n": len(ms["gaze"])}), flush=True)


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
    ap.add_argument("--leg", choices=["all", "kernels", "step", "gaze"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaze_shifter_time.txt"))
    args = ap.parse_args()
    require_gpu()
    if args.leg != "all":
        {"kernels": leg_kernels, "step": leg_step, "gaze": leg_gaze}[args.leg](args)
        return
    lines = ["gaze shifter: measured times (tools/gaze_shifter_time.py; HIP events, one MI355X, one box)", ""]
    for r in child("kernels", args):
        lines.append(f"{r['shape']} shape {tuple(r['dims'])} ({r['tensor_MB']} MB): median us {r['median_us']}; forward / clone "
                     f"{r['forward_over_clone']}, backward (dx + dshift) / clone {r['backward_over_clone']}; the clone moves "
                     f"{r['clone_GBps_read_plus_write']} GB/s read + write; n = {r['n']} per leg")
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
    for r in child("gaze", args, limit=500):
        lines.append(f"step with the gaze shifter {r['gaze_median_ms']} ms against the plain step {r['plain_median_ms']} ms "
                     f"(difference {r['gaze_minus_plain_us']} us; n = {r['n']} per side)")
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

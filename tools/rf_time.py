#!/usr/bin/env python3
"""What receptive-field mapping costs, HIP events, one box; writes profiles/rf_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  B = 32, N = 7863, T = 32, L = 12, a 36 x 64 window inside 64 x 64, at cell 1 and cell 2:
           dwn_sta_accumulate against the eval forward of the full-width model (expansion 7, bf16 compute, one readout of 7863
           neurons) on the same batch in the same process; the same time as a share of FLOP / 157.3 TF and of state bytes x 2 /
           the copy rate measured here; dwn_noise_forward against a clone of the tensor it writes; dwn_sta_finalize against a
           device copy of the state.
  step     the DEFAULT training step as the unchanged bench.py times it (--gpus 1 --steps K --warmup W, headline leg only), with this
           build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH), alternating parent / this.

There is no fallback: without a GPU the tool refuses to run.

python tools/rf_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 10]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, N, T, L, SIZE, WINDOW = 32, 7863, 32, 12, (64, 64), (14, 0, 36, 64)
PEAK_F32_TF = 157.3


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
    from sensorium_amd import DwiseNeuro, NoiseStimulus, ops
    dev = torch.device("cuda", 0)
    model = DwiseNeuro(readout_outputs=(N,), expansion_ratio=7, drop_rate=0.0, drop_path_rate=0.0, compute_dtype=torch.bfloat16).to(dev).eval()
    rows = {}
    for cell in (1, 2):
        stim = NoiseStimulus(B, T, SIZE, window=WINDOW, cell=cell, seed=1).to(dev)
        x = stim()
        with torch.no_grad():
            r = model(x, index=0).float().contiguous()
        r0 = r.mean(dim=(0, 2)).contiguous()
        numel = ops.sta_state_numel(N, L, WINDOW, cell)
        state = torch.zeros(numel, dtype=torch.float64, device=dev)
        G = (WINDOW[2] // cell) * (WINDOW[3] // cell)
        samples = B * (T - (L - 1))

        def forward():
            with torch.no_grad():
                model(x, index=0)

        legs = {"forward": forward,
                "accumulate": lambda: ops.sta_accumulate(state, x, r, lags=L, window=WINDOW, cell=cell, skip=L - 1, s0=127.5, r0=r0),
                "state_copy": lambda: state.clone(),
                "noise": lambda: stim(),
                "input_clone": lambda: x.clone(),
                "finalize": lambda: ops.sta_finalize(state, samples, N=N, lags=L, window=WINDOW, cell=cell)}
        ms = {k: [] for k in legs}
        for fn in legs.values():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k] += timed(fn, args.iters)
        med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
        flop = 2.0 * N * L * G * samples
        state_bytes = numel * 8
        copy_gbs = 2 * state_bytes / (med["state_copy"] * 1e-3) / 1e9            # a clone reads and writes the bytes once each
        rows[f"cell{cell}"] = {
            "cells": G, "samples_per_call": samples, "flop": flop, "state_MB": round(state_bytes / 1e6, 1), "median_ms": med,
            "n_per_leg": len(ms["accumulate"]), "accumulate_over_forward": round(med["accumulate"] / med["forward"], 3),
            "flop_floor_ms": round(flop / (PEAK_F32_TF * 1e12) * 1e3, 4), "achieved_TF": round(flop / (med["accumulate"] * 1e-3) / 1e12, 1),
            "share_of_f32_peak": round(flop / (PEAK_F32_TF * 1e12) * 1e3 / med["accumulate"], 3),
            "measured_copy_GBs": round(copy_gbs, 0), "state_traffic_floor_ms": med["state_copy"],
            "state_traffic_share": round(med["state_copy"] / med["accumulate"], 3),
            "noise_over_clone": round(med["noise"] / med["input_clone"], 3), "finalize_over_state_copy": round(med["finalize"] / med["state_copy"], 3)}
        del state
        torch.cuda.empty_cache()
    print(json.dumps({"leg": "kernels", **rows}), flush=True)


def child(cmd, lib=None, limit=300):
    env = dict(os.environ)
    env.pop("DWN_LIB_PATH", None)
    if lib:
        env["DWN_LIB_PATH"] = os.path.abspath(lib)
    res = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit(f"{cmd[0]} ({lib or 'this build'}) ended with status {res.returncode}: nothing more is started")
    rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    last = rows[-1] if rows else {}
    print(f"# {os.path.basename(cmd[0])} ({lib or 'this build'}): { {k: last[k] for k in ('ms_per_step',) if k in last} }", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "kernels"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bench-rounds", type=int, default=4)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rf_time.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rf_time: no GPU; this tool measures HIP kernels and has no fallback")
    if args.leg == "kernels":
        return leg_kernels(args)
    me = os.path.abspath(__file__)
    (r,) = child([me, "--leg", "kernels", "--rounds", str(args.rounds), "--iters", str(args.iters)], limit=400)
    lines = ["receptive-field mapping: measured times (tools/rf_time.py; HIP events, one MI355X, one box)", "",
             f"B = {B}, N = {N}, T = {T}, L = {L}, window {WINDOW[2]} x {WINDOW[3]} inside {SIZE[0]} x {SIZE[1]}; the forward is the eval forward of "
             "the full-width model (expansion 7, bf16 compute) on the same batch in the same process; medians in ms"]
    for name in ("cell1", "cell2"):
        c = r[name]
        lines += [f"  {name}: {c['cells']} cells, {c['samples_per_call']} samples per call, {c['flop']:.3e} FLOP, state {c['state_MB']} MB; n = {c['n_per_leg']} per leg",
                  f"    median ms: {c['median_ms']}",
                  f"    accumulate / forward {c['accumulate_over_forward']}; FLOP / {PEAK_F32_TF} TF = {c['flop_floor_ms']} ms = {c['share_of_f32_peak']} of the "
                  f"accumulate ({c['achieved_TF']} TF achieved)",
                  f"    state bytes x 2 / measured copy rate ({c['measured_copy_GBs']:.0f} GB/s) = {c['state_traffic_floor_ms']} ms = {c['state_traffic_share']} of the accumulate",
                  f"    noise / clone of the same tensor {c['noise_over_clone']}; finalize / device copy of the state {c['finalize_over_state_copy']}"]
    lines.append("")
    if args.parent_lib:
        bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                 "--no-cpu-baseline", "--no-inference", "--no-other-configs", "--no-rooflines"]
        runs = {"parent": [], "this": []}
        order = []
        for i in range(args.bench_rounds):              # parent, this, this, parent, ...: a drift over the call falls on both sides
            order += ["parent", "this"] if i % 2 == 0 else ["this", "parent"]
        for who in order:
            runs[who].append(child(bench, lib=args.parent_lib if who == "parent" else None, limit=400)[-1]["ms_per_step"])
        lo, hi = min(runs["parent"]), max(runs["parent"])
        lines += [f"default training step, bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} (headline leg), the parent "
                  f"commit's library against this build's, one process per leg in the order {', '.join(order)}:",
                  f"  parent ms/step: {runs['parent']}   own run-to-run spread {lo} .. {hi}",
                  f"  this   ms/step: {runs['this']}",
                  f"  this build inside the parent's spread (at or below its upper end): {[t <= hi for t in runs['this']]}; medians: parent "
                  f"{statistics.median(runs['parent'])}, this {statistics.median(runs['this'])}", ""]
    else:
        lines += ["default-step A/B against the parent commit: not run (no --parent-lib)", ""]
    text = "\n".join(lines)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

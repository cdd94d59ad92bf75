#!/usr/bin/env python3
"""What the trial-level evaluation costs, HIP events, one box; writes profiles/trial_score_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  N = 7863, 300-frame trials with the submission cut (249 kept frames), 10 groups x 5 repeats plus 10 single trials:
           the dwn_trial_moments launch (tables built once, outside the timed region) against a device clone of the same number of
           input bytes, the dwn_trial_score_finalize launch, and the host path they replace: the device-to-host copy of the same
           predictions plus metrics.corr on the cut concatenation (wall clock).  By bytes alone the moments launch reads what the
           clone reads and writes nothing, so it should be near half a clone if the second sweep stays on chip.
  step     the DEFAULT training step as the unchanged bench.py times it (--gpus 1 --steps K --warmup W, headline leg only), with this
           build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH), alternating parent / this.

There is no fallback: without a GPU the tool refuses to run.

python tools/trial_score_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, LENGTH, GROUPS, REPEATS, SINGLES = 7863, 300, 10, 5, 10


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
    import numpy as np
    import torch
    import sensorium_amd._lib as L
    from sensorium_amd import ops
    from sensorium_amd.evaluation import FrameCut
    from sensorium_amd.metrics import corr
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    first, stop = FrameCut.submission().bounds(LENGTH)
    K = stop - first
    trials, groups = [], []
    for R in [REPEATS] * GROUPS + [1] * SINGLES:
        s = torch.rand(N, LENGTH, device=dev, generator=g) * 4
        groups.append((len(trials), R, K))
        for _ in range(R):
            trials.append((0.8 * s + torch.randn(N, LENGTH, device=dev, generator=g) * 0.3, s + torch.randn(N, LENGTH, device=dev, generator=g),
                           first, K))
    td = np.zeros(len(trials), dtype=ops._TRIAL_DESC)
    for i, (p, y, f, k) in enumerate(trials):
        td[i] = (p.data_ptr(), y.data_ptr(), p.stride(0), y.stride(0), f, k)
    gd = np.array(groups, dtype=ops._TRIAL_GROUP)
    tt, gt = torch.from_numpy(td.view(np.uint8)).to(dev), torch.from_numpy(gd.view(np.uint8)).to(dev)
    state = torch.zeros(L.TRIAL_STATE_ROWS, N, dtype=torch.float64, device=dev)
    a = L.TrialScoreArgs()
    a.N, a.n_trials, a.n_groups, a.max_repeats, a.max_frames = N, len(trials), len(groups), REPEATS, K
    a.trials, a.groups, a.state = tt.data_ptr(), gt.data_ptr(), state.data_ptr()
    stream = torch.cuda.current_stream(dev).cuda_stream

    def moments():                                  # always into a state that counts as empty: the same work every time
        L.check(L.lib.dwn_trial_moments(C.byref(a), 0, stream), "dwn_trial_moments")

    counts = (len(trials) * K, GROUPS * REPEATS * K, GROUPS * K)
    kept_bytes = 2 * len(trials) * N * K * 4
    blob = torch.empty(kept_bytes, dtype=torch.uint8, device=dev)
    legs = {"clone": lambda: blob.clone(), "moments": moments, "finalize": lambda: ops.trial_scores(state, counts)}
    ms = {k: [] for k in legs}
    for fn in legs.values():
        timed(fn, 3)
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k] += timed(fn, args.iters)
    us = {k: round(1e3 * statistics.median(v), 1) for k, v in ms.items()}
    scores, summary = ops.trial_scores(state, counts)
    host = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        P = np.concatenate([p.cpu().numpy()[:, first:stop] for p, _, _, _ in trials], axis=1)
        t1 = time.perf_counter()
        Y = np.concatenate([y.cpu().numpy()[:, first:stop] for _, y, _, _ in trials], axis=1)
        t2 = time.perf_counter()
        r = corr(P, Y, axis=1)
        t3 = time.perf_counter()
        host.append((t1 - t0, t3 - t2, t2 - t1))
    diff = float(np.abs(scores[0].cpu().numpy() - r).max())
    copy_s, corr_s, tgt_s = (statistics.median(x) for x in zip(*host))
    print(json.dumps({"leg": "kernels", "trials": len(trials), "kept_frames": K, "input_MB": round(kept_bytes / 1e6, 1), "median_us": us,
                      "moments_over_clone": round(us["moments"] / us["clone"], 3), "n": len(ms["moments"]),
                      "host_ms": {"copy_predictions_to_host_and_cut": round(1e3 * copy_s, 1), "metrics_corr_float32": round(1e3 * corr_s, 1),
                                  "copy_targets_not_counted": round(1e3 * tgt_s, 1)},
                      "max_abs_difference_device_vs_host_corr": diff, "summary": [float(v) for v in summary.cpu()]}), flush=True)


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
    print(f"# {os.path.basename(cmd[0])} ({lib or 'this build'}): "
          f"{ {k: last[k] for k in ('median_us', 'moments_over_clone', 'ms_per_step') if k in last} }", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "kernels"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trial_score_time.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("trial_score_time: no GPU; this tool measures HIP kernels and has no fallback")
    if args.leg == "kernels":
        return leg_kernels(args)
    me = os.path.abspath(__file__)
    (r,) = child([me, "--leg", "kernels", "--rounds", str(args.rounds), "--iters", str(args.iters)], limit=400)
    lines = ["trial-level evaluation: measured times (tools/trial_score_time.py; HIP events, one MI355X, one box)", "",
             f"N = {N}, {r['trials']} trials of {LENGTH} frames ({GROUPS} groups x {REPEATS} repeats + {SINGLES} single), submission cut: "
             f"{r['kept_frames']} kept frames, {r['input_MB']} MB of kept prediction + target",
             f"  median us: {r['median_us']}; moments / clone of the same bytes {r['moments_over_clone']}; n = {r['n']} per leg",
             f"  the host path it replaces (wall clock, median of 3): {r['host_ms']} ms",
             f"  device single_trial_corr against metrics.corr on the float32 concatenation: at most {r['max_abs_difference_device_vs_host_corr']:.2e}",
             f"  summary {r['summary']}", ""]
    if args.parent_lib:
        bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                 "--no-cpu-baseline", "--no-inference", "--no-other-configs", "--no-rooflines"]
        runs = {"parent": [], "this": []}
        for _ in range(args.rounds):
            runs["parent"].append(child(bench, lib=args.parent_lib, limit=400)[-1]["ms_per_step"])
            runs["this"].append(child(bench, limit=400)[-1]["ms_per_step"])
        lo, hi = min(runs["parent"]), max(runs["parent"])
        lines += [f"default training step, bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} (headline leg), the parent "
                  "commit's library against this build's, alternating processes:",
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

#!/usr/bin/env python3
"""What the population-structure kernels cost, HIP events, one box; writes profiles/pairwise_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  N = 7863, 300-frame trials with the submission cut (249 kept frames), 10 groups x 5 repeats plus 10 single trials.
           Per kind: the dwn_pair_stage launch (tables built once, outside the timed region) against a device clone that moves the
           same number of bytes (a clone of X bytes reads X and writes X; the stage reads its kept input once per sweep and
           writes Z), the dwn_pair_syrk launch against torch.matmul(Z^T, Z) in float64 on the SAME staged matrix (the kernel does
           the tiles on and below the diagonal only: half the multiply-adds), and the float64 FLOP/s both reach.  Then
           dwn_pair_corr_finalize and dwn_pair_compare against a clone of one N x N float64 matrix.
  whole    population_structure (both accumulators, three kinds, three comparisons; the predictor is a stub that hands out
           device tensors, since the model's forward is not this feature's cost) against the host path: the device-to-host copy of
           the same predictions and targets plus numpy.corrcoef per matrix (wall clock).
  step     the DEFAULT training step as the unchanged bench.py times it (--gpus 1 --steps K --warmup W, headline leg only), with this
           build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH), alternating parent / this.

There is no fallback: without a GPU the tool refuses to run.

python tools/pairwise_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 5]
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
KINDS = ("total", "signal", "noise")


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


def make_trials(dev, seed, noise=1.0):
    """[(responses [N, LENGTH] on the device, group)]: a shared signal per group plus noise per trial."""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)
    out = []
    for u, R in enumerate([REPEATS] * GROUPS + [1] * SINGLES):
        s = torch.rand(N, LENGTH, device=dev, generator=g) * 4
        for _ in range(R):
            out.append((s + noise * torch.randn(N, LENGTH, device=dev, generator=g), f"video {u}" if R > 1 else None))
    return out


def leg_kernels(args):
    import torch
    import sensorium_amd._lib as L
    from sensorium_amd import ops
    from sensorium_amd.evaluation import FrameCut
    dev = torch.device("cuda", 0)
    first, stop = FrameCut.submission().bounds(LENGTH)
    K = stop - first
    trials = make_trials(dev, 0)
    groups, at = [], 0
    for R in [REPEATS] * GROUPS + [1] * SINGLES:
        groups.append((at, R, K))
        at += R
    tables = ops.pair_tables([(x, first, K) for x, _ in trials], groups, N, dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ldz = int(L.lib.dwn_pair_ldz(N))
    nt = ldz // L.PAIR_TILE
    report = {"leg": "kernels", "trials": len(trials), "kept_frames": K, "ldz": ldz, "kinds": {}}
    state = torch.zeros(N + 1, N, dtype=torch.float64, device=dev)
    for kind in KINDS:
        cols = sum(ops.pair_chunk_cols(kind, r, k) for _, r, k in groups)
        src = [(r, k) for _, r, k in groups if kind == "total" or r >= 2]
        read_bytes = 2 * sum(r * k for r, k in src) * N * 4                    # two sweeps over the kept input
        Z = torch.empty(cols * ldz, dtype=torch.float64, device=dev)
        state.zero_()
        a = L.PairArgs()
        a.N, a.kind, a.n_segs, a.n_groups = N, ops.PAIR_KINDS[kind], len(trials), len(groups)
        a.max_repeats, a.max_frames, a.cols, a.n = REPEATS, K, cols, 0
        a.segs, a.groups, a.state, a.ws, a.ws_bytes = tables[0].data_ptr(), tables[1].data_ptr(), state.data_ptr(), Z.data_ptr(), Z.numel() * 8
        blob = torch.empty((read_bytes + cols * ldz * 8) // 2, dtype=torch.uint8, device=dev)
        Zm = Z.view(cols, ldz)
        out = torch.empty(ldz, ldz, dtype=torch.float64, device=dev)
        legs = {"clone_same_bytes": lambda: blob.clone(),
                "stage": lambda: L.check(L.lib.dwn_pair_stage(C.byref(a), 0, stream), "dwn_pair_stage"),
                "syrk": lambda: L.check(L.lib.dwn_pair_syrk(C.byref(a), 0, stream), "dwn_pair_syrk"),
                "matmul_f64": lambda: torch.matmul(Zm.t(), Zm, out=out)}
        ms = {k: [] for k in legs}
        for fn in legs.values():
            timed(fn, 2)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k] += timed(fn, args.iters)
        med = {k: statistics.median(v) for k, v in ms.items()}
        # the product against the library's, once, on a fresh state: the same matrix up to the order of the sums
        state.zero_()
        legs["stage"](); legs["syrk"](); legs["matmul_f64"]()
        diff = float((state[:N] - out[:N, :N]).abs().max() / out[:N, :N].abs().max())
        useful = float(N) * N * cols                                           # multiply-adds of the lower triangle, twice = flops
        issued = nt * (nt + 1) / 2 * L.PAIR_TILE ** 2 * cols * 2
        report["kinds"][kind] = {
            "cols": cols, "Z_MB": round(cols * ldz * 8 / 1e6, 1), "stage_read_MB": round(read_bytes / 1e6, 1),
            "median_ms": {k: round(v, 3) for k, v in med.items()}, "n": len(ms["syrk"]),
            "stage_over_clone": round(med["stage"] / med["clone_same_bytes"], 3), "syrk_over_matmul": round(med["syrk"] / med["matmul_f64"], 3),
            "syrk_issued_TFLOPs": round(issued / med["syrk"] / 1e9, 2), "syrk_useful_TFLOPs_of_N2K": round(useful / med["syrk"] / 1e9, 2),
            "matmul_TFLOPs_of_2N2K": round(2.0 * ldz * ldz * cols / med["matmul_f64"] / 1e9, 2), "max_rel_difference_to_matmul": diff}
        del Z, Zm, blob, out
    # finalize and compare against a clone of one matrix
    count = len(trials) * K
    mat = torch.empty(N, N, dtype=torch.float64, device=dev)
    A = ops.pair_corr(state, GROUPS * REPEATS * K)
    B = A + 0.01 * torch.randn(N, N, dtype=torch.float64, device=dev)
    legs = {"clone_matrix": lambda: mat.clone(), "finalize_f64": lambda: ops.pair_corr(state, count),
            "finalize_f32": lambda: ops.pair_corr(state, count, dtype=torch.float32), "compare": lambda: ops.pair_compare(A, B)}
    ms = {k: [] for k in legs}
    for fn in legs.values():
        timed(fn, 2)
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k] += timed(fn, args.iters * 2)
    report["matrix_MB"] = round(N * N * 8 / 1e6, 1)
    report["matrix_median_us"] = {k: round(1e3 * statistics.median(v), 1) for k, v in ms.items()}
    print(json.dumps(report), flush=True)


class _StubPredictor:
    """Hands out device predictions made beforehand: population_structure's own cost, without a model's forward."""

    def __init__(self, dev, preds):
        self.model = type("M", (), {"device": dev})()
        self._preds = iter(preds)

    def predict_trial(self, inputs, mouse_index=None, to_numpy=True):
        return next(self._preds)


def leg_whole(args):
    import numpy as np
    import torch
    from sensorium_amd.population import population_structure
    dev = torch.device("cuda", 0)
    targets, preds = make_trials(dev, 0), make_trials(dev, 0, noise=0.3)
    trials = [(None, y, g) for y, g in targets]
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model, data, cmp_ = population_structure(_StubPredictor(dev, [p for p, _ in preds]), trials, 0)
        summaries = {k: c.summary() for k, c in cmp_.items()}                  # the one read-back per kind
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    # the host path on the data side: copy, cut, numpy.corrcoef of the total set; the signal and noise sets alike
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = [(y.cpu().numpy()[:, 50:299], g) for y, g in targets]
    t1 = time.perf_counter()
    total = np.concatenate([y for y, _ in host], axis=1).astype(np.float64)
    Rt = np.corrcoef(total)
    t2 = time.perf_counter()
    by_group = {}
    for y, g in host:
        if g is not None:
            by_group.setdefault(g, []).append(y.astype(np.float64))
    ybar = {g: np.mean(v, axis=0) for g, v in by_group.items()}
    Rs = np.corrcoef(np.concatenate(list(ybar.values()), axis=1))
    t3 = time.perf_counter()
    Rn = np.corrcoef(np.concatenate([y - ybar[g] for g, v in by_group.items() for y in v], axis=1))
    t4 = time.perf_counter()
    diffs = {k: float(np.abs(getattr(data, k).cpu().numpy() - R).max()) for k, R in (("total", Rt), ("signal", Rs), ("noise", Rn))}
    print(json.dumps({"leg": "whole", "device_wall_s_both_sides_three_kinds": [round(w, 3) for w in walls],
                      "host_s_one_side": {"copy_to_host_and_cut": round(t1 - t0, 2), "corrcoef_total": round(t2 - t1, 2),
                                          "corrcoef_signal": round(t3 - t2, 2), "corrcoef_noise": round(t4 - t3, 2)},
                      "max_abs_difference_device_vs_numpy_corrcoef": diffs, "counts": data.counts,
                      "summary_total": summaries["total"]}), flush=True)


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
    print(f"# {os.path.basename(cmd[0])} ({lib or 'this build'}): { {k: last[k] for k in ('leg', 'ms_per_step') if k in last} }", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "kernels", "whole", "step"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairwise_time.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pairwise_time: no GPU; this tool measures HIP kernels and has no fallback")
    if args.leg == "kernels":
        return leg_kernels(args)
    if args.leg == "whole":
        return leg_whole(args)
    me = os.path.abspath(__file__)
    lines = ["population structure: measured times (tools/pairwise_time.py; HIP events, one MI355X, one box)", ""]
    if args.leg == "all":
        (r,) = child([me, "--leg", "kernels", "--rounds", str(args.rounds), "--iters", str(args.iters)], limit=500)
        lines += [f"N = {N} (ldz {r['ldz']}), {r['trials']} trials of {LENGTH} frames ({GROUPS} groups x {REPEATS} repeats + {SINGLES} single), "
                  f"submission cut: {r['kept_frames']} kept frames"]
        for kind, v in r["kinds"].items():
            lines += [f"  {kind}: {json.dumps(v)}"]
        lines += [f"  one {r['matrix_MB']} MB matrix, median us: {r['matrix_median_us']}", ""]
        (w,) = child([me, "--leg", "whole"], limit=500)
        lines += [f"  whole: {json.dumps(w)}", ""]
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

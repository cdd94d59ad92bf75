#!/usr/bin/env python3
"""What the population-modes kernels cost, HIP events, one box; writes profiles/population_modes_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  N = 7863, the noise state of the profile case of section 12t (tools/pairwise_time.py: iid noise about a per-video signal)
           and the same with 16 planted shared noise sources.  dwn_modes_symm with a block of p = 24 columns against
           torch.matmul(A, Q) in float64 on the same operands and against a device clone of A (a clone reads and writes the
           matrix: half a clone is the byte floor of one read); then every other stage of a round on its own.
  whole    population.modes(k = 16, p = 24) on both matrices against torch.linalg.eigh, torch.svd_lowrank(q = 24, niter = rounds),
           torch.lobpcg(k = 16) on the same device and against the host path (read-back, scipy.sparse.linalg.eigsh).  A baseline
           that fails or is refused on this stack is recorded as such.
  step     the DEFAULT training step as the unchanged bench.py times it, this build's library against the parent commit's
           (``--parent-lib``, loaded through DWN_LIB_PATH), alternating parent / this.

There is no fallback: without a GPU the tool refuses to run.

python tools/population_modes_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.pairwise_time import N, child, make_trials, timed  # noqa: E402

K, P, PLANTED = 16, 24, 16


def noise_states(dev):
    """{"flat": (co-moments, count), "planted": ...}: the noise state of the 12t profile case, and of the same trials with PLANTED
    shared noise sources of decaying strength added along random directions."""
    import torch
    from sensorium_amd.population import PairwiseCorrelation
    out = {}
    for name in ("flat", "planted"):
        g = torch.Generator(device=dev).manual_seed(5)
        dirs = torch.linalg.qr(torch.randn(N, PLANTED, device=dev, generator=g))[0]
        amp = 40.0 * 0.9 ** torch.arange(PLANTED, device=dev)
        acc = PairwiseCorrelation(N, dev, kinds=("noise",))
        for x, group in make_trials(dev, 1):
            if name == "planted":
                x = x + dirs @ (amp[:, None] * torch.randn(PLANTED, x.shape[1], device=dev, generator=g))
            acc.add(x.float(), group)
        res = acc.compute()
        out[name] = (res.comoments("noise"), res.counts["noise"])
    return out


def med(fn, n, warm=2):
    for _ in range(warm):
        fn()
    return round(statistics.median(timed(fn, n)), 4)


def leg_kernels(args):
    import torch
    from sensorium_amd import ops
    dev = torch.device("cuda", 0)
    A, count = noise_states(dev)["planted"]
    scale = 1.0 / count
    Q = ops.modes_block(N, P, dev)
    Q.copy_(torch.randn(N, P, device=dev, dtype=torch.float64))
    Qc = Q.contiguous()
    Ac = A.contiguous()
    n = args.rounds * args.iters
    t = {"symm": med(lambda: ops.modes_symm(A, Q, scale), n), "matmul_f64": med(lambda: torch.matmul(Ac, Qc), n),
         "clone_matrix": med(lambda: Ac.clone(), n), "moments": med(lambda: ops.modes_moments(A, scale), n),
         "orth": med(lambda: ops.modes_orth(Q), n)}
    Qo = ops.modes_orth(Q)
    Y = ops.modes_symm(A, Qo, scale)
    H = Qo.t() @ Y
    H = 0.5 * (H + H.t())
    t["small_eigh_p24"] = med(lambda: ops.modes_small_eigh(H), n)
    H64 = torch.randn(64, 64, device=dev, dtype=torch.float64)
    H64 = H64 + H64.t()
    t["small_eigh_p64_random"] = med(lambda: ops.modes_small_eigh(H64), n)
    theta, W = ops.modes_small_eigh(H)
    t["ritz"] = med(lambda: ops.modes_ritz(Qo, Y, theta, W, K, 1e-10), n)
    t["overlap_with_matrix"] = med(lambda: ops.modes_overlap(Qo[:, :K], Qo[:, :K], A, scale), n)
    ref = scale * torch.matmul(Ac, Qc)
    got = ops.modes_symm(A, Q, scale)
    mb = N * N * 8 / 1e6
    print(json.dumps({"leg": "kernels", "matrix_MB": round(mb, 1), "median_ms": t, "n": n,
                      "symm_over_matmul": round(t["symm"] / t["matmul_f64"], 3),
                      "symm_over_half_clone": round(t["symm"] / (0.5 * t["clone_matrix"]), 2),
                      "symm_GB_per_s_of_one_read": round(mb / t["symm"], 1),
                      "max_rel_difference_to_matmul": float(((got - ref).abs().max() / ref.abs().max()).cpu())}))


def leg_whole(args):
    import torch
    from sensorium_amd.population import modes
    dev = torch.device("cuda", 0)
    out = {"leg": "whole"}
    for name, (A, count) in noise_states(dev).items():
        scale = 1.0 / count
        row = {}
        m = modes(A, K, scale=scale)
        s = m.summary()
        row["modes_summary"] = s
        row["modes_ms"] = [round(x, 2) for x in timed(lambda: modes(A, K, scale=scale), 3)]
        if name == "planted":
            cov = A * scale

            def wall(fn):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                try:
                    r = fn()
                    torch.cuda.synchronize()
                    return round((time.perf_counter() - t0) * 1e3, 1), r
                except Exception as e:                                                  # recorded, not hidden: the issue asks for it
                    return f"failed: {type(e).__name__}: {str(e)[:120]}", None
            row["eigh_ms"], full = wall(lambda: torch.linalg.eigh(cov))
            if full is not None:
                top = full[0].flip(0)[:K]
                row["max_rel_difference_to_eigh"] = float(((m.values - top).abs().max() / top[0]).cpu())
            row["svd_lowrank_ms"], _ = wall(lambda: torch.svd_lowrank(cov, q=P, niter=max(int(s["rounds"]), 1)))
            row["lobpcg_ms"], _ = wall(lambda: torch.lobpcg(cov, k=K, niter=64))

            def host():
                from scipy.sparse.linalg import eigsh
                return eigsh(cov.cpu().numpy(), k=K)
            row["host_readback_and_eigsh_ms"], _ = wall(host)
        out[name] = row
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "kernels", "whole", "step"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "population_modes_time.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("population_modes_time: no GPU; this tool measures HIP kernels and has no fallback")
    if args.leg == "kernels":
        return leg_kernels(args)
    if args.leg == "whole":
        return leg_whole(args)
    me = os.path.abspath(__file__)
    lines = ["population modes: measured times (tools/population_modes_time.py; HIP events, one MI355X, one box)", "",
             f"N = {N}, k = {K}, p = {P}; the noise state of the 12t profile case ('flat': iid noise, no shared mode) and the same "
             f"trials with {PLANTED} planted shared noise sources ('planted')"]
    if args.leg == "all":
        (r,) = child([me, "--leg", "kernels", "--rounds", str(args.rounds), "--iters", str(args.iters)], limit=300)
        lines += [f"  kernels: {json.dumps(r)}", ""]
        (w,) = child([me, "--leg", "whole"], limit=500)
        for name in ("flat", "planted"):
            lines += [f"  whole, {name}: {json.dumps(w[name])}"]
        lines += [""]
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

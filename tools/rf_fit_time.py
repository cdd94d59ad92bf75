#!/usr/bin/env python3
"""What the parametric receptive-field fits cost, HIP events, one box; writes profiles/rf_fit_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels  M = 7863 maps of 36 x 64 (cell 1) and 18 x 32 (cell 2), planted elliptical Gaussians at noise 0.1 (256 different maps,
           repeated): dwn_gauss2d_fit against the dwn_sta_accumulate call of the same geometry (B = 32, T = 32, L = 12) in the
           same process, and against a batched-torch statement of the same Levenberg-Marquardt iteration with a fixed iteration
           count equal to the kernel's worst (the alternative the kernel replaces; float64, one try per iteration, no read-back);
           dwn_gauss2d_profile (L = 12) against a device copy of the map it reads.
  variant  the same fit with another build of the library (``--variant-lib``: dwn_rf_fit.hip compiled with -DDWN_GF_STAGE=0, the
           map read through L2 on every pass instead of staged in LDS).
  quality  the worst relative excess of S (tests/test_gpu_rf_fit.py (a)) over the test's cases, by the float64 checker.
  step     the DEFAULT training step as the unchanged bench.py times it (--gpus 1 --steps K --warmup W, headline leg only), with this
           build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH), in the order parent, this,
           this, parent.

There is no fallback: without a GPU the tool refuses to run.

python tools/rf_fit_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--variant-lib build_var/libdwiseneuro_hip_nostage.so]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, B, T, L, SIZE, WINDOW = 7863, 32, 32, 12, (64, 64), (14, 0, 36, 64)


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


def planted(gh, gw, dev):
    import numpy as np
    import torch
    from tests import rf_fit_reference as gf
    base, _ = gf.planted_maps(gh, gw, 256, 0.1, 7)
    return torch.from_numpy(np.tile(base, (M // 256 + 1, 1, 1))[:M].copy()).to(dev)


def torch_lm(maps, start, iters):
    """The same iteration in batched float64 torch: normal equations, damped Cholesky solve, clamp, accept where S fell — one try
    per iteration, every map for the same number of iterations (a data-dependent stop would need a read-back)."""
    import math
    import torch
    Mn, gh, gw = maps.shape
    m = maps.double().view(Mn, -1)
    c = torch.arange(gh * gw, device=maps.device)
    y, x = (c // gw).double()[None], (c % gw).double()[None]
    p = start.clone()
    lam = torch.full((Mn, 1), 1e-3, dtype=torch.float64, device=maps.device)
    ulo, uhi = -math.log(2.0 * max(gh, gw)), -math.log(0.3)
    lo = torch.tensor([-math.inf, -math.inf, -1.0, -1.0, ulo, -math.inf, ulo], dtype=torch.float64, device=maps.device)
    hi = torch.tensor([math.inf, math.inf, float(gh), float(gw), uhi, math.inf, uhi], dtype=torch.float64, device=maps.device)

    def parts(q):
        l11, l21, l22 = q[:, 4:5].exp(), q[:, 5:6], q[:, 6:7].exp()
        dx, dy = x - q[:, 3:4], y - q[:, 2:3]
        u, v = l11 * dx, l21 * dx + l22 * dy
        e = torch.exp(-0.5 * (u * u + v * v))
        return e, u, v, dx, dy, l11, l21, l22

    def resid(q):
        return m - (q[:, 0:1] + q[:, 1:2] * parts(q)[0])
    S = resid(p).square().sum(1, keepdim=True)
    for _ in range(iters):
        e, u, v, dx, dy, l11, l21, l22 = parts(p)
        ae = p[:, 1:2] * e
        J = torch.stack([torch.ones_like(e), e, ae * (v * l22), ae * (u * l11 + v * l21), -(ae * (u * u)), -(ae * (v * dx)),
                         -(ae * (v * (l22 * dy)))], dim=2)
        r = m - (p[:, 0:1] + ae)
        A = J.transpose(1, 2) @ J
        g = (J.transpose(1, 2) @ r[:, :, None])
        A = A + lam[:, :, None] * torch.diag_embed(torch.diagonal(A, dim1=1, dim2=2))
        Lf, info = torch.linalg.cholesky_ex(A)
        dp = torch.cholesky_solve(g, Lf)[:, :, 0]
        pn = torch.minimum(torch.maximum(p + dp, lo), hi)
        Sn = resid(pn).square().sum(1, keepdim=True)
        ok = (Sn < S) & torch.isfinite(Sn) & (info[:, None] == 0)
        p, S = torch.where(ok, pn, p), torch.where(ok, Sn, S)
        lam = torch.where(ok, (lam / 10).clamp(min=1e-12), lam * 10)
    return p, S


def leg_kernels(args):
    import torch
    from sensorium_amd import NoiseStimulus, ops
    dev = torch.device("cuda", 0)
    rows = {}
    for cell in (1, 2):
        gh, gw = WINDOW[2] // cell, WINDOW[3] // cell
        maps = planted(gh, gw, dev)
        params, table, start = ops.gauss2d_fit(maps)
        torch.cuda.synchronize()
        worst = int(table[:, 1].max())
        status = torch.bincount(table[:, 0].long(), minlength=3).tolist()
        legs = {"fit": lambda: ops.gauss2d_fit(maps)}
        if not args.fit_only:
            x = NoiseStimulus(B, T, SIZE, window=WINDOW, cell=cell, seed=1).to(dev)()
            r = torch.rand(B, M, T, device=dev)
            r0 = r.mean(dim=(0, 2)).contiguous()
            state = torch.zeros(ops.sta_state_numel(M, L, WINDOW, cell), dtype=torch.float64, device=dev)
            lagged = maps[:, None].expand(M, L, gh, gw).contiguous()
            legs.update({"accumulate": lambda: ops.sta_accumulate(state, x, r, lags=L, window=WINDOW, cell=cell, skip=L - 1, s0=127.5, r0=r0),
                         "profile": lambda: ops.gauss2d_profile(params, lagged),
                         "map_copy": lambda: lagged.clone()})
            if cell == 2 or args.torch_full:
                legs["torch_lm"] = lambda: torch_lm(maps, start[:, :7], worst)
        ms = {k: [] for k in legs}
        for k, fn in legs.items():
            timed(fn, 1 if k == "torch_lm" else 3)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k] += timed(fn, 2 if k == "torch_lm" else args.iters)
        row = {"grid": [gh, gw], "iterations_mean": round(float(table[:, 1].mean()), 2), "iterations_worst": worst, "status_counts": status,
               "median_ms": {k: round(statistics.median(v), 4) for k, v in ms.items()},
               "min_ms": {k: round(min(v), 4) for k, v in ms.items()}, "max_ms": {k: round(max(v), 4) for k, v in ms.items()},
               "n": {k: len(v) for k, v in ms.items()}}
        if "torch_lm" in legs:
            pt, St = torch_lm(maps, start[:, :7], worst)
            row["torch_S_over_kernel_S_median"] = round(float((St[:, 0] / table[:, 9]).median()), 6)
        rows[f"cell{cell}"] = row
        del legs
        torch.cuda.empty_cache()
    print(json.dumps({"leg": "kernels", **rows}), flush=True)


def leg_quality(args):
    import numpy as np
    import torch
    from sensorium_amd import ops
    from tests import rf_fit_reference as gf
    dev = torch.device("cuda", 0)
    worst = {"noisy": -1.0, "noiseless": -1.0}
    ratio = 0.0
    for gh, gw in gf.GRIDS:
        for lv, noise in enumerate(gf.NOISE_LEVELS):
            maps, _ = gf.planted_maps(gh, gw, gf.maps_per_case(gh, gw), noise, gf.case_seed(gh, gw, lv))
            P, Tt, _, Cs = gf.fit(maps)
            pk = ops.gauss2d_fit(torch.from_numpy(maps).to(dev))[0].cpu().numpy()
            for k in range(len(maps)):
                mm = maps[k].astype(np.float64).ravel()
                Sc = gf.sse(P[k], mm, gh, gw)
                key = "noisy" if lv else "noiseless"
                worst[key] = max(worst[key], (gf.sse(pk[k], mm, gh, gw) - Sc) / Sc)
                ratio = max(ratio, float((np.abs(pk[k] - P[k]) / gf.param_bound(P[k], Tt[k, 9], Cs[k])).max()))
    print(json.dumps({"leg": "quality", "worst_relative_excess": worst, "worst_param_ratio": ratio}), flush=True)


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
    print(f"# {os.path.basename(cmd[0])} {' '.join(cmd[1:3])} ({lib or 'this build'}): { {k: last[k] for k in ('ms_per_step',) if k in last} }", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "kernels", "quality"], default="all")
    ap.add_argument("--fit-only", action="store_true")
    ap.add_argument("--torch-full", action="store_true", help="the torch comparison at cell 1 too (about 2 GB per temporary)")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--variant-lib", default=None, help="this build with dwn_rf_fit.hip compiled with -DDWN_GF_STAGE=0")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rf_fit_time.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rf_fit_time: no GPU; this tool measures HIP kernels and has no fallback")
    if args.leg == "kernels":
        return leg_kernels(args)
    if args.leg == "quality":
        return leg_quality(args)
    me = os.path.abspath(__file__)
    common = ["--rounds", str(args.rounds), "--iters", str(args.iters)]
    (r,) = child([me, "--leg", "kernels"] + common, limit=500)
    lines = ["parametric receptive-field fits: measured times (tools/rf_fit_time.py; HIP events, one MI355X, one box)", "",
             f"M = {M} planted maps (noise 0.1, 256 different ones repeated); the accumulate is dwn_sta_accumulate at B = {B}, T = {T}, L = {L}, "
             f"N = {M}, window {WINDOW[2]} x {WINDOW[3]}, in the same process; three warm-up calls, then rounds of {args.iters} calls per leg; ms"]
    for name in ("cell1", "cell2"):
        c = r[name]
        med = c["median_ms"]
        lines += [f"  {name}: grid {c['grid'][0]} x {c['grid'][1]}; iterations mean {c['iterations_mean']}, worst {c['iterations_worst']}; "
                  f"status counts (0, 1, 2) {c['status_counts']}; n per leg {c['n']}",
                  f"    median ms: {med}", f"    min ms:    {c['min_ms']}", f"    max ms:    {c['max_ms']}",
                  f"    fit / accumulate {med['fit'] / med['accumulate']:.3f}; profile / device copy of the map it reads {med['profile'] / med['map_copy']:.3f}"]
        if "torch_lm" in med:
            lines.append(f"    batched torch, {c['iterations_worst']} iterations for every map: {med['torch_lm']} ms = {med['torch_lm'] / med['fit']:.1f} x the kernel "
                         f"(median S_torch / S_kernel {c['torch_S_over_kernel_S_median']})")
    lines.append("")
    if args.variant_lib:
        (v,) = child([me, "--leg", "kernels", "--fit-only"] + common, lib=args.variant_lib, limit=300)
        (s,) = child([me, "--leg", "kernels", "--fit-only"] + common, limit=300)
        lines += ["the map staged in LDS once per wave (this build) against read through L2 on every pass (-DDWN_GF_STAGE=0), fit only, one "
                  "process each, variant first:"]
        for name in ("cell1", "cell2"):
            lines.append(f"  {name}: LDS {s[name]['median_ms']['fit']} ms ({s[name]['min_ms']['fit']} .. {s[name]['max_ms']['fit']}); "
                         f"L2 {v[name]['median_ms']['fit']} ms ({v[name]['min_ms']['fit']} .. {v[name]['max_ms']['fit']})")
        lines.append("")
    (q,) = child([me, "--leg", "quality"], limit=400)
    lines += [f"worst relative excess of S at the kernel's parameters over S at the checker's (the cases of tests/test_gpu_rf_fit.py): "
              f"noisy maps {q['worst_relative_excess']['noisy']:.3e}, noiseless maps {q['worst_relative_excess']['noiseless']:.3e}; "
              f"worst |p_kernel - p_checker| / bound {q['worst_param_ratio']:.3e}", ""]
    if args.parent_lib:
        bench = [os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup", str(args.bench_warmup),
                 "--no-cpu-baseline", "--no-inference", "--no-other-configs", "--no-rooflines"]
        runs = {"parent": [], "this": []}
        order = []
        for i in range(args.bench_rounds):              # parent, this, this, parent: a drift over the call falls on both sides
            order += ["parent", "this"] if i % 2 == 0 else ["this", "parent"]
        for who in order:
            runs[who].append(child(bench, lib=args.parent_lib if who == "parent" else None, limit=400)[-1]["ms_per_step"])
        lo, hi = min(runs["parent"]), max(runs["parent"])
        lines += [f"default training step, bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup} (headline leg), the parent "
                  f"commit's library against this build's, one process per leg in the order {', '.join(order)}:",
                  f"  parent ms/step: {runs['parent']}   own run-to-run spread {lo} .. {hi}",
                  f"  this   ms/step: {runs['this']}",
                  f"  this build inside the parent's spread (at or below its upper end): {[t <= hi for t in runs['this']]}", ""]
    else:
        lines += ["default-step A/B against the parent commit: not run (no --parent-lib)", ""]
    text = "\n".join(lines)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

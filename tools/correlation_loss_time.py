#!/usr/bin/env python3
"""What the correlation objective costs, HIP events, one box; writes profiles/correlation_loss_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  loss     at the metric shape (B = 32, N = 7863, T = 32), with ONE mouse owning every row and with TEN one-hot mice (the ten readout
           widths, 3 or 4 rows each): forward and backward of ops.CorrelationLossFn against forward and backward of ops.PoissonLossFn
           (the parent commit's kernels) on the same tensors, taking turns in one process.  By bytes the backward is 1.0 x the
           Poisson backward and the forward at most 2.0 x the Poisson forward (two sweeps); 1.5 x over the byte ratio is accepted.
  metric   CorrelationMetric.update with fused=True and fused=False, ten mice, taking turns in one process.
  step     the DEFAULT training step (metric configuration, B=32 T=32 36x64 bf16, expansion 7, one readout, EMA) with this build's
           library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH), alternating parent / this / ...
  onpath   the step with ``mice_poisson_correlation`` against the default step, two models in one process taking turns.

There is no fallback: without a GPU the tool refuses to run.

python tools/correlation_loss_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 20]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, T = 32, 32


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("correlation_loss_time: no GPU; this tool measures HIP kernels and has no fallback")


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


def mice_tensors(sizes, owners, seed=0):
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(seed)
    preds = [(torch.rand(B, n, T, device=dev, generator=g) * 4 + 0.05).requires_grad_(True) for n in sizes]
    targets = [torch.clamp(torch.randn(B, n, T, device=dev, generator=g), min=0) * 6 for n in sizes]
    weights = torch.eye(len(sizes), device=dev)[torch.tensor(owners, device=dev)].contiguous()
    return preds, targets, weights


def leg_loss(args):
    import torch
    import bench
    from sensorium_amd import ops
    cases = {"one_mouse_all_rows": ((bench.NUM_NEURONS_ALL[0],), [0] * B),
             "ten_one_hot_mice": (tuple(bench.NUM_NEURONS_ALL), [b % 10 for b in range(B)])}
    for name, (sizes, owners) in cases.items():
        preds, targets, weights = mice_tensors(sizes, owners)
        norm = weights / weights.sum()
        shares = weights.sum(0) / weights.sum()
        state = {}

        def corr_fwd():
            state["corr"] = [ops.CorrelationLossFn.apply(p, t, weights[:, m], shares[m], 1e-8, "mean")
                             for m, (p, t) in enumerate(zip(preds, targets))]

        def pois_fwd():
            state["pois"] = [ops.PoissonLossFn.apply(p, t, norm[:, m], 1e-8) for m, (p, t) in enumerate(zip(preds, targets))]

        def bwd(key):
            return lambda: [torch.autograd.grad(lo, p, retain_graph=True) for lo, p in zip(state[key], preds)]

        corr_fwd()
        pois_fwd()
        legs = {"poisson_fwd": pois_fwd, "corr_fwd": corr_fwd, "poisson_bwd": bwd("pois"), "corr_bwd": bwd("corr")}
        ms = {k: [] for k in legs}
        for fn in legs.values():
            timed(fn, 5)
        for _ in range(args.rounds):
            for k, fn in legs.items():
                ms[k] += timed(fn, args.iters)
        us = {k: round(1e3 * statistics.median(v), 1) for k, v in ms.items()}
        counted = sum(n * T * 4 * 2 * sum(1 for o in owners if o == m) for m, n in enumerate(sizes))
        print(json.dumps({"leg": "loss", "case": name, "mice": len(sizes), "counted_MB_pred_plus_target": round(counted / 1e6, 1),
                          "median_us": us, "fwd_ratio": round(us["corr_fwd"] / us["poisson_fwd"], 3),
                          "bwd_ratio": round(us["corr_bwd"] / us["poisson_bwd"], 3), "n": len(ms["corr_fwd"])}), flush=True)


def leg_metric(args):
    import torch
    import bench
    from sensorium_amd.metrics import CorrelationMetric
    sizes = tuple(bench.NUM_NEURONS_ALL)
    preds, targets, weights = mice_tensors(sizes, [b % 10 for b in range(B)])
    out = {"prediction": [p.detach() for p in preds], "target": (targets, weights)}
    metrics = {"unfused": CorrelationMetric(), "fused": CorrelationMetric(fused=True)}
    ms = {k: [] for k in metrics}
    for m in metrics.values():
        timed(lambda: m.update(out), 3)
    for _ in range(args.rounds):
        for k, m in metrics.items():
            ms[k] += timed(lambda: m.update(out), args.iters)
    vals = {k: m.compute() for k, m in metrics.items()}
    diff = max(abs(vals["fused"][k] - vals["unfused"][k]) for k in vals["fused"])
    print(json.dumps({"leg": "metric", "median_ms": {k: median(v) for k, v in ms.items()},
                      "unfused_over_fused": round(statistics.median(ms["unfused"]) / statistics.median(ms["fused"]), 2),
                      "max_abs_difference_of_the_two_results": diff, "n": len(ms["fused"])}), flush=True)


def make_model(loss):
    import torch
    import bench
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    readouts = bench.NUM_NEURONS_ALL[:1]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    if loss is not None:
        params["loss"] = loss
    torch.manual_seed(0)
    model = MouseModel(params)
    model.set_ema(0.999)
    return model, make_batch(32, 32, 36, 64, readouts, seed=1, device=torch.device("cuda", 0))


def leg_step(args):
    model, batch = make_model(None)
    timed(lambda: model.train_step(batch, sync_loss=False), 3)
    ms = timed(lambda: model.train_step(batch, sync_loss=False), args.iters)
    print(json.dumps({"leg": "step", "lib": os.environ.get("DWN_LIB_PATH", "this build"), "median_ms": median(ms),
                      "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}), flush=True)


def leg_onpath(args):
    models = {"default": make_model(None), "poisson_correlation": make_model(("mice_poisson_correlation", {}))}
    ms = {k: [] for k in models}
    for m, b in models.values():
        timed(lambda: m.train_step(b, sync_loss=False), 3)
    for _ in range(args.rounds):
        for k, (m, b) in models.items():
            ms[k] += timed(lambda: m.train_step(b, sync_loss=False), args.iters)
    d, c = statistics.median(ms["default"]), statistics.median(ms["poisson_correlation"])
    print(json.dumps({"leg": "onpath", "default_median_ms": median(ms["default"]), "poisson_correlation_median_ms": median(ms["poisson_correlation"]),
                      "difference_us": round(1e3 * (c - d), 1), "n": len(ms["default"])}), flush=True)


LEGS = {"loss": leg_loss, "metric": leg_metric, "step": leg_step, "onpath": leg_onpath}


def child(leg, args, lib=None, limit=300, iters=None):
    env = dict(os.environ)
    env.pop("DWN_LIB_PATH", None)
    if lib:
        env["DWN_LIB_PATH"] = os.path.abspath(lib)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--rounds", str(args.rounds),
           "--iters", str(iters or args.iters)]
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout[-2000:] + res.stderr[-4000:])
        raise SystemExit(f"leg {leg} ({lib or 'this build'}) ended with status {res.returncode}: nothing more is started")
    rows = [json.loads(line) for line in res.stdout.splitlines() if line.startswith("{")]
    print(f"# {leg} ({lib or 'this build'}): {rows}", flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all"] + list(LEGS), default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "correlation_loss_time.txt"))
    args = ap.parse_args()
    require_gpu()
    if args.leg != "all":
        LEGS[args.leg](args)
        return
    lines = ["correlation objective: measured times (tools/correlation_loss_time.py; HIP events, one MI355X, one box)", "",
             f"loss at the metric shape B = {B}, T = {T} (fp32), CorrelationLossFn against PoissonLossFn on the same tensors, one process:"]
    for r in child("loss", args):
        lines.append(f"  {r['case']} ({r['mice']} mice, {r['counted_MB_pred_plus_target']} MB of counted pred + target): median us "
                     f"{r['median_us']}; forward / Poisson forward {r['fwd_ratio']}, backward / Poisson backward {r['bwd_ratio']}; "
                     f"n = {r['n']} per leg")
    lines.append("")
    for r in child("metric", args):
        lines.append(f"CorrelationMetric.update, ten mice: median ms {r['median_ms']} (unfused / fused {r['unfused_over_fused']}); the two "
                     f"results differ by at most {r['max_abs_difference_of_the_two_results']:.2e}; n = {r['n']} per side")
    lines.append("")
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        for _ in range(args.rounds):
            runs["parent"] += child("step", args, lib=args.parent_lib, iters=args.step_iters)
            runs["this"] += child("step", args, iters=args.step_iters)
        pm, tm = [r["median_ms"] for r in runs["parent"]], [r["median_ms"] for r in runs["this"]]
        lo, hi = min(pm), max(pm)
        lines += ["default training step (plain dwiseneuro, mice_poisson), parent commit's library against this build's, alternating processes:",
                  f"  parent medians ms/step: {pm}   own run-to-run spread {lo} .. {hi}",
                  f"  this   medians ms/step: {tm}",
                  f"  this build at or below the upper end of the parent's spread: {[t <= hi for t in tm]}; "
                  f"median of medians: parent {median(pm)}, this {median(tm)}", ""]
    else:
        lines += ["default-step A/B against the parent commit: not run (no --parent-lib)", ""]
    for r in child("onpath", args, limit=500, iters=args.step_iters):
        lines.append(f"step with mice_poisson_correlation {r['poisson_correlation_median_ms']} ms against the default step "
                     f"{r['default_median_ms']} ms (difference {r['difference_us']} us; n = {r['n']} per side)")
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

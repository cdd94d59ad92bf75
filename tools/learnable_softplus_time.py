#!/usr/bin/env python3
"""What the learnable Softplus beta costs, HIP events, one box; writes profiles/learnable_softplus_time.txt.

Three legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  ab         the DEFAULT training step (feature off: metric configuration, B=32 T=32 36x64 bf16, expansion 7, one readout, EMA)
             with this build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH), alternating
             parent / this / parent / this ...  Reported: every process's median step, the parent's own run-to-run spread (min ..
             max of its medians) and whether this build's medians lie inside it.  Both sides run this tree's Python: with the
             feature off it differs from the parent's by one attribute test per readout call.
  learnable  the step with the feature off and on (softplus_param "beta"), two models in one process taking turns, with one
             readout and with ten.
  backward   dwn_readout_backward alone on one production readout (7863 neurons, Cin 4096, B x T = 32 x 32, bf16), fixed beta
             and the dbeta variant taking turns.

python tools/learnable_softplus_time.py --parent-lib build_ab/libdwiseneuro_hip_parent.so [--rounds 3] [--iters 8]
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


def make_model(n_readouts, learnable):
    import torch
    import bench
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    readouts = bench.NUM_NEURONS_ALL[:n_readouts]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    if learnable:
        params["nn_module"][1]["learnable_softplus"] = True
    torch.manual_seed(0)
    model = MouseModel(params)
    model.set_ema(0.999)
    return model, make_batch(32, 32, 36, 64, readouts, seed=1, device=torch.device("cuda", 0))


def leg_step(args):
    """one process: the default step, median over --iters after a warm-up"""
    model, batch = make_model(1, False)
    timed(lambda: model.train_step(batch, sync_loss=False), 3)
    ms = timed(lambda: model.train_step(batch, sync_loss=False), args.iters)
    print(json.dumps({"leg": "step", "lib": os.environ.get("DWN_LIB_PATH", "this build"), "median_ms": median(ms),
                      "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "n": len(ms)}), flush=True)


def leg_learnable(args):
    import torch
    for n in (1, 10):
        models = {"off": make_model(n, False), "on": make_model(n, True)}
        ms = {k: [] for k in models}
        for k, (m, b) in models.items():
            timed(lambda: m.train_step(b, sync_loss=False), 3)
        for _ in range(args.rounds):
            for k, (m, b) in models.items():
                ms[k] += timed(lambda: m.train_step(b, sync_loss=False), args.iters)
        betas = [float(r.beta()) for r in models["on"][0].nn_module.readouts]
        # |dbeta| against the global gradient norm of one more forward + backward (what the guarded step's clipping would see);
        # the "log" form's gradient is beta * dbeta by the chain rule: derived, not run
        m, b = models["on"]
        m.nn_module.train()
        m.optimizer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = m.loss(m.nn_module(b[0]), b[1])
        loss.backward()
        gate = {id(p) for p in m.nn_module.softplus_parameters()}
        rest = torch.stack([p.grad.double().pow(2).sum() for p in m.nn_module.parameters() if p.grad is not None and id(p) not in gate])
        dbeta = torch.stack([p.grad.double() for p in m.nn_module.softplus_parameters()])
        rest, db, dlog = float(rest.sum().sqrt()), float(dbeta.pow(2).sum().sqrt()), float((dbeta * torch.tensor(betas, device=dbeta.device)).pow(2).sum().sqrt())
        norms = {"other_grad_norm": rest, "dbeta_norm": db, "dbeta_share_of_global_norm": db / (rest ** 2 + db ** 2) ** 0.5,
                 "dlogbeta_norm": dlog, "dlogbeta_share_of_global_norm": dlog / (rest ** 2 + dlog ** 2) ** 0.5}
        print(json.dumps({"leg": "learnable", "readouts": n, "norms": {k: float(f"{v:.4g}") for k, v in norms.items()}, "off_median_ms": median(ms["off"]), "on_median_ms": median(ms["on"]),
                          "on_minus_off_us": round(1e3 * (statistics.median(ms["on"]) - statistics.median(ms["off"])), 1),
                          "n": len(ms["on"]), "beta_after": [round(b, 5) for b in betas]}), flush=True)
        del models
        torch.cuda.empty_cache()


def leg_backward(args):
    import torch
    import sensorium_amd._lib as L
    dev = torch.device("cuda", 0)
    B, T, Cin, groups, n = 32, 32, 4096, 2, 7863
    npad, Kg = n + n % 2, Cin // groups
    torch.manual_seed(0)
    x = torch.randn(B, T, Cin, device=dev).bfloat16()
    w = torch.randn(npad, Kg, device=dev) * (2.0 / 0.07 / Kg ** 0.5)
    bias = torch.randn(npad, device=dev) * (2.0 / 0.07)
    dout = torch.randn(B, n, T, device=dev)
    out = torch.empty(B, n, T, device=dev)
    dx, dw, db = torch.empty_like(x), torch.empty(npad, Kg, device=dev), torch.zeros(npad, device=dev)
    beta, dbeta = torch.tensor(0.07, device=dev), torch.zeros((), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    keep = []

    def args_for(learnable):
        a = L.ReadoutArgs()
        a.dtype = L.DWN_BF16; a.B = B; a.T = T; a.Cin = Cin; a.groups = groups; a.n_out = n; a.softplus_beta = 0.07
        a.x = x.data_ptr(); a.w = w.data_ptr(); a.bias = bias.data_ptr(); a.out = out.data_ptr()
        a.dout = dout.data_ptr(); a.dx = dx.data_ptr(); a.dw = dw.data_ptr(); a.dbias = db.data_ptr()
        if learnable:
            a.beta_dev = beta.data_ptr(); a.dbeta = dbeta.data_ptr()
        wt = torch.empty(L.lib.dwn_readout_wt_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
        ws = torch.empty(max(L.lib.dwn_readout_workspace_bytes(C.byref(a), k) for k in (0, 1)), dtype=torch.uint8, device=dev)
        keep.extend((wt, ws))
        a.wt = wt.data_ptr(); a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_readout_forward(C.byref(a), 0, stream), "dwn_readout_forward")
        return a

    calls = {k: args_for(k == "dbeta") for k in ("fixed", "dbeta")}
    run = lambda a: L.check(L.lib.dwn_readout_backward(C.byref(a), 0, stream), "dwn_readout_backward")
    ms = {k: [] for k in calls}
    for a in calls.values():
        timed(lambda: run(a), 3)
    for _ in range(args.rounds):
        for k, a in calls.items():
            ms[k] += timed(lambda: run(a), args.iters)
    print(json.dumps({"leg": "backward", "what": f"dwn_readout_backward B={B} T={T} Cin={Cin} n={n} bf16",
                      "fixed_median_us": round(1e3 * statistics.median(ms["fixed"]), 1),
                      "dbeta_median_us": round(1e3 * statistics.median(ms["dbeta"]), 1),
                      "dbeta_minus_fixed_us": round(1e3 * (statistics.median(ms["dbeta"]) - statistics.median(ms["fixed"])), 1),
                      "n": len(ms["fixed"]), "dbeta": float(dbeta)}), flush=True)


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
    print(f"# {leg} ({lib or 'this build'}): {rows}", flush=True)          # progress: the whole run takes minutes
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["all", "step", "learnable", "backward"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learnable_softplus_time.txt"))
    args = ap.parse_args()
    if args.leg != "all":
        {"step": leg_step, "learnable": leg_learnable, "backward": leg_backward}[args.leg](args)
        return
    lines = ["learnable Softplus beta: measured times (tools/learnable_softplus_time.py; HIP events, one MI355X, one box)", ""]
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        for _ in range(args.rounds):
            runs["parent"] += child("step", args, lib=args.parent_lib)
            runs["this"] += child("step", args)
        pm, tm = [r["median_ms"] for r in runs["parent"]], [r["median_ms"] for r in runs["this"]]
        lo, hi = min(pm), max(pm)
        lines += ["default training step (feature off), parent commit's library against this build's, alternating processes:",
                  f"  parent medians ms/step: {pm}   own run-to-run spread {lo} .. {hi}",
                  f"  this   medians ms/step: {tm}",
                  f"  this build inside the parent's spread: {[lo <= t <= hi for t in tm]}; "
                  f"median of medians: parent {median(pm)}, this {median(tm)}", ""]
    else:
        lines += ["default-step A/B against the parent commit: not run (no --parent-lib)", ""]
    for r in child("learnable", args, limit=500):
        lines.append(f"step with {r['readouts']} readout(s): feature off {r['off_median_ms']} ms, on {r['on_median_ms']} ms "
                     f"(on - off {r['on_minus_off_us']} us; n = {r['n']} per side; beta after the steps {r['beta_after']})")
        lines.append(f"  gradient norms of one more forward + backward: {r['norms']}")
    lines.append("")
    for r in child("backward", args):
        lines.append(f"{r['what']}: fixed {r['fixed_median_us']} us, dbeta variant {r['dbeta_median_us']} us "
                     f"(difference {r['dbeta_minus_fixed_us']} us; n = {r['n']} per side)")
    lines += ["", "Data parallelism over more than one GPU (N > 1) was not measured."]
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

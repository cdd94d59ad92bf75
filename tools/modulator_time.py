#!/usr/bin/env python3
"""What the behaviour modulator costs, HIP events, one box; writes profiles/behavior_modulator_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels   dwn_modulator_forward / _backward (all four outputs; dy alone; the three reductions alone) at the production geometry
            (B = 32, N = 7863, T = 32, K = 8) against y.clone() of the same tensor, taking turns in one process; then the ten-mouse
            case: ten forwards / ten backwards over the ten readouts' neuron counts against ten clones.  By bytes the forward is
            one clone (read y, write out), the backward 1.5 clones (read y and dout, write dy) plus the float64 partials.
  step      the DEFAULT training step (plain ``dwiseneuro``: metric configuration, B=32 T=32 36x64 bf16, expansion 7, one readout,
            EMA) with this build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH),
            alternating parent / this / ...; reported: every process's median, the parent's own spread, whether this build lies in it.
  behavior  the ``dwiseneuro_behavior`` step against the ``dwiseneuro`` step, two models in one process taking turns.

There is no fallback: without a GPU the tool refuses to run.

python tools/modulator_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 3] [--iters 8]
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
PRODUCTION = (32, 7863, 32, 8)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("modulator_time: no GPU; this tool measures HIP kernels and has no fallback")


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


class Case:
    """One mouse's tensors and argument blocks: all four outputs, dy alone, the three reductions alone."""

    def __init__(self, B, N, T, K, dev):
        import torch
        import sensorium_amd._lib as L
        self.L, self.stream = L, torch.cuda.current_stream(dev).cuda_stream
        g = torch.Generator(device=dev).manual_seed(N)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)
        self.y, self.dout = r(B, N, T).abs() + 0.01, r(B, N, T)
        self.h, self.u, self.c = r(B, T, K), r(N, K) * (0.7 / K ** 0.5), r(N) * 0.3
        self.out, self.dy = torch.empty_like(self.y), torch.empty_like(self.y)
        self.dh, self.du, self.dc = torch.empty_like(self.h), torch.empty_like(self.u), torch.empty_like(self.c)
        a = self.args()
        self.ws_bytes = int(L.lib.dwn_modulator_ws_bytes(C.byref(a)))
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)
        self.all = self.args("dy", "dh", "du", "dc")
        self.only_dy = self.args("dy")
        self.sums = self.args("dh", "du", "dc")
        self.B, self.N, self.T, self.K = B, N, T, K

    def args(self, *want):
        a = self.L.ModulatorArgs()
        a.B, a.N, a.T = self.y.shape
        a.K, a.max_log_gain = self.h.shape[2], 2.0
        a.y, a.h, a.u, a.c, a.out, a.dout = (t.data_ptr() for t in (self.y, self.h, self.u, self.c, self.out, self.dout))
        for k in want:
            setattr(a, k, getattr(self, k).data_ptr())
        if want:
            a.ws, a.ws_bytes = self.ws.data_ptr(), self.ws_bytes
        return a

    def forward(self):
        self.L.check(self.L.lib.dwn_modulator_forward(C.byref(self.all), 0, self.stream), "dwn_modulator_forward")

    def backward(self, a=None):
        self.L.check(self.L.lib.dwn_modulator_backward(C.byref(a or self.all), 0, self.stream), "dwn_modulator_backward")


def run_legs(legs, args):
    ms = {k: [] for k in legs}
    for fn in legs.values():
        timed(fn, 3)
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k] += timed(fn, args.iters)
    return {k: round(1e3 * statistics.median(v), 1) for k, v in ms.items()}, len(next(iter(ms.values())))


def leg_kernels(args):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    B, N, T, K = PRODUCTION
    c = Case(B, N, T, K, dev)
    us, n = run_legs({"clone": lambda: c.y.clone(), "forward": c.forward, "backward": c.backward,
                      "backward_dy_only": lambda: c.backward(c.only_dy), "backward_sums_only": lambda: c.backward(c.sums)}, args)
    nbytes = c.y.numel() * 4
    print(json.dumps({"leg": "kernels", "case": "production", "dims": PRODUCTION, "tensor_MB": round(nbytes / 1e6, 1),
                      "partials_MB": round(c.ws_bytes / 1e6, 2), "median_us": us,
                      "forward_over_clone": round(us["forward"] / us["clone"], 3),
                      "backward_over_clone": round(us["backward"] / us["clone"], 3),
                      "clone_GBps_read_plus_write": round(2 * nbytes / us["clone"] / 1e3, 1), "n": n}), flush=True)
    del c
    torch.cuda.empty_cache()
    mice = [Case(B, nn, T, K, dev) for nn in bench.NUM_NEURONS_ALL]
    us, n = run_legs({"clone": lambda: [m.y.clone() for m in mice], "forward": lambda: [m.forward() for m in mice],
                      "backward": lambda: [m.backward() for m in mice]}, args)
    nbytes = sum(m.y.numel() for m in mice) * 4
    print(json.dumps({"leg": "kernels", "case": "ten mice", "dims": (B, sum(bench.NUM_NEURONS_ALL), T, K),
                      "tensor_MB": round(nbytes / 1e6, 1), "partials_MB": round(sum(m.ws_bytes for m in mice) / 1e6, 2),
                      "median_us": us, "forward_over_clone": round(us["forward"] / us["clone"], 3),
                      "backward_over_clone": round(us["backward"] / us["clone"], 3),
                      "clone_GBps_read_plus_write": round(2 * nbytes / us["clone"] / 1e3, 1), "n": n}), flush=True)


def make_model(behavior):
    import torch
    import bench
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    readouts = bench.NUM_NEURONS_ALL[:1]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    if behavior:
        name, kw = params["nn_module"]
        params["nn_module"] = ("dwiseneuro_behavior", dict(kw, modulator=dict(behavior_mean=(30.0, 5.0), behavior_std=(10.0, 5.0))))
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


def leg_behavior(args):
    models = {"plain": make_model(False), "behavior": make_model(True)}
    ms = {k: [] for k in models}
    for m, b in models.values():
        timed(lambda: m.train_step(b, sync_loss=False), 3)
    for _ in range(args.rounds):
        for k, (m, b) in models.items():
            ms[k] += timed(lambda: m.train_step(b, sync_loss=False), args.iters)
    print(json.dumps({"leg": "behavior", "plain_median_ms": median(ms["plain"]), "behavior_median_ms": median(ms["behavior"]),
                      "behavior_minus_plain_us": round(1e3 * (statistics.median(ms["behavior"]) - statistics.median(ms["plain"])), 1),
                      "n": len(ms["behavior"])}), flush=True)


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
    ap.add_argument("--leg", choices=["all", "kernels", "step", "behavior"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "behavior_modulator_time.txt"))
    args = ap.parse_args()
    require_gpu()
    if args.leg != "all":
        {"kernels": leg_kernels, "step": leg_step, "behavior": leg_behavior}[args.leg](args)
        return
    cmdline = "python tools/modulator_time.py " + " ".join(sys.argv[1:])
    lines = ["behaviour modulator: measured times (tools/modulator_time.py; HIP events, one MI355X, one box)", f"command: {cmdline}", ""]
    for r in child("kernels", args):
        lines.append(f"{r['case']} (B, N, T, K) = {tuple(r['dims'])} ({r['tensor_MB']} MB per tensor, {r['partials_MB']} MB of float64 "
                     f"partials): median us {r['median_us']}; forward / clone {r['forward_over_clone']}, backward (dy + dh + du + dc) "
                     f"/ clone {r['backward_over_clone']}; the clone moves {r['clone_GBps_read_plus_write']} GB/s read + write; "
                     f"n = {r['n']} per leg")
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
    for r in child("behavior", args, limit=500):
        lines.append(f"step with the behaviour modulator {r['behavior_median_ms']} ms against the plain step {r['plain_median_ms']} ms "
                     f"(difference {r['behavior_minus_plain_us']} us; n = {r['n']} per side)")
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

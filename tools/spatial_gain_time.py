#!/usr/bin/env python3
"""What the retinotopic readout gain costs, HIP events, one box; writes profiles/spatial_gain_time.txt.

Legs, every one a fresh child process under a time limit of its own; the first that fails ends the run:
  kernels   dwn_spatial_gain_forward / _backward (all five outputs; dy alone; everything but dG) at B = 32, N = 7863, T = 32, an
            8 x 8 bf16 map, K = 16 and K = 32, against dwn_modulator_forward / _backward at the same B, N, T, K and against
            y.clone(), taking turns in one process.  Bytes and operations are computed from the shapes.
  step      the DEFAULT training step (plain ``dwiseneuro``: metric configuration, B=32 T=32 36x64 bf16, expansion 7, one readout,
            EMA) with this build's library and with the parent commit's (``--parent-lib``, loaded through DWN_LIB_PATH),
            in the order parent, this, this, parent, ... (a drift over the call falls on both sides); reported: every
            process's median, the parent's own spread, whether this build lies above it.
  spatial   the ``dwiseneuro_spatial`` step against the ``dwiseneuro`` step, two models in one process taking turns.

There is no fallback: without a GPU the tool refuses to run.

python tools/spatial_gain_time.py [--parent-lib build_ab/libdwiseneuro_hip_parent.so] [--rounds 4] [--iters 8]
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
B, N, T, HF, WF = 32, 7863, 32, 8, 8
KS = (16, 32)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("spatial_gain_time: no GPU; this tool measures HIP kernels and has no fallback")


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
    """The spatial gain's and the modulator's tensors and argument blocks at one K."""

    def __init__(self, K, dev):
        import torch
        import sensorium_amd._lib as L
        self.L, self.stream, self.K = L, torch.cuda.current_stream(dev).cuda_stream, K
        g = torch.Generator(device=dev).manual_seed(K)
        r = lambda *s: torch.randn(*s, device=dev, generator=g)
        self.y, self.dout = r(B, N, T).abs() + 0.01, r(B, N, T)
        self.g = r(B, T, HF, WF, K).bfloat16()
        self.pos = torch.rand(N, 2, device=dev, generator=g) * 2 - 1
        self.weight, self.bias = r(N, K) * (0.7 / K ** 0.5), r(N) * 0.3
        self.h = r(B, T, K)
        self.out, self.dy = torch.empty_like(self.y), torch.empty_like(self.y)
        self.dg = torch.empty(self.g.shape, dtype=torch.float32, device=dev)
        self.dpos, self.dweight, self.dbias = torch.empty_like(self.pos), torch.empty_like(self.weight), torch.empty_like(self.bias)
        self.dh = torch.empty_like(self.h)
        self.ws_bytes = int(L.lib.dwn_spatial_gain_ws_bytes(C.byref(self.spatial())))
        self.mws_bytes = int(L.lib.dwn_modulator_ws_bytes(C.byref(self.modulator())))
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.float64, device=dev)
        self.mws = torch.empty(self.mws_bytes // 8, dtype=torch.float64, device=dev)
        self.s_all = self.spatial("dy", "dg", "dpos", "dweight", "dbias")
        self.s_dy = self.spatial("dy")
        self.s_nodg = self.spatial("dy", "dpos", "dweight", "dbias")
        self.m_all = self.modulator("dy", "dh", "du", "dc")

    def spatial(self, *want):
        a = self.L.SpatialGainArgs()
        a.B, a.N, a.T, a.Hf, a.Wf, a.K, a.g_dtype, a.max_log_gain = B, N, T, HF, WF, self.K, self.L.DWN_BF16, 1.0
        a.y, a.g, a.pos, a.weight, a.bias, a.out, a.dout = (t.data_ptr() for t in (self.y, self.g, self.pos, self.weight, self.bias,
                                                                                    self.out, self.dout))
        for k in want:
            setattr(a, k, getattr(self, k).data_ptr())
        if want:
            a.ws, a.ws_bytes = self.ws.data_ptr(), self.ws_bytes
        return a

    def modulator(self, *want):
        a = self.L.ModulatorArgs()
        a.B, a.N, a.T, a.K, a.max_log_gain = B, N, T, self.K, 1.0
        a.y, a.h, a.u, a.c, a.out, a.dout = (t.data_ptr() for t in (self.y, self.h, self.weight, self.bias, self.out, self.dout))
        for k, t in zip(("dy", "dh", "du", "dc"), (self.dy, self.dh, self.dweight, self.dbias)):
            if k in want:
                setattr(a, k, t.data_ptr())
        if want:
            a.ws, a.ws_bytes = self.mws.data_ptr(), self.mws_bytes
        return a

    def sp_forward(self):
        self.L.check(self.L.lib.dwn_spatial_gain_forward(C.byref(self.s_all), 0, self.stream), "dwn_spatial_gain_forward")

    def sp_backward(self, a=None):
        self.L.check(self.L.lib.dwn_spatial_gain_backward(C.byref(a or self.s_all), 0, self.stream), "dwn_spatial_gain_backward")

    def mod_forward(self):
        self.L.check(self.L.lib.dwn_modulator_forward(C.byref(self.m_all), 0, self.stream), "dwn_modulator_forward")

    def mod_backward(self):
        self.L.check(self.L.lib.dwn_modulator_backward(C.byref(self.m_all), 0, self.stream), "dwn_modulator_backward")


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
    dev = torch.device("cuda", 0)
    for K in KS:
        c = Case(K, dev)
        us, n = run_legs({"clone": lambda: c.y.clone(), "forward": c.sp_forward, "backward": c.sp_backward,
                          "backward_dy_only": lambda: c.sp_backward(c.s_dy), "backward_without_dg": lambda: c.sp_backward(c.s_nodg),
                          "modulator_forward": c.mod_forward, "modulator_backward": c.mod_backward}, args)
        elems = B * N * T
        tensor = 4 * elems
        # streaming bytes: forward reads y and writes out; backward reads y and dout, writes dy, writes s and reads it back four
        # times (a neuron's row is staged once per corner cell) and moves the float64 partials once each way
        partial = c.ws_bytes - tensor
        fwd_bytes, bwd_bytes = 2 * tensor, 3 * tensor + 5 * tensor + 2 * partial
        # multiply-adds: four corner dots of K each way; backward adds the second sweep (4K) and dG's 4K per element
        fwd_fma, bwd_fma = elems * 4 * K, elems * 12 * K
        gathered = elems * 4 * K * 2                                # bytes of corner rows a pass over the elements reads from cache
        print(json.dumps({"leg": "kernels", "K": K, "dims": (B, N, T, HF, WF, K), "tensor_MB": round(tensor / 1e6, 1),
                          "map_MB": round(c.g.numel() * 2 / 1e6, 2), "ws_MB": round(c.ws_bytes / 1e6, 1), "median_us": us,
                          "forward_over_modulator": round(us["forward"] / us["modulator_forward"], 2),
                          "backward_over_modulator": round(us["backward"] / us["modulator_backward"], 2),
                          "forward_over_clone": round(us["forward"] / us["clone"], 2),
                          "backward_over_clone": round(us["backward"] / us["clone"], 2),
                          "forward_stream_MB": round(fwd_bytes / 1e6, 1), "backward_stream_MB": round(bwd_bytes / 1e6, 1),
                          "forward_bytes_over_clone": round(fwd_bytes / (2 * tensor), 2),
                          "backward_bytes_over_clone": round(bwd_bytes / (2 * tensor), 2),
                          "forward_GFMA": round(fwd_fma / 1e9, 2), "backward_GFMA": round(bwd_fma / 1e9, 2),
                          "gathered_MB_per_pass": round(gathered / 1e6, 1),
                          "forward_gather_TBps": round(gathered / us["forward"] / 1e6, 2),
                          "clone_GBps_read_plus_write": round(2 * tensor / us["clone"] / 1e3, 1), "n": n}), flush=True)
        del c
        torch.cuda.empty_cache()


def make_model(spatial):
    import torch
    import bench
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    readouts = bench.NUM_NEURONS_ALL[:1]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    if spatial:
        name, kw = params["nn_module"]
        params["nn_module"] = ("dwiseneuro_spatial", dict(kw, spatial=dict(features=16)))
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


def leg_spatial(args):
    models = {"plain": make_model(False), "spatial": make_model(True)}
    ms = {k: [] for k in models}
    for m, b in models.values():
        timed(lambda: m.train_step(b, sync_loss=False), 3)
    for _ in range(args.rounds):
        for k, (m, b) in models.items():
            ms[k] += timed(lambda: m.train_step(b, sync_loss=False), args.iters)
    size = models["spatial"][0].nn_module.spatial._map_size
    print(json.dumps({"leg": "spatial", "plain_median_ms": median(ms["plain"]), "spatial_median_ms": median(ms["spatial"]),
                      "spatial_minus_plain_us": round(1e3 * (statistics.median(ms["spatial"]) - statistics.median(ms["plain"])), 1),
                      "map": size, "n": len(ms["spatial"])}), flush=True)


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
    ap.add_argument("--leg", choices=["all", "kernels", "step", "spatial"], default="all")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdwiseneuro_hip.so (same ABI version)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spatial_gain_time.txt"))
    args = ap.parse_args()
    require_gpu()
    if args.leg != "all":
        {"kernels": leg_kernels, "step": leg_step, "spatial": leg_spatial}[args.leg](args)
        return
    cmdline = "python tools/spatial_gain_time.py " + " ".join(sys.argv[1:])
    lines = ["retinotopic readout gain: measured times (tools/spatial_gain_time.py; HIP events, one MI355X, one box)",
             f"command: {cmdline}", ""]
    for r in child("kernels", args):
        lines.append(f"(B, N, T, Hf, Wf, K) = {tuple(r['dims'])}, bf16 map ({r['tensor_MB']} MB per [B][N][T] tensor, map {r['map_MB']} MB, "
                     f"workspace {r['ws_MB']} MB): median us {r['median_us']}")
        lines.append(f"  forward  / modulator forward  {r['forward_over_modulator']},  / clone {r['forward_over_clone']}   (streamed "
                     f"{r['forward_stream_MB']} MB = {r['forward_bytes_over_clone']} clones; {r['forward_GFMA']} G multiply-adds; "
                     f"{r['gathered_MB_per_pass']} MB of corner rows gathered from cache, {r['forward_gather_TBps']} TB/s in the forward)")
        lines.append(f"  backward / modulator backward {r['backward_over_modulator']},  / clone {r['backward_over_clone']}   (streamed "
                     f"{r['backward_stream_MB']} MB = {r['backward_bytes_over_clone']} clones; {r['backward_GFMA']} G multiply-adds); the "
                     f"clone moves {r['clone_GBps_read_plus_write']} GB/s read + write; n = {r['n']} per leg")
    lines.append("")
    if args.parent_lib:
        runs = {"parent": [], "this": []}
        order = []
        for i in range(args.rounds):                    # parent, this, this, parent, ...: a drift over the call falls on both sides
            pair = ("parent", "this") if i % 2 == 0 else ("this", "parent")
            for who in pair:
                runs[who] += child("step", args, lib=args.parent_lib if who == "parent" else None)
                order.append(who)
        pm, tm = [r["median_ms"] for r in runs["parent"]], [r["median_ms"] for r in runs["this"]]
        lo, hi = min(pm), max(pm)
        lines += ["default training step (plain dwiseneuro), parent commit's library against this build's, one process each, in the order "
                  + " ".join(order) + ":",
                  f"  parent medians ms/step: {pm}   own run-to-run spread {lo} .. {hi}",
                  f"  this   medians ms/step: {tm}",
                  f"  this build not above the parent's spread: {[t <= hi for t in tm]}; "
                  f"median of medians: parent {median(pm)}, this {median(tm)}", ""]
    else:
        lines += ["default-step A/B against the parent commit: not run (no --parent-lib)", ""]
    for r in child("spatial", args, limit=500):
        lines.append(f"step with the spatial gain (features = 16, map {tuple(r['map'])}) {r['spatial_median_ms']} ms against the plain step "
                     f"{r['plain_median_ms']} ms (difference {r['spatial_minus_plain_us']} us; n = {r['n']} per side)")
    text = "\n".join(lines) + "\n"
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

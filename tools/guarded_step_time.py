#!/usr/bin/env python3
"""Cost of the guarded optimizer step, HIP events, same box, guard off and on interleaved.

At the metric configuration (B=32, T=32, 36x64, bf16, expansion 7, EMA 0.999), with one readout (25.2 M parameters) and with ten
(171 M), two FusedAdamWEma over the same parameters — one plain, one with max_grad_norm=1.0 and skip_nonfinite=True, each with its
own moments — take turns:
  optimizer  forward + loss + backward are queued, then ONE event pair around optimizer.step(): the gradients are as cold as they
             are in training, and the host is far ahead of the device, so the pair holds the optimizer's kernels alone;
  step       the whole MouseModel.train_step(sync_loss=False), one event pair per step.
Prediction (what the code adds): one more read of the gradients at the 5.2 TB/s copy rate plus three ~4.5 us launches (partials,
fold, finaliser) = ~33 us with one readout, ~145 us with ten; the acceptance figure is twice that.

python tools/guarded_step_time.py [--readouts 1 10] [--iters 6] [--rounds 4]
One process per call and a time limit on it are the caller's: e.g. `timeout -k 10 600 python tools/guarded_step_time.py`.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from sensorium_amd.argus_models import MouseModel
from sensorium_amd.synthetic import make_batch

dev = torch.device("cuda", 0)
COPY_TBPS, LAUNCH_US = 5.2, 4.5


def summary(ms):
    s = sorted(ms)
    return dict(median_ms=round(statistics.median(s), 4), min_ms=round(s[0], 4), max_ms=round(s[-1], 4), n=len(s))


def run(n_readouts, args):
    readouts = bench.NUM_NEURONS_ALL[:n_readouts]
    params = bench.model_params(7, readouts)
    params["device"] = "cuda:0"
    torch.manual_seed(0)
    model = MouseModel(params)
    model.set_ema(0.999)
    batch = make_batch(32, 32, 36, 64, readouts, seed=1, device=dev)
    plain = model.get_optimizer()
    oname, okw = params["optimizer"]
    guarded = MouseModel.optimizer[oname]([p for p in model.nn_module.parameters() if p.requires_grad],
                                          **dict(okw, max_grad_norm=1.0, skip_nonfinite=True))
    model.optimizer = guarded
    model._bind_ema_to_optimizer()                      # both optimizers carry the EMA leg, as the training step has it
    opts = {"off": plain, "on": guarded}
    nparam = sum(p.numel() for p in model.nn_module.parameters() if p.requires_grad)

    def fwd_bwd():
        model.nn_module.train()
        model.optimizer.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = model.loss(model.nn_module(batch[0]), batch[1])
        loss.backward()

    def opt_only(opt, n):
        out = []
        for _ in range(n):
            fwd_bwd()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            opt.step()
            b.record()
            out.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in out]

    def whole(opt, n):
        model.optimizer = opt
        out = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.train_step(batch, sync_loss=False)
            b.record()
            out.append((a, b))
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in out]

    ms = {(leg, m): [] for leg in ("optimizer", "step") for m in opts}
    for m, opt in opts.items():                          # warm-up: states, pointer tables, guard buffers
        opt_only(opt, 2)
        whole(opt, 2)
    for _ in range(args.rounds):
        for m, opt in opts.items():
            ms[("optimizer", m)] += opt_only(opt, args.iters)
        for m, opt in opts.items():
            ms[("step", m)] += whole(opt, args.iters)
    stats = guarded.guard_stats()
    predicted_us = nparam * 4 / (COPY_TBPS * 1e6) + 3 * LAUNCH_US
    out = {"what": f"B=32 T=32 36x64 bf16, {n_readouts} readout(s), {nparam} parameters", "guard": stats}
    for leg in ("optimizer", "step"):
        off, on = ms[(leg, "off")], ms[(leg, "on")]
        out[leg] = {"off": summary(off), "on": summary(on),
                    "on_minus_off_us": round(1e3 * (statistics.median(on) - statistics.median(off)), 1)}
    out["predicted_us"] = round(predicted_us, 1)
    out["acceptance_us"] = round(2 * predicted_us, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--readouts", type=int, nargs="*", default=[1, 10])
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    for n in args.readouts:
        run(n, args)
        torch.cuda.empty_cache()

"""Worker of tests/test_gpu_guarded_ddp.py: one rank of a 2-process data-parallel MouseModel with the guarded optimizer step
(max_grad_norm + skip_nonfinite) on the tiny ten-readout configuration, replicated or with the sharded readout optimizer.
Launched as fresh processes by torch.distributed.run (nothing touches the GPU before the process group exists)."""
import math
import os
import struct
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch
import torch.distributed as dist


def main():
    shard = "shard" in sys.argv[1:]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)                             # both ranks share cuda:0 and exchange through gloo
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    outputs = (24, 40, 17, 33, 8, 25, 31, 12, 40, 9)
    kw = dict(readout_outputs=outputs, in_channels=5, core_features=(8, 8, 16), spatial_strides=(2, 1, 2), spatial_kernel=3,
              temporal_kernel=5, expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), groups=2, softplus_beta=0.07,
              drop_rate=0.0, drop_path_rate=0.0)
    params = {"nn_module": ("dwiseneuro", kw), "loss": ("mice_poisson", {}),
              "optimizer": ("AdamW", {"lr": 1e-3, "weight_decay": 0.05, "max_grad_norm": 1.0, "skip_nonfinite": True}),
              "device": str(dev), "amp": False, "iter_size": 1, "ddp_shard_optimizer": shard}
    torch.manual_seed(100)
    model = MouseModel(params)
    model.set_ema(0.9)
    batch = make_batch(10, 6, 12, 16, outputs, seed=7 + rank, device=dev)
    opt = model.get_optimizer()
    net = model.nn_module
    assert opt.guarded and (model.buckets.shard == shard)

    def gather(t):
        out = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(out, t.contiguous())
        return out

    def same_on_all_ranks(t):
        g = gather(t)
        return all(torch.equal(g[0].view(torch.uint8), x.view(torch.uint8)) for x in g[1:])

    def checksums():
        flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
        eflat = torch.cat([p.detach().reshape(-1) for p in model.model_ema.ema.parameters()])
        return flat, eflat

    # ---- clean step: the guard's norm against float64 sums over the gradients this very step left in p.grad (replicated
    # parameters whole, sharded ones over the owned range, summed over the ranks)
    out = model.train_step(batch)
    model.sync_for_read()
    st = opt.guard_stats()
    assert math.isfinite(out["loss"]) and not st["skipped"] and st["nonfinite"] == 0 and (st["good_steps"], st["skipped_steps"]) == (1, 0)
    whole = torch.zeros((), dtype=torch.float64, device=dev)
    owned = torch.zeros((), dtype=torch.float64, device=dev)
    for p in net.parameters():
        if p.grad is None:
            continue
        rng = model.buckets.owned_range(p)
        g = p.grad.reshape(-1).double()
        if rng is None:
            whole += (g * g).sum()
        else:
            owned += (g[rng[0]:rng[1]] ** 2).sum()
    dist.all_reduce(owned)
    want = math.sqrt(float(whole + owned))
    err = abs(st["norm"] - want) / want
    assert err < 1e-9, f"guard norm {st['norm']!r} against {want!r}: {err:.3e}"
    assert 0.0 < st["coef"] <= 1.0 and abs(st["coef"] - min(1.0, 1.0 / (want + 1e-6))) <= 2e-7 * st["coef"]
    norm1 = st["norm"]
    bits = torch.tensor(list(struct.pack("<df", st["norm"], st["coef"])), dtype=torch.uint8, device=dev)
    assert same_on_all_ranks(bits), "the ranks report different norm bits"
    flat, eflat = checksums()
    assert same_on_all_ranks(flat) and same_on_all_ranks(eflat), "the ranks diverged on a clean guarded step"

    # ---- rank 1 alone produces an Inf, in an element of a readout weight gradient that rank 0 owns
    w = net.readouts[0].layer[1].weight
    if shard:
        rng = model.buckets.owned_range(w)
        ranges = gather(torch.tensor(list(rng), dtype=torch.int64, device=dev))
        a0, z0 = ranges[0].tolist()
        assert z0 > a0, "rank 0 owns no element of the first readout's weight"
        idx = a0
        assert rank != 1 or not (rng[0] <= idx < rng[1]), "the poisoned element must lie outside rank 1's own range"
    else:
        idx = 0

    def poison(g):
        g = g.clone()
        g.view(-1)[idx] = float("inf")
        return g

    handle = w.register_hook(poison) if rank == 1 else None
    flat0, eflat0 = checksums()
    flat0, eflat0 = flat0.clone(), eflat0.clone()
    model.train_step(batch)
    model.sync_for_read()
    if handle is not None:
        handle.remove()
    st = opt.guard_stats()
    assert st["skipped"] and st["nonfinite"] >= 1 and (st["good_steps"], st["skipped_steps"]) == (1, 1), (rank, st)
    flat, eflat = checksums()
    assert torch.equal(flat, flat0), f"rank {rank}: parameters moved on a step every rank had to skip"
    assert not torch.equal(eflat, eflat0), "the EMA leg must still run"
    assert same_on_all_ranks(flat) and same_on_all_ranks(eflat), "parameter / EMA checksums differ between the ranks after the skip"

    # ---- and training goes on
    model.train_step(batch)
    model.sync_for_read()
    st2 = opt.guard_stats()
    assert not st2["skipped"] and (st2["good_steps"], st2["skipped_steps"]) == (2, 1)
    flat, eflat = checksums()
    assert same_on_all_ranks(flat) and same_on_all_ranks(eflat) and not torch.equal(flat, flat0)
    # every parameter counts the two taken steps on every rank, also a sharded one of which this rank owns no element
    steps = torch.stack([opt.state[p]["step"] for p in net.parameters()])
    assert bool((steps == 2).all()) and same_on_all_ranks(steps), steps.tolist()
    assert all(s["step"] == 2 for s in opt.state_dict()["state"].values())
    torch.cuda.synchronize()
    if rank == 0:
        print(f"GUARD_DDP_OK shard={int(shard)} norm={norm1!r} guard_norm_err={err:.3e}", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

"""Worker of tests/test_gpu_model_spatial.py::test_one_rank_data_parallel: a MouseModel on ``dwiseneuro_spatial`` on a process
group of ONE rank over RCCL with the exchange machinery forced on (``ddp_single_rank``) — mode "dense" or "shard" (sharded readout
optimizer) — next to the same model trained without data parallelism in the same process.  The spatial branch's parameters are
registered last: they must sit in a mandatory bucket of their own, ahead of the readouts' optional buckets; the gradients of the
first step must be the non-parallel model's (to 1e-4 of their norm), and after two steps the parameters and their EMA copies must agree.  One
mode per process, started fresh by torch.distributed.run (nothing touches the GPU before the process group exists)."""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import numpy as np
import torch
import torch.distributed as dist


def run_mode(mode, dev):
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    outputs = (24, 40)
    kw = dict(readout_outputs=outputs, in_channels=5, core_features=(8, 8, 16), spatial_strides=(2, 1, 2), spatial_kernel=3,
              temporal_kernel=5, expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), groups=2, softplus_beta=0.07,
              drop_rate=0.0, drop_path_rate=0.0,
              spatial=dict(features=4, max_log_gain=1.5))
    base = {"nn_module": ("dwiseneuro_spatial", kw), "loss": ("mice_poisson", {}), "optimizer": ("AdamW", {"lr": 1e-3, "weight_decay": 0.05}),
            "device": str(dev), "amp": False, "iter_size": 1}
    ddp = dict(base, ddp_single_rank=True, ddp_shard_optimizer=mode == "shard")
    models = []
    for params in (base, ddp):
        torch.manual_seed(100)
        m = MouseModel(params)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():                           # heads that are not zero: every spatial parameter gets a gradient
            for head in m.nn_module.spatial.heads:
                head.weight.copy_(torch.randn(head.weight.shape, generator=g).to(dev) * 0.3)
                head.bias.copy_(torch.randn(head.bias.shape, generator=g).to(dev) * 0.2)
        m.set_ema(0.9)
        m.get_optimizer()
        models.append(m)
    ref, par = models
    assert ref.buckets is None and par.buckets is not None and par.buckets.active and par.buckets.shard == (mode == "shard")
    names = [n for n, _ in par.nn_module.named_parameters() if n.startswith("spatial.")]
    assert len(names) == 7
    # reverse registration order: the spatial branch's bucket comes first, holds nothing else, is mandatory; the readouts' optional
    # buckets follow it, then the cortex and the core as without the branch
    first = par.buckets.buckets[0]
    pnamed = dict(par.nn_module.named_parameters())
    assert not first["optional"] and not first["sharded"]
    assert {id(p) for p in first["params"]} == {id(pnamed[n]) for n in names}
    assert par.buckets.buckets[1]["optional"]
    kinds = [b["optional"] for b in par.buckets.buckets]
    assert kinds[1:] == sorted(kinds[1:], reverse=True)              # optional (readouts) first, then mandatory only
    init = {n: pnamed[n].detach().clone() for n in names}
    a, b = dict(ref.nn_module.named_parameters()), pnamed
    grads_equal = None
    for step in range(2):
        batch = make_batch(4, 6, 12, 16, outputs, seed=7 + step, device=dev)
        for m in models:
            out = m.train_step(batch)
            assert np.isfinite(out["loss"])
        if step == 0:
            # same parameters, same batch, one rank: the same gradients, up to the order of the fp32 sums of the trunk's product
            # build (its BatchNorm statistics are accumulated with atomics): 1e-4 of the norm, a tenth of the standing fp32 bound
            torch.cuda.synchronize()
            for n in names:
                d = float((a[n].grad.double() - b[n].grad.double()).norm() / a[n].grad.double().norm())
                grads_equal = d if grads_equal is None else max(grads_equal, d)
                assert d <= 1e-4, (n, d)
    for m in models:
        m.sync_for_read()
    torch.cuda.synchronize()
    ea, eb = dict(ref.model_ema.ema.named_parameters()), dict(par.model_ema.ema.named_parameters())
    worst = 0.0
    for name in names:
        assert not torch.equal(b[name].detach(), init[name]), f"{name} did not move"
        # Adam moves a parameter by about lr = 1e-3 per step whatever its gradient's size; 1e-5 absolute is the bound
        # tests/ddp_gpu_worker.py applies to parameters and EMA copies after a step
        for x, y in ((a[name], b[name]), (ea[name], eb[name])):
            d = float((x.detach() - y.detach()).abs().max())
            worst = max(worst, d)
            assert d <= 1e-5, (name, d)
        slot = next(v for bk in par.buckets.buckets for q, v in zip(bk["params"], bk["views"]) if q is b[name])
        assert b[name].grad is not None and b[name].grad.data_ptr() == slot.data_ptr()      # the gradient sits in its bucket slice
    print(f"SPATIAL_DDP_OK mode={mode} worst={worst:.3e} worst_grad_rel={grads_equal:.3e} buckets={len(par.buckets.buckets)}", flush=True)


def main():
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    from sensorium_amd.ddp import init_rccl
    init_rccl(dev)
    run_mode(sys.argv[1], dev)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()

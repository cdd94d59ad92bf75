"""Worker of tests/test_gpu_model_lsp.py::test_one_rank_data_parallel: a MouseModel with learnable Softplus beta on a process group
of ONE rank over RCCL with the exchange machinery forced on (``ddp_single_rank``) — mode "dense", "bf16comm" (bf16 exchange), "shard"
(sharded readout optimizer) or "log" (dense, ``softplus_param="log"``: the gate's gradient is produced by autograd's exp backward
and reaches its bucket slice through the hook's copy, not by the kernel writing there) — next to the same model trained without data
parallelism in the same process.  After two steps the gate parameters and their EMA copies must agree.  One mode per process, started
fresh by torch.distributed.run (nothing touches the GPU before the process group exists)."""
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
              drop_rate=0.0, drop_path_rate=0.0, learnable_softplus=True, softplus_param="log" if mode == "log" else "beta")
    leaf, init = ("log_beta", float(np.float32(np.log(0.07)))) if mode == "log" else ("beta", float(np.float32(0.07)))
    base = {"nn_module": ("dwiseneuro", kw), "loss": ("mice_poisson", {}), "optimizer": ("AdamW", {"lr": 1e-3, "weight_decay": 0.05}),
            "device": str(dev), "amp": False, "iter_size": 1}
    ddp = dict(base, ddp_single_rank=True, ddp_shard_optimizer=mode == "shard", ddp_comm_dtype="bf16" if mode == "bf16comm" else None)
    models = []
    for params in (base, ddp):
        torch.manual_seed(100)
        m = MouseModel(params)
        m.set_ema(0.9)
        m.get_optimizer()
        models.append(m)
    ref, par = models
    assert ref.buckets is None and par.buckets is not None and par.buckets.active and par.buckets.shard == (mode == "shard")
    gate_names = [f"readouts.{k}.gate.{leaf}" for k in range(2)]
    # the gate parameter rides in its readout's bucket (optional: forward(x, index) may leave it without a gradient)
    for k, name in enumerate(gate_names):
        p = dict(par.nn_module.named_parameters())[name]
        owners = [b for b in par.buckets.buckets if id(p) in b["index"]]
        assert len(owners) == 1 and owners[0]["optional"]
        assert id(par.nn_module.readouts[k].layer[1].weight) in owners[0]["index"]
        if mode == "shard":
            b = owners[0]
            off = b["offsets"][b["index"][id(p)]]
            assert b["sharded"] and b["owner"] == f"readouts.{k}" and p.data_ptr() == b["pflat"].data_ptr() + 4 * off
            e = dict(par.model_ema.ema.named_parameters())[name]
            assert e.data_ptr() == b["eflat"].data_ptr() + 4 * off          # adopt_ema: the flat EMA layout
    assert len(par.optimizer.param_groups) == 2 and par.optimizer.param_groups[1]["weight_decay"] == 0.0
    for step in range(2):
        batch = make_batch(4, 6, 12, 16, outputs, seed=7 + step, device=dev)
        for m in models:
            out = m.train_step(batch)
            assert np.isfinite(out["loss"])
    for m in models:
        m.sync_for_read()
    torch.cuda.synchronize()
    a, b = dict(ref.nn_module.named_parameters()), dict(par.nn_module.named_parameters())
    ea, eb = dict(ref.model_ema.ema.named_parameters()), dict(par.model_ema.ema.named_parameters())
    worst = 0.0
    for name in gate_names:
        pa, pb = float(a[name].detach()), float(b[name].detach())
        assert pa != init and pb != init, "the gate parameter did not move"
        # Adam moves a parameter by about lr = 1e-3 per step whatever its gradient's size; 1e-5 absolute is the bound
        # tests/ddp_gpu_worker.py applies to parameters and EMA copies after a step (bf16 exchange included: one element)
        for x, y in ((pa, pb), (float(ea[name].detach()), float(eb[name].detach()))):
            worst = max(worst, abs(x - y))
            assert abs(x - y) <= 1e-5, (name, x, y)
        assert float(eb[name].detach()) != init
        slot = next(v for bk in par.buckets.buckets for q, v in zip(bk["params"], bk["views"]) if q is b[name])
        assert b[name].grad is not None and b[name].grad.data_ptr() == slot.data_ptr()      # the gradient sits in its bucket slice
    print(f"LSP_DDP_OK mode={mode} worst={worst:.3e}", flush=True)


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

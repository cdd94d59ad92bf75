"""Worker of tests/test_gpu_train_input_grad.py (test 7): the training-mode input gradient under the ordered-reduction build.
Run as a fresh process so that DWN_DETERMINISTIC (read when sensorium_amd._lib is imported) selects the library.

One training-mode forward + Poisson loss + backward (DropPath / Dropout on, fixed seeds) three times from the same state: twice
with x.requires_grad, once without.  Then the stem alone through the C-ABI: dwn_stem_backward_input against dwn_stem_backward.
Prints one line: DET_INPUT_GRAD deterministic=<0|1> lib=<..> tensors=<n> dx_nonzero=<0|1> dx_identical=<0|1>
same_without_dx=<0|1> differing=<names> stem_identical=<0|1>"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch


def run(kind: str):
    from sensorium_amd import _lib as L
    from sensorium_amd.argus_models import MouseModel
    from sensorium_amd.synthetic import make_batch
    from tests.stem_abi_helpers import SHAPES, make_case, run_stem
    dev = torch.device("cuda:0")
    if kind.startswith("tiny"):
        kw = dict(readout_outputs=(24, 40), in_channels=5, core_features=(8, 8, 16), spatial_strides=(2, 1, 2), spatial_kernel=3,
                  temporal_kernel=5, expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), groups=2,
                  softplus_beta=0.07, drop_rate=0.2, drop_path_rate=0.1)
        shape = (3, 6, 12, 16)
    else:       # the metric architecture at a small batch, as tests/det_worker.py
        kw = dict(readout_outputs=(512,), in_channels=5, core_features=(64, 64, 64, 64, 128, 128, 128, 256, 256),
                  spatial_strides=(2, 1, 1, 1, 2, 1, 1, 2, 1), spatial_kernel=3, temporal_kernel=5, expansion_ratio=7,
                  se_reduce_ratio=32, cortex_features=(1024, 2048, 4096), groups=2, softplus_beta=0.07, drop_rate=0.4,
                  drop_path_rate=0.1)
        shape = (2, 8, 36, 64)
    amp = not kind.endswith("_f32")
    params = {"nn_module": ("dwiseneuro", kw), "loss": ("mice_poisson", {}), "optimizer": ("AdamW", {"lr": 1e-3, "weight_decay": 0.05}),
              "device": str(dev), "amp": amp, "iter_size": 1}
    results = []
    for want_dx in (True, True, False):
        torch.manual_seed(1234)
        torch.cuda.manual_seed_all(1234)
        model = MouseModel(params)
        net = model.nn_module
        net.train()
        inp, target = make_batch(*shape, kw["readout_outputs"], seed=7, device=dev)
        inp = inp.clone().requires_grad_(want_dx)
        torch.manual_seed(99)
        torch.cuda.manual_seed_all(99)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=amp):
            prediction = net(inp)
            loss = model.loss(prediction, target)
        loss.backward()
        torch.cuda.synchronize()
        snap = {"loss": loss.detach().double().cpu().clone()}
        for m, p in enumerate(prediction):
            snap[f"pred.{m}"] = p.detach().float().cpu().clone()
        for n, p in net.named_parameters():
            assert p.grad is not None, n
            snap[f"grad:{n}"] = p.grad.detach().cpu().clone()
        for n, t in net.state_dict().items():
            if "running" in n or "num_batches" in n:
                snap[f"state:{n}"] = t.detach().cpu().clone()
        results.append((snap, inp.grad.detach().cpu().clone() if want_dx else None))
    (a, dxa), (b, dxb), (c, _) = results
    assert a.keys() == b.keys() == c.keys()
    dx_nonzero = bool(torch.isfinite(dxa).all()) and float(dxa.abs().max()) > 0
    dx_identical = torch.equal(dxa, dxb) and all(torch.equal(a[k], b[k]) for k in a)
    differing = [k for k in a if not torch.equal(a[k], c[k])]

    stem_identical = True
    for name in ("metric", "odd", "wide8"):
        for dtype in (torch.bfloat16, torch.float32):
            case = make_case(SHAPES[name], dtype, "mixed")
            new, old = run_stem(case, "backward_input", dev), run_stem(case, "backward", dev)
            for key in ("dgamma", "dbeta", "dw"):
                ok = torch.equal(new[key], old[key]) and bool(torch.isfinite(new[key]).all())
                if not ok:
                    print(f"stem {name} {dtype} {key}: differs", flush=True)
                stem_identical = stem_identical and ok
    print(f"DET_INPUT_GRAD deterministic={int(L.DETERMINISTIC)} lib={L.LIB_PATH.name} tensors={len(a)} dx_nonzero={int(dx_nonzero)} "
          f"dx_identical={int(dx_identical)} same_without_dx={int(not differing)} differing={','.join(differing[:5])} "
          f"stem_identical={int(stem_identical)}", flush=True)


if __name__ == "__main__":
    run(sys.argv[1] if len(sys.argv) > 1 else "tiny")

#!/usr/bin/env python3
"""Writes tests/golden/temporal_kernel_7_9.npz: a tiny DwiseNeuro with temporal_kernel 7 and 9 run by the REAL reference module in
float64 — weights, two inputs (T = 3, shorter than the padding of either size, and T = 11), the eval and the training-mode
predictions and the input gradient of each — the fixture tests/test_temporal_kernel_cpu.py holds the oracle to at these sizes.

usage: tools/make_golden_temporal_kernel.py /path/to/reference/src/models/dwiseneuro.py [out.npz]

The reference is loaded by the path given; nothing of it is copied: the fixture holds arrays only.  Weights come from the oracle's
make_state_dict (float32 values, the reference's key names) and the float64 results are stored rounded to float32 (6e-8, far
below the test's 2e-5), as in tools/make_golden_spatial_kernel.py."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import dwiseneuro_oracle as orc  # noqa: E402

N_OUT = 9
CFG = dict(readout_outputs=(N_OUT,), in_channels=5, core_features=(8, 16), spatial_strides=(2, 1), spatial_kernel=3,
           expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), groups=2, softplus_beta=0.07, drop_rate=0.0,
           drop_path_rate=0.0)
FRAMES = (3, 11)


def main():
    ref_path = Path(sys.argv[1])
    out = Path(sys.argv[2]) if len(sys.argv) > 2 else ROOT / "tests" / "golden" / "temporal_kernel_7_9.npz"
    spec = importlib.util.spec_from_file_location("reference_dwiseneuro", ref_path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(79)
    arrays = {f"x{T}": rng.normal(size=(2, 5, T, 9, 11)).astype(np.float32) for T in FRAMES}
    for kt in (7, 9):
        sd = orc.make_state_dict(readout_outputs=(N_OUT,), core_features=(8, 16), spatial_kernel=3, temporal_kernel=kt,
                                 expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64), seed=70 + kt, randomize_bn=True)
        for k, v in sd.items():
            arrays[f"k{kt}:sd:{k}"] = v.numpy()
        for T in FRAMES:
            for mode in ("eval", "train"):
                # the training-mode forward moves the running statistics: a fresh module per run
                model = ref.DwiseNeuro(temporal_kernel=kt, **CFG).double()
                res = model.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, strict=True)
                assert not res.missing_keys and not res.unexpected_keys
                model.train(mode == "train")
                xt = torch.from_numpy(arrays[f"x{T}"]).double().requires_grad_(True)
                pred = model(xt, 0)
                pred.sum().backward()
                arrays[f"k{kt}:T{T}:{mode}:pred"] = pred.detach().numpy().astype(np.float32)
                arrays[f"k{kt}:T{T}:{mode}:dx"] = xt.grad.numpy().astype(np.float32)
    np.savez_compressed(out, **arrays)
    print(f"wrote {out}: {len(arrays)} arrays, {out.stat().st_size} bytes")


if __name__ == "__main__":
    main()

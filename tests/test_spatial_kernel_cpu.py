"""CPU: the oracle at spatial_kernel 5 and 7 against tests/golden/spatial_kernel_5_7.npz, which tools/make_golden_spatial_kernel.py
wrote from the real reference module in float64 (a tiny DwiseNeuro: weights, one input, eval and training-mode predictions, the
input gradient of each).  The GPU tests of these kernel sizes (tests/test_gpu_block_ks.py, test_gpu_model_ks.py) compare with the
oracle; this file pins that yardstick.  Tolerance: the 2e-5 tests/test_oracle_golden.py holds the tiny-model fixtures to."""
import numpy as np
import pytest
import torch

from oracle import dwiseneuro_oracle as orc

KW = dict(strides=(2, 1), readout_outputs=(9,), groups=2, softplus_beta=0.07)


def rel(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("ks", [5, 7])
def test_oracle_matches_reference_module(golden_dir, ks, training):
    z = np.load(golden_dir / "spatial_kernel_5_7.npz")
    pre = f"k{ks}:sd:"
    sd = {k[len(pre):]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    assert sd["core.blocks.1.spat_covn_dw.0.weight"].shape[2:] == (1, ks, ks)
    assert sd["core.blocks.3.spat_covn_dw.0.weight"].shape[2:] == (1, ks, ks)
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    x = torch.from_numpy(z["x"]).double().requires_grad_(True)
    assert x.shape == (2, 5, 4, 9, 11)
    mode = "train" if training else "eval"
    pred = orc.forward(sd, x, index=0, training=training, **KW)
    pred.sum().backward()
    assert pred.shape == z[f"k{ks}:{mode}:pred"].shape
    assert rel(pred.detach().numpy(), z[f"k{ks}:{mode}:pred"]) < 2e-5
    assert float(np.abs(z[f"k{ks}:{mode}:dx"]).max()) > 0
    assert rel(x.grad.numpy(), z[f"k{ks}:{mode}:dx"]) < 2e-5

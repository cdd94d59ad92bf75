#!/usr/bin/env python3
"""Golden fixture for the weight-init rule (tests/test_engine_cpu.py::test_init_weights_bit_exact_against_reference) from the
REAL reference (build container only; never runs on the GPU box).

  python oracle/make_golden_init.py <reference checkout>      (after build(): the probe net comes from the test module,
                                                              which imports the package)

init_weights.npz — the reference's ``init_weights`` (src/utils.py) applied to the test's probe network after
``torch.manual_seed(11)``: every state-dict entry, bit for bit, plus ``get_lr(3e-4, 32)``.  Only data is stored."""
from __future__ import annotations

import argparse
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
sys.path.insert(0, str(ROOT))

from tests.test_engine_cpu import _probe_net  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", type=Path, help="checkout of the reference project")
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("ref_utils_init", args.reference / "src" / "utils.py")
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)  # type: ignore[union-attr]
    net = _probe_net()
    torch.manual_seed(11)
    ref.init_weights(net)
    out = {f"sd/{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()}
    out["get_lr_3e-4_32"] = np.float64(ref.get_lr(3e-4, 32))
    np.savez_compressed(GOLD / "init_weights.npz", **out)
    print("wrote", GOLD / "init_weights.npz", sorted(out))


if __name__ == "__main__":
    main()

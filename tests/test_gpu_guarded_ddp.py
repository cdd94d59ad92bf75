"""The guarded optimizer step under data parallelism: two ranks sharing cuda:0 over gloo, started as fresh child
processes like tests/test_gpu_ddp.py, on the tiny ten-readout configuration, with ddp_shard_optimizer off and on.  The worker
(tests/guarded_ddp_worker.py) holds the guard's norm to 1e-9 of float64 sums over the step's own gradients, requires the same norm
bits on both ranks, and makes rank 1 alone produce an Inf inside rank 0's owned range: both ranks must skip, and parameters and
EMA must stay equal across the ranks — which fails when the sharded slices' [sumsq, nonfinite] pair is not all-reduced."""
import os
import re
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
MODES = {"replicated": (), "sharded": ("shard",)}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(*extra):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    # the ordered-reduction build, where it exists: the gradients of two runs are then the same bits, and so must the norms be
    # (with the product build the two runs' backward passes differ by the arrival order of their float atomics; each worker still
    # holds its guard's norm to 1e-9 of float64 sums over its own gradients, in both modes)
    if (ROOT / "sensorium_amd" / "csrc" / "libdwiseneuro_hip_det.so").exists() and not os.environ.get("DWN_LIB_PATH"):
        env["DWN_DETERMINISTIC"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "tests" / "guarded_ddp_worker.py"), *extra]
    return subprocess.run(cmd, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def runs():
    """Both modes, once per module, whichever of the tests below are selected."""
    return {mode: _run(*extra) for mode, extra in MODES.items()}


def _norm(res):
    assert res.returncode == 0 and "GUARD_DDP_OK" in res.stdout, res.stdout[-2000:] + res.stderr[-3000:]
    print(re.search(r"GUARD_DDP_OK.*", res.stdout).group(0))
    return float(re.search(r"GUARD_DDP_OK .*norm=(\S+) ", res.stdout).group(1))


@pytest.mark.parametrize("mode", list(MODES))
def test_two_ranks_guarded_step(runs, mode):
    _norm(runs[mode])


def test_sharded_and_replicated_norms_agree(runs):
    a, b = _norm(runs["replicated"]), _norm(runs["sharded"])
    assert abs(a - b) / a < 1e-9, f"replicated {a!r} against sharded {b!r}"

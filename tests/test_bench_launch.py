"""bench.py launch plumbing on CPU: `python bench.py --gpus 2` must start its own ranks and the same
command under an external torch.distributed.run must not start them twice."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def test_self_launch_two_ranks():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--dry-run", "--backend", "gloo"], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _last_json(r.stdout)
    assert j["n_gpus"] == 2 and j["ranks"] == 2 and j["steps"] == 3 and j["warmup"] == 1


def test_external_launcher_two_ranks():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "2",
                        "--steps", "2", "--warmup", "0", "--dry-run", "--backend", "gloo"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _last_json(r.stdout)["ranks"] == 2


def test_child_failure_is_relayed():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--dry-run", "--backend", "nosuchbackend"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0


def test_single_rank_dry_run_needs_no_launcher():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--dry-run", "--steps", "2"], env=_env(),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _last_json(r.stdout)["ranks"] == 1



def test_dump_outputs_writes_the_step_results_within_budget(tmp_path, monkeypatch):
    """bench.py --dump-outputs (CPU: dump_outputs on a stand-in step result): the step's predictions in full while they fit, a
    fixed seeded sample once they do not; the same sample on every run."""
    import numpy as np
    import torch
    sys.path.insert(0, str(ROOT))
    import bench

    torch.manual_seed(0)
    step = {"prediction": [torch.randn(2, 50, 4), torch.randn(2, 30, 4)], "loss": torch.tensor(1.25)}
    bench.dump_outputs(tmp_path / "a", step)
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["loss.npy", "prediction_0.npy", "prediction_1.npy"]
    loss = np.load(tmp_path / "a" / "loss.npy")
    assert loss.dtype == np.float64 and float(loss) == 1.25
    for m, p in enumerate(step["prediction"]):
        a = np.load(tmp_path / "a" / f"prediction_{m}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, p.numpy())
    # a budget the predictions do not fit in: seeded samples, repeatable, within the budget
    monkeypatch.setattr(bench, "DUMP_BUDGET", 8 + 400)
    for d in ("b", "c"):
        bench.dump_outputs(tmp_path / d, step)
    names = sorted(p.name for p in (tmp_path / "b").iterdir())
    assert names == ["loss.npy", "prediction_0_sample.npy", "prediction_1_sample.npy"]
    assert sum(np.load(p).nbytes for p in (tmp_path / "b").iterdir()) <= 8 + 400
    s0 = np.load(tmp_path / "b" / "prediction_0_sample.npy")
    assert s0.size == 62 and np.isin(s0, step["prediction"][0].numpy()).all()
    for p in (tmp_path / "b").iterdir():
        assert np.array_equal(np.load(p), np.load(tmp_path / "c" / p.name)), p.name


def test_restore_state_returns_the_model_to_its_snapshot():
    """bench.py --dump-outputs restarts the last timed step from the run's starting state: weights, BatchNorm buffers, EMA
    copies, Adam moments / step counts and the RNG all come back (CPU: a stand-in model)."""
    import copy
    import types

    import torch
    sys.path.insert(0, str(ROOT))
    import bench

    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(6, 4), torch.nn.BatchNorm1d(4))
    ema = types.SimpleNamespace(ema=copy.deepcopy(net))
    model = types.SimpleNamespace(nn_module=net, model_ema=ema, optimizer=None, sync_for_read=lambda: None)
    dev = torch.device("cpu")
    want = {k: v.clone() for k, v in net.state_dict().items()}
    snap = bench.snapshot_state(model, dev)
    draw = torch.rand(5)
    with torch.no_grad():                                    # what training does to the state
        net(torch.randn(8, 6))
        for p in net.parameters():
            p.add_(1.0)
        for v in ema.ema.parameters():
            v.mul_(2.0)
    model.optimizer = types.SimpleNamespace(state={p: {"step": 7, "exp_avg": torch.ones_like(p), "exp_avg_sq": torch.ones_like(p)}
                                                   for p in net.parameters()})
    ptrs = [v.data_ptr() for v in net.state_dict().values()]
    bench.restore_state(model, snap, dev)
    for k, v in net.state_dict().items():
        assert torch.equal(v, want[k]), k
        assert torch.equal(ema.ema.state_dict()[k], want[k]), k
    assert [v.data_ptr() for v in net.state_dict().values()] == ptrs          # in place
    for st in model.optimizer.state.values():
        assert st["step"] == 0 and not st["exp_avg"].any() and not st["exp_avg_sq"].any()
    assert torch.equal(torch.rand(5), draw)


def test_timed_steps_restores_before_the_second_to_last_step_untimed():
    """bench.py's timed loop with --dump-outputs: the restore runs once, between steps n-2 and n-1, and its time is not
    counted; without a restore nothing is drained mid-way; two steps are the fewest a dump run takes."""
    import time
    sys.path.insert(0, str(ROOT))
    import bench

    for n in (2, 3, 6):
        log = []

        def step():
            log.append("step")
            time.sleep(0.01)
            return len(log)

        def restore():
            log.append("restore")
            time.sleep(0.5)

        last, elapsed = bench.timed_steps(n, step, lambda: log.append("sync"), restore)
        steps = [e for e in log if e != "sync"]
        assert steps == ["step"] * (n - 2) + ["restore", "step", "step"], (n, log)
        i = log.index("restore")
        assert log[i - 1] == "sync" and log[i + 1] == "sync" and log[-1] == "sync"
        assert last == len(log) - 1                            # the last step's own result
        assert 0.01 * n <= elapsed < 0.01 * n + 0.3            # the 0.5 s restore is not in it
    log = []
    last, elapsed = bench.timed_steps(4, lambda: log.append("step") or 7, lambda: log.append("sync"))
    assert log == ["step"] * 4 + ["sync"] and last == 7


def test_dump_outputs_needs_two_steps():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--dry-run", "--steps", "1", "--dump-outputs", "unused"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps 2 or more" in r.stderr
    assert not (Path.cwd() / "unused").exists()

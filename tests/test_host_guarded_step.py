"""CPU tests of the host side of the guarded optimizer step (include/dwn.h dwn_grad_sumsq_multi, dwn_step_guard_finalize,
dwn_adamw_ema_multi_guarded, dwn_grad_guard_workspace_bytes): the entries are exported with ctypes prototypes and declared in the
header, the ABI is still 7, the two new structs have the layout ctypes expects, the old entry struct did not move, and every
argument check answers before anything touches a device."""
import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
NEW = ("dwn_grad_guard_workspace_bytes", "dwn_grad_sumsq_multi", "dwn_step_guard_finalize", "dwn_adamw_ema_multi_guarded")
PTR = 256            # never dereferenced on the host


def test_symbols_prototypes_and_header():
    import sensorium_amd._lib as L
    assert L.lib.dwn_abi_version() == 7
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header)
    for name in NEW:
        assert hasattr(L.lib, name) and name in L.SYMBOLS, name
        assert re.search(r"\b(int|size_t) %s\(" % name, header), name
    assert L.SYMBOLS["dwn_grad_guard_workspace_bytes"][0] is C.c_size_t
    for name, nargs in (("dwn_grad_sumsq_multi", 9), ("dwn_step_guard_finalize", 9), ("dwn_adamw_ema_multi_guarded", 13)):
        restype, argtypes = L.SYMBOLS[name]
        assert restype is C.c_int and len(argtypes) == nargs, name
    assert "typedef struct dwn_guarded_entry" in header and "typedef struct dwn_step_guard" in header


def test_struct_layouts():
    import sensorium_amd._lib as L
    assert L.lib.dwn_sizeof(b"dwn_guarded_entry") == C.sizeof(L.GuardedEntry) == 64
    assert L.lib.dwn_sizeof(b"dwn_step_guard") == C.sizeof(L.StepGuard) == 40
    # additive: the entry of dwn_adamw_ema_multi / dwn_ema_lerp_multi is where it was
    assert L.lib.dwn_sizeof(b"dwn_tensor_entry") == C.sizeof(L.TensorEntry) == 56
    # the guarded entry is the old one plus the counter: same offsets for the shared fields
    for name in ("param", "grad", "exp_avg", "exp_avg_sq", "ema", "numel", "is_int64"):
        assert getattr(L.GuardedEntry, name).offset == getattr(L.TensorEntry, name).offset, name
    assert L.GuardedEntry.step.offset == 56
    assert (L.StepGuard.norm.offset, L.StepGuard.coef.offset, L.StepGuard.skip.offset, L.StepGuard.nonfinite.offset,
            L.StepGuard.good_steps.offset, L.StepGuard.skipped_steps.offset) == (0, 8, 12, 16, 24, 32)


def test_workspace_bytes():
    import sensorium_amd._lib as L
    ws = L.lib.dwn_grad_guard_workspace_bytes
    assert ws(1, 1) == 16 and ws(37, 64) == 64 * 16 and ws(0, 16) == 16 * 16       # one [sumsq, count] partial per workgroup
    assert ws(1024, 8) == 8 * 16 and ws(1025, 8) == 2 * 8 * 16                     # a second launch's partials past 1024 tensors
    assert ws(-1, 8) == 0 and ws(4, 0) == 0


def test_sumsq_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    f, err = L.lib.dwn_grad_sumsq_multi, L.lib.dwn_last_error
    need = L.lib.dwn_grad_guard_workspace_bytes(37, 64)
    assert f(None, 37, 64, 1.0, PTR, need, PTR, 0, None) == -1 and b"grad_sumsq_multi" in err()        # null table
    assert f(PTR, 37, 64, 1.0, None, need, PTR, 0, None) == -1 and b"grad_sumsq_multi" in err()        # null workspace
    assert f(PTR, 37, 64, 1.0, PTR, need, None, 0, None) == -1 and b"grad_sumsq_multi" in err()        # null result pair
    assert f(PTR, 37, 64, 1.0, PTR, need - 1, PTR, 0, None) == -6 and b"grad_sumsq_multi" in err()     # workspace too small
    assert f(PTR, 1025, 64, 1.0, PTR, need, PTR, 0, None) == -6                                        # (two launches' partials)
    assert f(PTR, -1, 64, 1.0, PTR, need, PTR, 0, None) == -2 and b"grad_sumsq_multi" in err()         # ntensors < 0
    assert f(PTR, 37, 0, 1.0, PTR, need, PTR, 0, None) == -2
    assert f(PTR, 37, 64, 1.0, PTR + 8, need, PTR, 0, None) == -2                                      # misaligned workspace


def test_finalize_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    f, err = L.lib.dwn_step_guard_finalize, L.lib.dwn_last_error
    assert f(PTR, None, 1.0, 1, PTR, 3, None, 0, None) == -1 and b"step_guard_finalize" in err()       # null guard
    assert f(None, None, 1.0, 1, PTR, 3, PTR, 0, None) == -1 and b"step_guard_finalize" in err()       # null pair
    assert f(PTR, None, 1.0, 1, None, 3, PTR, 0, None) == -1 and b"step_guard_finalize" in err()       # null table
    assert f(PTR, None, 1.0, 1, PTR, -1, PTR, 0, None) == -2 and b"step_guard_finalize" in err()       # ntensors < 0
    assert f(PTR, None, float("nan"), 1, PTR, 3, PTR, 0, None) == -2


def test_guarded_adamw_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    f, err = L.lib.dwn_adamw_ema_multi_guarded, L.lib.dwn_last_error
    tail = (1e-3, 0.9, 0.999, 1e-8, 0.05, 0.999, 1.0)
    assert f(None, 3, 16, *tail, PTR, 0, None) == -1 and b"adamw_ema_multi_guarded" in err()           # null table
    assert f(PTR, 3, 16, *tail, None, 0, None) == -1 and b"adamw_ema_multi_guarded" in err()           # null guard
    assert f(PTR, -1, 16, *tail, PTR, 0, None) == -2 and b"adamw_ema_multi_guarded" in err()           # ntensors < 0
    assert f(PTR, 3, 0, *tail, PTR, 0, None) == -2
    assert f(PTR, 70000, 16, *tail, PTR, 0, None) == -2                                                # a grid dimension


def test_python_surface_without_a_device():
    import pytest
    import torch
    from sensorium_amd.optim import FusedAdamWEma
    p = torch.nn.Parameter(torch.zeros(3))
    opt = FusedAdamWEma([p])
    assert not opt.guarded and opt.guard_stats() is None
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        opt = FusedAdamWEma([p], **kw)
        assert opt.guarded
        assert opt.guard_stats() == {"norm": 0.0, "coef": 1.0, "skipped": False, "nonfinite": 0, "good_steps": 0, "skipped_steps": 0}
    with pytest.raises(ValueError):
        FusedAdamWEma([p], max_grad_norm=0.0)


def test_trajectory_figure_is_well_conditioned_for_any_seed(monkeypatch):
    """A guard on the fixture of tests/test_gpu_guarded_step.py::test_ten_step_trajectory_with_two_skipped_steps, not on the feature:
    the kernel's formulas restated in float32 on the CPU stay within 5e-7 — half the 1e-6 bound, the other half being left to the
    device's own order of float32 operations (contraction, division) — of the float64 reference in the figure the GPU test asserts
    (guarded_helpers.traj_error), for twenty seeds and not for a chosen one (they spread over 2.5e-7 .. 4.6e-7: sixteen roundings of a
    single element's p; the norm-relative figure of the same 1-element tensor spread over 2.7e-7 .. 1e-4); and the reference tells a trajectory that counted a skipped step from one that did not."""
    import torch
    from tests import guarded_helpers as G
    from tests.gpu_helpers import ADAMW_BOUND, rel
    has_ema = [i != 2 for i in range(len(G.TRAJ_SIZES))]
    for seed in range(G.TRAJ_SEED, G.TRAJ_SEED + 20):
        monkeypatch.setattr(G, "TRAJ_SEED", seed)
        for step0 in G.TRAJ_STEP0:
            case = G.traj_case(step0)
            for clip in (False, True):
                want, scale = G.traj_reference(case, step0, clip, has_ema, with_scale=True)
                f32 = G.traj_reference(case, step0, clip, has_ema, dtype=torch.float32)
                worst = max(G.traj_error(f32[i][k], want[i][k], scale[i][k]) for i in range(len(case)) for k in ("p", "m", "v", "ema"))
                assert worst <= 5e-7, (seed, step0, clip, worst)
    monkeypatch.undo()
    for step0 in G.TRAJ_STEP0[:2]:        # (at 100 000 the bias corrections have converged: a count off by two changes nothing measurable)
        case = G.traj_case(step0)
        late = G.traj_reference(case, step0 + 2, False, has_ema)           # as if the two skipped steps had been counted
        want = G.traj_reference(case, step0, False, has_ema)
        assert max(rel(late[i]["p"], want[i]["p"]) for i in range(len(case)) if G.TRAJ_SIZES[i] > G.TINY) > 10 * ADAMW_BOUND


def test_epoch_line_reports_skipped_steps(caplog):
    """engine._DefaultLogging: `skipped_steps` joins the train epoch line when the model's optimizer has a guard (one guard_stats()
    call per epoch), and only then.  LoggingToFile writes what this logger emits."""
    import logging
    from types import SimpleNamespace
    from sensorium_amd.engine import _DefaultLogging

    class Opt:
        calls = 0

        def __init__(self, stats):
            self.stats = stats

        def guard_stats(self):
            Opt.calls += 1
            return self.stats

    def line(optimizer, phase="train"):
        logger = logging.getLogger("sensorium_amd.test_epoch_line")
        model = SimpleNamespace(optimizer=optimizer, get_lr=lambda: 1e-3)
        state = SimpleNamespace(phase=phase, epoch=3, model=model, metrics={"train_loss": 1.5, "val_loss": 2.5}, logger=logger)
        caplog.clear()
        with caplog.at_level(logging.INFO, logger=logger.name):
            _DefaultLogging().epoch_complete(state)
        return caplog.records[-1].getMessage()

    on = Opt({"norm": 1.0, "coef": 1.0, "skipped": False, "nonfinite": 0, "good_steps": 40, "skipped_steps": 2})
    assert line(on).endswith("train_loss: 1.5, skipped_steps: 2") and Opt.calls == 1
    assert "skipped_steps" not in line(on, "val") and Opt.calls == 1
    assert "skipped_steps" not in line(Opt(None)) and "skipped_steps" not in line(None) and "skipped_steps" not in line(object())


def test_documents_have_the_section():
    design = (ROOT / "DESIGN.md").read_text()
    assert re.search(r"^#+ *12d\b", design, re.M), "DESIGN.md section 12d"
    integration = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW[1:]:
        assert name in design and name in integration, name
    assert "max_grad_norm" in integration and "skip_nonfinite" in integration and "guard_stats" in integration
    assert "tools/guarded_step_time.py" in design

"""The gradient w.r.t. the model input in TRAINING mode, through the stem's batch statistics (include/dwn.h
dwn_stem_backward_input).

Ground truth everywhere is float64 autograd: torch on the CPU at stem level (tests/stem_abi_helpers.py), the oracle with
``training=True`` at model level; never the code under test.  Bounds: fp32 1e-3 as everywhere in this project, as a cap; where a
bound had no precedent it is 2 x the value measured on an MI355X, rounded up to one digit, and both figures stand beside the
assert, as in tests/test_gpu_frozen_bn.py.  Every test prints what it measured before it asserts.
"""
import math
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests.gpu_helpers import dev, rel, synth_inputs  # noqa: E402
from tests.stem_abi_helpers import EPS, SHAPES, make_case, run_stem  # noqa: E402
from tests.test_gpu_frozen_bn import FULL_STRIDES, INPUT_SCALE, N_FULL, TINY, _model_input, full_model, sd64, tiny_model  # noqa: E402

F32_EPS = 2.0 ** -24           # unit roundoff of fp32


def fp32_level(C0, Cin):
    """Relative size of what fp32 leaves of a sum that is zero in exact arithmetic: an n-term fp32 dot product is off by at most
    n * 2^-24 of the sum of its terms' magnitudes; dx is a C0-term and a (Cin + 1)-term product plus one add, and the factor 2
    covers the ratio of the terms' magnitudes to the norm of the first term they are compared with."""
    return 2 * (C0 + Cin + 2) * F32_EPS


# ------------------------------------------------------------------------------------------------ 1. stem through the C-ABI
# dx against float64 autograd, relative L2: measured on an MI355X / bound = 2 x measured rounded up to one digit (cap 1e-3)
STEM_DX = {
    ("metric", "float32"): (2.437e-7, 5e-7), ("metric", "bfloat16"): (2.454e-7, 5e-7),
    ("odd", "float32"): (2.278e-7, 5e-7), ("odd", "bfloat16"): (2.133e-7, 5e-7),
    ("tiny", "float32"): (2.471e-7, 5e-7), ("tiny", "bfloat16"): (2.083e-7, 5e-7),
    ("wide8", "float32"): (2.499e-7, 5e-7), ("wide8", "bfloat16"): (3.304e-7, 7e-7),
    ("ragged", "float32"): (1.601e-7, 4e-7), ("ragged", "bfloat16"): (1.595e-7, 4e-7),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stem_backward_input_c_abi(name, dtype):
    """dwn_stem_forward (batch statistics) then dwn_stem_backward_input: dx against autograd of conv1x1 -> batch_norm(training),
    production-range inputs, dout = r + 0.5 zhat + c so that the batch-statistics terms are a large part of dx (asserted first,
    in float64: the frozen-mode formula alone is off by more than 0.1).  bf16 dout is exact in both (the reference sees the rounded
    values), so both dtypes are held to the fp32 treatment."""
    case = make_case(SHAPES[name], dtype, "mixed")
    off = rel(case["first"], case["dx"])
    assert off > 0.1, f"the case does not exercise the batch-statistics terms: frozen formula alone is off by {off:.3e}"
    got = run_stem(case, "backward_input")
    e = rel(got["dx"], case["dx"])
    print(f"stem backward_input {name} {case['shape']} {dtype}: dx rel err {e:.3e} (frozen formula alone: {off:.3e})")
    assert bool(torch.isfinite(got["dx"]).all())
    measured, bound = STEM_DX[(name, str(dtype)[6:])]
    assert bound is not None, f"bound not set yet; measured now {e:.3e}"
    assert bound <= 1e-3
    assert e < bound, f"measured on MI355X {measured}, bound {bound}, now {e:.3e}"


# ------------------------------------------------------------------------------------------------------- 2. null directions
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", ["metric", "odd", "wide8"])
def test_constant_dout_is_annihilated(name, dtype):
    """dout constant per channel: BatchNorm's backward removes the mean, dx = 0 in exact arithmetic (the first term and q0 cancel,
    Q = 0).  No oracle: |dx| / |first term alone| below the fp32 level.  Catches a wrong sign or a wrong M in q0."""
    case = make_case(SHAPES[name], dtype, "const")
    got = run_stem(case, "backward_input")
    B, S, Cin, C0 = case["shape"]
    ratio = float(got["dx"].double().cpu().norm() / case["first"].norm())
    level = fp32_level(C0, Cin)
    print(f"constant dout {name} {dtype}: |dx| / |first term| = {ratio:.3e} (fp32 level {level:.3e})")
    assert ratio < level


@pytest.mark.parametrize("name", ["metric", "odd", "wide8"])
def test_zhat_dout_is_annihilated_up_to_eps(name):
    """dout = zhat (fp32): BatchNorm's backward removes the projection on zhat; the eps inside the variance leaves exactly
    scale_c zhat_c eps invstd_c^2 per channel, i.e. at most eps * max invstd^2 of the first term.  Bound: 10 x that + the fp32
    level.  Catches a wrong sign or a wrong M in Q."""
    case = make_case(SHAPES[name], torch.float32, "zhat")
    got = run_stem(case, "backward_input")
    B, S, Cin, C0 = case["shape"]
    ratio = float(got["dx"].double().cpu().norm() / case["first"].norm())
    bound = 10 * EPS * float(case["invstd"].max()) ** 2 + fp32_level(C0, Cin)
    print(f"zhat dout {name}: |dx| / |first term| = {ratio:.3e} (bound {bound:.3e}; float64 autograd {rel(case['first'] - case['dx'], case['first']):.3e})")
    assert ratio < bound


# ------------------------------------------------------------------------------------ 3. parameter gradients of the same call
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name", list(SHAPES))
def test_parameter_gradients_of_the_same_call(name, dtype):
    """dgamma, dbeta, dW of dwn_stem_backward_input against float64 autograd at the bounds tests/test_gpu_stem.py holds
    dwn_stem_backward to (1e-3 fp32, 8e-2 bf16), and against dwn_stem_backward on the same inputs to 1e-6 relative (the product
    build adds its fp64 replica sums in arrival order; bit for bit under the deterministic build: test 7)."""
    case = make_case(SHAPES[name], dtype, "mixed")
    new, old = run_stem(case, "backward_input"), run_stem(case, "backward")
    gt = 1e-3 if dtype == torch.float32 else 8e-2
    for key in ("dgamma", "dbeta", "dw"):
        e_ref, e_old = rel(new[key], case[key]), rel(new[key], old[key])
        print(f"stem {name} {dtype} {key}: against autograd {e_ref:.3e}, against dwn_stem_backward {e_old:.3e}")
        assert e_ref < gt, key
        assert e_old < 1e-6, key


# ----------------------------------------------------------------------------------------------- 4. whole model, training mode
def _train_case(which, dtype):
    """Poisson loss of a training-mode forward (DropPath / Dropout rates 0), float64 oracle: x.grad and every parameter gradient"""
    if which == "tiny":
        model, sd = tiny_model(dtype)
        xn, tn, wn = synth_inputs(np.random.default_rng(2), 3, 6, 9, 11, TINY["readout_outputs"])
        kw = dict(strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"])
    else:
        model, sd = full_model(dtype)
        xn, tn, wn = synth_inputs(np.random.default_rng(2), 1, 16, 64, 64, (N_FULL,))
        kw = dict(strides=FULL_STRIDES, readout_outputs=(N_FULL,))
    x, targets, w = torch.from_numpy(xn) * INPUT_SCALE, [torch.from_numpy(t) for t in tn], torch.from_numpy(wn)
    ref_sd = sd64(sd, grads=True)
    x64 = x.double().requires_grad_(True)
    po = orc.forward(ref_sd, x64, training=True, **kw)
    orc.mice_poisson_loss(po, [t.double() for t in targets], w.double()).backward()
    grads = {k: v.grad for k, v in ref_sd.items() if getattr(v, "grad", None) is not None}
    return model, x, targets, w, x64.grad, grads, po


def _param_grad_errors(model, grads, dtype):
    gnorm = math.sqrt(sum(float(g.norm()) ** 2 for g in grads.values()))
    named = dict(model.named_parameters())
    assert set(grads) == set(named)
    worst = ("", 0.0)
    for k, g in grads.items():
        assert named[k].grad is not None, k
        floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm        # tests/test_gpu_model.py: analytically-zero gradients
        err = float((named[k].grad.double().cpu() - g).norm()) / (float(g.norm()) + floor)
        if err > worst[1]:
            worst = (k, err)
    return worst


# bf16 x.grad of the whole model in training mode against the oracle: measured on an MI355X / bound = 2 x measured, rounded up
# (the frozen twins: 1.36e-2 tiny, 1.20e-1 full)
BF16_TRAIN_DX = {"tiny": (2.28e-2, 5e-2), "full": (7.25e-2, 2e-1)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_model_train_mode_input_gradient(which, dtype):
    """model.train(); x.requires_grad_(); loss(model(x), target).backward(): x.grad against the oracle, and in the same run every
    parameter gradient at the bounds of tests/test_gpu_model.py::test_tiny_model_train_step_matches_reference (asking for dx
    costs the other gradients nothing).  Full width: B=1, T=16, 64x64, one 7863-neuron readout."""
    from sensorium_amd import MicePoissonLoss
    model, x, targets, w, g_ref, grads, po = _train_case(which, dtype)
    model.train()
    xd = x.to(dev()).requires_grad_()
    preds = model(xd)
    MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape and xd.grad.dtype == torch.float32
    assert float(g_ref.abs().max()) > 0
    e = rel(xd.grad, g_ref)
    worst = _param_grad_errors(model, grads, dtype)
    e_pred = max(rel(p, q) for p, q in zip(preds, po))
    print(f"train-mode input gradient {which} {dtype}: x.grad rel err {e:.3e}; predictions {e_pred:.3e}; worst parameter gradient "
          f"{worst[0]} {worst[1]:.3e}")
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)
    assert e_pred < ft
    assert worst[1] < gt, worst
    if dtype == torch.float32:
        assert e < 1e-3
    else:
        measured, bound = BF16_TRAIN_DX[which]
        assert bound is not None, f"bf16 bound not set yet; measured now {e:.3e}"
        assert e < bound, f"measured on MI355X {measured}, bound {bound}, now {e:.3e}"


# ----------------------------------------------------------------------------------------- 5. directional finite difference
# |fd - <grad, d>| / |<grad, d>| in fp32, training mode; measured on an MI355X / bound = 2 x measured, rounded up to one digit.
# The step is chosen as in tests/test_gpu_frozen_bn.py: the last one at which the error still falls with h^2 and the fp32 rounding
# of f has not taken over.  The test prints the whole scan and asserts at TRAIN_FD_STEP.  Measured (two runs where they differ):
#   h      1e-1    3e-2    1e-2    3e-3    1e-3               3e-4    1e-4
#   tiny   6.1e-1  1.9e-1  2.3e-2  1.9e-3  2.75e-4 / 2.10e-4  2.2e-5  1.4e-4
#   full   1.6e-1  1.35    7.5e-1  1.4e-1  1.75e-2 / 1.25e-2  3.7e-3  1.2e-2
# Batch statistics over one or two clips make f far more curved than the frozen twin's (there h = 1e-2 sufficed; here the full-width
# model is not even in the quadratic regime above 3e-3).  At 3e-4 the error is smaller still, but there the product build's
# run-to-run noise of f (float atomics in arrival order: it moved fd by 7e-5 (tiny) / 5e-3 (full) of its value at h = 1e-3, and
# grows with 1 / h) is as large as what is measured, so 1e-3 is the step; the bounds take the larger of the two runs.
TRAIN_FD_SCAN = (1e-1, 3e-2, 1e-2, 3e-3, 1e-3, 3e-4, 1e-4)
TRAIN_FD_STEP = 1e-3
TRAIN_FD = {"tiny": (2.75e-4, 6e-4), "full": (1.75e-2, 4e-2)}


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_model_train_mode_input_gradient_finite_difference(which):
    """Oracle-independent: (f(x + h d) - f(x - h d)) / 2h against <x.grad, d>, f = the selected neurons' responses summed in
    float64, training mode (DropPath / Dropout rates 0).  Every forward updates the running statistics; a training-mode output
    does not depend on them (it normalises with the batch's own statistics), so f is the same function at every evaluation."""
    if which == "tiny":
        model, _ = tiny_model()
        x, index, neurons = _model_input(2, 6, 9, 11), 1, torch.tensor([0, 3, 4, 9])
    else:
        model, _ = full_model()
        x, index = _model_input(1, 16, 64, 64), 0
        neurons = torch.from_numpy(np.random.default_rng(1).choice(N_FULL, 32, replace=False))
    model.train()
    x, neurons = x.to(dev()), neurons.to(dev())

    def f(xx, want_grad=False):
        xx = xx.clone().requires_grad_()
        out = model(xx, index=index)[:, neurons].double().sum()
        if want_grad:
            out.backward()
            return xx.grad
        return float(out)
    grad = f(x, True)
    d = torch.randn(x.shape, generator=torch.Generator().manual_seed(11)).to(dev())
    an = float((grad.double() * d.double()).sum())
    errs = {}
    for h in TRAIN_FD_SCAN:
        fd = (f(x + h * d) - f(x - h * d)) / (2 * h)
        errs[h] = abs(fd - an) / abs(an)
        print(f"train-mode finite difference {which} h {h}: fd {fd:.6e} analytic {an:.6e} rel {errs[h]:.3e}")
    measured, bound = TRAIN_FD[which]
    assert bound is not None and TRAIN_FD_STEP is not None, f"finite-difference step / bound not set yet; measured now {errs}"
    e = errs[TRAIN_FD_STEP]
    assert e < bound, f"measured on MI355X {measured}, bound {bound}, now {e:.3e}"


# ------------------------------------------------------------------------------------------------ 6. a trainable front end
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_trainable_front_end(dtype):
    """A per-channel gain and offset (plain torch) in front of the tiny model in training mode: their gradients against the
    oracle with the same front end in float64.  Each is a contraction of the input gradient, g = sum_i dx_i a_i (a = x for the
    gain, 1 for the offset), so it can be as wrong as dx is, term by term: |g - g_ref| <= tol * sum_i |dx_i a_i|, with the sum taken
    from the oracle and tol the bound x.grad itself is held to on this model (fp32 1e-3; bf16 the tiny bound of BF16_TRAIN_DX).
    A bound relative to |g_ref| alone cannot be used: the offset's gradient is analytically zero (batch statistics remove a
    per-channel shift of the input; 1.9e-14 in the oracle), a cancelling sum of terms that are not small."""
    from sensorium_amd import MicePoissonLoss
    model, sd = tiny_model(dtype)
    xn, tn, wn = synth_inputs(np.random.default_rng(5), 3, 6, 9, 11, TINY["readout_outputs"])
    x, targets, w = torch.from_numpy(xn) * INPUT_SCALE, [torch.from_numpy(t) for t in tn], torch.from_numpy(wn)
    gain0 = torch.tensor([1.0, 0.8, 1.2, 0.9, 1.1])
    offset0 = torch.tensor([0.1, -0.2, 0.0, 0.3, -0.1])
    g64, o64 = gain0.double().requires_grad_(True), offset0.double().requires_grad_(True)
    xin64 = x.double() * g64.view(1, 5, 1, 1, 1) + o64.view(1, 5, 1, 1, 1)
    xin64.retain_grad()
    po = orc.forward(sd64(sd), xin64, training=True, strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"])
    orc.mice_poisson_loss(po, [t.double() for t in targets], w.double()).backward()

    model.train()
    gain, offset = gain0.to(dev()).requires_grad_(True), offset0.to(dev()).requires_grad_(True)
    xd = x.to(dev())
    preds = model(xd * gain.view(1, 5, 1, 1, 1) + offset.view(1, 5, 1, 1, 1))
    MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev()))).backward()
    torch.cuda.synchronize()
    tol = 1e-3 if dtype == torch.float32 else BF16_TRAIN_DX["tiny"][1]
    assert float(g64.grad.norm()) > 0
    l1 = {"gain": (xin64.grad * x.double()).abs().sum(dim=(0, 2, 3, 4)), "offset": xin64.grad.abs().sum(dim=(0, 2, 3, 4))}
    for name, mine, ref in (("gain", gain.grad, g64.grad), ("offset", offset.grad, o64.grad)):
        assert mine is not None, name
        err = float(((mine.double().cpu() - ref).abs() / l1[name]).max())
        print(f"front end {dtype} {name}: |ref| {float(ref.norm()):.3e} worst |g - g_ref| / sum|terms| {err:.3e} (bound {tol:.0e})")
        assert err < tol, name


def test_input_gradient_accumulates_over_two_backward_calls():
    """iter_size-style accumulation, fp32: a second forward / backward of the same batch adds into x.grad and into the front end's
    gradients (2 x the first within the fp32 bound: the product build's run-to-run noise is ~6e-6 in fp32)."""
    from sensorium_amd import MicePoissonLoss
    model, _ = tiny_model()
    xn, tn, wn = synth_inputs(np.random.default_rng(5), 3, 6, 9, 11, TINY["readout_outputs"])
    x = (torch.from_numpy(xn) * INPUT_SCALE).to(dev()).requires_grad_()
    targets, w = [torch.from_numpy(t).to(dev()) for t in tn], torch.from_numpy(wn).to(dev())
    gain = torch.ones(5, device=dev(), requires_grad=True)
    model.train()
    first = None
    for _ in range(2):
        MicePoissonLoss()(model(x * gain.view(1, 5, 1, 1, 1)), (targets, w)).backward()
        if first is None:
            first = (x.grad.clone(), gain.grad.clone())
    torch.cuda.synchronize()
    assert float(first[0].norm()) > 0
    e_x, e_g = rel(x.grad, 2 * first[0]), rel(gain.grad, 2 * first[1])
    print(f"accumulation: x.grad against 2 x first {e_x:.3e}, gain.grad {e_g:.3e}")
    assert e_x < 1e-3 and e_g < 1e-3


def test_frozen_stem_parameters_still_give_the_input_gradient():
    """The stem's parameters frozen by the caller (requires_grad False): x.grad is the same, their .grad stays None."""
    model, _ = tiny_model()
    model.train()
    x = _model_input(2, 6, 9, 11).to(dev())
    xa = x.clone().requires_grad_()
    model(xa, index=1).sum().backward()
    stem = [model.core.stem[0].weight, model.core.stem[1].bn.weight, model.core.stem[1].bn.bias]
    for p in stem:
        p.requires_grad_(False)
        p.grad = None
    xb = x.clone().requires_grad_()
    model(xb, index=1).sum().backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in stem)
    e = rel(xb.grad, xa.grad)
    print(f"frozen stem parameters: x.grad against the unfrozen run {e:.3e}")
    assert e < 1e-3


# ------------------------------------------------------------------------------------- 7. bit for bit, deterministic build
@pytest.mark.parametrize("kind", ["tiny", "tiny_f32", "metric", "metric_f32"])
def test_deterministic_build_input_gradient_bit_for_bit(kind):
    """tests/det_input_grad_worker.py in a fresh process on libdwiseneuro_hip_det.so, DropPath / Dropout on with fixed seeds:
    (a) two runs of the same step give identical x.grad; (b) the step with and without x.requires_grad give identical predictions,
    loss, parameter gradients and BatchNorm buffers; (c) at stem level dwn_stem_backward_input's dgamma, dbeta, dW are identical
    to dwn_stem_backward's."""
    env = dict(os.environ, DWN_DETERMINISTIC="1")
    env.pop("DWN_LIB_PATH", None)
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "det_input_grad_worker.py"), kind], cwd=str(ROOT), env=env,
                         capture_output=True, text=True, timeout=900)
    m = re.search(r"DET_INPUT_GRAD deterministic=(\d) lib=(\S+) tensors=(\d+) dx_nonzero=(\d) dx_identical=(\d) "
                  r"same_without_dx=(\d) differing=(\S*) stem_identical=(\d)", res.stdout)
    assert res.returncode == 0 and m, res.stdout[-2000:] + res.stderr[-3000:]
    print(m.group(0))
    assert m.group(1) == "1" and m.group(2) == "libdwiseneuro_hip_det.so"
    assert int(m.group(3)) > 50
    assert m.group(4) == "1", "x.grad is zero"
    assert m.group(5) == "1", "two runs of the same step give different x.grad"
    assert m.group(6) == "1", f"asking for x.grad changed: {m.group(7)}"
    assert m.group(8) == "1", "dwn_stem_backward_input and dwn_stem_backward disagree on dgamma / dbeta / dW"

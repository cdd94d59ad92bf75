"""Backward through frozen BatchNorm (include/dwn.h DWN_BN_FROZEN): eval-mode statistics, training-path kernels, a backward.

Ground truth is the float64 CPU oracle, which autograd differentiates with ``training=False``.  Running statistics are always
randomised (a wrong invstd or a missed statistic passes with mean 0 / var 1).  Bounds: the block tests use the bounds of their
training twin in tests/test_gpu_block.py (same kernels, a simpler BatchNorm term); the whole-model bf16 and finite-difference
bounds had no precedent and are 2 x the value measured on an MI355X, rounded up to one digit — both figures stand beside each
assert.  Every test prints what it measured before it asserts.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests.gpu_helpers import dev, rel, synth_inputs  # noqa: E402
from tests.test_gpu_block import CASES, make_block, y1_free_case  # noqa: E402

TINY = dict(readout_outputs=(7, 10), in_channels=5, core_features=(8, 8, 16), spatial_strides=(2, 1, 2),
            spatial_kernel=3, temporal_kernel=5, expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64),
            groups=2, softplus_beta=0.07, drop_rate=0.0, drop_path_rate=0.0)
TINY_SD = dict(readout_outputs=(7, 10), core_features=(8, 8, 16), expansion_ratio=3, se_reduce_ratio=4, cortex_features=(32, 64))
FULL_STRIDES = (2, 1, 1, 1, 2, 1, 1, 2, 1)
N_FULL = 7863


def tiny_model(dtype=torch.float32, seed=3):
    from sensorium_amd import DwiseNeuro
    sd = orc.make_state_dict(seed=seed, randomize_bn=True, **TINY_SD)
    model = DwiseNeuro(compute_dtype=dtype, **TINY)
    model.load_state_dict(sd, strict=True)
    return model.to(dev()), sd


def full_model(dtype=torch.float32, seed=5):
    from sensorium_amd import DwiseNeuro
    sd = orc.make_state_dict(readout_outputs=(N_FULL,), seed=seed, randomize_bn=True)      # full width, expansion 6
    model = DwiseNeuro(readout_outputs=(N_FULL,), expansion_ratio=6, drop_rate=0.0, drop_path_rate=0.0, compute_dtype=dtype)
    model.load_state_dict(sd, strict=True)
    return model.to(dev()), sd


def sd64(sd, grads=False):
    out = {}
    for k, v in sd.items():
        if v.is_floating_point():
            v = v.double()
            if grads and "running" not in k and "inv_freq" not in k:
                v = v.clone().requires_grad_(True)
        out[k] = v
    return out


def buffers_of(module):
    return {k: v.clone() for k, v in module.state_dict().items() if "running" in k or "num_batches" in k}


def assert_buffers_untouched(module, before):
    after = module.state_dict()
    assert before, "no BatchNorm buffers found"
    for k, v in before.items():
        assert torch.equal(after[k], v), f"{k} changed in frozen mode"


# ---------------------------------------------------------------------------------------------------------------- 1. block level
# the geometries of tests/test_gpu_block.py thinned to both strides x 64 / 128 / 256 input channels, plus block 4 of the
# benchmarked model (128 channels, stride 2: the one combination that file has no case for)
BLOCK_CASES = [CASES[3], CASES[4], CASES[11], CASES[12], (128, 128, 2, 7, 32, 1, 4, 18, 32), CASES[15], CASES[16]]


def _block_params():
    out = []
    for case in BLOCK_CASES:
        for dtype in (torch.float32, torch.bfloat16):
            for y1 in ("auto", "all", "materialise"):
                if y1 == "materialise" and not y1_free_case(case, dtype, "all"):
                    continue
                if y1 == "all" and y1_free_case(case, dtype, "all") == y1_free_case(case, dtype, "auto"):
                    continue
                out.append(pytest.param(case, dtype, y1, id=f"{'-'.join(map(str, case))}-{str(dtype)[6:]}-{y1}"))
    return out


@pytest.mark.parametrize("case,dtype,y1", _block_params())
def test_block_frozen_forward_backward(case, dtype, y1):
    """out, dx and every parameter gradient of one block in frozen mode against the oracle's eval-mode autograd; BatchNorm
    buffers bit-identical afterwards.  Measured maxima over all cases (MI355X): see DESIGN.md section 12."""
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=cin + stride)
    sd = {"blk." + k: v.clone() for k, v in blk.state_dict().items()}
    torch.manual_seed(1)
    x = torch.randn(B, T, H, W, cin) * 1.5 + 0.3

    ref_sd = sd64(sd, grads=True)
    x64 = x.double().requires_grad_(True)
    a0 = x64 + orc.pe_table(cin, T, H, W, pe.inv_freq, torch.float64)
    ref = orc.inverted_residual(a0, "blk", ref_sd, stride, False, None, None)
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(7)).double()
    (ref * gout).sum().backward()

    blk = blk.to(dev()).eval()
    pe = pe.to(dev())
    blk._capture = True
    blk._dwn_y1_mode = {"auto": 0, "materialise": 1, "all": 2}[y1]
    before = buffers_of(blk)
    xd = x.to(dev()).to(dtype).requires_grad_(True)
    out = blk(xd, pe, dtype)               # eval mode + an input that requires grad: frozen statistics
    out.backward(gout.to(dev()).to(dtype))
    torch.cuda.synchronize()

    # fp32: the training twin's 1e-3.  bf16: the twin's 4e-2 / 8e-2 hold with a wide margin (measured maxima over these cases on an
    # MI355X: output 5.1e-3, input gradient 8.7e-3, parameter gradients 1.45e-2), so they are tightened to 2 x measured, rounded up
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (2e-2, 3e-2)
    assert (blk._captured["y1"] is None) == y1_free_case(case, dtype, y1), "y1 materialisation is not what the case expects"
    assert_buffers_untouched(blk, before)
    e_out = rel(out.float(), ref)
    named = dict(blk.named_parameters())
    gnorm = math.sqrt(sum(float(v.grad.norm()) ** 2 for v in ref_sd.values() if getattr(v, "grad", None) is not None))
    errs = {}
    for key, p in named.items():
        g_ref = ref_sd["blk." + key].grad
        assert p.grad is not None, key
        errs[key] = float((p.grad.double().cpu() - g_ref).norm()) / (float(g_ref.norm()) + 1e-4 * gnorm)
    e_dx = rel(xd.grad.float(), x64.grad)
    worst = max(errs, key=errs.get)
    print(f"frozen block {case} {dtype} {y1}: out {e_out:.3e} dx {e_dx:.3e} worst grad {worst} {errs[worst]:.3e}")
    assert e_out < ft, f"block output rel err {e_out:.3e}"
    assert len(errs) == 18
    for key, e in errs.items():
        assert e < gt, f"grad {key}: rel err {e:.3e}"
    assert e_dx < gt, f"input grad rel err {e_dx:.3e}"


# ------------------------------------------------------------------------------------------------- 3. stem input gradient, C-ABI
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 16 * 64 * 64, 5, 64), (3, 7 * 9 * 11, 5, 64), (1, 61, 5, 8), (2, 1000, 8, 128), (2, 333, 3, 24)],
                         ids=["metric", "odd", "tiny", "wide8", "ragged"])
def test_stem_input_grad_c_abi(shape, dtype):
    """dwn_stem_input_grad against float64 W0^T diag(scale) dout: the metric plane size (B=2, T=16, 64x64), a row count that is no
    multiple of the 64-row tile, and stem widths that leave channel lanes idle / need two loads per lane."""
    from sensorium_amd import _lib as L
    B, S, Cin, C0 = shape
    if dtype == torch.float32:
        C0 = min(C0, 64)                      # fp32 rows: at most 64 channels are built (dwn.h); 64 already takes two loads per lane
    g = torch.Generator().manual_seed(B + S)
    w = torch.randn(C0, Cin, generator=g) * 0.3
    coef = torch.cat([torch.rand(C0, generator=g) + 0.5, torch.randn(3 * C0, generator=g)])
    dout = torch.randn(B * S, C0, generator=g).to(dtype)
    ref = torch.einsum("ck,c,bsc->bks", w.double(), coef[:C0].double(), dout.double().view(B, S, C0))
    wd, cd, dd = w.to(dev()), coef.to(dev()), dout.to(dev())
    dx = torch.full((B, Cin, S), float("nan"), device=dev())
    a = L.StemInputGradArgs()
    a.dtype = L.DWN_F32 if dtype == torch.float32 else L.DWN_BF16
    a.training = L.BN_FROZEN; a.B = B; a.Cin = Cin; a.C0 = C0; a.S = S
    a.w = wd.data_ptr(); a.coef = cd.data_ptr(); a.dout = dd.data_ptr(); a.dx = dx.data_ptr()
    L.check(L.lib.dwn_stem_input_grad(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_stem_input_grad")
    torch.cuda.synchronize()
    e = rel(dx, ref)
    print(f"stem input grad {shape} {dtype}: rel err {e:.3e}")
    # dout is exact in both dtypes (the reference sees the same rounded values): what is left is fp32 accumulation
    assert e < (1e-3 if dtype == torch.float32 else 8e-2)
    for mode in (L.BN_EVAL, L.BN_TRAIN):          # not built: an error, not a wrong answer
        a.training = mode
        assert L.lib.dwn_stem_input_grad(C.byref(a), 0, torch.cuda.current_stream().cuda_stream) == -7


# ---------------------------------------------------------------------------------------------------- 4. the user's three lines
# Inputs of the whole-model tests: the synthetic clips of the other model tests (grey levels 0..255, behaviour traces up to ~100)
# times INPUT_SCALE.  A trained model's running statistics match its data; the randomised ones here (mean ~ N(0, 0.2), variance
# in 0.5..1.5) match inputs of order one.  Fed raw grey levels, such a net sits where no trained one does: stem outputs of order
# 1e2 normalised by a variance near 1, pre-activations in the thousands, predictions that underflow the Poisson loss's eps — and
# what is then compared is how rounding is amplified, not the kernels (measured with raw inputs on an MI355X: fp32 input gradient
# of the full-width model 9.0e-4, bf16 0.84; tiny-model fp32 Poisson-loss gradients 6e-2 through predictions below 1e-8, while the
# same run with inputs / 100 gives 2e-6).
INPUT_SCALE = 0.01


def _model_input(b, t, h, w, seed=0):
    x, _, _ = synth_inputs(np.random.default_rng(seed), b, t, h, w, (1,))
    return torch.from_numpy(x) * INPUT_SCALE


def _input_grad_case(which, dtype):
    if which == "tiny":
        model, sd = tiny_model(dtype)
        x = _model_input(2, 6, 9, 11)
        kw = dict(strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"])
        index, neurons = 1, torch.tensor([0, 3, 4, 9])
    else:
        model, sd = full_model(dtype)
        x = _model_input(1, 16, 64, 64)
        kw = dict(strides=FULL_STRIDES, readout_outputs=(N_FULL,))
        index, neurons = 0, torch.from_numpy(np.random.default_rng(1).choice(N_FULL, 32, replace=False))
    x64 = x.double().requires_grad_(True)
    orc.forward(sd64(sd), x64, index=index, training=False, **kw)[:, neurons].sum().backward()
    return model, x, x64.grad, index, neurons


# bf16 input gradient of the whole model against the oracle: measured / bound = 2 x measured, rounded up to one digit
BF16_DX = {"tiny": (1.36e-2, 3e-2), "full": (1.20e-1, 3e-1)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("which", ["tiny", "full"])
def test_model_input_gradient(which, dtype):
    """model.eval(); x.requires_grad_(); model(x, index=k)[:, neurons].sum().backward() -> x.grad against the oracle.
    Full width: B=1, T=16, 64x64, 7863 neurons, 32 of them as the objective."""
    model, x, g_ref, index, neurons = _input_grad_case(which, dtype)
    model.eval()
    before = buffers_of(model)
    xd = x.to(dev()).requires_grad_()
    model(xd, index=index)[:, neurons.to(dev())].sum().backward()
    torch.cuda.synchronize()
    assert xd.grad is not None and xd.grad.shape == x.shape and xd.grad.dtype == torch.float32
    assert float(g_ref.abs().max()) > 0
    e = rel(xd.grad, g_ref)
    print(f"model input gradient {which} {dtype}: rel err {e:.3e} (|dx| mean {float(g_ref.abs().mean()):.3e} max {float(g_ref.abs().max()):.3e})")
    assert_buffers_untouched(model, before)          # 2. statistics untouched: stem, blocks, cortex
    if dtype == torch.float32:
        assert e < 1e-3
    else:
        measured, bound = BF16_DX[which]
        assert bound is not None, f"bf16 bound not set yet; measured now {e:.3e}"
        assert e < bound, f"measured on MI355X {measured}, bound {bound}, now {e:.3e}"


# directional finite difference, fp32: |fd - <grad, d>| / |<grad, d>|; measured / bound = 2 x measured, rounded up to one digit.
# Step h = 0.01 (inputs of order one): on the full-width model the truncation error falls with h^2 (1.8e-1, 3.2e-2, 3.7e-3 at
# h = 0.1, 0.03, 0.01) until the fp32 rounding of f takes over (3.3e-3 at 0.003, 6e-2 at 0.001: f is ~5e3, 2 h <grad, d> ~ 2)
FD_STEP = 1e-2
FD = {"tiny": (8.07e-4, 2e-3), "full": (3.68e-3, 8e-3)}


@pytest.mark.parametrize("which", ["tiny", "full"])
def test_model_input_gradient_finite_difference(which):
    """Oracle-independent: (f(x + h d) - f(x - h d)) / 2h against <x.grad, d> in fp32, f summed in float64, d a random direction
    with unit RMS over all five channels."""
    from sensorium_amd import attribution
    if which == "tiny":
        model, _ = tiny_model()
        x, index, neurons = _model_input(2, 6, 9, 11), 1, torch.tensor([0, 3, 4, 9])
    else:
        model, _ = full_model()
        x, index = _model_input(1, 16, 64, 64), 0
        neurons = torch.from_numpy(np.random.default_rng(1).choice(N_FULL, 32, replace=False))
    model.eval()
    x, neurons = x.to(dev()), neurons.to(dev())
    grad = attribution.input_gradient(model, x, index, neurons)
    d = torch.randn(x.shape, generator=torch.Generator().manual_seed(11)).to(dev())
    def f(xx):      # the same (frozen-statistics) forward the gradient belongs to
        with torch.enable_grad():
            return float(model(xx.clone().requires_grad_(), index=index)[:, neurons].double().sum())
    an = float((grad.double() * d.double()).sum())
    h = FD_STEP
    fd = (f(x + h * d) - f(x - h * d)) / (2 * h)
    e = abs(fd - an) / abs(an)
    print(f"finite difference {which} h {h}: fd {fd:.6e} analytic {an:.6e} rel {e:.3e}")
    measured, bound = FD[which]
    assert bound is not None, f"finite-difference bound not set yet; measured now {e:.3e}"
    assert e < bound, f"measured on MI355X {measured}, bound {bound}, now {e:.3e}"


# ----------------------------------------------------------------------------------------------------------- 5. frozen fine-tune
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_frozen_finetune_parameter_gradients(dtype):
    """freeze_batchnorm(), eval mode, an input that needs no gradient: every parameter gradient of the tiny model's Poisson loss
    against the oracle's eval-mode autograd.  Bounds as tests/test_gpu_model.py::test_tiny_model_train_step_matches_reference."""
    from sensorium_amd import MicePoissonLoss
    model, sd = tiny_model(dtype)
    xn, tn, wn = synth_inputs(np.random.default_rng(2), 3, 6, 9, 11, TINY["readout_outputs"])
    x, targets, w = torch.from_numpy(xn) * INPUT_SCALE, [torch.from_numpy(t) for t in tn], torch.from_numpy(wn)
    ref_sd = sd64(sd, grads=True)
    po = orc.forward(ref_sd, x.double(), strides=TINY["spatial_strides"], readout_outputs=TINY["readout_outputs"], training=False)
    lo = orc.mice_poisson_loss(po, [t.double() for t in targets], w.double())
    lo.backward()

    model.eval().freeze_batchnorm()
    before = buffers_of(model)
    preds = model(x.to(dev()))
    loss = MicePoissonLoss()(preds, ([t.to(dev()) for t in targets], w.to(dev())))
    loss.backward()
    torch.cuda.synchronize()
    assert_buffers_untouched(model, before)
    ft, gt = (1e-3, 1e-3) if dtype == torch.float32 else (3e-2, 1e-1)
    for m in range(2):
        assert rel(preds[m], po[m]) < ft
    grads = {k: v.grad for k, v in ref_sd.items() if getattr(v, "grad", None) is not None}
    gnorm = math.sqrt(sum(float(g.norm()) ** 2 for g in grads.values()))
    named = dict(model.named_parameters())
    assert set(grads) == set(named)
    worst = ("", 0.0)
    for k, g in grads.items():
        assert named[k].grad is not None, k
        floor = (1e-4 if dtype == torch.float32 else 1e-2) * gnorm
        err = float((named[k].grad.double().cpu() - g).norm()) / (float(g.norm()) + floor)
        if err > worst[1]:
            worst = (k, err)
    print(f"frozen fine-tune {dtype}: worst parameter gradient {worst[0]} {worst[1]:.3e}")
    assert worst[1] < gt, worst
    # a gradient that is analytically zero under batch statistics is not zero here: the stem's BN bias reaches the output
    assert float(grads["core.stem.1.bn.bias"].abs().max()) > 0


# --------------------------------------------------------------------------------------------------------- 6. nothing else moved
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eval_path_untouched_and_mode_selection(dtype):
    model, _ = tiny_model(dtype)
    model.eval()
    x = _model_input(2, 6, 9, 11).to(dev())
    with torch.no_grad():
        ref = model(x)
    xg = x.clone().requires_grad_()
    frozen = model(xg)
    sum(p.sum() for p in frozen).backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        again = model(x)
    assert all(torch.equal(a, b) for a, b in zip(again, ref)), "the eval forward changed after a frozen forward / backward"
    # the frozen forward follows the training kernels: equal to the eval forward within the forward bound, not bit for bit
    for a, b in zip(frozen, ref):
        assert rel(a, b) < (1e-3 if dtype == torch.float32 else 3e-2)
    # switch off, plain data, grad enabled: still the eval kernels (bit-identical to the no_grad forward) and no backward
    for p in model.parameters():
        p.grad = None
    plain = model(x)
    assert all(torch.equal(a, b) for a, b in zip(plain, ref))
    with pytest.raises(RuntimeError, match="backward through eval-mode BatchNorm is not built"):
        sum(p.sum() for p in plain).backward()
    # switch on: a backward exists; switch off again: back to the eval kernels
    model.freeze_batchnorm()
    sum(p.sum() for p in model(x)).backward()
    assert model.core.stem[0].weight.grad is not None
    model.freeze_batchnorm(False)
    assert all(torch.equal(a, b) for a, b in zip(model(x), ref))


def test_c_abi_eval_mode_backward_still_refused():
    """mode 0 keeps its -7 in dwn_block_backward / dwn_cortex_backward (device present this time)."""
    from sensorium_amd import _lib as L
    a = L.BlockArgs(); a.dtype = L.DWN_BF16; a.B = 2; a.T = 4; a.Hin = 8; a.Win = 16; a.Hout = 8; a.Wout = 16
    a.Cin = 64; a.Cmid = 448; a.Cout = 64; a.stride = 1; a.ks = 3; a.kt = 5; a.se_r = 14; a.training = L.BN_EVAL
    assert L.lib.dwn_block_backward(C.byref(a), 0, None) == -7
    c = L.CortexArgs(); c.dtype = L.DWN_BF16; c.training = L.BN_EVAL; c.B = 2; c.T = 4; c.Cin = 64; c.C = 128; c.groups = 2
    assert L.lib.dwn_cortex_backward(C.byref(c), 0, None) == -7


# ------------------------------------------------------------------------------------------------------------------------- 7. MEI
def test_most_exciting_input_raises_the_response():
    from sensorium_amd import attribution
    model, _ = tiny_model()
    init = _model_input(1, 6, 9, 11, seed=4)
    init[:, 0] = init[:, 0] * 0.25 + 96          # a start well inside the range
    video, trace = attribution.most_exciting_input(model, 1, [0, 3, 4, 9], steps=20, lr=2.0, init=init.to(dev()),
                                                   video_range=(0, 255))
    torch.cuda.synchronize()
    trace = trace.cpu()
    print("MEI response trace:", " ".join(f"{float(v):.4f}" for v in trace))
    assert trace.shape == (21,)
    assert float(trace[-1]) > float(trace[0])        # the only assert on the response: final > initial
    assert model.training                            # (tiny_model() comes in training mode: restored after the ascent)
    assert video.shape == init.shape
    assert float(video[:, 0].min()) >= 0.0 and float(video[:, 0].max()) <= 255.0
    assert torch.equal(video[:, 1:].cpu(), init[:, 1:])
    assert not torch.equal(video[:, 0].cpu(), init[:, 0])
    # a norm budget holds too
    video2, _ = attribution.most_exciting_input(model, 1, [0, 3], shape=(6, 9, 11), steps=5, lr=4.0, norm_budget=50.0,
                                                behavior=(30.0, 5.0), pupil_center=(100.0, 70.0))
    assert float((video2[:, 0] - 127.5).norm()) <= 50.0 * (1 + 1e-5)
    assert float(video2[0, 1].min()) == 30.0 == float(video2[0, 1].max()) and float(video2[0, 4].max()) == 70.0

"""CPU checks that the inputs of tests/test_gpu_tail.py have teeth, and that its float64 references meet its fp32 bounds by
themselves: a wrong formula must show on those inputs, and a right one must have room."""
import numpy as np
import torch

from oracle import dwiseneuro_oracle as orc
from tests import gpu_helpers as H
from tests.gpu_helpers import rel


def test_int64_ema_pairs_tell_contracted_from_separately_rounded():
    """num_batches_tracked under ModelEma.update: decay * e + (1 - decay) * m on float32, truncated.  On the pairs the GPU test
    runs, a fused multiply-add (one product unrounded) lands on another integer in hundreds of cases; oracle.ema_update is the
    separately rounded form on every one of them."""
    e, m = H.ema_int_pairs()
    differ = 0
    for decay in H.EMA_DECAYS:
        sep, con = H.ema_int_separate(e, m, decay), H.ema_int_contracted(e, m, decay)
        assert torch.equal(orc.ema_update(e, m, decay), sep)
        differ += int((sep != con).sum())
    assert differ >= 100, differ
    i = int(torch.nonzero((e == 11) & (m == 11)).flatten()[0])           # the smallest example: 10 against 11
    assert int(H.ema_int_separate(e, m, 0.9999)[i]) == 10 and int(H.ema_int_contracted(e, m, 0.9999)[i]) == 11


def _softplus_f32(z, beta):
    """the forward as the readout epilogue forms it, in float32: log1p(exp(beta z)) / beta, identity above the threshold"""
    bz = (z * np.float32(beta)).astype(np.float32)
    with np.errstate(over="ignore"):
        soft = (np.log1p(np.exp(bz).astype(np.float32)).astype(np.float32) / np.float32(beta)).astype(np.float32)
    return np.where(bz > 20, z, soft).astype(np.float32)


def test_low_rate_readout_inputs_expose_the_cancelling_derivative():
    """sigmoid(beta z) from the stored output: 1 - exp(-beta * out) in float32 misses the per-neuron bound of the GPU test on more
    than a quarter of the low-rate neurons, -expm1(-beta * out) meets it on all of them."""
    for beta in (1.0, 0.07):
        bias = H.low_rate_bias(beta)
        ref = H.low_rate_reference(bias, beta, 1, 1)                     # dbias = sigmoid(beta z) per neuron, dout = 1
        out = _softplus_f32(bias.numpy(), beta)
        arg = (-np.float32(beta) * out).astype(np.float32)
        naive = (np.float32(1) - np.exp(arg).astype(np.float32)).astype(np.float32)
        good = (-np.expm1(arg)).astype(np.float32)
        e_naive = np.abs(naive.astype(np.float64) - ref["dbias"].numpy()) / ref["sumabs"].numpy()
        e_good = np.abs(good.astype(np.float64) - ref["dbias"].numpy()) / ref["sumabs"].numpy()
        assert (e_naive > H.TAIL_F32_BOUND).sum() >= bias.numel() / 4, (beta, int((e_naive > H.TAIL_F32_BOUND).sum()))
        assert e_good.max() < H.TAIL_F32_BOUND and e_good.max() < 1e-5, (beta, e_good.max())


def test_float64_references_meet_the_fp32_bounds_when_rounded():
    """Every fp32 bound the GPU tests assert, applied to the float64 reference rounded to float32 (and, for the optimizer, to the
    same formulas carried in float32 for ten steps): the bounds leave room for a correct kernel."""
    d = H.cortex_inputs(1, torch.float32, 2, 65, 48, 96, 2, True, True, offset=100.0)
    for training in (True, False):
        for k, v in H.cortex_reference(d, 2, training).items():
            if v.is_floating_point():
                assert rel(v.float(), v) < H.TAIL_F32_BOUND, k
    d = H.readout_inputs(2, torch.float32, 3, 5, 16, 2, 7, 0.07, True)
    for k, v in H.readout_reference(d, 2, 7, 0.07).items():
        assert rel(v.float(), v) < H.TAIL_F32_BOUND, k
    for beta in (1.0, 0.07):
        r = H.low_rate_reference(H.low_rate_bias(beta), beta, 3, 5)
        assert bool(((r["dbias"].float().double() - r["dbias"]).abs() <= H.TAIL_F32_BOUND * r["sumabs"]).all())
    pred, target, w = H.poisson_inputs(3, 32, 1020, "onehot")
    loss, dpred = H.poisson_reference(pred, target, w)
    assert rel(loss.float(), loss) < H.TAIL_F32_BOUND and rel(dpred.float(), dpred) < H.TAIL_F32_BOUND
    x = torch.randn(33, 16, 24, dtype=torch.float64)
    out, dx = H.pool_reference(x, torch.randn(33, 24, dtype=torch.float64))
    assert rel(out.float(), out) < H.TAIL_F32_BOUND and rel(dx.float(), dx) < H.TAIL_F32_BOUND
    # AdamW + EMA: ten steps with the state in float32 against float64, at the first step and late in a run
    sizes = [1, 3, 255, 256, 257, 4097, 16 * 256 + 1, 1_000_003]
    worst = 0.0
    for step0 in (1, 2, 1000, 100_000):
        for wd in (0.0, 0.05):
            case = H.adamw_case(7 + step0, sizes, step0)
            r64 = H.adamw_reference(case, step0, 2.4e-3, wd, 0.999, 0.37)
            r32 = H.adamw_reference(case, step0, 2.4e-3, wd, 0.999, 0.37, torch.float32)
            worst = max(worst, max(rel(a[k], b[k]) for a, b in zip(r32, r64) for k in a))
    assert worst < 3.5e-7 < H.ADAMW_BOUND / 2, worst          # 3.4e-7 measured: the 1e-6 of the existing optimizer test stands

"""BatchNorm finalisation through the C ABI: dwn_bn_finalize (training and eval) and dwn_bn_bwd_finalize against the same formulas
in float64.

Shapes: C in {8, 12, 20, 448} (12 and 20 leave the last 8-channel workgroup partly filled), the shortcut form C = 16 over
stat_c = 8 sums (channel c reads the sums of c % stat_c), count in {1, 37} (count = 1 takes the `var`, not the unbiased, branch),
with and without running statistics / dgamma, dbeta.  Every output buffer carries eight sentinel floats behind its last channel
that must stay as they were.

Inputs: the 32 replicas of every sum are integer-valued doubles, so the replica sum is exact in any order.  Forward sums give
var >= 0.5 (or, in the clamp test, var < 0 in exact arithmetic: sum of squares below sum^2 / count).

Bound (derived, not measured): every float result is a chain of correctly rounded operations, except that the compiler may
contract a - b * c or a * b + c * d into a fused multiply-add.  Contracted or not, the error against the float64 value of the
expression (from the float operands), rounded once, is at most 2^-23 x (sum of the magnitudes of the expression's terms): each
of the at most two roundings is half a unit in the last place of something no larger than that sum.  mean, invstd, dgamma and
dbeta are single roundings of a float64 value and must equal it rounded to float; the eval invstd is three correctly rounded
float operations and must equal the same three in numpy.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_helpers import dev, stats_buffer, stream  # noqa: E402

EPS = np.float32(1e-5)
MOM = np.float32(0.1)
U = 2.0 ** -23
PAD, SENTINEL = 8, 12345.0
SHAPES = [(8, 8), (12, 12), (20, 20), (448, 448), (16, 8)]          # (C, stat_c)


def replica_sums(rng, total):
    """[32][n] integer-valued doubles whose column sums are `total` (int64 [n]); the single terms are up to 2^20 in magnitude"""
    r = rng.integers(-2 ** 20, 2 ** 20, size=(32, total.shape[0]), dtype=np.int64)
    r[31] = total - r[:31].sum(0)
    return r.astype(np.float64)


def upload_stats(first, second):
    """the two sums' replicas, [32][n] each, in the kernels' layout [32][2][n]"""
    n = first.shape[1]
    buf = stats_buffer(n)
    buf.copy_(torch.from_numpy(np.stack([first, second], axis=1).reshape(-1)))
    return buf


def padded(values):
    """float32 device buffer: `values` followed by PAD sentinels"""
    v = np.concatenate([np.asarray(values, dtype=np.float32).reshape(-1), np.full(PAD, SENTINEL, dtype=np.float32)])
    return torch.from_numpy(v).to(dev())


def body(t):
    """host copy without the sentinels, which must be untouched"""
    h = t.cpu().numpy()
    assert np.array_equal(h[-PAD:], np.full(PAD, SENTINEL, dtype=np.float32)), "wrote behind the last channel"
    return h[:-PAD]


def exact(got, want64, what):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    bad = int((got != want).sum())
    print(f"{what}: {bad} of {got.size} differ from the rounded float64 value")
    assert bad == 0, what


def within(got, want64, mag64, what):
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    bound = U * np.asarray(mag64, dtype=np.float64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: worst error {worst:.3f} of its bound (max abs error {float(err.max()):.3e})")
    assert (err <= bound).all(), what


def forward_sums(rng, stat_c, count, negative_var=False):
    """integer sums s, ss [stat_c] of `count` values with mean in about [-4, 4] and var in [0.5, 3]; negative_var: every other
    channel gets ss just below s^2 / count instead (var < 0 in exact arithmetic, by less than 2 / count)"""
    s = rng.integers(-4 * count, 4 * count + 1, size=stat_c, dtype=np.int64)
    var = rng.uniform(0.5, 3.0, size=stat_c)
    ss = np.ceil(s.astype(np.float64) ** 2 / count + count * var).astype(np.int64)
    if negative_var:
        s[::2] = np.where(np.abs(s[::2]) < 7, 7, s[::2])
        ss[::2] = -(-(s[::2] ** 2) // count) - 1                  # ceil(s^2 / count) - 1 < s^2 / count
        assert (ss[::2] * count < s[::2] ** 2).all()
    return s, ss


def run_train(C_, stat_c, count, running, negative_var=False, seed=0):
    import sensorium_amd._lib as L
    rng = np.random.default_rng(1000 * C_ + 10 * count + seed)
    s, ss = forward_sums(rng, stat_c, count, negative_var)
    stats = upload_stats(replica_sums(rng, s), replica_sums(rng, ss))
    gamma = (1 + 0.2 * rng.normal(size=C_)).astype(np.float32)
    beta = (0.3 * rng.normal(size=C_)).astype(np.float32)
    rm0 = (0.3 * rng.normal(size=C_)).astype(np.float32)
    rv0 = (0.5 + rng.uniform(size=C_)).astype(np.float32)
    d_gamma, d_beta = torch.from_numpy(gamma).to(dev()), torch.from_numpy(beta).to(dev())
    d_rm, d_rv, d_coef = padded(rm0), padded(rv0), padded(np.zeros(4 * C_))
    d_nbt = torch.tensor([5], dtype=torch.int64, device=dev())
    bn = L.BN()
    bn.gamma, bn.beta, bn.coef = d_gamma.data_ptr(), d_beta.data_ptr(), d_coef.data_ptr()
    if running:
        bn.running_mean, bn.running_var, bn.num_batches_tracked = d_rm.data_ptr(), d_rv.data_ptr(), d_nbt.data_ptr()
    L.check(L.lib.dwn_bn_finalize(stats.data_ptr(), stat_c, float(count), C.byref(bn), C_, 1, float(MOM), float(EPS),
                                  dev().index, stream()), "dwn_bn_finalize")
    torch.cuda.synchronize()

    # the same formulas in float64 (channel c reads the sums of c % stat_c)
    idx = np.arange(C_) % stat_c
    mean = s[idx] / float(count)
    var = np.maximum(ss[idx] / float(count) - mean * mean, 0.0)
    if negative_var:
        assert (var[::2] == 0).all() and (var[1::2] > 0).all()
    invstd = (1.0 / np.sqrt(var + np.float64(EPS))).astype(np.float32)
    mean_f = mean.astype(np.float32)
    scale = gamma * invstd                                                   # one float product: the rounded float64 product
    coef = body(d_coef).reshape(4, C_)
    tag = f"train C={C_} stat_c={stat_c} count={count}"
    exact(coef[2], mean, tag + " mean")
    exact(coef[3], invstd, tag + " invstd")
    within(coef[0], gamma.astype(np.float64) * invstd, np.abs(gamma.astype(np.float64) * invstd), tag + " scale")
    ms = mean_f.astype(np.float64) * scale
    within(coef[1], beta - ms, np.abs(beta.astype(np.float64)) + np.abs(ms), tag + " shift")
    rm, rv = body(d_rm), body(d_rv)
    if not running:
        assert np.array_equal(rm, rm0) and np.array_equal(rv, rv0) and int(d_nbt.item()) == 5
        return
    assert int(d_nbt.item()) == 6, "num_batches_tracked must advance by exactly 1"
    unbiased = (var * count / (count - 1) if count > 1 else var).astype(np.float32)
    om = np.float64(np.float32(1) - MOM)
    t1, t2 = om * rm0, np.float64(MOM) * mean_f
    within(rm, t1 + t2, np.abs(t1) + np.abs(t2), tag + " running_mean")
    t1, t2 = om * rv0, np.float64(MOM) * unbiased
    within(rv, t1 + t2, np.abs(t1) + np.abs(t2), tag + " running_var")


@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("count", [1, 37])
@pytest.mark.parametrize("C_,stat_c", SHAPES)
def test_bn_finalize_train(C_, stat_c, count, running):
    run_train(C_, stat_c, count, running)


@pytest.mark.parametrize("count", [1, 37])
def test_bn_finalize_train_clamps_negative_variance(count):
    run_train(12, 12, count, True, negative_var=True, seed=1)


@pytest.mark.parametrize("C_", [8, 12, 20, 448])
def test_bn_finalize_eval(C_):
    import sensorium_amd._lib as L
    rng = np.random.default_rng(77 + C_)
    gamma = (1 + 0.2 * rng.normal(size=C_)).astype(np.float32)
    beta = (0.3 * rng.normal(size=C_)).astype(np.float32)
    rm0 = (0.3 * rng.normal(size=C_)).astype(np.float32)
    rv0 = (0.05 + 2 * rng.uniform(size=C_)).astype(np.float32)
    d_gamma, d_beta = torch.from_numpy(gamma).to(dev()), torch.from_numpy(beta).to(dev())
    d_rm, d_rv, d_coef = padded(rm0), padded(rv0), padded(np.zeros(4 * C_))
    d_nbt = torch.tensor([5], dtype=torch.int64, device=dev())
    bn = L.BN()
    bn.gamma, bn.beta, bn.coef = d_gamma.data_ptr(), d_beta.data_ptr(), d_coef.data_ptr()
    bn.running_mean, bn.running_var, bn.num_batches_tracked = d_rm.data_ptr(), d_rv.data_ptr(), d_nbt.data_ptr()
    L.check(L.lib.dwn_bn_finalize(None, C_, 37.0, C.byref(bn), C_, 0, float(MOM), float(EPS), dev().index, stream()),
            "dwn_bn_finalize")
    torch.cuda.synchronize()
    invstd = np.float32(1) / np.sqrt(rv0 + EPS)                              # float32 throughout: three correctly rounded operations
    assert invstd.dtype == np.float32
    coef = body(d_coef).reshape(4, C_)
    tag = f"eval C={C_}"
    bad = int((coef[3] != invstd).sum())
    print(f"{tag} invstd: {bad} of {C_} differ from the float32 chain")
    assert bad == 0
    assert np.array_equal(coef[2], rm0)
    scale = gamma * invstd
    within(coef[0], gamma.astype(np.float64) * invstd, np.abs(gamma.astype(np.float64) * invstd), tag + " scale")
    ms = rm0.astype(np.float64) * scale
    within(coef[1], beta - ms, np.abs(beta.astype(np.float64)) + np.abs(ms), tag + " shift")
    assert np.array_equal(body(d_rm), rm0) and np.array_equal(body(d_rv), rv0) and int(d_nbt.item()) == 5, "eval must not touch the buffers"


@pytest.mark.parametrize("grads", [True, False])
@pytest.mark.parametrize("count", [1, 37])
@pytest.mark.parametrize("C_", [8, 12, 20, 448])
def test_bn_bwd_finalize(C_, count, grads):
    import sensorium_amd._lib as L
    rng = np.random.default_rng(5000 + 10 * C_ + count)
    # sum dh and sum dh * yhat: totals up to 2^27 in magnitude, so that their float values are rounded ones
    s1 = rng.integers(-2 ** 27, 2 ** 27, size=C_, dtype=np.int64)
    s2 = rng.integers(-2 ** 27, 2 ** 27, size=C_, dtype=np.int64)
    stats = upload_stats(replica_sums(rng, s1), replica_sums(rng, s2))
    invstd = (1.0 / np.sqrt(rng.uniform(0.5, 3.0, size=C_))).astype(np.float32)
    scale = ((1 + 0.2 * rng.normal(size=C_)) * invstd).astype(np.float32)
    mean = (2 * rng.normal(size=C_)).astype(np.float32)
    coef0 = np.stack([scale, (0.3 * rng.normal(size=C_)).astype(np.float32), mean, invstd])
    d_coef, d_abc = padded(coef0), padded(np.zeros(3 * C_))
    d_dgamma, d_dbeta = padded(np.zeros(C_)), padded(np.zeros(C_))
    bn = L.BN()
    bn.coef = d_coef.data_ptr()
    if grads:
        bn.dgamma, bn.dbeta = d_dgamma.data_ptr(), d_dbeta.data_ptr()
    L.check(L.lib.dwn_bn_bwd_finalize(stats.data_ptr(), float(count), C.byref(bn), d_abc.data_ptr(), C_, dev().index, stream()),
            "dwn_bn_bwd_finalize")
    torch.cuda.synchronize()
    tag = f"bwd C={C_} count={count}"
    assert np.array_equal(body(d_coef), coef0.reshape(-1)), "coef is an input"
    dgamma, dbeta = body(d_dgamma), body(d_dbeta)
    if grads:
        exact(dgamma, s2, tag + " dgamma")
        exact(dbeta, s1, tag + " dbeta")
    else:
        assert not dgamma.any() and not dbeta.any()
    abc = body(d_abc).reshape(3, C_)
    assert np.array_equal(abc[0], scale)
    m1, m2 = s1 / float(count), s2 / float(count)
    sc, inv, mu = scale.astype(np.float64), invstd.astype(np.float64), mean.astype(np.float64)
    a2 = -sc * inv * m2
    within(abc[1], a2, np.abs(a2), tag + " A2")
    within(abc[2], sc * (-m1 + mu * inv * m2), np.abs(sc * m1) + np.abs(sc * mu * inv * m2), tag + " A3")

"""The model's tail held to float64 at kernel level, through the C-ABI structs of sensorium_amd/_lib.py: the H x W pool, the
cortex ShuffleLayers, the readout, the Poisson loss and the multi-tensor AdamW / EMA.

References are float64 torch on the CPU: oracle.cortex_layer / readout / softplus / mice_poisson_loss / adamw_step /
ema_update and autograd through them (tests/gpu_helpers.py builds the inputs and the references, because
tests/test_tail_reference_cpu.py checks the same inputs on the CPU).  For bf16 the inputs, the weights included, are rounded
to bf16 first and both sides see the rounded values, so a bound measures the kernel's own arithmetic.

Bounds.  fp32: gpu_helpers.rel < 1e-3 for every tensor.  bf16: four times the largest error of the family measured against
float64 on an MI355X, never above the suite's 4e-2 (BF16_BOUND below; the measured values are in the table of DESIGN.md 12c).
Low-rate readout: per neuron, |dbias - ref| <= 1e-3 * sum |dz_ref| in fp32 and 2^-8 in bf16 (every dz term is rounded to bf16,
unit roundoff 2^-8, before it is summed; measured 3.0e-3).  AdamW / EMA: 1e-6 after ten steps, the bound of
test_gpu_model.py::test_adamw_ema_multi_matches_reference; float32 storage of the state alone stays below 3.4e-7 on these inputs
(tests/test_tail_reference_cpu.py).  Integer pool, zero-weight dpred, padded readout rows, guard bands, int64 EMA and the
kept / re-packed transposed weight: torch.equal.

No gradient is skipped: at kernel level dout is free, so the shortcut BatchNorm biases whose gradient is analytically zero inside
the model (gpu_helpers.analytically_zero_grad) receive sum(dout) here like any other bias.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import gpu_helpers as H  # noqa: E402
from tests.gpu_helpers import dev, rel, stream  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
DTYPES = [F32, BF16]
NAN = float("nan")
SENT = 12345.678            # guard-band sentinel (no result of these tests comes near it)

# bf16: 4 x the largest error measured per family and tensor on an MI355X, capped at the suite's 4e-2
BF16_BOUND = {
    ("pool", "out"): 7.2e-3, ("pool", "dx"): 7.0e-3,                                    # measured 1.79e-3, 1.73e-3
    ("cortex", "out"): 9.8e-3, ("cortex", "dx"): 2.3e-2, ("cortex", "dw"): 2.4e-2,      # 2.44e-3, 5.67e-3, 5.77e-3
    ("cortex", "dgamma"): 1.3e-2, ("cortex", "dbeta"): 5.9e-3, ("cortex", "running"): 2.8e-3,   # 3.11e-3, 1.45e-3, 6.86e-4
    ("readout", "out"): 5.2e-3, ("readout", "dx"): 1.3e-2, ("readout", "dw"): 1.1e-2, ("readout", "dbias"): 1.2e-2,
}                                                                                       # 1.30e-3, 3.11e-3, 2.73e-3, 2.85e-3


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    return lib


def _dt(L, dtype):
    return L.DWN_BF16 if dtype == BF16 else L.DWN_F32


def _close(family, name, dtype, got, ref, what=""):
    e = rel(got, ref)
    bound = H.TAIL_F32_BOUND if dtype == F32 else BF16_BOUND[(family, name)]
    print(f"TAILFIG {family} {name} {str(dtype).split('.')[-1]} {e:.3e} {what}")
    assert math.isfinite(e) and e < bound, f"{family} {name} {dtype} {what}: {e:.3e} against {bound:.1e}"


def _bytes(n):
    return torch.empty(int(n), dtype=torch.uint8, device=dev())


# ------------------------------------------------------------------------------------------------ pool
def _pool_call(L, dtype, BT, HW, Cc, x=None, dout=None, out=None, dx=None):
    a = L.PoolArgs()
    a.dtype = _dt(L, dtype); a.BT = BT; a.HW = HW; a.C = Cc
    a.x = None if x is None else x.data_ptr(); a.out = None if out is None else out.data_ptr()
    a.dout = None if dout is None else dout.data_ptr(); a.dx = None if dx is None else dx.data_ptr()
    return a


def _pool_run(L, dtype, x, dout):
    BT, HW, Cc = x.shape
    out = torch.full((BT, Cc), NAN, dtype=dtype, device=dev())
    dx = torch.full((BT, HW, Cc), NAN, dtype=dtype, device=dev())
    a = _pool_call(L, dtype, BT, HW, Cc, x=x, out=out, dout=dout, dx=dx)
    L.check(L.lib.dwn_pool_forward(C.byref(a), 0, stream()), "dwn_pool_forward")
    L.check(L.lib.dwn_pool_backward(C.byref(a), 0, stream()), "dwn_pool_backward")
    torch.cuda.synchronize()
    return out, dx


# every HW of {1, 7, 144, 18*32, 36*64}, C of {8, 24, 64, 256, 264} and BT of {1, 31, 33, 1024} (around the 32-row grid stride);
# (1024, 144, 256) is the last block's output at the metric batch
POOL_CASES = [(1, 1, 8), (31, 7, 24), (33, 144, 64), (1024, 144, 256), (33, 576, 264), (31, 2304, 8), (1, 2304, 264),
              (1024, 1, 24), (1024, 7, 264), (33, 7, 256), (31, 576, 64), (1, 144, 24), (33, 1, 264)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("BT,HW,Cc", POOL_CASES)
def test_pool_matches_float64(L, dtype, BT, HW, Cc):
    torch.manual_seed(BT * 7 + HW * 3 + Cc)
    x = (torch.randn(BT, HW, Cc, device=dev()) + 0.5).to(dtype)
    dout = torch.randn(BT, Cc, device=dev()).to(dtype)
    out, dx = _pool_run(L, dtype, x, dout)
    ref_out, ref_dx = H.pool_reference(x.cpu().double(), dout.cpu().double())
    _close("pool", "out", dtype, out, ref_out)
    _close("pool", "dx", dtype, dx, ref_dx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_exact_on_small_integers(L, dtype):
    """HW = 16 and integers in -4 ... 4: sums stay below 2^7, the mean is a multiple of 1/16 with at most 7 significant bits and
    dout / 16 is a shifted integer, so forward and backward are exact in bf16 as in fp32."""
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-4, 5, (33, 16, 24), generator=g).float()
    dout = torch.randint(-100, 101, (33, 24), generator=g).float()
    out, dx = _pool_run(L, dtype, x.to(dev()).to(dtype), dout.to(dev()).to(dtype))
    ref_out, ref_dx = H.pool_reference(x.double(), dout.double())
    assert torch.equal(out.cpu().double(), ref_out)
    assert torch.equal(dx.cpu().double(), ref_dx)


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_rejects_ragged_channel_count(L, dtype):
    """C = 12 is no multiple of the 8-channel vector: both directions answer -2.  The answer is first read from a call over an
    EMPTY tensor (BT = 0: nothing is read or written whatever the library does with it), and only a library that refused it is
    then given real rows, whose buffers must stay untouched."""
    Cc, HW = 12, 5
    buf = torch.full((4 * HW * 16,), SENT, dtype=dtype, device=dev())
    for fn in (L.lib.dwn_pool_forward, L.lib.dwn_pool_backward):
        a = _pool_call(L, dtype, 0, HW, Cc, x=buf, out=buf, dout=buf, dx=buf)
        rc = fn(C.byref(a), 0, stream())
        assert rc == -2, f"{fn.__name__}: rc {rc} for C = 12 on an empty tensor"
    x = torch.full((3, HW, 16), 1.0, dtype=dtype, device=dev())
    small = torch.full((3, 16), 1.0, dtype=dtype, device=dev())
    out = torch.full((3 * 16,), SENT, dtype=dtype, device=dev())
    for fn in (L.lib.dwn_pool_forward, L.lib.dwn_pool_backward):
        a = _pool_call(L, dtype, 3, HW, Cc, x=x, out=out, dout=small, dx=buf)
        assert fn(C.byref(a), 0, stream()) == -2
    torch.cuda.synchronize()
    assert bool((out == torch.tensor(SENT, dtype=dtype)).all()) and bool((buf == torch.tensor(SENT, dtype=dtype)).all())


# ------------------------------------------------------------------------------------------------ cortex
def _bn_struct(L, t, coef, dgamma=None, dbeta=None):
    s = L.BN()
    s.gamma = t["weight"].data_ptr(); s.beta = t["bias"].data_ptr()
    s.running_mean = t["running_mean"].data_ptr(); s.running_var = t["running_var"].data_ptr()
    s.num_batches_tracked = t["num_batches_tracked"].data_ptr(); s.coef = coef.data_ptr()
    s.dgamma = None if dgamma is None else dgamma.data_ptr(); s.dbeta = None if dbeta is None else dbeta.data_ptr()
    return s


def _cortex_run(L, d, dtype, mode, groups, f32_products=0, backward=True):
    B, T, Cin = d["x"].shape
    Cc, Kg = d["w"].shape
    f = dict(dtype=torch.float32, device=dev())
    x, dout = d["x"].to(dev()).to(dtype), d["dout"].to(dev()).to(dtype)
    w = d["w"].to(dev())
    bn = {p: {k: v.clone().to(dev()) for k, v in d[p].items()} for p in ("bn", "bnsc")}
    ds = None if d["drop_scale"] is None else d["drop_scale"].to(dev())
    gm = None if d["dout_mask"] is None else d["dout_mask"].to(dev())
    y = torch.full((B, T, Cc), NAN, dtype=dtype, device=dev())
    out = torch.full((B, T, Cc), NAN, dtype=dtype, device=dev())
    coef, coefsc = torch.empty(4 * Cc, **f), torch.empty(4 * Cc, **f)
    a = L.CortexArgs()
    a.dtype = _dt(L, dtype); a.training = mode; a.B = B; a.T = T; a.Cin = Cin; a.C = Cc; a.groups = groups
    a.eps = orc.BN_EPS; a.momentum = orc.BN_MOMENTUM
    a.x = x.data_ptr(); a.out = out.data_ptr(); a.y = y.data_ptr(); a.w = w.data_ptr()
    a.bn = _bn_struct(L, bn["bn"], coef); a.bnsc = _bn_struct(L, bn["bnsc"], coefsc)
    a.drop_scale = None if ds is None else ds.data_ptr(); a.f32_products = f32_products
    ws = _bytes(L.lib.dwn_cortex_workspace_bytes(C.byref(a), 0))
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_cortex_forward(C.byref(a), 0, stream()), "dwn_cortex_forward")
    res = dict(out=out, y=y)
    for p in ("bn", "bnsc"):
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            res[p + "." + k] = bn[p][k]
    if backward:
        dx = torch.full((B, T, Cin), NAN, dtype=dtype, device=dev())
        dw = torch.full((Cc, Kg), NAN, **f)
        g = {k: torch.full((Cc,), NAN, **f) for k in ("bn.dgamma", "bn.dbeta", "bnsc.dgamma", "bnsc.dbeta")}
        a.bn = _bn_struct(L, bn["bn"], coef, g["bn.dgamma"], g["bn.dbeta"])
        a.bnsc = _bn_struct(L, bn["bnsc"], coefsc, g["bnsc.dgamma"], g["bnsc.dbeta"])
        a.dout = dout.data_ptr(); a.dx = dx.data_ptr(); a.dw = dw.data_ptr()
        if gm is not None:
            a.dout_mask = gm.data_ptr(); a.dout_mask_ld = Cc
        ws2 = _bytes(L.lib.dwn_cortex_workspace_bytes(C.byref(a), 1))
        a.ws = ws2.data_ptr(); a.ws_bytes = ws2.numel()
        L.check(L.lib.dwn_cortex_backward(C.byref(a), 0, stream()), "dwn_cortex_backward")
        res.update(dx=dx, dw=dw, **g)
    torch.cuda.synchronize()
    return res


def _cortex_check(L, dtype, mode, B, T, Cin, Cc, groups, drop, mask, seed, offset=0.0, f32_products=0, keep=None):
    d = H.cortex_inputs(seed, dtype, B, T, Cin, Cc, groups, drop, mask, offset, keep)
    backward = mode != L.BN_EVAL
    got = _cortex_run(L, d, dtype, mode, groups, f32_products, backward)
    ref = H.cortex_reference(d, groups, training=mode == L.BN_TRAIN)
    what = f"mode{mode} B{B} T{T} {Cin}->{Cc} g{groups} drop{int(drop)} mask{int(mask)}"
    _close("cortex", "out", dtype, got["out"], ref["out"], what)
    for p in ("bn", "bnsc"):
        if mode == L.BN_TRAIN:
            # (the statistics are fp32 buffers in both dtypes; bf16 enters through the stored conv output only)
            _close("cortex", "running", dtype, got[p + ".running_mean"], ref[p + ".running_mean"], what + " " + p + ".running_mean")
            _close("cortex", "running", dtype, got[p + ".running_var"], ref[p + ".running_var"], what + " " + p + ".running_var")
            assert int(got[p + ".num_batches_tracked"]) == int(ref[p + ".num_batches_tracked"]) == 6
        else:
            assert torch.equal(got[p + ".running_mean"].cpu(), d[p]["running_mean"])
            assert torch.equal(got[p + ".running_var"].cpu(), d[p]["running_var"])
            assert int(got[p + ".num_batches_tracked"]) == 5
    if backward:
        _close("cortex", "dx", dtype, got["dx"], ref["dx"], what)
        _close("cortex", "dw", dtype, got["dw"], ref["dw"], what)
        for p in ("bn", "bnsc"):
            _close("cortex", "dgamma", dtype, got[p + ".dgamma"], ref[p + ".dgamma"], what + " " + p)
            _close("cortex", "dbeta", dtype, got[p + ".dbeta"], ref[p + ".dbeta"], what + " " + p)


VARIANTS = [(False, False), (True, False), (False, True), (True, True)]       # (drop_scale, dout_mask)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])                                        # DWN_BN_TRAIN, DWN_BN_FROZEN
@pytest.mark.parametrize("drop,mask", VARIANTS)
@pytest.mark.parametrize("B,T", [(1, 3), (3, 5), (2, 65)])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("Cin,Cc", [(16, 32), (32, 32), (48, 96)])
def test_cortex_small_matches_float64(L, dtype, mode, drop, mask, B, T, groups, Cin, Cc):
    _cortex_check(L, dtype, mode, B, T, Cin, Cc, groups, drop, mask, seed=B * 100 + T + Cin + groups)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,T", [(1, 3), (3, 5), (2, 65)])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("Cin,Cc", [(16, 32), (32, 32), (48, 96)])
def test_cortex_small_eval_forward(L, dtype, B, T, groups, Cin, Cc):
    for f32p, drop in ((L.F32_AUTO, True), (L.F32_NATIVE, False)):
        _cortex_check(L, dtype, L.BN_EVAL, B, T, Cin, Cc, groups, drop, False, seed=B * 100 + T + Cin + groups, f32_products=f32p)


# DwiseNeuro's defaults: core_features[-1] = 256 -> cortex_features (1024, 2048, 4096), groups 2, at the metric batch 32 x 32
PRODUCTION_CORTEX = [(256, 1024), (1024, 2048), (2048, 4096)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("Cin,Cc", PRODUCTION_CORTEX)
def test_cortex_production_matches_float64(L, dtype, mode, Cin, Cc):
    _cortex_check(L, dtype, mode, 32, 32, Cin, Cc, 2, True, True, seed=Cc + mode)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Cin,Cc", PRODUCTION_CORTEX)
def test_cortex_production_eval_forward(L, dtype, Cin, Cc):
    _cortex_check(L, dtype, L.BN_EVAL, 32, 32, Cin, Cc, 2, True, False, seed=Cc, f32_products=L.F32_AUTO)


@pytest.mark.parametrize("B,T,Cin,Cc", [(2, 65, 48, 96), (32, 32, 256, 1024)])
def test_cortex_fp32_products_follow_the_request(L, B, T, Cin, Cc):
    """f32_products of the fp32 layer (include/dwn.h DWN_F32_*): in the eval forward SPLIT3 and NATIVE both meet the bound but are
    different products (different bits), and AUTO is SPLIT3 bit for bit; in training AUTO is NATIVE and an explicit SPLIT3 is still
    honoured.  Compared on the raw conv output y, which no atomic touches."""
    d = H.cortex_inputs(Cc + B, F32, B, T, Cin, Cc, 2, False, False)
    ref = H.cortex_reference(d, 2, training=False)["out"]
    ev = {p: _cortex_run(L, d, F32, L.BN_EVAL, 2, p, backward=False) for p in (L.F32_AUTO, L.F32_NATIVE, L.F32_SPLIT3)}
    for p, r in ev.items():
        _close("cortex", "out", F32, r["out"], ref, f"eval f32_products {p}")
    assert torch.equal(ev[L.F32_AUTO]["y"], ev[L.F32_SPLIT3]["y"]) and torch.equal(ev[L.F32_AUTO]["out"], ev[L.F32_SPLIT3]["out"])
    assert not torch.equal(ev[L.F32_NATIVE]["y"], ev[L.F32_SPLIT3]["y"]), "SPLIT3 and NATIVE gave the same bits: one was ignored"
    for mode in (L.BN_TRAIN, L.BN_FROZEN):
        tr = {p: _cortex_run(L, d, F32, mode, 2, p, backward=False)["y"] for p in (L.F32_AUTO, L.F32_NATIVE, L.F32_SPLIT3)}
        assert torch.equal(tr[L.F32_AUTO], tr[L.F32_NATIVE]) and torch.equal(tr[L.F32_NATIVE], ev[L.F32_NATIVE]["y"])
        assert torch.equal(tr[L.F32_SPLIT3], ev[L.F32_SPLIT3]["y"])


@pytest.mark.parametrize("groups", [1, 2])
def test_cortex_train_large_channel_mean(L, groups):
    """Inputs 100 + N(0, 1): the batch variance of the conv output and of the shortcut is the small difference of large sums (as the
    Gram test does for BatchNorm-1).  fp32 only: in bf16 the input spacing around 100 is 0.5 and the stored conv output is rounded to
    the same grid, so a bf16 figure here would measure the storage format (0.14 of a standard deviation), not the variance.

    With the sums of y and y^2 added in float32 within a GEMM tile (before the float64 atomics) this case measured out 4.8e-4 ...
    6.2e-4, dx 5.9e-4 ... 7.8e-4, running_var 1.6e-4 and dw 1.21e-3 (groups 2) / 1.57e-3 (groups 1) against the 1e-3 bound: with
    mean^2 / var = 1e4 the variance keeps 1.6e-4 of error, and dw = dy^T x multiplies the then non-zero batch sum of dy by the input
    mean of 100.  The training forward now sums the stored y and x in double (cortex_stats_kernel; DESIGN.md 12c, finding 4)."""
    _cortex_check(L, F32, L.BN_TRAIN, 2, 65, 48, 96, groups, True, True, seed=77, offset=100.0, keep=1)


# ------------------------------------------------------------------------------------------------ readout
def _readout_args(L, dtype, B, T, Cin, groups, n_out, beta, t):
    a = L.ReadoutArgs()
    a.dtype = _dt(L, dtype); a.B = B; a.T = T; a.Cin = Cin; a.groups = groups; a.n_out = n_out; a.softplus_beta = beta
    a.x = t["x"].data_ptr(); a.w = t["w"].data_ptr(); a.bias = t["bias"].data_ptr()
    a.drop_mask = None if t.get("drop_mask") is None else t["drop_mask"].data_ptr()
    return a


def _readout_forward(L, a, B, T, n_out, f32_products, keep_wt):
    """out [B][n_out][T] in front of a 64-float guard band; NaN-filled, so an element the kernel skips shows."""
    buf = torch.full((B * n_out * T + 64,), SENT, dtype=torch.float32, device=dev())
    buf[:B * n_out * T] = NAN
    a.out = buf.data_ptr(); a.f32_products = f32_products
    wt = None
    if keep_wt:
        wt = _bytes(L.lib.dwn_readout_wt_bytes(C.byref(a)))
        a.wt = wt.data_ptr()
    else:
        a.wt = None
    ws = _bytes(L.lib.dwn_readout_workspace_bytes(C.byref(a), 0))
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_readout_forward(C.byref(a), 0, stream()), "dwn_readout_forward")
    torch.cuda.synchronize()
    assert bool((buf[B * n_out * T:] == SENT).all()), "readout forward wrote past out[B][n_out][T]"
    return buf[:B * n_out * T].view(B, n_out, T), wt


def _readout_backward(L, a, dtype, x_shape, npad, Kg, dout, wt, dbias_fill=0.0, misalign_dw=False):
    f = dict(dtype=torch.float32, device=dev())
    dx = torch.full(x_shape, NAN, dtype=dtype, device=dev())
    dwbuf = torch.full((npad * Kg + 1,), NAN, **f)
    dw = dwbuf[1:] if misalign_dw else dwbuf[:-1]       # one float off 16-byte alignment: the zero-and-accumulate branch
    assert (dw.data_ptr() % 16 != 0) == misalign_dw
    dbias = torch.full((npad,), dbias_fill, **f)
    a.dout = dout.data_ptr(); a.dx = dx.data_ptr(); a.dw = dw.data_ptr(); a.dbias = dbias.data_ptr()
    a.wt = None if wt is None else wt.data_ptr()
    ws = _bytes(L.lib.dwn_readout_workspace_bytes(C.byref(a), 1))
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_readout_backward(C.byref(a), 0, stream()), "dwn_readout_backward")
    torch.cuda.synchronize()
    return dx, dw.view(npad, Kg), dbias


# (n_out, groups, Cin, B, T, beta, drop_mask): every n_out of {7, 64, 65, 127, 1000, 7863}, both group counts (odd n_out with two
# groups leaves a padded row), Cin 16 / 64 / 4096, T of {1, 5, 16, 32}, B of {1, 3}; the last line is a production readout
READOUT_CASES = [
    (7, 1, 16, 1, 1, 1.0, False), (7, 2, 16, 3, 5, 0.07, True), (64, 1, 64, 3, 16, 0.07, False), (64, 2, 64, 1, 32, 1.0, True),
    (65, 2, 16, 3, 1, 1.0, False), (65, 1, 64, 1, 5, 0.07, True), (127, 2, 64, 3, 16, 1.0, True), (127, 1, 16, 3, 32, 0.07, False),
    (1000, 2, 64, 3, 5, 0.07, True), (1000, 1, 16, 1, 16, 1.0, False), (7863, 2, 64, 3, 5, 0.07, False),
    (7863, 1, 16, 1, 32, 1.0, True), (1000, 2, 4096, 3, 16, 0.07, True), (7863, 2, 4096, 32, 32, 0.07, True),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n_out,groups,Cin,B,T,beta,mask", READOUT_CASES)
def test_readout_matches_float64(L, dtype, n_out, groups, Cin, B, T, beta, mask):
    """Forward (fp32: native and split-3 products), then the backward twice: with the transposed weight kept from the forward, an
    aligned dw and a zeroed dbias; and with a null wt (packed by the backward), dw one float off alignment and dbias pre-filled
    with 0.25 (it is accumulated).  dx of the two must be the same bits: the re-packed weight is the kept one."""
    d = H.readout_inputs(n_out * 3 + Cin + B + T, dtype, B, T, Cin, groups, n_out, beta, mask)
    ref = H.readout_reference(d, groups, n_out, beta)
    npad, Kg = d["w"].shape
    what = f"n{n_out} g{groups} Cin{Cin} B{B} T{T} beta{beta} mask{int(mask)}"
    t = {k: (None if v is None else v.to(dev())) for k, v in d.items()}
    t["x"] = t["x"].to(dtype)
    a = _readout_args(L, dtype, B, T, Cin, groups, n_out, beta, t)
    if dtype == F32:
        out, _ = _readout_forward(L, a, B, T, n_out, L.F32_SPLIT3, False)
        _close("readout", "out", dtype, out, ref["out"], what + " split3")
    out, wt = _readout_forward(L, a, B, T, n_out, L.F32_NATIVE, True)
    _close("readout", "out", dtype, out, ref["out"], what)
    dx1, dw1, db1 = _readout_backward(L, a, dtype, d["x"].shape, npad, Kg, t["dout"], wt)
    dx2, dw2, db2 = _readout_backward(L, a, dtype, d["x"].shape, npad, Kg, t["dout"], None, dbias_fill=0.25, misalign_dw=True)
    assert torch.equal(dx1, dx2), "dx differs between the kept and the re-packed transposed weight"
    for dx, dw, db, fill, tag in ((dx1, dw1, db1, 0.0, " kept"), (dx2, dw2, db2, 0.25, " repacked")):
        _close("readout", "dx", dtype, dx, ref["dx"], what + tag)
        _close("readout", "dw", dtype, dw, ref["dw"], what + tag)
        _close("readout", "dbias", dtype, db, ref["dbias"] + fill, what + tag)
        if npad > n_out:            # the padded row: no neuron behind it
            assert bool((dw[n_out:] == 0).all()) and bool((db[n_out:] == fill).all())
        if mask:                    # the channel dropped in every sample
            assert bool((dx[..., 3] == 0).all())


def _low_rate_run(L, dtype, beta, groups, B, T, target=None, w=None):
    """Zero weights, bias spread over beta * z in [-30, 25]: forward on the device, dout = the Poisson gradient on the device's own
    prediction (target None: the constant 1 of a zero target under unit weights), backward; returns dbias [N] and the forward."""
    bias = H.low_rate_bias(beta)
    n, Cin = bias.numel(), 16
    npad, Kg = (n + groups - 1) // groups * groups, Cin // groups
    g = torch.Generator().manual_seed(11)
    t = dict(x=torch.randn(B, T, Cin, generator=g).to(dev()).to(dtype), w=torch.zeros(npad, Kg, device=dev()),
             bias=torch.cat([bias, torch.zeros(npad - n)]).to(dev()))
    a = _readout_args(L, dtype, B, T, Cin, groups, n, beta, t)
    out, wt = _readout_forward(L, a, B, T, n, L.F32_NATIVE, True)
    if target is None:
        dout = torch.ones(B, n, T, device=dev())
    else:
        dout = torch.full((B, n, T), NAN, device=dev())
        tg, wd = target.to(dev()), w.to(dev())
        L.check(L.lib.dwn_poisson_loss_backward(out.data_ptr(), tg.data_ptr(), wd.data_ptr(), None, n * T, B * n * T, 1e-8,
                                                dout.data_ptr(), 0, stream()), "dwn_poisson_loss_backward")
    _, _, dbias = _readout_backward(L, a, dtype, (B, T, Cin), npad, Kg, dout, wt)
    return bias, out.cpu(), dbias.cpu()[:n]


def _per_neuron(dtype, beta, bias, dbias, ref, what):
    bound = H.TAIL_F32_BOUND if dtype == F32 else H.TAIL_BF16_NEURON_BOUND
    err = (dbias.double() - ref["dbias"]).abs() / ref["sumabs"]
    worst = int(err.argmax())
    print(f"TAILFIG lowrate {what} {str(dtype).split('.')[-1]} beta{beta} worst {float(err[worst]):.3e} at beta*z = "
          f"{float(bias[worst]) * beta:.1f}; neurons over the bound: {int((err > bound).sum())} of {err.numel()}")
    bad = [(round(float(bias[i]) * beta, 1), float(err[i])) for i in torch.nonzero(err > bound).flatten().tolist()]
    assert not bad, f"low-rate readout {what} {dtype} beta {beta}: per-neuron error over {bound:.1e} at (beta*z, error) {bad[:6]} ..."


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("beta", [1.0, 0.07])
def test_readout_low_rate_neurons_constant_dout(L, dtype, groups, beta):
    """dbias[n] = sum of same-signed terms sigmoid(beta * z_n): a true per-neuron relative error, down to beta * z = -30 where
    the stored prediction is 1e-13 / beta.  1 - exp(-beta * out) fails this from beta * z of about -10 down."""
    B, T = 3, 5
    bias, out, dbias = _low_rate_run(L, dtype, beta, groups, B, T)
    ref = H.low_rate_reference(bias, beta, B, T)
    assert rel(out, ref["out"]) < H.TAIL_F32_BOUND           # (the prediction is fp32 in both dtypes)
    _per_neuron(dtype, beta, bias, dbias, ref, "constant")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("beta", [1.0, 0.07])
def test_readout_low_rate_neurons_poisson_dout(L, dtype, beta):
    """The same neurons under the real Poisson gradient w * (1 - y / (out + eps)) of targets > 0, formed on the device from the
    device's own prediction: of order 1 / out on a quiet neuron, so dL/dz stays O(y) there.  Per neuron, relative to sum |dz_ref|."""
    B, T = 3, 5
    n = H.low_rate_bias(beta).numel()
    g = torch.Generator().manual_seed(13)
    target = torch.empty(B, n, T).uniform_(0.5, 5.0, generator=g)
    w = torch.full((B,), 1.0 / B)
    bias, out, dbias = _low_rate_run(L, dtype, beta, 2, B, T, target, w)
    ref = H.low_rate_reference(bias, beta, B, T, target, w)
    _per_neuron(dtype, beta, bias, dbias, ref, "poisson")


# ------------------------------------------------------------------------------------------------ Poisson loss
def _poisson_run(L, pred, target, w, gscale=None):
    B, per = target.shape
    acc = torch.zeros(1, dtype=torch.float64, device=dev())
    dpred = torch.full((B, per), NAN, device=dev())
    gs = None if gscale is None else torch.tensor([gscale], dtype=torch.float32, device=dev())
    L.check(L.lib.dwn_poisson_loss_forward(pred.data_ptr(), target.data_ptr(), w.data_ptr(), per, B * per, 1e-8, acc.data_ptr(),
                                           0, stream()), "dwn_poisson_loss_forward")
    L.check(L.lib.dwn_poisson_loss_backward(pred.data_ptr(), target.data_ptr(), w.data_ptr(), None if gs is None else gs.data_ptr(),
                                            per, B * per, 1e-8, dpred.data_ptr(), 0, stream()), "dwn_poisson_loss_backward")
    torch.cuda.synchronize()
    return acc.cpu()[0], dpred.cpu()


# per_sample of {1, 3, 4, 1020, 1024, 1028, 4096*4 + 4, 7863*32, 7863*31 (odd: the scalar kernel)} with B of {1, 3, 32, 600}
# (at 600 the chunk cap ceil(512 / B) is 1); the longest samples stay with B <= 32 (600 x 7863 x 32 floats is 600 MB a tensor)
POISSON_CASES = [(1, 1), (1, 600), (3, 3), (3, 32), (4, 1), (4, 600), (1020, 3), (1020, 32), (1024, 1), (1024, 32), (1024, 600),
                 (1028, 3), (1028, 600), (16388, 1), (16388, 32), (16388, 600), (251616, 3), (251616, 32), (243753, 1), (243753, 32)]


def _poisson_check(L, per, B, kind, offset):
    pred, target, w = H.poisson_inputs(per + B, B, per, kind)
    live = w != 0
    garbage = pred.clone()
    garbage[~live] = -5.0                  # a prediction no live sample may have (log of it is NaN): it must never be read
    buf = torch.empty(B * per + 1, device=dev())
    pd = buf[offset:offset + B * per].view(B, per)
    pd.copy_(garbage)
    assert pd.data_ptr() % 16 == 4 * offset
    for gscale in (None, 0.37):
        loss, dpred = _poisson_run(L, pd, target.to(dev()), w.to(dev()), gscale)
        ref_loss, ref_d = H.poisson_reference(pred, target, w, 1.0 if gscale is None else gscale)
        e = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss))
        print(f"TAILFIG poisson loss float32 {e:.3e} per{per} B{B} {kind} offset{offset}")
        assert e < H.TAIL_F32_BOUND
        _close("poisson", "dpred", F32, dpred, ref_d, f"per{per} B{B} {kind} gscale{gscale} offset{offset}")
        assert bool((dpred[~live] == 0).all()), "dpred of a zero-weight sample is not exactly 0"


@pytest.mark.parametrize("kind", ["equal", "onehot", "general"])
@pytest.mark.parametrize("per,B", POISSON_CASES)
def test_poisson_loss_matches_float64(L, per, B, kind):
    _poisson_check(L, per, B, kind, 0)


@pytest.mark.parametrize("kind", ["equal", "onehot", "general"])
@pytest.mark.parametrize("per,B", [(4, 600), (1024, 32), (16388, 3)])
def test_poisson_loss_unaligned_prediction(L, per, B, kind):
    """pred is a view one float into its buffer: a multiple-of-4 sample length still has to take the scalar kernels."""
    _poisson_check(L, per, B, kind, 1)


def test_poisson_loss_ignores_zero_weight_neighbours(L):
    """Three live samples alone, and the same three inside 32 and inside 600 samples of weight 0: the same loss (to the bound: the
    grid, hence the summation order, follows B) and the same gradient on the live rows."""
    per = 16388
    pred, target, _ = H.poisson_inputs(99, 3, per, "equal")
    w3 = torch.full((3,), 1 / 3)
    ref_loss, ref_d = H.poisson_reference(pred, target, w3)
    for B in (3, 32, 600):
        rows = torch.arange(3) * (B // 3)
        p = torch.full((B, per), -5.0); t = torch.zeros(B, per); w = torch.zeros(B)
        p[rows], t[rows], w[rows] = pred, target, w3
        loss, dpred = _poisson_run(L, p.to(dev()), t.to(dev()), w.to(dev()))
        assert abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)) < H.TAIL_F32_BOUND
        assert rel(dpred[rows], ref_d) < H.TAIL_F32_BOUND
        dpred[rows] = 0
        assert bool((dpred == 0).all())


# ------------------------------------------------------------------------------------------------ AdamW + EMA
GUARD = 64
_ENTRY = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("ema", "<u8"),
                   ("numel", "<i8"), ("is_int64", "<i4"), ("pad", "<i4")])


def _layout(sizes):
    """Slices of one arena: a 64-float guard band on either side of each, and every other slice starting at an odd float offset
    (4 bytes times an odd count into the arena: the sharded optimizer's layout, never 16-byte aligned)."""
    pos, spans = 0, []
    for i, n in enumerate(sizes):
        pos += GUARD
        if i % 2 == 0 and pos % 2 == 0:
            pos += 1
        spans.append((pos, n))
        pos += n
    return spans, pos + GUARD


def _arena(spans, total, tensors):
    a = torch.full((total,), SENT)
    for (s, n), t in zip(spans, tensors):
        a[s:s + n] = t
    return a.to(dev())


def _outside_untouched(arena, spans):
    m = torch.ones(arena.numel(), dtype=torch.bool)
    for s, n in spans:
        m[s:s + n] = False
    return bool((arena.cpu()[m] == torch.tensor(SENT)).all())


def _table(entries):
    return torch.from_numpy(np.frombuffer(entries.tobytes(), dtype=np.uint8).copy()).to(dev())


SIZES = [1, 3, 255, 256, 257, 4097, 16 * 256 + 1, 1_000_003]


def _sizes(ntensors):
    if ntensors == 1:
        return [1_000_003]
    if ntensors == 2:
        return [257, 1_000_003]
    return [SIZES[i % 7] for i in range(ntensors - 1)] + [1_000_003]       # every size, the long one once


@pytest.mark.parametrize("ntensors,max_blocks,wd,step0", [(1, 1, 0.0, 1), (2, 16, 0.05, 2), (37, 64, 0.05, 1000), (37, 1, 0.0, 100_000),
                                                          (37, 16, 0.05, 1), (2, 64, 0.0, 100_000), (1, 64, 0.05, 2), (37, 64, 0.0, 2)])
def test_adamw_ema_multi_ten_steps(L, ntensors, max_blocks, wd, step0):
    """Ten consecutive steps of one launch each against float64 oracle.adamw_step / ema_update, per tensor, for p, exp_avg,
    exp_avg_sq and ema; every third entry has no EMA; grad_scale 0.37.  float32 storage of the state alone deviates by at most
    3.4e-7 on these inputs (tests/test_tail_reference_cpu.py), inside the 1e-6 of the existing optimizer test, which is the bound."""
    lr, decay, gscale = 2.4e-3, 0.999, 0.37
    sizes = _sizes(ntensors)
    case = H.adamw_case(7 + step0, sizes, step0)
    has_ema = [i % 3 != 2 for i in range(ntensors)]
    ref = H.adamw_reference(case, step0, lr, wd, decay, gscale, has_ema=has_ema)
    spans, total = _layout(sizes)
    ar = {k: _arena(spans, total, [c[k] for c in case]) for k in ("p", "m", "v", "ema")}
    grad = torch.full((total,), SENT, device=dev())
    ent = np.zeros(ntensors, dtype=_ENTRY)
    for i, (s, n) in enumerate(spans):
        ent[i] = (ar["p"].data_ptr() + 4 * s, grad.data_ptr() + 4 * s, ar["m"].data_ptr() + 4 * s, ar["v"].data_ptr() + 4 * s,
                  ar["ema"].data_ptr() + 4 * s if has_ema[i] else 0, n, 0, 0)
    table = _table(ent)
    assert L.lib.dwn_adamw_ema_multi(table.data_ptr(), ntensors, max_blocks, lr, 0.9, 0.999, 1e-8, wd, 0, decay, gscale, 0,
                                     stream()) == -2, "step = 0 must be refused"
    for s in range(10):
        grad.copy_(_arena(spans, total, [c["grads"][s] for c in case]))
        L.check(L.lib.dwn_adamw_ema_multi(table.data_ptr(), ntensors, max_blocks, lr, 0.9, 0.999, 1e-8, wd, step0 + s, decay,
                                          gscale, 0, stream()), "dwn_adamw_ema_multi")
    torch.cuda.synchronize()
    worst = {}
    for k in ("p", "m", "v", "ema"):
        assert _outside_untouched(ar[k], spans), f"{k}: a guard band was written"
        host = ar[k].cpu()
        for i, (s, n) in enumerate(spans):
            if k == "ema" and not has_ema[i]:
                assert torch.equal(host[s:s + n], case[i]["ema"]), "an entry without EMA had its slice of the EMA arena written"
                continue
            e = rel(host[s:s + n], ref[i][k])
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < H.ADAMW_BOUND, f"{k} of tensor {i} ({n} elements): {e:.3e}"
    assert _outside_untouched(grad, spans)
    print(f"TAILFIG adamw n{ntensors} blocks{max_blocks} wd{wd} step{step0} " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("max_blocks", [1, 16, 64])
def test_ema_lerp_multi_float_entries(L, max_blocks):
    sizes = [SIZES[i % 8] for i in range(11)]
    g = torch.Generator().manual_seed(3)
    model = [torch.randn(n, generator=g) for n in sizes]
    ema0 = [m + 0.01 * torch.randn(m.numel(), generator=g) for m in model]
    spans, total = _layout(sizes)
    am, ae = _arena(spans, total, model), _arena(spans, total, ema0)
    ent = np.zeros(len(sizes), dtype=_ENTRY)
    for i, (s, n) in enumerate(spans):
        ent[i] = (am.data_ptr() + 4 * s, 0, 0, 0, ae.data_ptr() + 4 * s, n, 0, 0)
    table = _table(ent)
    L.check(L.lib.dwn_ema_lerp_multi(table.data_ptr(), len(sizes), max_blocks, 0.999, 0, stream()), "dwn_ema_lerp_multi")
    torch.cuda.synchronize()
    assert _outside_untouched(ae, spans) and torch.equal(am.cpu(), _arena(spans, total, model).cpu())
    host = ae.cpu()
    for (s, n), m, e0 in zip(spans, model, ema0):
        assert rel(host[s:s + n], orc.ema_update(e0.double(), m.double(), 0.999)) < H.ADAMW_BOUND


@pytest.mark.parametrize("decay", H.EMA_DECAYS)
def test_ema_lerp_int64_pairs_match_reference_arithmetic(L, decay):
    """num_batches_tracked: every pair (ema, model) of gpu_helpers.ema_int_pairs in one 9000-element int64 tensor (the kernel loops
    over it), next to a float entry in the same launch.  Expected: torch's own int64 * float -> float32 -> int64 arithmetic on the
    CPU (oracle.ema_update): two rounded products and a rounded sum.  A contracted multiply-add gives another integer in 581 of the
    27 000 pairs (tests/test_tail_reference_cpu.py)."""
    e, m = H.ema_int_pairs()
    ed, md = e.to(dev()), m.to(dev())
    fm, fe = torch.randn(300, device=dev()), torch.randn(300, device=dev())
    fe0 = fe.clone()
    ent = np.zeros(2, dtype=_ENTRY)
    ent[0] = (fm.data_ptr(), 0, 0, 0, fe.data_ptr(), 300, 0, 0)
    ent[1] = (md.data_ptr(), 0, 0, 0, ed.data_ptr(), e.numel(), 1, 0)
    table = _table(ent)
    L.check(L.lib.dwn_ema_lerp_multi(table.data_ptr(), 2, 16, decay, 0, stream()), "dwn_ema_lerp_multi")
    torch.cuda.synchronize()
    want = orc.ema_update(e, m, decay)
    diff = torch.nonzero(ed.cpu() != want).flatten()
    first = [(int(e[i]), int(m[i]), int(ed[i]), int(want[i])) for i in diff[:4].tolist()]
    assert torch.equal(ed.cpu(), want), f"decay {decay}: {diff.numel()} of {e.numel()} pairs differ; (ema, model, got, want) {first}"
    assert torch.equal(md.cpu(), m)
    assert rel(fe, orc.ema_update(fe0.double().cpu(), fm.double().cpu(), decay)) < H.ADAMW_BOUND


def test_ema_lerp_int64_trajectory(L):
    """30 000 steps at decay 0.9999 from an EMA counter of 0 against model counters 1, 2, 3, ... (and two other strides in the same
    tensor), one launch per step, compared every 5000 steps.  The reference arithmetic ends column 0 at 19 997; with the second
    product contracted the trajectory leaves it at step 10 011 and ends at 20 001."""
    steps, decay, chunk = 30_000, 0.9999, 5000
    M = H.ema_trajectory(steps, decay)
    Md = M.to(dev())
    ema = torch.zeros(M.shape[1], dtype=torch.int64, device=dev())
    ent = np.zeros(steps, dtype=_ENTRY)
    for k in range(steps):
        ent[k] = (Md.data_ptr() + 8 * M.shape[1] * k, 0, 0, 0, ema.data_ptr(), M.shape[1], 1, 0)
    table = _table(ent)
    want = torch.zeros(M.shape[1], dtype=torch.int64)
    for k in range(steps):
        L.check(L.lib.dwn_ema_lerp_multi(table.data_ptr() + _ENTRY.itemsize * k, 1, 1, decay, 0, stream()), "dwn_ema_lerp_multi")
        want = orc.ema_update(want, M[k], decay)
        if (k + 1) % chunk == 0:
            torch.cuda.synchronize()
            assert torch.equal(ema.cpu(), want), f"after {k + 1} steps: {ema.cpu().tolist()} against {want.tolist()}"
    assert int(want[0]) == 19_997

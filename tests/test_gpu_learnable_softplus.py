"""Learnable Softplus beta at kernel level, through the C-ABI (dwn_readout_args.beta_dev / .dbeta).

Same bits: with the same float value of beta in device memory, out / dx / dw are bit-identical to the fixed path (dbias: atomics,
identical in the deterministic build, TAIL_F32_BOUND otherwise).  dbeta is held (a) to the float64 formula on the device's OWN out
and the same dout — this isolates the fp32 term and the float64 reduction; bound 4 x lsp_helpers.TERM_BOUND of the sum of |terms|,
the factor for device expf / log1pf / expm1f being allowed an ulp or two more than the host's — and (b) end to end to float64
autograd through oracle.readout with beta a float64 leaf, to the bound tests/test_gpu_tail.py applies to the readout's dbias.
Shapes: B of {1, 3}, T of {1, 5, 16}, groups of {1, 2}, Cin of {16, 32}, n_out of {1, 63, 65, 130} (a padded row with two groups,
a ragged 64-neuron tile, more than one tile), both dtypes, with and without a dropout mask, beta of {0.07, 1, 5}.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_helpers as H  # noqa: E402
from tests import lsp_helpers as S  # noqa: E402
from tests.gpu_helpers import dev, rel, stream  # noqa: E402
from tests.test_gpu_tail import BF16_BOUND  # noqa: E402

F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
DBETA_OWN_OUT_BOUND = 4 * S.TERM_BOUND

# (n_out, groups, Cin, B, T, beta, drop_mask)
CASES = [
    (1, 1, 16, 1, 1, 1.0, False), (1, 2, 16, 3, 5, 0.07, True), (1, 2, 32, 1, 16, 5.0, False),
    (63, 1, 32, 3, 16, 5.0, False), (63, 2, 16, 1, 5, 1.0, True), (63, 2, 32, 3, 1, 0.07, False),
    (65, 2, 32, 3, 1, 0.07, True), (65, 1, 16, 1, 16, 5.0, True), (65, 2, 16, 3, 5, 1.0, False),
    (130, 1, 16, 3, 5, 0.07, True), (130, 2, 32, 1, 16, 1.0, False), (130, 2, 16, 3, 16, 5.0, True),
]


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    return lib


def _bytes(n):
    return torch.empty(int(n), dtype=torch.uint8, device=dev())


def _args(L, dtype, B, T, Cin, groups, n_out, beta, t, beta_dev=None):
    a = L.ReadoutArgs()
    a.dtype = L.DWN_BF16 if dtype == BF16 else L.DWN_F32
    a.B = B; a.T = T; a.Cin = Cin; a.groups = groups; a.n_out = n_out
    # learnable: the scalar is ignored — a value that would show if it were read
    a.softplus_beta = beta if beta_dev is None else 123.0
    a.beta_dev = None if beta_dev is None else beta_dev.data_ptr()
    a.x = t["x"].data_ptr(); a.w = t["w"].data_ptr(); a.bias = t["bias"].data_ptr()
    a.drop_mask = None if t.get("drop_mask") is None else t["drop_mask"].data_ptr()
    a.f32_products = L.F32_NATIVE
    return a


def _forward(L, a, B, T, n_out):
    out = torch.full((B, n_out, T), NAN, dtype=torch.float32, device=dev())
    a.out = out.data_ptr()
    wt = _bytes(L.lib.dwn_readout_wt_bytes(C.byref(a)))
    a.wt = wt.data_ptr()
    ws = _bytes(L.lib.dwn_readout_workspace_bytes(C.byref(a), 0))
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_readout_forward(C.byref(a), 0, stream()), "dwn_readout_forward")
    torch.cuda.synchronize()
    return out, wt


def _backward(L, a, dtype, x_shape, npad, Kg, dout, learnable):
    f = dict(dtype=torch.float32, device=dev())
    dx = torch.full(x_shape, NAN, dtype=dtype, device=dev())
    dw = torch.full((npad, Kg), NAN, **f)
    dbias = torch.zeros(npad, **f)
    # dbeta sits between two sentinels: the finaliser writes one float
    dbeta = torch.full((3,), NAN, **f)
    a.dout = dout.data_ptr(); a.dx = dx.data_ptr(); a.dw = dw.data_ptr(); a.dbias = dbias.data_ptr()
    a.dbeta = dbeta[1:].data_ptr() if learnable else None
    ws = _bytes(L.lib.dwn_readout_workspace_bytes(C.byref(a), 1))
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_readout_backward(C.byref(a), 0, stream()), "dwn_readout_backward")
    torch.cuda.synchronize()
    if learnable:
        assert math.isnan(float(dbeta[0])) and math.isnan(float(dbeta[2])), "the dbeta finaliser wrote past its one float"
    return dx, dw, dbias, dbeta[1].clone()


_RUNS = {}


def _run(L, dtype, case):
    """fixed and learnable forward + backward of one case, the learnable backward twice; computed once, shared by the tests"""
    key = (dtype, case)
    if key in _RUNS:
        return _RUNS[key]
    n_out, groups, Cin, B, T, beta, mask = case
    d = H.readout_inputs(n_out * 3 + Cin + B + T, dtype, B, T, Cin, groups, n_out, beta, mask)
    npad, Kg = d["w"].shape
    t = {k: (None if v is None else v.to(dev())) for k, v in d.items()}
    t["x"] = t["x"].to(dtype)
    res = dict(d=d)
    a = _args(L, dtype, B, T, Cin, groups, n_out, beta, t)
    res["out_fixed"], _ = _forward(L, a, B, T, n_out)
    res["fixed"] = _backward(L, a, dtype, d["x"].shape, npad, Kg, t["dout"], False)
    beta_dev = torch.tensor(beta, dtype=torch.float32, device=dev())
    a = _args(L, dtype, B, T, Cin, groups, n_out, beta, t, beta_dev)
    res["out"], _ = _forward(L, a, B, T, n_out)
    res["learn"] = _backward(L, a, dtype, d["x"].shape, npad, Kg, t["dout"], True)
    res["again"] = _backward(L, a, dtype, d["x"].shape, npad, Kg, t["dout"], True)
    _RUNS[key] = res
    return res


def _own_out_reference(out_dev, dout, beta):
    """float64 formula on the device's own out: (dbeta, sum of |terms|)"""
    terms = dout.double().cpu().numpy() * S.dgdbeta(S.term_f64(out_dev.cpu().numpy(), beta), beta)
    return float(terms.sum()), float(np.abs(terms).sum())


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", CASES)
def test_same_bits_as_the_fixed_path(L, dtype, case):
    r = _run(L, dtype, case)
    assert not bool(torch.isnan(r["out"]).any())
    assert torch.equal(r["out"], r["out_fixed"]), "out differs from the fixed path at the same beta"
    (dx0, dw0, db0, _), (dx1, dw1, db1, _) = r["fixed"], r["learn"]
    assert torch.equal(dx1, dx0) and torch.equal(dw1, dw0), "dx / dw differ from the fixed path at the same beta"
    if L.DETERMINISTIC:
        assert torch.equal(db1, db0)
    else:
        e = rel(db1, db0)
        assert e < H.TAIL_F32_BOUND, f"dbias {e:.3e}"


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", CASES)
def test_dbeta_matches_float64_on_the_devices_own_out(L, dtype, case):
    r = _run(L, dtype, case)
    ref, sumabs = _own_out_reference(r["out"], r["d"]["dout"], case[5])
    got = float(r["learn"][3])
    err = abs(got - ref) / sumabs
    print(f"LSPFIG own-out {str(dtype).split('.')[-1]} {case} dbeta {got:.6e} err {err:.3e}")
    assert math.isfinite(got) and err <= DBETA_OWN_OUT_BOUND, f"{err:.3e} against {DBETA_OWN_OUT_BOUND:.1e}"


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", CASES)
def test_dbeta_matches_oracle_autograd(L, dtype, case):
    n_out, groups, Cin, B, T, beta, mask = case
    r = _run(L, dtype, case)
    ref = S.readout_reference_beta(r["d"], groups, n_out, beta)
    _, sumabs = _own_out_reference(ref["out"], r["d"]["dout"], beta)          # |terms| of the float64 oracle's own out
    got = float(r["learn"][3])
    err = abs(got - ref["dbeta"]) / sumabs
    bound = H.TAIL_F32_BOUND if dtype == F32 else BF16_BOUND[("readout", "dbias")]
    print(f"LSPFIG oracle {str(dtype).split('.')[-1]} {case} dbeta {got:.6e} ref {ref['dbeta']:.6e} err {err:.3e}")
    assert err < bound, f"{err:.3e} against {bound:.1e}"
    assert rel(r["out"], ref["out"]) < (H.TAIL_F32_BOUND if dtype == F32 else BF16_BOUND[("readout", "out")])


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("case", CASES[::4])
def test_dbeta_is_bit_reproducible(L, dtype, case):
    """the same backward a second time: no atomics on the way to dbeta, so the same bits — in the product build too"""
    r = _run(L, dtype, case)
    assert torch.equal(r["learn"][3], r["again"][3])


SWEEP_BZ = (-120.0, -60.0, -30.0, -17.0, -5.0, 0.0, 5.0, 10.0, 15.0, 18.0, 19.5, 20.5, 25.0)


@pytest.mark.parametrize("beta", S.BETAS)
def test_single_element_sweep(L, beta):
    """n_out = B = T = 1 and zero weights: z is the bias.  Every value finite; dbeta exactly 0 where out underflowed to 0; per
    element within the own-out bound of the float64 formula."""
    Cin = 16
    t = dict(x=torch.randn(1, 1, Cin, device=dev()), w=torch.zeros(1, Cin, device=dev()), drop_mask=None)
    dout = torch.ones(1, 1, 1, device=dev())
    beta_dev = torch.tensor(beta, dtype=torch.float32, device=dev())
    zero_seen = False
    for bz in SWEEP_BZ:
        t["bias"] = torch.tensor([bz / float(np.float32(beta))], dtype=torch.float32, device=dev())
        a = _args(L, F32, 1, 1, Cin, 1, 1, beta, t, beta_dev)
        out, _ = _forward(L, a, 1, 1, 1)
        _, _, dbias, dbeta = _backward(L, a, F32, (1, 1, Cin), 1, Cin, dout, True)
        o, g = float(out), float(dbeta)
        ref, sumabs = _own_out_reference(out, dout, beta)
        print(f"LSPFIG sweep beta {beta} bz {bz} out {o:.6e} dbeta {g:.6e} ref {ref:.6e}")
        assert math.isfinite(o) and math.isfinite(g) and math.isfinite(float(dbias)), (bz, o, g)
        if o == 0.0:
            zero_seen = True
            assert g == 0.0, (bz, g)
        else:
            assert abs(g - ref) <= DBETA_OWN_OUT_BOUND * sumabs, (bz, g, ref)
    assert zero_seen            # beta z = -120 is below the underflow of out for every beta here


@pytest.mark.parametrize("form", ["beta", "log"])
def test_compact_backward(form):
    """ReadoutFn.backward on the active rows only (ctx.active): no row -> exactly 0; a subset -> the dense result on dout zeroed
    elsewhere (own-out bound); every row -> the dense path itself, bit for bit."""
    from sensorium_amd.dwiseneuro import Readout
    torch.manual_seed(3)
    B, T, Cin, n = 3, 5, 32, 65
    ro = Readout(Cin, n, groups=2, softplus_beta=0.07, drop_rate=0.0, learnable_softplus=True, softplus_param=form).to(dev()).train()
    with torch.no_grad():
        ro.layer[1].weight.mul_(2.0 / 0.07)
        ro.layer[1].bias.mul_(2.0 / 0.07)
    x = torch.randn(B, T, Cin, device=dev())
    dout = torch.randn(B, n, T, device=dev())
    leaf = next(ro.gate.parameters())

    def grads(active, gout):
        ro._dwn_active = active
        for p in ro.parameters():
            p.grad = None
        xin = x.clone().requires_grad_()
        out = ro(xin)
        out.backward(gout)
        ro._dwn_active = None
        return out.detach(), leaf.grad.clone(), xin.grad.clone(), ro.layer[1].weight.grad.clone()

    one = dout.clone()
    one[0] = 0
    one[2] = 0
    out, g_dense, dx_dense, dw_dense = grads(None, one)
    _, g_sub, dx_sub, dw_sub = grads(torch.tensor([1], device=dev()), one)
    ref, sumabs = _own_out_reference(out, one, 0.07)
    scale = 0.07 if form == "log" else 1.0                     # d/d log(beta) = beta d/d beta
    for g in (g_dense, g_sub):
        assert abs(float(g) - ref * scale) <= DBETA_OWN_OUT_BOUND * sumabs * scale, (float(g), ref * scale)
    assert rel(dx_sub, dx_dense) < H.TAIL_F32_BOUND and rel(dw_sub, dw_dense) < H.TAIL_F32_BOUND
    assert not bool(dx_sub[0].any()) and not bool(dx_sub[2].any())
    _, g_none, dx_none, _ = grads(torch.empty(0, dtype=torch.int64, device=dev()), torch.zeros_like(dout))
    assert float(g_none) == 0.0 and not bool(dx_none.any())
    _, g_all0, dx_all0, dw_all0 = grads(None, dout)
    _, g_all1, dx_all1, dw_all1 = grads(torch.arange(B, device=dev()), dout)
    assert torch.equal(g_all0, g_all1) and torch.equal(dx_all0, dx_all1) and torch.equal(dw_all0, dw_all1)
    assert float(g_all0) != 0.0

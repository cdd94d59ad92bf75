"""dwn_dw_spatial_fwd / dwn_dw_spatial_bwd with ks = 3 through the C-ABI on every dispatch path, element by element (reference,
bounds, restated dispatch and case lists: tests/dws3_reference.py, itself checked by tests/test_dws3_reference_cpu.py; the table
of paths: DESIGN.md 12s).

  exact   integer operands (SiLU = identity to the last bit): y2, dh1, dW and all four sums equal float64 BIT FOR BIT.
  random  Gaussian operands: |got - ref| <= the per-element bound on EVERY element of y2, dh1 and dW; the statistics within their
          bound of the float64 sums of the values the kernel stored.

Outputs are pre-filled with NaN and must come back finite; dW and the statistics are zeroed as the header asks.  Each test prints
`DWS3 <id> max_ratio ...` before it asserts.  Default library only: the ordered build's spatial kernels keep their existing tests
(tests/test_gpu_dws_ks_det.py, test_gpu_determinism.py)."""
import ctypes as C

import pytest
import torch

from tests import dws3_reference as R
from tests.gpu_helpers import dev, load_desc, read_stats, stats_buffer, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    if lib.DETERMINISTIC:
        pytest.skip("the default library only: the ordered build's spatial kernels keep their existing tests")
    return lib


def _finish(L, rc, what):
    """Check the return code and wait for the kernel.  A device error (not a wrong result) ends the session: after a fault nothing
    further is launched on that device."""
    try:
        L.check(rc, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if rc > 0 or "HIP" in str(e) or "hip" in str(e):
            pytest.exit(f"{what}: device error, stopping: {e}", returncode=3)
        raise


def _report(cid, **kw):
    print("DWS3", cid, " ".join(f"{k}={v:.4e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()), flush=True)


def _nan(rows, cols, dtype):
    return torch.full((rows, cols), float("nan"), device=dev()).to(dtype)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _rebuilt(a, o):
    c = o.case
    if c.cin:
        a.a0 = o.a0.data_ptr(); a.a0_ld = c.cin + c.ld_pad; a.w1 = o.w1.data_ptr(); a.Cin = c.cin


def fwd_args(L, o, y2, st):
    c = o.case
    a = L.DwSpatialFwdArgs()
    d = L.LoadDesc()
    d.p = None if c.cin else o.y1.data_ptr()
    d.ld = c.C + c.ld_pad; d.rows_per_sample = 1; d.v1 = o.scale.data_ptr(); d.v2 = o.shift.data_ptr(); d.act = 1
    a.inp = d
    a.w = o.w.data_ptr(); a.out = y2.data_ptr(); a.planes = c.planes; a.Hin = c.Hin; a.Win = c.Win; a.Hout = o.Hout; a.Wout = o.Wout
    a.C = c.C; a.stride = c.stride; a.ks = 3; a.stats = _ptr(st); a.rows_band = c.rows_band; a.impl = c.impl
    _rebuilt(a, o)
    return a


def bwd_args(L, o, dh1, dw, st):
    c = o.case
    a = L.DwSpatialBwdArgs()
    a.dy = load_desc(L, o.dh2, c.C + c.ld_pad, q=o.y2in, v1=o.A1, v2=o.A2, v3=o.A3)
    y = L.LoadDesc()
    y.p = None if c.cin else o.y1.data_ptr()
    y.ld = c.C + c.ld_pad; y.rows_per_sample = 1
    y.v1 = o.scale.data_ptr(); y.v2 = o.shift.data_ptr(); y.v3 = o.mean.data_ptr(); y.v4 = o.invstd.data_ptr()
    a.y1 = y
    a.w = o.w.data_ptr(); a.dh1 = dh1.data_ptr(); a.dw = dw.data_ptr(); a.planes = c.planes; a.Hin = c.Hin; a.Win = c.Win
    a.Hout = o.Hout; a.Wout = o.Wout; a.C = c.C; a.stride = c.stride; a.ks = 3; a.stats = _ptr(st); a.rows_band = c.rows_band
    a.impl = c.impl
    _rebuilt(a, o)
    return a


def run_fwd(L, o):
    c = o.case
    y2 = _nan(o.Mout, c.C, R.DT[c.dtype])
    st = stats_buffer(c.C)
    a = fwd_args(L, o, y2, st)
    _finish(L, L.lib.dwn_dw_spatial_fwd(C.byref(a), L.DWN_BF16 if c.dtype == "bf16" else L.DWN_F32, dev().index, stream()),
            "dwn_dw_spatial_fwd")
    return y2, read_stats(st, c.C)


def run_bwd(L, o):
    c = o.case
    dh1 = _nan(o.Min, c.C, R.DT[c.dtype])
    dw = torch.zeros(c.C, 9, device=dev())
    st = stats_buffer(c.C)
    a = bwd_args(L, o, dh1, dw, st)
    _finish(L, L.lib.dwn_dw_spatial_bwd(C.byref(a), L.DWN_BF16 if c.dtype == "bf16" else L.DWN_F32, dev().index, stream()),
            "dwn_dw_spatial_bwd")
    return dh1, dw, read_stats(st, c.C)


FWD_RANDOM = [c for c in R.RANDOM_CASES if c.direction == "fwd"]
BWD_RANDOM = [c for c in R.RANDOM_CASES if c.direction == "bwd"]
FWD_EXACT = [c for c in R.EXACT_CASES if c.direction == "fwd"]
BWD_EXACT = [c for c in R.EXACT_CASES if c.direction == "bwd"]


@pytest.mark.parametrize("case", FWD_RANDOM, ids=R.case_id)
def test_fwd_paths(L, case):
    o = R.make_operands(case, dev())
    ref, bound = R.forward_reference(o)
    y2, (s0, s1) = run_fwd(L, o)
    ry, oy = R.max_ratio(y2, ref, bound)
    (r0, r1), (b0, b1) = R.forward_stats(o, y2)
    rs0, os0 = R.max_ratio(s0, r0, b0)
    rs1, os1 = R.max_ratio(s1, r1, b1)
    _report(R.case_id(case), max_ratio_y2=ry, over_y2=oy, max_ratio_sum=rs0, max_ratio_sumsq=rs1)
    assert not torch.isnan(y2.float()).any(), "an output element was not written"
    assert oy == 0, ("y2", ry, oy)
    assert os0 == 0 and os1 == 0, ("statistics", rs0, rs1)


@pytest.mark.parametrize("case", BWD_RANDOM, ids=R.case_id)
def test_bwd_paths(L, case):
    o = R.make_operands(case, dev())
    b = R.backward_reference(o)
    dh1, dw, (s0, s1) = run_bwd(L, o)
    rd, od = R.max_ratio(dh1, b["dh1"], b["dh1_bound"])
    rw, ow = R.max_ratio(dw, b["dW"], b["dW_bound"])
    (r0, r1), (b0, b1) = R.backward_stats(o, dh1, b["yhat"])
    rs0, os0 = R.max_ratio(s0, r0, b0)
    rs1, os1 = R.max_ratio(s1, r1, b1)
    _report(R.case_id(case), max_ratio_dh1=rd, over_dh1=od, max_ratio_dW=rw, max_ratio_sum=rs0, max_ratio_sum_yhat=rs1)
    assert not torch.isnan(dh1.float()).any(), "an output element was not written"
    assert od == 0, ("dh1", rd, od)
    assert ow == 0, ("dW", rw, ow)
    assert os0 == 0 and os1 == 0, ("statistics", rs0, rs1)


def _neq(got, ref):
    return int((got.double() != ref).sum())


@pytest.mark.parametrize("case", FWD_EXACT, ids=R.case_id)
def test_fwd_exact(L, case):
    o = R.make_operands(case, dev(), "exact")
    ref = R.exact_reference(o)
    y2, (s0, s1) = run_fwd(L, o)
    ny, n0, n1 = _neq(y2, ref["y2"]), _neq(s0, ref["st_fwd"][0]), _neq(s1, ref["st_fwd"][1])
    _report("x-" + R.case_id(case), differing_y2=ny, differing_sum=n0, differing_sumsq=n1)
    assert ny == 0, "y2"
    assert n0 == 0 and n1 == 0, "BatchNorm-2 sums"


@pytest.mark.parametrize("case", BWD_EXACT, ids=R.case_id)
def test_bwd_exact(L, case):
    o = R.make_operands(case, dev(), "exact")
    ref = R.exact_reference(o)
    dh1, dw, (s0, s1) = run_bwd(L, o)
    nd, nw = _neq(dh1, ref["dh1"]), _neq(dw, ref["dW"])
    n0, n1 = _neq(s0, ref["st_bwd"][0]), _neq(s1, ref["st_bwd"][1])
    _report("x-" + R.case_id(case), differing_dh1=nd, differing_dW=nw, differing_sum=n0, differing_sum_yhat=n1)
    assert nd == 0, "dh1"
    assert nw == 0, "dW"
    assert n0 == 0 and n1 == 0, "BatchNorm-1 backward sums"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
REFUSALS = [
    # case, return code, message fragment
    (R.Case("fwd", "f32", 1, 4, 4, 12, 1, 0, 0, 0, 0, True, "refuse"), -2, b"multiple of 8"),
    (R.Case("bwd", "bf16", 1, 4, 4, 12, 1, 0, 0, 0, 0, True, "refuse"), -2, b"multiple of 8"),
    (R.Case("fwd", "f32", 1, 1, 2048, 8, 1, 0, 0, 0, 0, True, "refuse"), -5, b"too wide for the LDS tile"),
    (R.Case("fwd", "bf16", 1, 1, 2048, 8, 1, 1, 0, 0, 0, True, "refuse"), -5, b"too wide for the LDS tile"),
    (R.Case("bwd", "f32", 1, 1, 2048, 8, 1, 0, 0, 0, 0, True, "refuse"), -5, b"too wide for the LDS tile"),
    (R.Case("bwd", "bf16", 1, 1, 2048, 8, 1, 1, 0, 0, 0, True, "refuse"), -5, b"too wide for the LDS tile"),
    (R.Case("fwd", "bf16", 2, 9, 11, 64, 1, 0, 0, 64, 0, True, "refuse"), -3, b"a0 != NULL"),          # a width the walk refuses
    (R.Case("bwd", "bf16", 2, 9, 11, 64, 1, 0, 0, 64, 0, True, "refuse"), -3, b"a0 != NULL"),
    (R.Case("fwd", "f32", 2, 9, 16, 64, 1, 0, 0, 64, 0, True, "refuse"), -3, b"a0 != NULL"),           # fp32 storage
    (R.Case("bwd", "bf16", 2, 9, 16, 72, 1, 0, 0, 64, 0, True, "refuse"), -3, b"rebuilt-y1 mode needs"),    # a ragged channel slice
    (R.Case("fwd", "bf16", 2, 9, 16, 72, 1, 0, 0, 64, 0, True, "refuse"), -3, b"rebuilt-input mode needs"),
]


@pytest.mark.parametrize("case,code,fragment", REFUSALS, ids=[f"{c.direction}-{c.dtype}-{c.Win}x{c.C}-cin{c.cin}-i{c.impl}" for c, _, _ in REFUSALS])
def test_refusals(L, case, code, fragment):
    """A shape a path cannot honour is refused before anything is enqueued: return code, message, outputs untouched."""
    assert R.case_dispatch(case) == ("refuse", code)
    o = R.make_operands(case, dev())
    dt = L.DWN_BF16 if case.dtype == "bf16" else L.DWN_F32
    st = stats_buffer(case.C)
    if case.cin:
        sup = L.lib.dwn_dw_spatial_fwd_rc_supported if case.direction == "fwd" else L.lib.dwn_dw_spatial_bwd_rc_supported
    if case.direction == "fwd":
        out = [_nan(o.Mout, case.C, R.DT[case.dtype])]
        a = fwd_args(L, o, out[0], st)
        if case.cin:
            assert sup(C.byref(a), dt) == 0
        rc = L.lib.dwn_dw_spatial_fwd(C.byref(a), dt, dev().index, stream())
    else:
        out = [_nan(o.Min, case.C, R.DT[case.dtype]), torch.zeros(case.C, 9, device=dev())]
        a = bwd_args(L, o, out[0], out[1], st)
        if case.cin:
            assert sup(C.byref(a), dt) == 0
        rc = L.lib.dwn_dw_spatial_bwd(C.byref(a), dt, dev().index, stream())
    msg = L.lib.dwn_last_error()
    torch.cuda.synchronize()
    assert rc == code, (rc, msg)
    assert fragment in msg, msg
    assert bool(torch.isnan(out[0].float()).all()), "a refused call wrote its output"
    assert all(not bool(t.any()) for t in out[1:] + [st]), "a refused call wrote dW or the statistics"

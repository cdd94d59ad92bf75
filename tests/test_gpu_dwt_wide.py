"""temp_covn_dw at kernel sizes 7 and 9, at kernel level: the depth-wise (k,1,1) convolution along T over SiLU(BatchNorm-2(y2)) and its
backward (reference ops src/models/dwiseneuro.py:105-111) through the C-ABI entries dwn_dw_temporal_wide_fwd / dwn_dw_temporal_wide_bwd,
against the float64 reference of the same operation (tests/dw_reference.py, pinned at these sizes to torch's conv3d by
tests/test_temporal_kernel_cpu.py) — both sizes, both storage types, the one loader of the output gradient that is built
(DWN_LD_PLAIN: y3 recomputed from a ring of z2, the form the block backward runs), at the frame counts, channel counts and position
counts where the prologue, the unrolled batches, the rolling look-ahead loads, the ragged channel slice and the persistent grid
change behaviour.  The method, the operands (Case) and the checks (_check_backward) are those of tests/test_gpu_dwt.py.

Bounds take that file's forms: element-wise outputs against the ROUNDING FLOOR OF THE SAME CASE, floor = rel_l2(ref.to(dtype), ref):
err <= M_BF16 * floor + F32_L2 (bf16), err <= F32_L2 (fp32).  Every constant carries the worst case measured on the MI355X over the
shapes of this file and the margin tests/test_gpu_dwt.py gave its own (2x on the fp32 figure, +25 % on the bf16 floor ratio, 1.5x on
dW and on the (b) bound); none was fitted to anything else, and each stays under the ceiling named beside it (table: DESIGN.md
section 12f)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import sensorium_amd._lib as L  # noqa: E402
from tests.dw_reference import _dwt, dw_temporal_fwd_f64, rel_l2  # noqa: E402
from tests.gpu_helpers import dev, load_desc, read_stats, stats_buffer, stream  # noqa: E402
from tests.test_gpu_dwt import STATS, Case, _check_backward, _floor, _report, _stats_match_stored  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32

# ---- bounds (see the module docstring) ------------------------------------------------------------------------------------------
# fp32, y3 / z3 / dh2 against float64: 2x the worst case measured (1.067e-7: dh2 against (a), (3, 11, 9, 8) kt 9, v2 big; forward y3
# 8.23e-8 at (1, 10, 1, 64) kt 9, z3 1.01e-7 at (2, 16, 144, 192) kt 9); ceiling 2e-6.  In bf16 the same fp32 arithmetic error is the
# epsilon beside the floor.
F32_L2 = 2.14e-7
# bf16, y3 / z3 / dh2 (reference (a)) as a multiple of the case's own rounding floor: worst measured ratio 1.0002 (dh2, (3, 11, 9, 200)
# kt 7, v2 big; y3 1.0000, z3 1.0001) + 25 %; ceiling 1.5
M_BF16 = 1.25
# bf16 dh2 against reference (b) (y3 not rounded), |v2| <= 0.1: the extra term is the bf16 rounding of y3 times v2.  Worst measured
# 1.8425e-3 ((3, 11, 9, 8) kt 9, 1.006 floors of that case) x 1.5; ceiling 3.5e-3
BWD_B_L2 = 2.77e-3
# dW against float64, 1.5x the worst case; ceiling 2e-3.  Against (a): 6.75e-6 (bf16, (3, 11, 9, 200) kt 7, v2 of order 1: the
# float64-against-fp32 rounding ties of y3; fp32 1.2e-7).  Against (b): 1.073e-4 (bf16, (1, 10, 1, 64) kt 7: 10 products per tap)
BWD_DW, BWD_DW_B = 1.02e-5, 1.61e-4
# statistics against float64 sums of the kernel's own stored values: STATS of tests/test_gpu_dwt.py (1e-4); worst measured here 5.0e-6
CEILINGS = dict(F32_L2=2e-6, M_BF16=1.5, BWD_B_L2=3.5e-3, BWD_DW=2e-3, BWD_DW_B=2e-3, STATS=1e-4)


def test_constants_stay_under_their_ceilings():
    assert F32_L2 <= CEILINGS["F32_L2"] and M_BF16 <= CEILINGS["M_BF16"] and BWD_B_L2 <= CEILINGS["BWD_B_L2"]
    assert BWD_DW <= CEILINGS["BWD_DW"] and BWD_DW_B <= CEILINGS["BWD_DW_B"] and STATS <= CEILINGS["STATS"]


def _l2_bound(dtype, floor):
    return M_BF16 * floor + F32_L2 if dtype == BF else F32_L2


class WideCase(Case):
    """tests/test_gpu_dwt.py::Case (same draws) launched through the entries of sizes 7 and 9."""

    def forward(self):
        Cc = self.C
        y3 = torch.full((self.M, Cc), float("nan"), device=dev()).to(self.dtype)
        st = stats_buffer(Cc)
        a = L.DwTemporalFwdArgs()
        a.inp = load_desc(L, self.y2, Cc, v1=self.c2(0), v2=self.c2(1), act=1)
        a.w = self.w.data_ptr(); a.out = y3.data_ptr(); a.B = self.B; a.T = self.T; a.HW = self.HW; a.C = Cc; a.kt = self.kt
        a.stats = st.data_ptr()
        L.check(L.lib.dwn_dw_temporal_wide_fwd(C.byref(a), self.dt, dev().index, stream()), "dwn_dw_temporal_wide_fwd")
        torch.cuda.synchronize()
        return y3, st.view(32, 2, Cc).sum(0)

    def backward(self, kind=L.LD_PLAIN, y3=None):
        Cc = self.C
        dh2 = torch.full((self.M, Cc), float("nan"), device=dev()).to(self.dtype)
        dw = torch.zeros(Cc, self.kt, device=dev())
        st = stats_buffer(Cc)
        a = self.bwd_args(kind, y3, dh2, dw, st)
        L.check(L.lib.dwn_dw_temporal_wide_bwd(C.byref(a), self.dt, dev().index, stream()), "dwn_dw_temporal_wide_bwd")
        torch.cuda.synchronize()
        return dh2, dw, st.view(32, 2, Cc).sum(0)


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
# T below, at and just over P (3 / 4), 2P (6 / 8), kt (7 / 9), kt + 1, 2 kt -+ 1 (13, 15 / 17, 19) of both sizes, and 32: the prologue
# (j < T), the first batch that starts before frame 0, the break in the last unrolled batch, the clamped look-ahead loads
T_EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 15, 17, 19, 32)
SHAPES = (
    [(2, T, 35, 72) for T in T_EDGES]
    # channel counts that end a slice raggedly (a slice is 64 bf16 / 32 fp32 channels) and whole slices
    + [(3, 11, 9, Cc) for Cc in (8, 24, 40, 200, 64, 128, 448)]
    # B * HW below one workgroup's positions (16 bf16 / 32 fp32), off their multiples, and more than one stride of the persistent grid
    # with pos / HW crossing sample boundaries inside a wave
    + [(1, 10, 1, 64), (3, 10, 3, 40), (1, 10, 131, 64), (7, 10, 40, 72), (3, 9, 576, 72)]
    # one production geometry per block width (blocks 0-3, 4-6, 7-8 of the benchmarked model)
    + [(2, 32, 576, 448), (2, 32, 144, 896), (4, 32, 40, 1792)]
)
_dtype_kt = [pytest.param(dt, kt, id=f"{str(dt)[6:]}-kt{kt}") for dt in (BF, F32) for kt in (7, 9)]


def _sid(s):
    return "x".join(map(str, s))


@pytest.mark.parametrize("dtype,kt", _dtype_kt)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_forward_against_float64(shape, dtype, kt):
    """Training-mode forward: raw y3 against float64, and the BatchNorm-3 statistics against the sums of the values as stored."""
    c = WideCase(*shape, kt, dtype)
    y3, st = c.forward()
    ref = dw_temporal_fwd_f64(c.y2, c.c2(0), c.c2(1), c.w, c.B, c.T, c.HW)
    floor = _floor(ref, dtype)
    e = rel_l2(y3, ref)
    mine = torch.stack([y3.double().sum(0), (y3.double() ** 2).sum(0)])
    es = _stats_match_stored(st, mine)
    _report("fwd", dtype=str(dtype)[6:], kt=kt, shape=shape, y3=e, floor=floor, stats=es)
    assert not torch.isnan(y3.float()).any(), "y3 not fully written"
    assert e <= _l2_bound(dtype, floor), (e, floor)
    assert es < STATS, es


@pytest.mark.parametrize("v2", ["big", "small"])
@pytest.mark.parametrize("dtype,kt", _dtype_kt)
@pytest.mark.parametrize("shape", SHAPES, ids=_sid)
def test_backward_against_float64(shape, dtype, kt, v2):
    """dw_temporal_bwd_wide_kernel.  Reference (a) rounds the recomputed y3 to the storage type, the kernel's stated contract; reference
    (b) does not — the operation proper — and is asked for at |v2| <= 0.1 only, where the difference (v2 times the bf16 rounding of y3)
    is what training sees.  dh2, dW and both BatchNorm-2 backward sums; dh2 is pre-filled with NaN and none may remain."""
    c = WideCase(*shape, kt, dtype, v2=v2)
    out = c.backward()
    ref_a = c.reference_bwd(c.dy3_plain(dtype))
    _check_backward(c, out, ref_a, f"wide-a-{v2}", l2_bound=_l2_bound(dtype, _floor(ref_a[0], dtype)), dw_bound=BWD_DW)
    if v2 == "small":
        _check_backward(c, out, c.reference_bwd(c.dy3_plain(None)), "wide-b-small", l2_bound=BWD_B_L2 if dtype == BF else F32_L2,
                        dw_bound=BWD_DW_B)


@pytest.mark.parametrize("dtype,kt", _dtype_kt)
@pytest.mark.parametrize("B,T,HW,Cc", [(3, 8, 40, 64), (2, 6, 35, 24), (2, 16, 144, 192)])
def test_forward_eval_epilogue(dtype, kt, B, T, HW, Cc):
    """z_scale / z_shift / pooled as tests/test_gpu_dwt_eval.py checks them at 3 and 5: z3 = SiLU(BN3(y3)) of the y3 a plain launch
    stores, the pooling sums those of the stored z3 and the same from launch to launch, z3 against float64 at the floor bound."""
    c = WideCase(B, T, HW, Cc, kt, dtype)
    coef3 = c.coef3
    M = c.M

    def run():
        out = torch.full((M, Cc), float("nan"), device=dev()).to(dtype)
        pooled = torch.zeros(B, Cc, dtype=torch.int64, device=dev())      # 64-bit fixed point, units of 2^-32 (include/dwn.h)
        a = L.DwTemporalFwdArgs()
        a.inp = load_desc(L, c.y2, Cc, v1=c.c2(0), v2=c.c2(1), act=1)
        a.w = c.w.data_ptr(); a.out = out.data_ptr(); a.B = B; a.T = T; a.HW = HW; a.C = Cc; a.kt = kt
        a.z_scale = coef3.data_ptr(); a.z_shift = coef3[Cc:].data_ptr(); a.pooled = pooled.data_ptr()
        L.check(L.lib.dwn_dw_temporal_wide_fwd(C.byref(a), c.dt, dev().index, stream()), "dwn_dw_temporal_wide_fwd")
        torch.cuda.synchronize()
        return out, pooled

    y3, _ = c.forward()
    z3, pooled_fix = run()
    _, again = run()
    assert torch.equal(pooled_fix, again), "integer pooling sums must not depend on the arrival order"
    pooled = pooled_fix.double() / 2.0 ** 32
    h = y3.float() * coef3[:Cc] + coef3[Cc:]
    want = (h * torch.sigmoid(h)).to(dtype)
    tol = 2e-2 if dtype == BF else 2e-6
    assert not torch.isnan(z3.float()).any()
    assert float((z3.float() - want.float()).abs().max() / want.float().abs().max()) < tol
    want_pool = z3.double().view(B, T * HW, Cc).sum(1)           # sums of the values as stored
    assert float((pooled - want_pool).abs().max() / want_pool.abs().max()) < 1e-5
    h64 = dw_temporal_fwd_f64(c.y2, c.c2(0), c.c2(1), c.w, B, T, HW).to(dtype).double() * coef3[:Cc].double() + coef3[Cc:].double()
    ref = h64 * torch.sigmoid(h64)
    floor, e = rel_l2(ref.to(dtype), ref), rel_l2(z3, ref)
    _report("eval-z3", dtype=str(dtype)[6:], kt=kt, shape=(B, T, HW, Cc), z3=e, floor=floor)
    assert e <= _l2_bound(dtype, floor), (e, floor)
    # statistics and the eval epilogue exclude each other
    a = L.DwTemporalFwdArgs()
    a.inp = load_desc(L, c.y2, Cc, v1=c.c2(0), v2=c.c2(1), act=1)
    a.w = c.w.data_ptr(); a.out = z3.data_ptr(); a.B = B; a.T = T; a.HW = HW; a.C = Cc; a.kt = kt
    a.z_scale = coef3.data_ptr()
    assert L.lib.dwn_dw_temporal_wide_fwd(C.byref(a), c.dt, dev().index, stream()) < 0


# ---- exact integers ---------------------------------------------------------------------------------------------------------------
def _exact_case(Bn, Tn, HW, E, kt, dtype):
    """tests/test_gpu_fullsize.py::_exact_temporal_case for 7 and 9 with operands small enough that dW and every sum are exact too.

    y2 in {0, 1}, BatchNorm-2 the map y + 17 (fp32 sigmoid(17) == 1: z2 = h in {17, 18}, SiLU' = 1), taps 0 / +-1 with two +1 and two -1
    (kt 7) or three +1 and two -1 (kt 9) per channel at random places, dh3 in {-1, 0, 1}, dy3 = dh3 + y3.  At kt 9, the wider case:
    y3 in [-36, 54], dy3 in [-37, 55], and dh2 = sum of three dy3 minus two dy3 lies in [-3 * 37 - 2 * 55, 3 * 55 + 2 * 37] =
    [-221, 239]: integers below 256, which bf16 holds.  A term of dW is at most 18 * 55 = 990 and a channel has B * T * HW = 5120 of
    them: every partial sum, in whatever order the lanes, waves and workgroups add, is an integer below 5.1e6 < 2^24; the same
    holds for sum y3 (2.8e5),
    sum y3^2 (1.5e7), sum dh2 and sum dh2 * y2 (1.3e6)."""
    d, s = dev(), stream()
    dt = L.DWN_BF16 if dtype == BF else L.DWN_F32
    g = torch.Generator(device="cuda").manual_seed(HW + E + kt)
    M = Bn * Tn * HW
    assert Bn * Tn * HW * 990 < 2 ** 24 and Bn * Tn * HW * 54 * 54 < 2 ** 24
    npos, nneg = (3, 2) if kt == 9 else (2, 2)
    y2 = torch.randint(0, 2, (M, E), generator=g, device=d, dtype=torch.int8).to(dtype)
    order = torch.rand(E, kt, generator=g, device=d).argsort(1)
    taps = torch.zeros(E, kt, device=d)
    taps.scatter_(1, order[:, :npos], 1.0)
    taps.scatter_(1, order[:, npos:npos + nneg], -1.0)
    assert bool(((taps != 0).sum(1) == npos + nneg).all())
    taps = taps.t().contiguous()                                                                           # [kt][E]
    dh3 = torch.randint(-1, 2, (M, E), generator=g, device=d, dtype=torch.int8).to(dtype)
    ones, zeros = torch.ones(E, device=d), torch.zeros(E, device=d)
    shift = torch.full((E,), 17.0, device=d)
    h = (y2.double().view(Bn, Tn, HW, E) + 17.0).requires_grad_(True)
    wd = taps.double().clone().requires_grad_(True)
    y3_ref = _dwt(h, wd)
    y3_ref.backward(dh3.double().view(Bn, Tn, HW, E) + y3_ref.detach())
    y3_ref = y3_ref.detach().reshape(M, E)
    dh2_ref = h.grad.reshape(M, E)
    dw_ref = wd.grad.t().contiguous()                                                                      # [E][kt]
    del h
    assert float(y3_ref.abs().max()) <= 54 and float(dh2_ref.abs().max()) <= 239 and float(dw_ref.abs().max()) < 2 ** 24
    # ---- forward
    y3 = torch.full((M, E), float("nan"), dtype=dtype, device=d)
    st = stats_buffer(E)
    f = L.DwTemporalFwdArgs()
    f.inp = load_desc(L, y2, E, v1=ones, v2=shift, act=1)
    f.w = taps.data_ptr(); f.out = y3.data_ptr(); f.B = Bn; f.T = Tn; f.HW = HW; f.C = E; f.kt = kt; f.stats = st.data_ptr()
    L.check(L.lib.dwn_dw_temporal_wide_fwd(C.byref(f), dt, 0, s), "dwn_dw_temporal_wide_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y3.double(), y3_ref), "y3"
    s0, s1 = read_stats(st, E)
    assert torch.equal(s0, y3_ref.sum(0)), "sum y3"
    assert torch.equal(s1, (y3_ref ** 2).sum(0)), "sum y3^2"
    del y3
    # ---- backward
    dh2 = torch.full((M, E), float("nan"), dtype=dtype, device=d)
    dw = torch.zeros(E, kt, device=d)
    st = stats_buffer(E)
    b = L.DwTemporalBwdArgs()
    b.dy = load_desc(L, dh3, E, v1=ones, v2=ones, v3=zeros); b.dy_kind = L.LD_PLAIN
    b.y2 = load_desc(L, y2, E, v1=ones, v2=shift, v3=zeros, v4=ones)                    # mean 0, invstd 1: yhat2 = y2
    b.w = taps.data_ptr(); b.dh2 = dh2.data_ptr(); b.dw = dw.data_ptr()
    b.B = Bn; b.T = Tn; b.HW = HW; b.C = E; b.kt = kt; b.stats = st.data_ptr()
    L.check(L.lib.dwn_dw_temporal_wide_bwd(C.byref(b), dt, 0, s), "dwn_dw_temporal_wide_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dh2.double(), dh2_ref), "dh2"
    assert torch.equal(dw.double(), dw_ref), "dW"
    s0, s1 = read_stats(st, E)
    assert torch.equal(s0, dh2_ref.sum(0)), "sum dh2"
    assert torch.equal(s1, (dh2_ref * y2.double()).sum(0)), "sum dh2 * y2"


@pytest.mark.parametrize("dtype,kt", _dtype_kt)
def test_exact_integers(dtype, kt):
    _exact_case(4, 32, 40, 448, kt, dtype)


def test_backward_repeated_launches_are_identical():
    """50 launches of the backward on the same data at a production geometry (bf16, kt 9), dh2 bit-identical every time (the weight
    gradient and the sums are atomics: order-dependent in the last bits, not compared).  A launch that fails ends the test."""
    c = WideCase(2, 32, 144, 896, 9, BF, seed=7)
    first, _, _ = c.backward()
    assert not torch.isnan(first.float()).any()
    again = torch.empty_like(first)
    dw = torch.zeros(c.C, c.kt, device=dev())
    st = stats_buffer(c.C)
    a = c.bwd_args(L.LD_PLAIN, None, again, dw, st)
    bad = torch.zeros((), dtype=torch.int64, device=dev())
    for _ in range(50):
        again.fill_(float("nan"))
        rc = L.lib.dwn_dw_temporal_wide_bwd(C.byref(a), c.dt, dev().index, stream())
        assert rc == 0, (rc, L.lib.dwn_last_error())
        bad += (again.view(torch.int16) != first.view(torch.int16)).sum()
    torch.cuda.synchronize()
    assert int(bad) == 0


def test_argument_errors():
    """kt outside {7, 9} -> -4, C not a multiple of 8 -> -2, any loader but DWN_LD_PLAIN -> -3; nothing is launched."""
    c = WideCase(2, 6, 9, 64, 7, BF)
    dh2 = torch.zeros(c.M, c.C, dtype=BF, device=dev())
    dw = torch.zeros(c.C, 16, device=dev())
    st = stats_buffer(c.C)
    for dt in (L.DWN_BF16, L.DWN_F32):
        for kt in (0, 1, 3, 4, 5, 8, 11):
            a = c.bwd_args(L.LD_PLAIN, dh2, dh2, dw, st); a.kt = kt
            assert L.lib.dwn_dw_temporal_wide_bwd(C.byref(a), dt, dev().index, stream()) == -4
        for kt in (7, 9):
            a = c.bwd_args(L.LD_PLAIN, dh2, dh2, dw, st); a.kt = kt; a.C = 12
            assert L.lib.dwn_dw_temporal_wide_bwd(C.byref(a), dt, dev().index, stream()) == -2
            for kind in (L.LD_AFFINE2, L.LD_DY3, L.LD_PE, L.LD_BNACT, L.LD_GATE, 99, -1):
                a = c.bwd_args(kind if kind in (L.LD_AFFINE2, L.LD_DY3) else L.LD_PLAIN, dh2, dh2, dw, st); a.kt = kt; a.dy_kind = kind
                assert L.lib.dwn_dw_temporal_wide_bwd(C.byref(a), dt, dev().index, stream()) == -3
        f = L.DwTemporalFwdArgs()
        f.inp = load_desc(L, c.y2, c.C, v1=c.c2(0), v2=c.c2(1), act=1)
        f.w = c.w.data_ptr(); f.out = dh2.data_ptr(); f.B = c.B; f.T = c.T; f.HW = c.HW; f.C = c.C; f.stats = st.data_ptr()
        for kt in (0, 1, 3, 4, 5, 8, 11):
            f.kt = kt
            assert L.lib.dwn_dw_temporal_wide_fwd(C.byref(f), dt, dev().index, stream()) == -4
        f.kt = 9; f.C = 12
        assert L.lib.dwn_dw_temporal_wide_fwd(C.byref(f), dt, dev().index, stream()) == -2
    torch.cuda.synchronize()
    assert not dh2.float().any() and not dw.any() and not st.any()

"""spat_covn_dw with kernel sizes 5 and 7 at kernel level: the depth-wise (1,k,k) convolution over SiLU(BatchNorm-1(y1)) and its
backward (reference ops src/models/dwiseneuro.py:96-102), through the C-ABI entries dwn_dw_spatial_fwd / dwn_dw_spatial_bwd,
against a float64 reference written here with torch.nn.functional.conv2d and its autograd (the form of tests/dw_reference.py's
dw_spatial_fwd_f64 / dw_spatial_bwd_f64, which are 3x3 only).

Shapes are the smallest at which these kernels can go wrong: planes smaller than the halo, odd extents at stride 2, ragged and whole
channel slices, forced band heights whose seams fall inside the halo, more planes than the resident grid, one production geometry
per stride, and one stride-3 case for the generic-stride instantiation.  Outputs are pre-filled with NaN, dW and the statistics
zeroed.

Bounds, in the form of tests/test_gpu_dwt.py.  Element-wise outputs (y2, dh1) are judged against the ROUNDING FLOOR OF THE SAME
CASE, floor = rel_l2(ref.to(dtype), ref), computed from the reference alone; dW and the sums against float64.  In bf16 both
kernels keep their LDS tile in bf16 (the activated input forward, the staged gradient backward: the reference's autocast stores
both in bf16 too), so an output carries two independent bf16 roundings: sqrt(2) floors are expected, not one.  Every constant
carries the worst value measured on the MI355X and its margin (table in DESIGN.md section 12e) and stays under the ceiling named
beside it."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import sensorium_amd._lib as L  # noqa: E402
from tests.dw_reference import rel_l2  # noqa: E402
from tests.gpu_helpers import dev, load_desc, read_stats, stream  # noqa: E402

BF, F32 = torch.bfloat16, torch.float32

# ---- bounds (see the module docstring; measurements: DESIGN.md section 12e) ---------------------------------------------------------
# Worst values measured on the MI355X over every case of this file (the figures each test prints before it asserts):
#   fp32  y2 1.36e-7 ((3, 36, 64, 64) stride 2, k 7, rows_band 3)   dh1 1.31e-7 ((3, 18, 32, 64) stride 1, k 7, rows_band 3)
#   bf16  y2 1.4293 floors, dh1 1.4268 floors (both (3, 36, 64, 64) stride 2, k 7, rows_band 3); largest absolute 2.38e-3 / 2.41e-3
#         ((37, 1, 1, 72) stride 1, k 5: one-pixel planes, whose floor is 1.7e-3)
#   dW    bf16 1.70e-3 ((37, 1, 1, 72) stride 1, k 5: 37 products per channel, each of two bf16-rounded factors; 3.2e-4 at most on
#         every plane of more than a few pixels), fp32 1.08e-7
#   statistics  forward 6.7e-7, backward 2.15e-6
# fp32, y2 and dh1 against float64: 2x the worst measured; ceiling 2e-6 (tests/test_gpu_dwt.py / test_gpu_dwt_eval.py)
F32_L2 = 2.8e-7
# bf16, y2 and dh1: multiple of the case's own floor.  Two independent bf16 roundings (tile, output) predict sqrt(2) = 1.414; worst
# measured 1.4293 + 25 %; and never above the 3.5e-3 that tests/test_gpu_dwfwd.py (FWD_L2) and tests/test_gpu_dwbwd.py (BWD_L2) grant
# one bf16 stencil pass
M_BF16 = 1.79
BF16_L2_CEILING = 3.5e-3
# dW against float64.  bf16: the ceiling itself, 2e-3 (BWD_DW of tests/test_gpu_dwbwd.py) = 1.18x the worst measured, which is the
# one-pixel case above and does not depend on summation order beyond 1e-7.  fp32: 3x the worst measured (the order of the float
# atomics changes from run to run)
BWD_DW_BF16, BWD_DW_F32 = 2e-3, 3.3e-7
# statistics against float64 sums of the kernel's own stored values (the form of tests/test_gpu_dwbwd.py, _check_bwd, whose
# figure 1e-4 is the ceiling): 4.6x the worst measured
STATS = 1e-5


def _report(what, **kw):
    """One line per figure, printed before anything is asserted (pytest -s or a failure shows them)."""
    print("DWSKS", what, " ".join(f"{k}={v:.4e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()), flush=True)


# ---- float64 reference ------------------------------------------------------------------------------------------------------------
def _conv(z, w, stride, ks):
    """z [P, H, W, C] float64, w [ks*ks, C] tap-major (dy * ks + dx) -> [P, Hout, Wout, C]; zero padding ks // 2."""
    Cc = z.shape[3]
    wt = w.t().reshape(Cc, 1, ks, ks)
    out = torch.nn.functional.conv2d(z.permute(0, 3, 1, 2), wt, stride=stride, padding=ks // 2, groups=Cc)
    return out.permute(0, 2, 3, 1)


def dw_spatial_ks_fwd_f64(y1, scale, shift, w, planes, Hin, Win, stride, ks):
    """y1 [planes*Hin*Win, C] -> y2 [planes*Hout*Wout, C] (float64): dwS * SiLU(scale * y1 + shift)."""
    Cc = y1.shape[1]
    h = y1.double().view(planes, Hin, Win, Cc) * scale.double() + shift.double()
    return _conv(h * torch.sigmoid(h), w.double(), stride, ks).reshape(-1, Cc)


def dw_spatial_ks_bwd_f64(y1, scale, shift, mean, invstd, g, w, planes, Hin, Win, stride, ks):
    """Backward of the above for the output gradient g [planes*Hout*Wout, C]: (dh1 [rows, C], dW [C, ks*ks], sum dh1 [C],
    sum dh1 * yhat1 [C]) in float64, yhat1 = (y1 - mean) * invstd."""
    Cc = y1.shape[1]
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    y1 = y1.double()
    h = (y1.view(planes, Hin, Win, Cc) * scale.double() + shift.double()).requires_grad_(True)
    wd = w.double().clone().requires_grad_(True)
    _conv(h * torch.sigmoid(h), wd, stride, ks).backward(g.double().view(planes, Hout, Wout, Cc))
    dh1 = h.grad.reshape(-1, Cc)
    yhat = (y1 - mean.double()) * invstd.double()
    return dh1, wd.grad.t().contiguous(), dh1.sum(0), (dh1 * yhat).sum(0)


# ---- operands and launches ----------------------------------------------------------------------------------------------------------
class Case:
    """Seeded random operands of one (planes, Hin, Win, C, stride, ks, dtype) case."""

    def __init__(self, planes, Hin, Win, Cc, stride, ks, dtype, seed=0):
        d = dev()
        g = torch.Generator(device=d); g.manual_seed(1000 * seed + 131 * Hin + 17 * Win + Cc + 7 * ks + stride + planes)
        self.planes, self.Hin, self.Win, self.C, self.stride, self.ks, self.dtype = planes, Hin, Win, Cc, stride, ks, dtype
        self.Hout, self.Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
        self.Min, self.Mout = planes * Hin * Win, planes * self.Hout * self.Wout
        self.dt = L.DWN_BF16 if dtype == BF else L.DWN_F32

        def randn(*s):
            return torch.randn(*s, device=d, generator=g)

        def rand(*s):
            return torch.rand(*s, device=d, generator=g)

        self.y1 = randn(self.Min, Cc).to(dtype)
        self.dh2 = randn(self.Mout, Cc).to(dtype)
        self.y2in = randn(self.Mout, Cc).to(dtype)
        self.coef = torch.cat([rand(Cc) + 0.5, randn(Cc) * 0.3, randn(Cc) * 0.2, rand(Cc) + 0.5])     # BN1 scale, shift, mean, invstd
        self.abc = randn(3 * Cc) * 0.5                                                                # BN2-backward A1, A2, A3
        self.w = randn(ks * ks, Cc) / ks                                                              # [k*k][C], fp32

    def c1(self, i):
        return self.coef[i * self.C:(i + 1) * self.C]

    def v(self, i):
        return self.abc[i * self.C:(i + 1) * self.C]

    def fwd_args(self, y2, st, rows_band=0):
        a = L.DwSpatialFwdArgs()
        a.inp = load_desc(L, self.y1, self.C, v1=self.c1(0), v2=self.c1(1), act=1)
        a.w = self.w.data_ptr(); a.out = y2.data_ptr(); a.planes = self.planes; a.Hin = self.Hin; a.Win = self.Win
        a.Hout = self.Hout; a.Wout = self.Wout; a.C = self.C; a.stride = self.stride; a.ks = self.ks
        a.stats = st.data_ptr(); a.rows_band = rows_band
        return a

    def forward(self, rows_band=0):
        """-> (y2 as stored, (sum, sum of squares) float64)"""
        y2 = torch.full((self.Mout, self.C), float("nan"), device=dev()).to(self.dtype)
        st = torch.zeros(32 * 2 * self.C, dtype=torch.float64, device=dev())
        a = self.fwd_args(y2, st, rows_band)
        L.check(L.lib.dwn_dw_spatial_fwd(C.byref(a), self.dt, dev().index, stream()), "dwn_dw_spatial_fwd")
        torch.cuda.synchronize()
        return y2, read_stats(st, self.C)

    def bwd_args(self, dh1, dw, st, rows_band=0):
        a = L.DwSpatialBwdArgs()
        a.dy = load_desc(L, self.dh2, self.C, q=self.y2in, v1=self.v(0), v2=self.v(1), v3=self.v(2))
        a.y1 = load_desc(L, self.y1, self.C, v1=self.c1(0), v2=self.c1(1), v3=self.c1(2), v4=self.c1(3))
        a.w = self.w.data_ptr(); a.dh1 = dh1.data_ptr(); a.dw = dw.data_ptr(); a.planes = self.planes; a.Hin = self.Hin
        a.Win = self.Win; a.Hout = self.Hout; a.Wout = self.Wout; a.C = self.C; a.stride = self.stride; a.ks = self.ks
        a.stats = st.data_ptr(); a.rows_band = rows_band
        return a

    def backward(self, rows_band=0):
        """-> (dh1 as stored, dW [C][k*k], (sum dh1, sum dh1 * yhat1) float64)"""
        dh1 = torch.full((self.Min, self.C), float("nan"), device=dev()).to(self.dtype)
        dw = torch.zeros(self.C, self.ks * self.ks, device=dev())
        st = torch.zeros(32 * 2 * self.C, dtype=torch.float64, device=dev())
        a = self.bwd_args(dh1, dw, st, rows_band)
        L.check(L.lib.dwn_dw_spatial_bwd(C.byref(a), self.dt, dev().index, stream()), "dwn_dw_spatial_bwd")
        torch.cuda.synchronize()
        return dh1, dw, read_stats(st, self.C)

    def reference(self):
        """float64 (y2, dh1, dW, yhat1) from the operands as the kernels get them; computed once per case."""
        if not hasattr(self, "_ref"):
            g = self.v(0).double() * self.dh2.double() + self.v(1).double() * self.y2in.double() + self.v(2).double()
            y2 = dw_spatial_ks_fwd_f64(self.y1, self.c1(0), self.c1(1), self.w, self.planes, self.Hin, self.Win, self.stride, self.ks)
            dh1, dw, _, _ = dw_spatial_ks_bwd_f64(self.y1, self.c1(0), self.c1(1), self.c1(2), self.c1(3), g, self.w, self.planes,
                                                  self.Hin, self.Win, self.stride, self.ks)
            yhat = (self.y1.double() - self.c1(2).double()) * self.c1(3).double()
            self._ref = (y2, dh1, dw, yhat)
        return self._ref


def _floor(ref, dtype):
    return rel_l2(ref.to(dtype), ref)


def _stats_err(st, mine):
    st, mine = torch.stack(list(st)), torch.stack(list(mine))
    return float(((st - mine).abs() / (mine.abs() + 1e-2 * mine.abs().mean())).max())


def _check(case, rows_band=0, tag=""):
    y2_ref, dh1_ref, dw_ref, yhat = case.reference()
    dtype = case.dtype
    y2, st_f = case.forward(rows_band)
    dh1, dw, st_b = case.backward(rows_band)
    fy, fd = _floor(y2_ref, dtype), _floor(dh1_ref, dtype)
    ey, ed, ew = rel_l2(y2, y2_ref), rel_l2(dh1, dh1_ref), rel_l2(dw, dw_ref)
    sf = _stats_err(st_f, (y2.double().sum(0), (y2.double() ** 2).sum(0)))
    sb = _stats_err(st_b, (dh1.double().sum(0), (dh1.double() * yhat).sum(0)))
    _report(tag or "case", geom=(case.planes, case.Hin, case.Win, case.C, case.stride), ks=case.ks,
            dtype=str(dtype).split(".")[1], rows_band=rows_band, y2=ey, y2_floor=fy, y2_ratio=ey / max(fy, 1e-30), dh1=ed,
            dh1_floor=fd, dh1_ratio=ed / max(fd, 1e-30), dW=ew, stats_fwd=sf, stats_bwd=sb)
    assert not torch.isnan(y2.float()).any() and not torch.isnan(dh1.float()).any()
    if dtype == BF:
        assert ey <= M_BF16 * fy + F32_L2 and ey <= BF16_L2_CEILING, ("y2", ey, fy)
        assert ed <= M_BF16 * fd + F32_L2 and ed <= BF16_L2_CEILING, ("dh1", ed, fd)
        assert ew <= BWD_DW_BF16, ("dW", ew)
    else:
        assert ey <= F32_L2, ("y2", ey)
        assert ed <= F32_L2, ("dh1", ed)
        assert ew <= BWD_DW_F32, ("dW", ew)
    assert sf < STATS, ("forward statistics", sf)
    assert sb < STATS, ("backward statistics", sb)


KS_DT = [(5, BF), (5, F32), (7, BF), (7, F32)]
KS_DT_IDS = ["k5-bf16", "k5-fp32", "k7-bf16", "k7-fp32"]

GEOMS = (
    # planes, Hin, Win, C, stride
    # planes smaller than the halo, both strides (ragged channel slice; 37 planes so that the centre taps sum over tens of pixels)
    [(37, h, w, 72, s) for (h, w) in ((1, 1), (1, 2), (2, 3), (3, 8)) for s in (1, 2)]
    # odd extents at stride 2 (ragged 200 / whole 64), and the first of them at stride 1
    + [(3, 9, 11, 200, 2), (3, 7, 5, 64, 2), (2, 9, 11, 72, 1)]
    # more planes than the resident grid: the persistent loop wraps
    + [(130, 9, 16, 448, 1), (130, 9, 16, 448, 2)]
    # one production geometry per stride (blocks 0 and 1 of the benchmarked model)
    + [(4, 36, 64, 448, 2), (4, 18, 32, 448, 1)]
    # the generic-stride instantiation
    + [(3, 10, 13, 72, 3)]
)


@pytest.mark.parametrize("ks,dtype", KS_DT, ids=KS_DT_IDS)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_forward_and_backward_match_float64(geom, ks, dtype):
    _check(Case(*geom, ks, dtype), tag="geom")


@pytest.mark.parametrize("ks,dtype", KS_DT, ids=KS_DT_IDS)
@pytest.mark.parametrize("stride", [1, 2])
def test_forced_bands(stride, ks, dtype):
    """Band heights 1, 2, 3 and the library's choice: every seam falls inside the halo of its neighbours."""
    H, W = (18, 32) if stride == 1 else (36, 64)
    case = Case(3, H, W, 64, stride, ks, dtype, seed=1)
    for rows_band in (1, 2, 3, 0):
        _check(case, rows_band=rows_band, tag="bands")


# The library's own band plan (rows_band = 0) at stride 1 on planes of 28 columns that need several bands and whose height the
# largest band that fits does not divide, so that the even split lowers the band.  Worked by hand from the launchers' rule (tile
# bytes ((rb - 1) + k) * (28 + 2P) * 128 forward against 48 KB; ((rb + 2P) + rb) * (28 + 2P) * 128 backward against 79 KB less the
# static weight and sum tables, (k * k + 6) * 64 or 32 channels * 4 bytes).  Hin: largest band -> band x bands
#   k 5  25: forward 8 -> 7 x 4 (both types), backward bf16 6 -> 5 x 5 (fp32: 7 x 4 as it is)    22: backward fp32 7 -> 6 x 4
#   k 7  16: forward 5 -> 4 x 4 (both types), backward fp32 5 -> 4 x 4 (bf16: 4 x 4 as it is)     9: backward bf16 4 -> 3 x 3
AUTO_HIN = {5: (25, 22), 7: (16, 9)}


@pytest.mark.parametrize("ks,dtype", KS_DT, ids=KS_DT_IDS)
def test_automatic_bands(ks, dtype):
    for Hin in AUTO_HIN[ks]:
        _check(Case(2, Hin, 28, 72, 1, ks, dtype, seed=3), tag="auto_bands")


# ---- exact cases: small integers that bf16 holds, as tests/test_gpu_fullsize.py builds its 3x3 stencil cases -------------------------
#   y1 integers 0 .. 16, BatchNorm-1 scale 1, shift 17  ->  h >= 17, where the fp32 SiLU is the identity to the last bit bf16 keeps
#   and SiLU' = 1  ->  z1 = h in 17 .. 33; three non-zero taps of +-1 per channel  ->  |y2| <= 99; g = dh2 in {-1, 0, 1}
#   (A1 = 1, A2 = A3 = 0)  ->  |dh1| <= 3.  Stencil sums, dW and the sums must EQUAL float64 arithmetic on the same integers.
def _exact_operands(planes, Hin, Win, E, stride, ks):
    d = dev()
    g = torch.Generator(device=d).manual_seed(planes + Hin + E + stride + ks)
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    kk = ks * ks
    y1 = torch.randint(0, 17, (planes * Hin * Win, E), generator=g, device=d).to(BF)
    taps = torch.zeros(E, kk, device=d)
    taps.scatter_(1, torch.rand(E, kk, generator=g, device=d).argsort(1)[:, :3], 1.0)
    taps = (taps * (torch.randint(0, 2, (E, kk), generator=g, device=d) * 2 - 1)).t().contiguous()       # [k*k][E], +-1 / 0
    dh2 = torch.randint(-1, 2, (planes * Hout * Wout, E), generator=g, device=d).to(BF)
    return y1, taps, dh2, Hout, Wout


EXACT = [(5, 1), (5, 2), (7, 1), (7, 2)]


@pytest.mark.parametrize("ks,stride", EXACT)
def test_forward_exact_integers(ks, stride):
    planes, Hin, Win, E = 5, 9, 16, 72
    y1, taps, _, Hout, Wout = _exact_operands(planes, Hin, Win, E, stride, ks)
    d = dev()
    ones, shift = torch.ones(E, device=d), torch.full((E,), 17.0, device=d)
    h = y1.double().view(planes, Hin, Win, E) + 17.0
    y2_ref = _conv(h, taps.double(), stride, ks).reshape(-1, E)
    y2 = torch.full((planes * Hout * Wout, E), float("nan"), dtype=BF, device=d)
    st = torch.zeros(32 * 2 * E, dtype=torch.float64, device=d)
    f = L.DwSpatialFwdArgs()
    f.inp = load_desc(L, y1, E, v1=ones, v2=shift, act=1)
    f.w = taps.data_ptr(); f.out = y2.data_ptr(); f.planes = planes; f.Hin = Hin; f.Win = Win; f.Hout = Hout; f.Wout = Wout
    f.C = E; f.stride = stride; f.ks = ks; f.stats = st.data_ptr()
    L.check(L.lib.dwn_dw_spatial_fwd(C.byref(f), L.DWN_BF16, d.index, stream()), "dwn_dw_spatial_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y2.double(), y2_ref), "y2"
    s0, s1 = read_stats(st, E)
    assert torch.equal(s0, y2_ref.sum(0)), "sum y2"                 # integers below 2^24 in every partial sum
    assert torch.equal(s1, (y2_ref ** 2).sum(0)), "sum y2^2"         # 720 outputs * 99^2 < 2^24


@pytest.mark.parametrize("ks,stride", EXACT)
def test_backward_exact_integers(ks, stride):
    planes, Hin, Win, E = 5, 9, 16, 72
    y1, taps, dh2, Hout, Wout = _exact_operands(planes, Hin, Win, E, stride, ks)
    d = dev()
    ones, zeros, shift = torch.ones(E, device=d), torch.zeros(E, device=d), torch.full((E,), 17.0, device=d)
    h = (y1.double().view(planes, Hin, Win, E) + 17.0).requires_grad_(True)
    wd = taps.double().clone().requires_grad_(True)
    _conv(h, wd, stride, ks).backward(dh2.double().view(planes, Hout, Wout, E))
    dh1_ref, dw_ref = h.grad.reshape(-1, E), wd.grad.t().contiguous()
    dh1 = torch.full((planes * Hin * Win, E), float("nan"), dtype=BF, device=d)
    dw = torch.zeros(E, ks * ks, device=d)
    st = torch.zeros(32 * 2 * E, dtype=torch.float64, device=d)
    y2in = torch.zeros(planes * Hout * Wout, E, dtype=BF, device=d)                                      # weighted with A2 = 0
    b = L.DwSpatialBwdArgs()
    b.dy = load_desc(L, dh2, E, q=y2in, v1=ones, v2=zeros, v3=zeros)
    b.y1 = load_desc(L, y1, E, v1=ones, v2=shift, v3=zeros, v4=ones)                                    # mean 0, invstd 1: yhat1 = y1
    b.w = taps.data_ptr(); b.dh1 = dh1.data_ptr(); b.dw = dw.data_ptr(); b.planes = planes; b.Hin = Hin; b.Win = Win
    b.Hout = Hout; b.Wout = Wout; b.C = E; b.stride = stride; b.ks = ks; b.stats = st.data_ptr()
    L.check(L.lib.dwn_dw_spatial_bwd(C.byref(b), L.DWN_BF16, d.index, stream()), "dwn_dw_spatial_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dh1.double(), dh1_ref), "dh1"
    assert torch.equal(dw.double(), dw_ref), "dW"
    s0, s1 = read_stats(st, E)
    assert torch.equal(s0, dh1_ref.sum(0)) and torch.equal(s1, (dh1_ref * y1.double()).sum(0)), "BatchNorm-1 backward sums"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_unbuilt_sizes_and_rebuilt_mode_are_refused():
    case = Case(2, 9, 16, 64, 1, 5, BF)
    y2 = torch.empty(case.Mout, 64, dtype=BF, device=dev())
    dh1 = torch.empty(case.Min, 64, dtype=BF, device=dev())
    dw = torch.zeros(64, 81, device=dev())
    st = torch.zeros(32 * 2 * 64, dtype=torch.float64, device=dev())
    a0 = torch.zeros(case.Min, 64, dtype=BF, device=dev())
    w1 = torch.zeros(64, 64, dtype=BF, device=dev())
    for ks in (4, 9):
        f, b = case.fwd_args(y2, st), case.bwd_args(dh1, dw, st)
        f.ks = b.ks = ks
        for rc in (L.lib.dwn_dw_spatial_fwd(C.byref(f), L.DWN_BF16, 0, stream()),
                   L.lib.dwn_dw_spatial_bwd(C.byref(b), L.DWN_BF16, 0, stream())):
            assert rc == -4
            assert b"3, 5 or 7" in L.lib.dwn_last_error()
    # rebuilt-input / rebuilt-y1 mode is built into the 3x3 row-walk kernels only: the message that says so stays
    f, b = case.fwd_args(y2, st), case.bwd_args(dh1, dw, st)
    for a in (f, b):
        a.a0 = a0.data_ptr(); a.a0_ld = 64; a.w1 = w1.data_ptr(); a.Cin = 64
    assert L.lib.dwn_dw_spatial_fwd_rc_supported(C.byref(f), L.DWN_BF16) == 0
    assert L.lib.dwn_dw_spatial_bwd_rc_supported(C.byref(b), L.DWN_BF16) == 0
    assert L.lib.dwn_dw_spatial_fwd(C.byref(f), L.DWN_BF16, 0, stream()) == -3
    assert b"a0 != NULL" in L.lib.dwn_last_error()
    assert L.lib.dwn_dw_spatial_bwd(C.byref(b), L.DWN_BF16, 0, stream()) == -3
    assert b"a0 != NULL" in L.lib.dwn_last_error()
    torch.cuda.synchronize()


# ---- repeated launches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [5, 7])
def test_repeated_launches_are_bit_identical(ks):
    """50 launches of each direction at (9, 16), 130 planes (the persistent loop wraps): the bf16 outputs must not depend on which
    workgroup computed which tile or on the order of anything."""
    for stride in (1, 2):
        case = Case(130, 9, 16, 448, stride, ks, BF, seed=2)
        y2_0, _ = case.forward()
        dh1_0, _, _ = case.backward()
        for _ in range(49):
            y2, _ = case.forward()
            dh1, _, _ = case.backward()
            assert torch.equal(y2.view(torch.int16), y2_0.view(torch.int16)), "y2 differs between launches"
            assert torch.equal(dh1.view(torch.int16), dh1_0.view(torch.int16)), "dh1 differs between launches"

"""float64 reference, per-element error bounds, restated dispatch and case lists of the 3x3 spatial depth-wise kernels
(dwn_dw_spatial_fwd / dwn_dw_spatial_bwd with ks = 3; reference ops src/models/dwiseneuro.py:90-102) for the kernel-level tests
tests/test_gpu_dws3_paths.py (device) and tests/test_dws3_reference_cpu.py (the checker itself).  Values come from
tests/dw_reference.py's arithmetic (padded-slice sums; pinned to it and through it to the oracle by the CPU test); this module adds
the MAGNITUDE sums the bounds need.  Plain torch, on whatever device the operands live on.  Test infrastructure only.

Notation.  u = 2^-24 (fp32 unit roundoff).  u_out = unit roundoff of the stored output (2^-8 bf16, 2^-24 fp32).  u_tile = the same
for the LDS tile (the bf16 kernels keep z1 forward and g backward in bf16; the fp32 kernels keep fp32: u_tile = 0).  u_w = 2^-8 on
the bf16 paths when the weights handed in are not bf16-representable (the dot2 kernels round w with pk_bf16; a path that does not
round still satisfies an upper bound), else 0.  Every constant below is derived here; none is fitted to a kernel's output.

Activation (csrc/dwn_common.h sigmoidf_ / sigmoid2f_ / silu_gradf_), input pixel by input pixel:
  h   = fma(scale, y1, shift): one rounding,            e_h <= u (|scale y1| + |shift|)
        rebuilt forms: y1 is an fp32 matrix-core sum of Cin products,  + |scale| 2 Cin u SY,  SY = sum_k |a0_k||w1_k|
        (the factor 2 for the matrix cores' accumulate rounding as tests/gemm_reference.py grants it)
  t   = h * (-log2 e): the constant is rounded (u) and so is the product (u): |dt| <= 2u|t|, which moves e = exp2(t) = exp(-h)
        relatively by ln2 |dt| = 2u|h|  (the issue's sketch has |h| ln2 u for the product alone; the rounded constant doubles it
        and ln2 log2e = 1)
  e   : v_exp_f32, 1 ulp <= 2u relative;   D = 1 + e: one rounding u, and e's relative error enters D scaled by e/D = 1 - sig
  sig : v_rcp_f32, 1 ulp <= 2u;            rho = relative error of sig <= u ((1 - sig)(2|h| + 2) + 3)
  z   = h * sig: one rounding;             e_z <= 1.1 e_h + u |z| ((1 - sig)(2|h| + 2) + 4)        (max |SiLU'| = 1.0998 < 1.1)
  d   = SiLU'(h) = sig (1 + h (1 - sig)), silu_gradf_: two more roundings on top of sig's (1 - sig, then the fma / product):
        e_d <= 0.5 e_h + |d| (rho + 2u) + sig |h| (sig rho + 2u (1 - sig))                          (max |SiLU''| = 0.5)
  g   = A1 dh2 + (A2 y2 + A3): three roundings, each of a quantity bounded by the magnitude sum:
        e_g <= 3u (|A1 dh2| + |A2 y2| + |A3|)
A bf16 operand COMPUTED by the kernel in fp32 (x^ = x + e) may round to the other neighbour than the float64 value x does.  No
"flip" constant is needed:  |rd(x^) - x| <= |rd(x^) - x^| + |x^ - x| <= u_tile |x^| + e <= u_tile |x| + (1 + u_tile) e, because
u_tile is the FULL unit roundoff of whatever value is rounded, not half an ulp around the float64 value's midpoint.  So a tile
operand carries  u_tile |x| + e_t,  e_t = (1 + u_tile) e.  The stored output is treated the same way: u_out (|ref| + E) + E.

Bounds (S = sum_t |w_t||z_t|, SG = sum_t |w_t||g_t|, G = sum_t w_t g_t, nine terms per stencil output: 9 products and 9 sums,
18 roundings of at most the magnitude sum, which also covers the two-products-per-step order of the dot2 kernels):
  forward  E = ((1 + u_tile)(1 + u_w) - 1 + 18u) S + sum_t |w_t| e_t          bound = u_out (|ref| + E) + E
  dh1      EG = ((1 + u_tile)(1 + u_w) - 1 + 18u) SG + sum_t |w_t| e_gt
           E = |d| EG + (|G| + EG) e_d + u |ref|                                  bound = u_out (|ref| + E) + E
  dW       (fp32 accumulators and float atomics; n = number of contributing outputs, any order, factor 2 as above)
           u |ref| + ((1 + u_tile)^2 - 1 + 2 n u) SW + sum (|g| e_z + |z| e_g)(1 + u_tile)^2,   SW = sum |g||z|
           (the last sum is this module's addition to the issue's sketch: z and g are computed in fp32 before they are rounded
           to the tile, and for fp32 storage, u_tile = 0, it is the only term that accounts for the activation at all)
  rebuilt  e_h gains |scale| 2 Cin u SY as above (through 1.1 e_h this is the issue's 1.1 |scale| 2 Cin u SY).

Statistics (the 32-replica float64 buffer).  EVERY path sums the values AS STORED (after pk_bf16 / the fp32 store; read from the
kernels: chain forward `finish`, pair and generic forward after V4::pack, every backward kernel "statistics of the values as
stored"), so the float64 reference is formed from the kernel's own output.  The fp32 partial sums that precede the float64 atomics
run per thread over every tile the thread's workgroup takes, then through the wave fold and the LDS atomics of the workgroup; how
many workgroups share a column is an occupancy query's answer, so the longest fp32 chain readable from the code alone is "one
workgroup takes every row": n_partial = rows of the column (an upper bound for any order).  Columns:
  sum v           n u sum |v|                              sum v^2         (n + 1) u sum v^2   (the product is rounded too)
  sum dh1 yhat1   yhat1 = (y1 - mean) invstd is formed as y1 invstd + (-mean invstd) (generic) or the raw sum dh1 y1 is normalised
                  once at the end (row-walk): both are within (n + 3) u |invstd| (sum |dh1 y1| + |mean| sum |dh1|); the rebuilt forms
                  use their own fp32 y1: + |invstd| 2 Cin u sum |dh1| SY.
"""
import collections
import zlib

import torch

from tests.dw_reference import conv_pw_f64

BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "f32": F32}
U32 = 2.0 ** -24
U = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
EXACT_LIMIT = 2.0 ** 24


# ---- dispatch: launch_dw_spatial_fwd / _bwd and what they call, restated -------------------------------------------------------------
def _fwd_walk_supported(dtype, Hin, Win, Hout, Wout, C, stride, impl, ld):
    if impl == 1 or dtype != "bf16" or C % 8:
        return False
    if stride not in (1, 2) or Wout not in (32, 16, 8):
        return False
    if Win != Wout * stride or Hout != (Hin - 1) // stride + 1:
        return False
    return Hin * Win * ld < 2 ** 31


def _bwd_walk_supported(dtype, Hin, Win, Hout, Wout, C, stride, impl, ld):
    if impl == 1 or dtype != "bf16" or C % 8:
        return False
    if stride == 1:
        ok = Win in (32, 16, 8) and Hout == Hin and Wout == Win
    elif stride == 2:
        ok = Win in (64, 32, 16) and Hout == (Hin - 1) // 2 + 1 and Wout == Win // 2
    else:
        return False
    return ok and Hin * Win * ld < 2 ** 31


def _rc_supported(Hin, Win, C, cin, a0_ld):
    return cin in (64, 128) and C % 64 == 0 and a0_ld % 8 == 0 and a0_ld >= cin and Hin * Win * a0_ld < 2 ** 31


def _round_up(rb, built):
    for b in built:
        if rb <= b:
            return b
    return built[-1]


S2_LDS_BUDGET = 50 * 1024          # WK_LDS_BUDGET: three workgroups per CU (rebuilt form: 3/2 of it)


def s2_band(Hin, LPW, cin, rows_band):
    """launch_s2: input rows per band R (even) of the stride-2 backward."""
    row_bytes = (16 // LPW) * (LPW + 1) * 256
    budget = S2_LDS_BUDGET * 3 // 2 if cin else S2_LDS_BUDGET
    R = rows_band
    if R <= 0:
        R = 2
        while R < Hin and ((R + 2) // 2 + 1) * row_bytes <= budget:
            R += 2
        nb = (Hin + R - 1) // R
        R = (Hin + nb - 1) // nb
    R = (R + 1) & ~1
    if R > Hin:
        R = (Hin + 1) & ~1
    return R


def banded_plan(direction, dtype, Hin, Win, stride, rows_band=0):
    """spatial_fwd_t / spatial_bwd_t (the pair and generic kernels): -> (greedy band, None for a given rows_band; band; bands per
    plane; LDS tile bytes).  Bands are output rows forward, input rows backward."""
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    if direction == "fwd":
        pair = dtype == "bf16" and stride in (1, 2)
        Wp = Win + 2
        rows, budget = Hout, (80 if stride >= 2 else 48) * 1024

        def tile_bytes(rb):
            return ((rb - 1) * stride + 3) * ((Wp + 1) // 2) * 256 if pair else ((rb - 1) * stride + 3) * Wp * 128
    else:
        pair = dtype == "bf16" and stride == 1
        Wq = Wout + 2
        row_bytes = ((Wq + 1) // 2) * 256 if pair else Wq * 128
        rows, budget = Hin, 44 * 1024

        def tile_bytes(rb):
            return ((rb - 1 + 2) // stride + 2) * row_bytes
    greedy, rb = None, rows_band
    if rb <= 0:
        rb = 1
        while rb < rows and tile_bytes(rb + 1) <= budget:
            rb += 1
        greedy = rb
        nb = (rows + rb - 1) // rb
        rb = (rows + nb - 1) // nb
    rb = min(rb, rows)
    return greedy, rb, (rows + rb - 1) // rb, tile_bytes(rb)


def dws3_dispatch(direction, dtype, planes, Hin, Win, C, stride, impl=0, rows_band=0, cin=0, ld=None):
    """-> (path name, template parameters) of the kernel dwn_dw_spatial_fwd / _bwd launches for ks = 3, or ("refuse", code).
    ld = in.ld (forward) / dy.ld = y1.ld (backward), default C; the rebuilt forms' a0_ld is cin + (ld - C)."""
    ld = C if ld is None else ld
    a0_ld = cin + (ld - C)
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    fwd = direction == "fwd"
    walk = (_fwd_walk_supported if fwd else _bwd_walk_supported)(dtype, Hin, Win, Hout, Wout, C, stride, impl, ld)
    if cin and not walk:
        return ("refuse", -3)
    if walk:
        if cin and not _rc_supported(Hin, Win, C, cin, a0_ld):
            return ("refuse", -3)
        if fwd:
            LPW = Wout // 2
            if cin:                                                               # launch_fc_rb, CIN > 0
                rb = rows_band if rows_band > 0 else (4 if stride == 1 else 2)
                RB = _round_up(rb, (4, 8) if stride == 1 else (2, 4))
            else:
                rb = rows_band if rows_band > 0 else ((4 if LPW == 16 else 6) if stride == 1 else (1 if LPW == 4 else 2))
                RB = _round_up(rb, (2, 4, 6, 8) if stride == 1 else (1, 2, 3, 4))
            return ("fwd_chain", (stride, LPW, RB, cin))
        if stride == 1:                                                           # launch_s1c_rb
            LPW = Win // 2
            rb = rows_band if rows_band > 0 else (4 if LPW == 16 else 2)
            return ("bwd_s1c", (LPW, _round_up(rb, (2, 4, 6, 8)), cin))
        LPW = Win // 4                                                            # launch_s2
        R = s2_band(Hin, LPW, cin, rows_band)
        lds = max((R // 2 + 1) * (16 // LPW) * (LPW + 1) * 256 + (64 * cin * 2 if cin > 64 else 0), 9 * 64 * 4)
        if lds > 150 * 1024:
            return ("refuse", -5)
        return ("bwd_s2", (LPW, cin))
    # spatial_fwd_t / spatial_bwd_t
    if C % 8:
        return ("refuse", -2)
    lds = banded_plan(direction, dtype, Hin, Win, stride, rows_band)[3]
    if fwd:
        if lds > 156 * 1024:
            return ("refuse", -5)
        nt = 512 if Hin * Win >= 512 else 256
        if dtype == "bf16" and stride in (1, 2):
            return ("fwd_pair", (stride, nt))
        return ("fwd_generic", (dtype, 3, stride, nt)) if stride in (1, 2) else ("fwd_generic", (dtype, 3, 0, 256))
    if lds > 150 * 1024:
        return ("refuse", -5)
    if dtype == "bf16" and stride == 1:
        return ("bwd_pair", ())
    return ("bwd_generic", (dtype, 3, stride if stride in (1, 2) else 0))


# ---- the persistent grid: dwn_launch.h resident_grid_x, with an upper bound of the workgroups per CU ------------------------------------
DWN_CUS, LDS_PER_CU, WAVES_PER_CU = 256, 160 * 1024, 32


def resident_grid_x(bpc, slices, work, xcd=False):
    gx = max(DWN_CUS * bpc // slices, 1)
    gx = min(gx, max(work, 1))
    if xcd:
        gx = (gx & ~7) if gx >= 8 else 8
    return gx


def grid_bound(c):
    """(a lower bound of the work items of the case's launch, an upper bound of its gridDim.x).  The library asks the runtime how
    many workgroups of the kernel a CU holds; whatever it answers is at most 32 waves per CU / 4 waves per 256-thread workgroup
    and at most 160 KB / the launch's dynamic LDS (FcLds / S1cLds / S2Lds restated; the rebuilt forms' W1 copy and the generic
    kernels' tile are left out, which only raises the bound).  work: plane groups (x bands for s2); planes (x bands >= 1) for the
    pair and generic kernels."""
    path, par = case_dispatch(c)
    lds, threads, xcd = 0, 256, bool(c.cin)
    if path == "fwd_chain":
        st, lpw, rb, cin = par
        ng, npc, rq = 16 // lpw, st * lpw + (2 if cin else 1), (rb + 2 if st == 1 else 2 * rb + 1)
        lds, slices, work = ng * rq * npc * 64 * 4, (c.C + 63) // 64, (c.planes + ng - 1) // ng
    elif path == "bwd_s1c":
        lpw, rb, cin = par
        ng = 16 // lpw
        lds = ng * (rb + 2) * (lpw + 1) * 64 * 4 + (0 if cin else rb * 4096)
        slices, work = (c.C + 63) // 64, (c.planes + ng - 1) // ng
    elif path == "bwd_s2":
        lpw, cin = par
        ng, R = 16 // lpw, s2_band(c.Hin, lpw, cin, c.rows_band)
        lds = (R // 2 + 1) * ng * (lpw + 1) * 256
        slices, work = (c.C + 63) // 64, ((c.planes + ng - 1) // ng) * ((c.Hin + R - 1) // R)
    else:
        cs = 64 if c.dtype == "bf16" else 32
        threads = par[-1] if path in ("fwd_pair", "fwd_generic") else 256
        slices, work, xcd = (c.C + cs - 1) // cs, c.planes, False
    bpc = WAVES_PER_CU * 64 // threads
    if lds:
        bpc = min(bpc, LDS_PER_CU // lds)
    return work, resident_grid_x(max(bpc, 1), slices, work, xcd)


def _built():
    """Every ks = 3 instantiation the launchers can reach, as (path, parameters, storage type), enumerated the way they branch."""
    b = []
    for st in (1, 2):
        for lpw in (16, 8, 4):
            b += [("fwd_chain", (st, lpw, rb, 0), "bf16") for rb in ((2, 4, 6, 8) if st == 1 else (1, 2, 3, 4))]
            b += [("fwd_chain", (st, lpw, rb, cin), "bf16") for rb in ((4, 8) if st == 1 else (2, 4)) for cin in (64, 128)]
        b += [("fwd_pair", (st, nt), "bf16") for nt in (512, 256)]
        b += [("fwd_generic", ("f32", 3, st, nt), "f32") for nt in (512, 256)]
    b += [("fwd_generic", (dt, 3, 0, 256), dt) for dt in ("bf16", "f32")]       # bf16 strides 1, 2 always take the pair kernel
    for lpw in (16, 8, 4):
        b += [("bwd_s1c", (lpw, rb, cin), "bf16") for rb in (2, 4, 6, 8) for cin in (0, 64, 128)]
        b += [("bwd_s2", (lpw, cin), "bf16") for cin in (0, 64, 128)]
    b += [("bwd_pair", (), "bf16")]
    b += [("bwd_generic", ("f32", 3, st), "f32") for st in (1, 2, 0)]
    b += [("bwd_generic", ("bf16", 3, st), "bf16") for st in (2, 0)]           # bf16 stride 1 always takes the pair kernel
    return b


BUILT = _built()
# the statistics of every path sum the values as stored (module docstring); kept as a table so a path that changes shows here
STATS_SUM = {p: "stored" for p in ("fwd_chain", "fwd_pair", "fwd_generic", "bwd_s1c", "bwd_s2", "bwd_pair", "bwd_generic")}
# arithmetic traits of the paths, for the float32 emulation of the room test: tap order and whether w is rounded to bf16
DOT2_PATHS = ("fwd_chain", "fwd_pair", "bwd_s1c", "bwd_s2", "bwd_pair")


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "direction dtype planes Hin Win C stride impl rows_band cin ld_pad wround rule")


def case_dispatch(c):
    return dws3_dispatch(c.direction, c.dtype, c.planes, c.Hin, c.Win, c.C, c.stride, c.impl, c.rows_band, c.cin, c.C + c.ld_pad)


def case_id(c):
    path, par = case_dispatch(c)
    par = "_".join(str(p) for p in par) if isinstance(par, tuple) else str(par)
    return (f"{path}-{par}-{c.dtype}-{c.planes}x{c.Hin}x{c.Win}x{c.C}-s{c.stride}-i{c.impl}-rb{c.rows_band}-cin{c.cin}"
            f"-ld{c.ld_pad}-{'wr' if c.wround else 'wu'}-{c.rule}")


def _hin(stride, Hout, odd):
    return Hout if stride == 1 else (2 * Hout - 1 if odd else 2 * Hout)


def _cases(kind):
    """The case list by rule (issue: "Case lists").  kind = "random" | "exact".  Exact cases keep the Σy2² precondition by using
    one plane where the random case uses three, and leave out the rules that are about operand values (unrounded weights) or whose
    many rows per column cannot keep Σy2² below 2^24 (the wrap and 130-plane cases)."""
    rnd = kind == "random"
    out = []

    def add(direction, dtype, planes, Hin, Win, C, stride, impl=0, rows_band=0, cin=0, ld_pad=0, wround=True, rule=""):
        out.append(Case(direction, dtype, planes, Hin, Win, C, stride, impl, rows_band, cin, ld_pad, wround, rule))

    # -- chained forward, stored and rebuilt input
    for st in (1, 2):
        for wi, Wout in enumerate((32, 16, 8)):
            ng = 16 // (Wout // 2)
            for rb in ((2, 4, 6, 8) if st == 1 else (1, 2, 3, 4)):
                add("fwd", "bf16", ng + 1, _hin(st, 2 * rb + 1, wi == 0), Wout * st, 72, st, rows_band=rb, rule="chain")
            for rb in ((4, 8) if st == 1 else (2, 4)):
                for cin in (64, 128):
                    add("fwd", "bf16", ng + 1, _hin(st, 2 * rb + 1, wi == 0), Wout * st, 64, st, rows_band=rb, cin=cin, rule="chain_rc")
    add("fwd", "bf16", 3, 9, 16, 128, 1, rows_band=4, cin=64, ld_pad=8, rule="chain_rc_ld")
    # -- chained / banded backward
    for wi, Win in enumerate((32, 16, 8)):
        ng = 16 // (Win // 2)
        for rb in (2, 4, 6, 8):
            for cin in (0, 64, 128):
                add("bwd", "bf16", ng + 1, 2 * rb + 1, Win, 64 if cin else 72, 1, rows_band=rb, cin=cin, rule="s1c")
    for wi, Win in enumerate((64, 32, 16)):
        ng = 16 // (Win // 4)
        for cin in (0, 64, 128):
            for bi, band in enumerate((0, 2, 4)):
                add("bwd", "bf16", ng + 1, 9 if (bi + wi) % 2 == 0 else 10, Win, 64 if cin else 72, 2, rows_band=band, cin=cin, rule="s2")
    # -- planes shorter than a chunk, at the library's chunk height, once per LPW and stride
    for st in (1, 2):
        for Wout in (32, 16, 8):
            for Hin in (1, 2):
                for d in ("fwd", "bwd"):
                    add(d, "bf16", 16 // (Wout // 2) + 1, Hin, Wout * st, 72, st, rule="short")
    # -- pair and generic kernels, bf16 and fp32
    P3 = 3 if rnd else 1
    for dt in ("bf16", "f32"):
        for d in ("fwd", "bwd"):
            for st in (1, 2):
                add(d, dt, 3, 7, 16 * st, 72, st, impl=1, rule="impl1")
                for Win in ((11, 24) if st == 1 else (22, 13)):
                    add(d, dt, 3, 7, Win, 72, st, rule="refused_width")
                for hw in ((1, 1), (1, 2), (2, 3)):
                    add(d, dt, 37, hw[0], hw[1], 72, st, rule="tiny")
                for hw in ((16, 32), (9, 16)):
                    add(d, dt, P3, hw[0], hw[1], 72, st, impl=1, rule="nt_512_256")
                for rb in (1, 2, 3):
                    add(d, dt, P3, 18 * st, 32 * st, 72, st, impl=1, rows_band=rb, rule="bands")
            add(d, dt, P3, 10, 13, 72, 3, rule="stride3")
    # -- the library's own band plan (rows_band = 0) on planes that need more than one band, where the even split moves the band off
    # the largest that fits (banded_plan; the CPU test asserts it case by case): fp32 generic at strides 1 and 2, the bf16 pair
    # kernels, the bf16 generic backward at stride 2.  25 rows; the stride-2 backward stages half the rows, so it needs 62 columns
    P2 = 2 if rnd else 1
    for dt in ("f32", "bf16"):
        for st in (1, 2):
            add("fwd", dt, P2, 25, 30, 72, st, impl=1, rule="auto_bands")
            add("bwd", dt, P2, 25, 30 if st == 1 else 62, 72, st, impl=1, rule="auto_bands")
    # -- leading dimensions: one case per kernel family (the rebuilt chain has its own above)
    for st in (1, 2):
        for d in ("fwd", "bwd"):
            add(d, "bf16", 3, 9, 16 * st, 72, st, ld_pad=8, rule="ld")                      # chain / s1c / s2
            add(d, "bf16", 3, 9, 16 * st, 72, st, impl=1, ld_pad=8, rule="ld")              # pair / bf16 generic backward
            add(d, "f32", 3, 9, 16 * st, 72, st, ld_pad=8, rule="ld")                       # generic fp32
        add("bwd", "bf16", 3, 9, 16 * st, 64, st, cin=64, ld_pad=8, rule="ld_rc")
    if rnd:
        # -- the persistent loop takes a second iteration: work > gridDim.x for EVERY occupancy the hardware allows (grid_bound
        # below restates resident_grid_x with the upper bound of workgroups per CU; the CPU test asserts it case by case).  A grid
        # is 256 * bpc / slices wide, so many channel slices and small planes keep the cases cheap; the row-walk kernels at the
        # widest plane and the tallest chunk, whose LDS ring caps bpc at 2 or 3
        add("fwd", "bf16", 55, 3, 32, 896, 1, rows_band=8, rule="wrap")                      # chain, stride 1: bpc <= 3, grid <= 54
        add("fwd", "bf16", 37, 3, 64, 896, 2, rows_band=4, rule="wrap")                      # chain, stride 2: bpc <= 2, grid <= 36
        add("bwd", "bf16", 37, 3, 32, 896, 1, rows_band=8, rule="wrap")                      # s1c: bpc <= 2, grid <= 36
        add("bwd", "bf16", 145, 4, 16, 1792, 2, rows_band=2, rule="wrap")                    # s2: bpc <= 8, grid <= 73, 37 groups x 2 bands
        # -- 130 planes of 9x16 at 448 channels, the shape tests/test_gpu_dws_ks.py wraps its kernels with: here only the fp32 generic
        # kernels (14 slices) are sure to come round; kept beside the derived cases for every family
        for st in (1, 2):
            for d in ("fwd", "bwd"):
                add(d, "bf16", 130, 9, 16, 448, st, rule="planes130")                        # chain / s1c / s2
                add(d, "bf16", 130, 9, 16, 448, st, impl=1, rule="planes130")                # pair / bf16 generic backward
                add(d, "f32", 130, 9, 16, 448, st, rule="planes130")                         # generic fp32
        for st in (1, 2):
            for d in ("fwd", "bwd"):
                add(d, "bf16", 300, 2, 3, 448, st, rule="wrap")                              # pair / bf16 generic backward: grid <= 292
                add(d, "f32", 300, 2, 3, 448, st, rule="wrap")                               # generic fp32: grid <= 146
        # -- unrounded fp32 weights on every bf16 family: u_w in the bound
        for st in (1, 2):
            for d in ("fwd", "bwd"):
                add(d, "bf16", 3, 9, 16 * st, 72, st, wround=False, rule="w_unrounded")
                add(d, "bf16", 3, 9, 16 * st, 72, st, impl=1, wround=False, rule="w_unrounded")
                add(d, "bf16", 3, 9, 16 * st, 64, st, cin=64, wround=False, rule="w_unrounded")
        add("bwd", "bf16", 3, 10, 13, 72, 3, wround=False, rule="w_unrounded")
        add("fwd", "bf16", 3, 10, 13, 72, 3, wround=False, rule="w_unrounded")
    return out


RANDOM_CASES = _cases("random")
EXACT_CASES = _cases("exact")


# ---- operands ------------------------------------------------------------------------------------------------------------------------
class Operands:
    """What one case hands the kernels.  y1 / dh2 / y2in / a0 are [rows, C] views (of a NaN-filled buffer ld_pad columns wider when
    the case has a leading dimension; *_buf is that buffer), w [9, C] fp32 tap-major, coefficient vectors fp32."""
    pass


def _gen(case, kind, device):
    g = torch.Generator(device=device)
    g.manual_seed(zlib.crc32(repr((kind,) + tuple(case[:12])).encode()))
    return g


def _strided(x, pad):
    """x [rows, C] -> (view [rows, C] of a NaN-filled [rows, C + pad] buffer holding x, the buffer)."""
    if not pad:
        return x.contiguous(), None
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=x.dtype, device=x.device)
    buf[:, :x.shape[1]] = x
    return buf[:, :x.shape[1]], buf


def make_operands(case, device, kind="random"):
    c, d = case, device
    g = _gen(case, kind, device)
    dt = DT[c.dtype]
    o = Operands()
    o.case, o.kind = c, kind
    o.Hout, o.Wout = (c.Hin - 1) // c.stride + 1, (c.Win - 1) // c.stride + 1
    o.Min, o.Mout = c.planes * c.Hin * c.Win, c.planes * o.Hout * o.Wout
    Cc = c.C

    def randn(*s):
        return torch.randn(*s, device=d, generator=g)

    def rand(*s):
        return torch.rand(*s, device=d, generator=g)

    def randint(lo, hi, *s):
        return torch.randint(lo, hi + 1, s, device=d, generator=g)

    if kind == "random":
        y1 = randn(o.Min, Cc).to(dt)
        dh2, y2in = randn(o.Mout, Cc).to(dt), randn(o.Mout, Cc).to(dt)
        o.scale, o.shift, o.mean, o.invstd = rand(Cc) + 0.5, randn(Cc) * 0.3, randn(Cc) * 0.2, rand(Cc) + 0.5
        o.A1, o.A2, o.A3 = randn(Cc) * 0.5, randn(Cc) * 0.5, randn(Cc) * 0.5
        o.w = randn(9, Cc) / 3.0
        if c.wround and c.dtype == "bf16":
            o.w = o.w.to(BF16).float()
        a0 = randn(o.Min, c.cin).to(BF16) if c.cin else None
        o.w1 = (randn(Cc, c.cin) / c.cin ** 0.5).to(BF16) if c.cin else None
    else:
        y1 = randint(0, 16, o.Min, Cc).to(dt)
        dh2, y2in = randint(-1, 1, o.Mout, Cc).to(dt), torch.zeros(o.Mout, Cc, dtype=dt, device=d)
        o.scale, o.shift = torch.ones(Cc, device=d), torch.full((Cc,), 17.0, device=d)
        o.mean, o.invstd = torch.zeros(Cc, device=d), torch.ones(Cc, device=d)
        o.A1, o.A2, o.A3 = torch.ones(Cc, device=d), torch.zeros(Cc, device=d), torch.zeros(Cc, device=d)
        order = rand(Cc, 9).argsort(1)
        if c.dtype == "bf16":
            # three non-zero +-1 taps drawn per channel: any permutation of the taps shows in some channel; |y2| <= 99 < 256
            taps = torch.zeros(Cc, 9, device=d)
            taps.scatter_(1, order[:, :3], 1.0)
            taps = taps * (randint(0, 1, Cc, 9) * 2 - 1)
        else:
            # fp32: nine non-zero, distinct integer weights per channel.  -4 .. 4 holds only eight non-zero integers, so the nine
            # are 1 .. 5 and -2 .. -5 (sum 1: keeps the column's sum of squares small), in an order drawn per channel
            vals = torch.tensor([1., 2., 3., 4., 5., -2., -3., -4., -5.], device=d)
            taps = vals[order] * (randint(0, 1, Cc, 1) * 2 - 1)
        o.w = taps.t().contiguous()
        a0 = None
        o.w1 = None
        if c.cin:
            # W1[c, k] = s_k m_ck, m in 0 .. 4, a0[r, k] in {0, s_k} with at most four non-zeros per row: y1 = a0 . W1^T in 0 .. 16
            sk = (randint(0, 1, c.cin) * 2 - 1).float()
            o.w1 = (randint(0, 4, Cc, c.cin).float() * sk).to(BF16)
            pick = torch.zeros(o.Min, c.cin, device=d)
            pick.scatter_(1, rand(o.Min, c.cin).argsort(1)[:, :4], 1.0)
            a0 = (pick * (rand(o.Min, c.cin) < 0.75) * sk).to(BF16)
            y1 = (a0.double() @ o.w1.double().t()).to(dt)           # what a stored y1 would hold (not handed to the kernel)
    o.y1, o.y1_buf = _strided(y1, c.ld_pad)
    o.dh2, o.dh2_buf = _strided(dh2, c.ld_pad)
    o.y2in, o.y2in_buf = _strided(y2in, c.ld_pad)
    o.a0, o.a0_buf = _strided(a0, c.ld_pad) if c.cin else (None, None)
    return o


# ---- float64 arithmetic ---------------------------------------------------------------------------------------------------------------
def _pad(x, mode="zero"):
    """[P, H, W, C] -> [P, H + 2, W + 2, C].  mode "neighbour": the halo COLUMNS repeat the edge column (a mutation)."""
    xp = torch.nn.functional.pad(x, (0, 0, 1, 1, 1, 1))
    if mode == "neighbour":
        xp[:, 1:-1, 0] = x[:, :, 0]
        xp[:, 1:-1, -1] = x[:, :, -1]
    return xp


def _views(xp, stride, Hout, Wout, phase=0):
    for dy in range(3):
        for dx in range(3):
            yield dy * 3 + dx, xp[:, dy + phase:dy + phase + stride * (Hout - 1) + 1:stride, dx + phase:dx + phase + stride * (Wout - 1) + 1:stride, :]


def stencil(x, w, stride, Hout, Wout, pad="zero", phase=0):
    """out[p, ho, wo, c] = sum_t w[t, c] x[p, s ho + dy - 1, s wo + dx - 1, c]  (dw_reference._dw3x3's sum, same tap order)."""
    xp = _pad(x, pad)
    if phase:
        xp = torch.nn.functional.pad(xp, (0, 0, 0, phase, 0, phase))
    out = None
    for t, v in _views(xp, stride, Hout, Wout, phase):
        out = v * w[t] if out is None else out + v * w[t]
    return out


def stencil_t(g, w, stride, Hin, Win):
    """The transpose: in[p, hi, wi, c] = sum over the outputs (ho, wo) and taps t that read it of w[t, c] g[p, ho, wo, c]."""
    P, Hout, Wout, Cc = g.shape
    buf = torch.zeros(P, Hin + 2, Win + 2, Cc, dtype=g.dtype, device=g.device)
    for t, v in _views(buf, stride, Hout, Wout):
        v += g * w[t]
    return buf[:, 1:-1, 1:-1]


def tap_sums(x, g, stride):
    """[C, 9]: sum over planes and outputs of x[input pixel of tap t] * g[output]."""
    P, Hout, Wout, Cc = g.shape
    return torch.stack([(v * g).sum((0, 1, 2)) for _, v in _views(_pad(x), stride, Hout, Wout)], 1)


def y1_f64(o):
    """(y1 float64 [rows, C], SY or None): the stored tensor, or a0 . W1^T and its magnitude sum for the rebuilt forms."""
    if o.case.cin:
        return conv_pw_f64(o.a0, o.w1), o.a0.double().abs() @ o.w1.double().abs().t()
    return o.y1.double(), None


def activation(o):
    """float64 h, sig, z, d = SiLU'(h) and the fp32 error terms e_z, e_d of the module docstring, all [P, Hin, Win, C]."""
    c = o.case
    y1, SY = y1_f64(o)
    sc, sh = o.scale.double(), o.shift.double()
    h = y1 * sc + sh
    e_h = U32 * ((y1 * sc).abs() + sh.abs())
    if SY is not None:
        e_h = e_h + sc.abs() * 2.0 * c.cin * U32 * SY
    sig = torch.sigmoid(h)
    z = h * sig
    d = sig * (1.0 + h * (1.0 - sig))
    rho = U32 * ((1.0 - sig) * (2.0 * h.abs() + 2.0) + 3.0)
    e_z = 1.1 * e_h + z.abs() * (rho + U32)
    e_d = 0.5 * e_h + d.abs() * (rho + 2.0 * U32) + sig * h.abs() * (sig * rho + 2.0 * U32 * (1.0 - sig))
    v = lambda x: x.view(c.planes, c.Hin, c.Win, c.C)            # noqa: E731
    return dict(y1=y1, SY=SY, h=v(h), sig=v(sig), z=v(z), d=v(d), e_z=v(e_z), e_d=v(e_d))


def units(case):
    """(u_out, u_tile, u_w) of a case."""
    bf = case.dtype == "bf16"
    return U[case.dtype], (U["bf16"] if bf else 0.0), (U["bf16"] if bf and not case.wround else 0.0)


def forward_reference(o, mut=None):
    """float64 y2 [rows, C] and its per-element bound.  mut names a mutation of the VALUES (teeth test); the bound never changes."""
    c = o.case
    u_out, u_tile, u_w = units(c)
    a = activation(o)
    z, w = a["z"], o.w.double()
    pad, phase = "zero", 0
    if mut == "drop_tap":
        w = w.clone(); w[5] = 0.0
    if mut == "w_rounded":
        w = o.w.to(BF16).double()
    if mut == "halo_neighbour":
        pad = "neighbour"
    if mut == "phase":
        phase = 1
    if mut == "seam_row":
        rb = case_dispatch(c)[1][2] * c.stride
        z = z.clone(); z[:, rb] = z[:, 0]
    if mut == "ld_ignored":
        buf = o.y1_buf if not c.cin else o.a0_buf
        dense = buf.reshape(-1)[:buf.shape[0] * (buf.shape[1] - c.ld_pad)].view(buf.shape[0], -1)
        o2 = Operands(); o2.__dict__.update(o.__dict__)
        if c.cin:
            o2.a0 = dense
        else:
            o2.y1 = dense
        z = activation(o2)["z"]
    y2 = stencil(z, w, c.stride, o.Hout, o.Wout, pad, phase)
    y2 = _mutate_out(y2, mut)
    w = o.w.double()
    S = stencil(a["z"].abs(), w.abs(), c.stride, o.Hout, o.Wout)
    Et = stencil(a["e_z"] * (1.0 + u_tile), w.abs(), c.stride, o.Hout, o.Wout)
    E = ((1.0 + u_tile) * (1.0 + u_w) - 1.0 + 18.0 * U32) * S + Et
    ref = stencil(a["z"], w, c.stride, o.Hout, o.Wout)
    bound = u_out * (ref.abs() + E) + E
    return y2.reshape(-1, c.C), bound.reshape(-1, c.C)


def _mutate_out(x, mut):
    """Mutations of an output [P, H, W, C]."""
    if mut == "last_plane":
        x = x.clone(); x[-1] = 0.0
    if mut == "swap_planes":
        x = x.clone(); x[[0, 1]] = x[[1, 0]]
    if mut == "chan_tail":
        x = x.clone(); x[..., 64:] = 0.0
    return x


def gradient(o):
    """float64 g = A1 dh2 + A2 y2 + A3 [P, Hout, Wout, C] and its fp32 error term e_g."""
    c = o.case
    t1, t2, t3 = o.A1.double() * o.dh2.double(), o.A2.double() * o.y2in.double(), o.A3.double()
    g = t1 + t2 + t3
    e_g = 3.0 * U32 * (t1.abs() + t2.abs() + t3.abs())
    v = lambda x: x.view(c.planes, o.Hout, o.Wout, c.C)          # noqa: E731
    return v(g), v(e_g)


def backward_reference(o, mut=None):
    """float64 (dh1 [rows, C], dW [C, 9]), their per-element bounds and yhat1 (float64; the rebuilt forms': from a0 . W1^T)."""
    c = o.case
    u_out, u_tile, u_w = units(c)
    a = activation(o)
    g, e_g = gradient(o)
    w = o.w.double()
    gm, wm = g, w
    if mut == "drop_tap":
        wm = w.clone(); wm[5] = 0.0
    if mut == "w_rounded":
        wm = o.w.to(BF16).double()
    if mut == "seam_row":
        rb = case_dispatch(c)[1][1]
        gm = g.clone(); gm[:, rb] = gm[:, 0]
    if mut == "lost_output":                                     # one contributing output (a corner: its taps reach the halo) dropped
        gm = g.clone(); gm[0, 0, 0] = 0.0
    if mut == "ld_ignored":
        buf = o.dh2_buf
        dense = buf.reshape(-1)[:buf.shape[0] * c.C].view(buf.shape[0], c.C)
        o2 = Operands(); o2.__dict__.update(o.__dict__); o2.dh2 = dense
        gm = gradient(o2)[0]
    G = stencil_t(g, w, c.stride, c.Hin, c.Win)
    dh1_m = _mutate_out(a["d"] * stencil_t(gm, wm, c.stride, c.Hin, c.Win), mut)
    SG = stencil_t(g.abs(), w.abs(), c.stride, c.Hin, c.Win)
    Eg = stencil_t(e_g * (1.0 + u_tile), w.abs(), c.stride, c.Hin, c.Win)
    EG = ((1.0 + u_tile) * (1.0 + u_w) - 1.0 + 18.0 * U32) * SG + Eg
    ref = a["d"] * G
    E = a["d"].abs() * EG + (G.abs() + EG) * a["e_d"] + U32 * ref.abs()
    dh1_b = u_out * (ref.abs() + E) + E
    dW = tap_sums(a["z"], gm, c.stride)
    dW_ref = tap_sums(a["z"], g, c.stride)
    SW = tap_sums(a["z"].abs(), g.abs(), c.stride)
    SWe = (tap_sums(a["e_z"], g.abs(), c.stride) + tap_sums(a["z"].abs(), e_g, c.stride)) * (1.0 + u_tile) ** 2
    n = tap_sums(torch.ones_like(a["z"][..., :1]), torch.ones_like(g[..., :1]), c.stride)          # [1, 9] term counts
    dW_b = U32 * dW_ref.abs() + ((1.0 + u_tile) ** 2 - 1.0 + 2.0 * n * U32) * SW + SWe
    yhat = (a["y1"] - o.mean.double()) * o.invstd.double()
    return dict(dh1=dh1_m.reshape(-1, c.C), dh1_bound=dh1_b.reshape(-1, c.C), dW=dW, dW_bound=dW_b, yhat=yhat, n=n)


def forward_stats(o, y2_stored):
    """Reference and bound of (sum y2, sum y2^2) from the values the kernel stored (every path sums those: STATS_SUM)."""
    v = y2_stored.double()
    n = v.shape[0]
    return (v.sum(0), (v * v).sum(0)), (n * U32 * v.abs().sum(0), (n + 1) * U32 * (v * v).sum(0))


def backward_stats(o, dh1_stored, yhat):
    """Reference and bound of (sum dh1, sum dh1 yhat1) from the stored dh1 and the float64 yhat1."""
    c = o.case
    v = dh1_stored.double()
    n = v.shape[0]
    y1, SY = y1_f64(o)
    inv, mean = o.invstd.double().abs(), o.mean.double().abs()
    b1 = (n + 3) * U32 * inv * ((v * y1).abs().sum(0) + mean * v.abs().sum(0))
    if SY is not None:
        b1 = b1 + inv * 2.0 * c.cin * U32 * (v.abs() * SY).sum(0)
    return (v.sum(0), (v * yhat).sum(0)), (n * U32 * v.abs().sum(0), b1)


def max_ratio(got, ref, bound):
    """(max |got - ref| / bound, number of elements NOT within the bound: NaN counts as over)."""
    err = (got.double() - ref).abs()
    over = int((~(err <= bound)).sum())
    ratio = err / bound.clamp_min(1e-300)
    return float(torch.nan_to_num(ratio, nan=float("inf")).max()), over


# ---- exact cases: preconditions, asserted from the reference alone ---------------------------------------------------------------------
def assert_exact_preconditions(o):
    """Everything an exact case needs so that ANY summation order gives the same bits (issue: "Exact cases")."""
    c = o.case
    assert o.kind == "exact"
    a = activation(o)
    y1 = a["y1"]
    assert bool((y1 == y1.round()).all()) and float(y1.min()) >= 0 and float(y1.max()) <= 16
    if c.cin:
        assert float(o.a0.double().abs().max()) <= 1 and bool((o.w1.double() == o.w1.double().round()).all())
    h32 = (y1.float() + 17.0)
    sig32 = 1.0 / (1.0 + torch.exp(-h32))
    assert bool((sig32 == 1.0).all()), "fp32 rcp(1 + exp(-h)) must be exactly 1 for h >= 17"
    hi = (y1 + 17.0).view(c.planes, c.Hin, c.Win, c.C)
    w = o.w.double()
    y2 = stencil(hi, w, c.stride, o.Hout, o.Wout)
    S = stencil(hi, w.abs(), c.stride, o.Hout, o.Wout)
    if c.dtype == "bf16":
        assert float(y2.abs().max()) <= 256, "bf16 holds integers up to 256"
    assert float(S.max()) < EXACT_LIMIT
    assert float((y2 * y2).sum((0, 1, 2)).max()) < EXACT_LIMIT and float(y2.abs().sum((0, 1, 2)).max()) < EXACT_LIMIT
    g = o.dh2.double().view(c.planes, o.Hout, o.Wout, c.C)
    dh1 = stencil_t(g, w, c.stride, c.Hin, c.Win)
    SG = stencil_t(g.abs(), w.abs(), c.stride, c.Hin, c.Win)
    if c.dtype == "bf16":
        assert float(dh1.abs().max()) <= 256
    assert float(tap_sums(hi, g.abs(), c.stride).max()) < EXACT_LIMIT
    assert float((SG * hi).sum((0, 1, 2)).max()) < EXACT_LIMIT
    return y2.reshape(-1, c.C), dh1.reshape(-1, c.C), tap_sums(hi, g, c.stride), y1


def exact_reference(o):
    """float64 (y2, dh1, dW, sums forward, sums backward) of an exact case: integers, SiLU = identity, SiLU' = 1."""
    y2, dh1, dW, y1 = assert_exact_preconditions(o)
    return dict(y2=y2, dh1=dh1, dW=dW, st_fwd=(y2.sum(0), (y2 * y2).sum(0)), st_bwd=(dh1.sum(0), (dh1 * y1).sum(0)))


# ---- float32 emulation of each path's arithmetic (room test) ---------------------------------------------------------------------------
LOG2E_NEG = -1.4426950216293335          # -0x1.715476p+0f


def _sig32(h):
    return 1.0 / (torch.exp2(h * LOG2E_NEG) + 1.0)


def _tile(x, case):
    return x.to(BF16).float() if case.dtype == "bf16" else x


def _acc_taps(terms, dot2):
    """Sum nine fp32 product operand pairs [(w, x)] tap-major: dot2 paths add two products per step with one rounding
    (v_dot2_f32_bf16, per tap row: taps 0 + 1, then tap 2); the generic kernels a chain of multiply-adds, each step rounded twice."""
    acc = None
    if dot2:
        for dy in range(3):
            (w0, x0), (w1, x1), (w2, x2) = terms[3 * dy:3 * dy + 3]
            s = w0.double() * x0.double() + w1.double() * x1.double()
            acc = s.float() if acc is None else (acc.double() + s).float()
            acc = (acc.double() + w2.double() * x2.double()).float()
        return acc
    for w, x in terms:
        acc = w * x if acc is None else acc + w * x
    return acc


def _y1_f32(o):
    c = o.case
    if c.cin:
        return o.a0.float() @ o.w1.float().t()
    return o.y1.float()


def emulate_forward(o):
    """y2 as the path of the case computes it, in float32 on the operands' device, rounded to the storage type."""
    c = o.case
    dot2 = case_dispatch(c)[0] in DOT2_PATHS
    h = _y1_f32(o) * o.scale + o.shift
    z = _tile(h * _sig32(h), c).view(c.planes, c.Hin, c.Win, c.C)
    w = o.w.to(BF16).float() if dot2 else o.w
    terms = [(w[t], v) for t, v in _views(_pad(z), c.stride, o.Hout, o.Wout)]
    return _acc_taps(terms, dot2).to(DT[c.dtype]).reshape(-1, c.C)


def emulate_backward(o):
    """(dh1 in the storage type, dW fp32 [C, 9]) as the path of the case computes them, in float32."""
    c = o.case
    dot2 = case_dispatch(c)[0] in DOT2_PATHS
    y1 = _y1_f32(o)
    h = y1 * o.scale + o.shift
    sg = _sig32(h)
    z = (h * sg).view(c.planes, c.Hin, c.Win, c.C)
    if dot2:
        z = _tile(z, c)                                          # the row-walk and pair kernels feed dW from the bf16 z1
    d = (sg * (1.0 + h * (1.0 - sg))).view(c.planes, c.Hin, c.Win, c.C)
    g = _tile(o.A1 * o.dh2.float() + (o.A2 * o.y2in.float() + o.A3), c).view(c.planes, o.Hout, o.Wout, c.C)
    w = o.w.to(BF16).float() if dot2 else o.w
    buf = torch.zeros(c.planes, c.Hin + 2, c.Win + 2, c.C, dtype=torch.float32, device=g.device)
    for t, v in _views(buf, c.stride, o.Hout, o.Wout):
        v += g * w[t]
    dh1 = (buf[:, 1:-1, 1:-1] * d).to(DT[c.dtype]).reshape(-1, c.C)
    dW = torch.stack([(v * g).sum((0, 1, 2)) for _, v in _views(_pad(z), c.stride, o.Hout, o.Wout)], 1)
    return dh1, dW

// Host-side launch policy of the persistent kernels (launch lessons 1 and 2), in one place:
//   * occupancy is decided by the unified VGPR + AGPR budget and the LDS a launch asks for, so it is ASKED of the runtime per
//     (kernel, workgroup size, dynamic LDS) and never derived from a register count;
//   * a persistent grid is exactly one resident round, 256 CUs x workgroups per CU, capped by the work: a partial second round
//     costs a whole workgroup duration.
// This is the only file of csrc/ that names the occupancy query or the dynamic-LDS attribute.
#pragma once
#include "dwn_common.h"

constexpr int DWN_CUS = 256;                  // MI355X

// More than 48 KB of dynamic LDS needs the opt-in (160 KB per CU on gfx950, minus the kernel's static part).  The attribute
// belongs to the (function, device) pair, so it is repeated per launch: a host-side table write.  The error is returned AND left
// pending: a caller that goes on to the launch (which reports a too-large tile itself) clears it, the others return it.
template <typename K>
static inline hipError_t lds_opt_in(K kernel, size_t dyn_lds) {
    if (dyn_lds <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn_lds);
}

// Resident workgroups per CU of this launch; `fallback` when the runtime cannot say (the pending error is cleared: the
// DWN_CHECK_LAUNCH() after the launch must report the launch, not the query).
template <typename K>
static inline int resident_bpc(K kernel, int threads, size_t dyn_lds, int fallback) {
    if (lds_opt_in(kernel, dyn_lds) != hipSuccess) (void)hipGetLastError();
    int bpc = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, kernel, threads, dyn_lds) != hipSuccess || bpc < 1) {
        (void)hipGetLastError();
        bpc = fallback;
    }
    return bpc;
}

// Grid x of one resident round when `slices` workgroups (grid y) share each x index: at least 1, at most the work.  xcd: the kernel
// maps the slices of an x index to one XCD (wf_block / wk_block), which needs a multiple of 8 (a workgroup past the work just exits).
constexpr i64 resident_grid_x(int bpc, int slices, i64 work, bool xcd = false) {
    i64 gx = ((i64)DWN_CUS * bpc) / slices;
    if (gx < 1) gx = 1;
    if (gx > (work > 1 ? work : 1)) gx = work > 1 ? work : 1;
    if (xcd) gx = gx >= 8 ? (gx & ~(i64)7) : 8;
    return gx;
}

// Row bands of the LDS-tiled depth-wise kernels: the one statement of how a plane of `rows` rows is cut into bands, used by
// spatial_fwd_t / spatial_bwd_t / spatial_fwd_ks_t / spatial_bwd_ks_t (dwn_dwconv.hip) and launch_s2 (dwn_dwbwd.hip), which keep
// their own tile_bytes(band height), budget, limit and refusal text.  rows_band <= 0: the largest band whose tile fits `budget`
// (fewer halo rows re-read, fewer barriers per byte), then an even split so that the last band is not ragged; rows_band > 0: the
// caller's height.  Either is then rounded up to a multiple of `step` (launch_s2 takes input rows in pairs) and clipped to the plane.
struct BandPlan { int rows, nbands; size_t lds; bool ok; };      // rows per band, bands per plane, tile_bytes(rows), lds <= limit
template <typename F>
constexpr BandPlan plan_bands(int rows, F tile_bytes, size_t budget, size_t limit, int step, int rows_band) {
    int rb = rows_band;
    if (rb <= 0) {
        rb = step;
        while (rb < rows && (size_t)tile_bytes(rb + step) <= budget) rb += step;
        const int nb = (rows + rb - 1) / rb;
        rb = (rows + nb - 1) / nb;
    }
    rb = (rb + step - 1) / step * step;
    if (rb > rows) rb = (rows + step - 1) / step * step;
    const size_t lds = (size_t)tile_bytes(rb);
    return BandPlan{rb, (rows + rb - 1) / rb, lds, lds <= limit};
}

// The bands the five launchers' own loops gave before they shared plan_bands, worked by hand from those loops (3x3: cross-checked
// with tests/dws3_reference.py), at their tile bytes, budgets and limits ("greedy": before the even split).  A moved band fails the build.
constexpr bool band_is(BandPlan p, int rows, int nbands, size_t lds) { return p.ok && p.rows == rows && p.nbands == nbands && p.lds == lds; }
constexpr size_t LDS_KB = 1024;
// spatial_fwd_t, 3x3 (budget 48 KB at stride 1, 80 KB at stride 2; limit 156 KB)
static_assert(band_is(plan_bands(18, [](int rb) { return (rb + 2) * 34 * 128; }, 48 * LDS_KB, 156 * LDS_KB, 1, 0), 9, 2, 47872), "fp32 s1, Hout 18, Win 32: greedy 9");
static_assert(band_is(plan_bands(25, [](int rb) { return (rb + 2) * 32 * 128; }, 48 * LDS_KB, 156 * LDS_KB, 1, 0), 9, 3, 45056), "fp32 s1, Hout 25, Win 30: greedy 10");
static_assert(band_is(plan_bands(13, [](int rb) { return (2 * rb + 1) * 32 * 128; }, 80 * LDS_KB, 156 * LDS_KB, 1, 0), 7, 2, 61440), "fp32 s2, Hout 13, Win 30: greedy 9");
static_assert(!plan_bands(1, [](int rb) { return (rb + 2) * 2050 * 128; }, 48 * LDS_KB, 156 * LDS_KB, 1, 0).ok, "fp32 s1, Win 2048: refused");
// spatial_bwd_t, 3x3 (budget 44 KB; limit 150 KB)
static_assert(band_is(plan_bands(25, [](int rb) { return (rb + 3) * 32 * 128; }, 44 * LDS_KB, 150 * LDS_KB, 1, 0), 7, 4, 40960), "fp32 s1, Hin 25, Wout 30: greedy 8");
static_assert(band_is(plan_bands(25, [](int rb) { return ((rb + 1) / 2 + 2) * 33 * 128; }, 44 * LDS_KB, 150 * LDS_KB, 1, 0), 13, 2, 38016), "s2, Hin 25, Wout 31: greedy 16");
// spatial_fwd_ks_t (budget: the smaller of the 3x3 forward budget and 79 KB - STATIC; limit 156 KB - STATIC)
static_assert(band_is(plan_bands(25, [](int rb) { return (rb + 4) * 32 * 128; }, 48 * LDS_KB, 156 * LDS_KB - 3456, 1, 0), 7, 4, 45056), "k5 fp32 s1, Hout 25, Win 28: greedy 8");
static_assert(band_is(plan_bands(16, [](int rb) { return (rb + 6) * 34 * 128; }, 48 * LDS_KB, 156 * LDS_KB - 13056, 1, 0), 4, 4, 43520), "k7 bf16 s1, Hout 16, Win 28: greedy 5");
static_assert(band_is(plan_bands(18, [](int rb) { return (2 * rb + 5) * 70 * 128; }, 79 * LDS_KB - 13056, 156 * LDS_KB - 13056, 1, 0), 1, 18, 62720),
              "k7 bf16 s2, Hout 18, Win 64: 2 rows (80 640 bytes) fit the forward budget, not 79 KB - STATIC");
// spatial_bwd_ks_t (budget 79 KB - STATIC; limit 156 KB - STATIC)
static_assert(band_is(plan_bands(22, [](int rb) { return ((rb + 4) * 32 + rb * 32) * 128; }, 79 * LDS_KB - 3968, 156 * LDS_KB - 3968, 1, 0), 6, 4, 65536), "k5 fp32 s1, Hin 22, Win 28: greedy 7");
static_assert(band_is(plan_bands(9, [](int rb) { return ((rb + 6) * 34 + rb * 34) * 128; }, 79 * LDS_KB - 14080, 156 * LDS_KB - 14080, 1, 0), 3, 3, 52224), "k7 bf16 s1, Hin 9, Win 28: greedy 4");
// launch_s2 (row pairs; budget 50 KB, 75 KB in the rebuilt form; limit 150 KB less the W1 copy): even again after the split and the clip
static_assert(band_is(plan_bands(50, [](int R) { return (R / 2 + 1) * 4352; }, 50 * LDS_KB, 150 * LDS_KB, 2, 0), 18, 3, 43520), "Win 64, Hin 50: greedy 20, split 17");
static_assert(band_is(plan_bands(70, [](int R) { return (R / 2 + 1) * 4352; }, 75 * LDS_KB, 150 * LDS_KB - 16384, 2, 0), 24, 3, 56576), "Win 64 rebuilt, Hin 70: greedy 32");
static_assert(band_is(plan_bands(37, [](int R) { return (R / 2 + 1) * 5120; }, 50 * LDS_KB, 150 * LDS_KB, 2, 0), 14, 3, 40960), "Win 16, Hin 37: greedy 18, split 13");
static_assert(band_is(plan_bands(9, [](int R) { return (R / 2 + 1) * 5120; }, 50 * LDS_KB, 150 * LDS_KB, 2, 3), 4, 3, 15360), "rows_band 3: 4");
static_assert(band_is(plan_bands(3, [](int R) { return (R / 2 + 1) * 5120; }, 50 * LDS_KB, 150 * LDS_KB, 2, 8), 4, 1, 15360), "rows_band 8 of 3 rows: 4");

// query, grid (x = one resident round, y = slices), launch, check
template <typename K, typename... Args>
static inline int launch_resident(K kernel, int threads, size_t dyn_lds, int fallback, int slices, i64 work, bool xcd,
                                  hipStream_t s, const Args&... args) {
    const int bpc = resident_bpc(kernel, threads, dyn_lds, fallback);
    const dim3 grid((unsigned)resident_grid_x(bpc, slices, work, xcd), (unsigned)slices);
    hipLaunchKernelGGL(kernel, grid, dim3(threads), dyn_lds, s, args...);
    DWN_CHECK_LAUNCH();
    return 0;
}

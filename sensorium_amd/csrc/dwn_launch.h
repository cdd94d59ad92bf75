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

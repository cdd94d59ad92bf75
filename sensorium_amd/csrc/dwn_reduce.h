// The fixed-order float64 reductions and the small predicates of the analysis families (dwn_gaze, dwn_corr, dwn_stim,
// dwn_modulator, dwn_mei, dwn_trial_score, dwn_spatial, dwn_rf, dwn_rf_fit, dwn_pairwise).  One definition each.
// The rule: a caller's bits are part of its contract (the *_digest() tests), so nothing here may ever reorder or re-associate an
// addition or change the width of a shuffle.  A barrier may be added; an addition may not move.
// (dwn_elementwise.hip keeps its own float wave_sum / gs_block_sum: those run in the timed step and do not include this file.)
#pragma once
#include "dwn_common.h"
#include <float.h>

// sum over the 64 lanes; lane i and lane i ^ m add the same two values, so every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// fixed tree over the NT threads of the workgroup, NV values per thread through red[NV][NT]: s = NT/2, NT/4, ..., 1, thread i adds
// the value of thread i + s to its own.  The total is returned in EVERY thread.  The leading barrier lets a caller call this
// again (or in a loop) without one of its own: red[] of the previous call has been read.
template <int NT, int NV>
__device__ __forceinline__ void wg_tree_sum(double (&v)[NV], double (*red)[NT]) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int q = 0; q < NV; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = red[q][0];
}
template <int NT>
__device__ __forceinline__ double wg_tree_sum(double a, double (&red)[NT]) {
    double v[1] = {a};
    wg_tree_sum<NT, 1>(v, &red);
    return v[0];
}

// the other form: the butterfly inside each wave, then the NT / 64 wave totals in ascending order; in every thread
template <int NT>
__device__ __forceinline__ double wg_wave_sum(double a, double (&red)[NT / 64]) {
    a = wave_sum(a);
    __syncthreads();                                           // red[] of the previous call has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) s += red[w];
    return s;
}

// false for NaN and +-Inf, true for +-FLT_MAX / +-DBL_MAX.  (fabs(v) < inf is the same predicate: both forms answer false, false,
// true on NaN, +-Inf, +-DBL_MAX, and every other value is below both bounds.)
__device__ __forceinline__ bool is_finite(float v) { return fabsf(v) <= FLT_MAX; }
__device__ __forceinline__ bool is_finite(double v) { return fabs(v) <= DBL_MAX; }

// the quiet NaN every family writes for "undefined": 0x7fc00000 / 0x7ff8000000000000
__device__ __forceinline__ float qnan_f() { return __builtin_nanf(""); }
__device__ __forceinline__ double qnan_d() { return __longlong_as_double(0x7ff8000000000000ll); }

// host: may this pointer take 16-byte vector loads
inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

// Depth-wise convolution kernels of InvertedResidual3d (reference: src/models/dwiseneuro.py:96-111):
//   spatial  (1,k,k) stride (1,s,s) pad k/2   and   temporal (k,1,1) pad k/2, groups = channels.
//
// HBM-bound: every kernel reads its input tensor(s) once and writes its output once, in
// 128-byte channel segments of channels-last rows.  The producer's BatchNorm+SiLU is applied while loading,
// the BN Σ/Σ² of the output are accumulated in the same pass, and the backward kernels fuse data-gradient,
// weight-gradient, SiLU' and the BN-backward sums.
//
// Work decomposition: a workgroup owns one 128-byte channel slice (V4<T>::NCV vectors of 4 channels: 64 bf16 /
// 32 fp32 channels); a thread's 4 channels never change, so its BN coefficients, stencil weights,
// weight-gradient and statistics accumulators live in registers for the whole persistent (grid-stride) kernel.
// Loads are issued in batches of 4 independent 8/16-byte vectors per tensor so that, at 3-5 waves per SIMD,
// each CU keeps tens of KB in flight (the HBM latency-bandwidth product).
//
// Kernel families in this file, in its order (3x3 spatial row-walk kernels: dwn_dwfwd.hip / dwn_dwbwd.hip; dwn_dwrc.hip):
//   dw_spatial_fwd_kernel<T, 3, ST, NT>                 3x3 generic, packed-fp32 taps: fp32 at any stride, bf16 at the generic stride only
//   dw_spatial_fwd_pair_kernel<ST, NT> (stride 1, 2)    3x3 bf16: x-pair-packed LDS tile + v_dot2c_f32_bf16 taps
//   dw_spatial_bwd_kernel<T, 3, ST>                     3x3 generic: fp32 at any stride, bf16 at stride 2 and the generic stride
//   dw_temporal_fwd_kernel<T, KT, ZOUT>                 KT 3, 5, 7, 9: register sliding window along T; ZOUT: the eval z3 epilogue
//   dw_temporal_bwd_kernel<T, KT, LD_*, 4>              KT 3, 5 with a stored y3 (LD_AFFINE2, LD_DY3)
//   dw_spatial_fwd_ks_kernel / dw_spatial_bwd_ks_kernel 5x5 and 7x7, both storage types, every stride: weights in LDS
//   dw_spatial_bwd_pair_kernel (stride 1)               3x3 bf16: the pair-packed tile for the data and weight gradients
//   dw_temporal_bwd_rc_kernel<T, KT>                    KT 3, 5, y3 recomputed (LD_PLAIN)
//   dw_temporal_bwd_wide_kernel<T, KT>                  KT 7, 9, y3 recomputed, rings in LDS
// Launchers: row bands from plan_bands (dwn_launch.h), the (stride, workgroup size) instantiation from by_stride / by_stride_threads,
// one temporal launcher per direction switching on kt.  Only what a launch can reach is instantiated.
// Integer index math is kept off the per-tap path (FastDiv / 24-bit multiplies / per-pixel tile index): on gfx950 an
// integer VALU op costs ~1.5 FMAs and a bf16->fp32 unpack is such an op (profiles/r1c_valu_rates.txt).
#include "dwn_internal.h"
#include "dwn_launch.h"
#include <stdlib.h>
#include <type_traits>

extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];

#define DWS_BWD_THREADS 256
#ifndef DWS_BWD_PAIR_MINW
#define DWS_BWD_PAIR_MINW 3       // waves per SIMD the pair-packed stride-1 backward is compiled for
#endif
#ifndef DWS_BWD_PAIR_XB
#define DWS_BWD_PAIR_XB 2
#endif
#ifndef DWS_BWD_MINB1
#define DWS_BWD_MINB1 3          // resident workgroups per CU the stride-1 spatial backward is compiled for
#endif
#ifndef DWT_RC_MINW
#define DWT_RC_MINW 2        // waves per SIMD the y3-recomputing temporal backward is compiled for
#endif
// LDS tile budgets of the spatial kernels (bytes); tuned on MI355X with tools/microbench.py
#ifndef DWS_FWD_LDS_BUDGET
#define DWS_FWD_LDS_BUDGET (a.stride >= 2 ? 80 * 1024 : 48 * 1024)
#endif
#ifndef DWS_BWD_LDS_BUDGET
#define DWS_BWD_LDS_BUDGET (44 * 1024)
#endif

template <typename T> struct SL {
    static constexpr int NCV = V4<T>::NCV;       // vectors per slice
    static constexpr int CS = NCV * 4;           // channels per slice
    static constexpr int LP = 256 / NCV;         // pixel lanes per workgroup
    typedef typename V4<T>::raw_t raw_t;
};

template <typename T>
__device__ __forceinline__ void block_stats_flush(float* lstat, const float* s0, const float* s1, int cv, int c0, int C,
                                                 double* stats, int rep) {
    constexpr int CS = SL<T>::CS;
    DET_WAVES_BEGIN
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        atomicAdd(&lstat[cv * 4 + i], s0[i]);
        atomicAdd(&lstat[CS + cv * 4 + i], s1[i]);
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
    const int tid = threadIdx.x;
    if (tid < 2 * CS) {
        int which = tid / CS, c = c0 + tid % CS;
        if (c < C) stat_add(stats, rep, C, which, c, lstat[tid]);
    }
}

#ifndef DWT_PRIO
#define DWT_PRIO 1         // issue priority while a wave issues its next global loads (0 = off)
#endif
typedef float f2_t __attribute__((ext_vector_type(2)));
// two adjacent channels as one register pair: the compiler emits v_pk_fma_f32 / v_pk_mul_f32 without shuffles
template <typename T> __device__ __forceinline__ void unpack_pairs(const typename V4<T>::raw_t& r, f2_t& lo, f2_t& hi);
template <> __device__ __forceinline__ void unpack_pairs<bf16_t>(const uint2& r, f2_t& lo, f2_t& hi) {
    lo = f2_t{__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u)};
    hi = f2_t{__uint_as_float(r.y << 16), __uint_as_float(r.y & 0xffff0000u)};
}
template <> __device__ __forceinline__ void unpack_pairs<float>(const uint4& r, f2_t& lo, f2_t& hi) {
    lo = f2_t{__uint_as_float(r.x), __uint_as_float(r.y)};
    hi = f2_t{__uint_as_float(r.z), __uint_as_float(r.w)};
}

__device__ __forceinline__ void bn_silu4(float* v, const float* s, const float* t) {
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = fmaf(v[i], s[i], t[i]);
    silu_n<4>(v);
}

// ------------------------------------------------------------------------------------------------
// spatial forward
// ------------------------------------------------------------------------------------------------
template <typename T, int KS, int ST, int NT>
__global__ __launch_bounds__(NT, 4) void dw_spatial_fwd_kernel(const DwSpatialFwd a) {
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = NT / NCV, P = KS / 2;
    constexpr int XB = 4;                              // x-iterations batched per row (loads in flight per thread)
    typedef typename SL<T>::raw_t raw_t;
    const int stride = ST > 0 ? ST : a.stride;
    __shared__ float lstat[2 * CS];
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;               // safe channel for predicated loads
    if (tid < 2 * CS) lstat[tid] = 0.f;
    __syncthreads();

    float w[KS * KS][4], bs[4], bt[4];
#pragma unroll
    for (int k = 0; k < KS * KS; ++k) {
        ldc4(a.w + (i64)k * a.C + chs, w[k]);
        if (!chan_ok) { w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0.f; }
    }
    ldc4(a.in.v1 + chs, bs);
    ldc4(a.in.v2 + chs, bt);
    float st0[4] = {0.f, 0.f, 0.f, 0.f}, st1[4] = {0.f, 0.f, 0.f, 0.f};

    const int Wp = a.Win + 2 * P;
    const FastDiv dvp(Wp), dvo(a.Wout);
    const int nbands = (a.Hout + a.rows_band - 1) / a.rows_band;
    const int ntiles = a.planes * nbands;
    const T* inp = reinterpret_cast<const T*>(a.in.p);
    T* outp = reinterpret_cast<T*>(a.out);
    raw_t* tile = reinterpret_cast<raw_t*>(dyn_smem);
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int plane = tile_id / nbands, band = tile_id % nbands;
        const int ho0 = band * a.rows_band;
        const int nro = (a.Hout - ho0 < a.rows_band) ? a.Hout - ho0 : a.rows_band;
        const int hi0 = ho0 * stride - P;
        const int rows_in = (nro - 1) * stride + KS;
        const i64 plane_row0 = (i64)plane * a.Hin * a.Win;
        // stage the activated input rows (zero padded).  The (row, x) walk is flat and NB loads are issued before
        // the first one is consumed: a row-by-row loop would serialise one HBM round trip per input row.
        const int total_st = rows_in * Wp;                  // flat (row, column) walk: flat index == tile index
        const T* in0 = inp + plane_row0 * a.in.ld;
        if constexpr (TT<T>::IS_BF16) {
            // bf16: stage 8 channels (16 B) per thread — halves the per-vector address/predicate/LDS-store overhead of
            // this VALU-bound pass; the tile keeps the [pixel][64 ch] layout the 4-channel compute lanes read
            constexpr int NB = 8, SV = 8, LPS = NT / SV;          // 8 x 16-B vectors per pixel slice
            const int scv = tid % SV, spl = tid / SV;
            const int sch = c0 + scv * 8;
            const bool sch_ok = sch < a.C;                        // C % 8 == 0: a vector is all-valid or all-invalid
            const int schs = sch_ok ? sch : 0;
            f2_t s8[4], t8[4];
            {
                float sf[8], tf[8];
                ldc4(a.in.v1 + schs, sf); ldc4(a.in.v1 + schs + 4, sf + 4);
                ldc4(a.in.v2 + schs, tf); ldc4(a.in.v2 + schs + 4, tf + 4);
#pragma unroll
                for (int i = 0; i < 4; ++i) { s8[i] = f2_t{sf[2 * i], sf[2 * i + 1]}; t8[i] = f2_t{tf[2 * i], tf[2 * i + 1]}; }
            }
            uint4* tile16 = reinterpret_cast<uint4*>(dyn_smem);
            for (int f0 = spl; f0 < total_st; f0 += NB * LPS) {
                uint4 raw[NB];
                bool okv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LPS;
                    const int r = dvp.div(f);
                    const int hi = hi0 + r, wi = dvp.rem(f, r) - P;
                    okv[u] = sch_ok && f < total_st && (unsigned)hi < (unsigned)a.Hin && (unsigned)wi < (unsigned)a.Win;
                    const unsigned off = okv[u] ? __umul24(__mul24(hi, a.Win) + wi, (unsigned)a.in.ld) : 0u;
                    raw[u] = *reinterpret_cast<const uint4*>(in0 + off + schs);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LPS;
                    if (f < total_st) {
                        const unsigned rw[4] = {raw[u].x, raw[u].y, raw[u].z, raw[u].w};
                        unsigned o[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const f2_t y = f2_t{__uint_as_float(rw[i] << 16), __uint_as_float(rw[i] & 0xffff0000u)};
                            const f2_t h = y * s8[i] + t8[i];
                            const f2_t z = h * sigmoid2f_(h);
                            o[i] = pk_bf16(z.x, z.y);
                        }
                        tile16[f * SV + scv] = okv[u] ? make_uint4(o[0], o[1], o[2], o[3]) : make_uint4(0, 0, 0, 0);
                    }
                }
            }
        } else {
            constexpr int NB = 12;
            for (int f0 = pl; f0 < total_st; f0 += NB * LP) {
                raw_t raw[NB];
                bool okv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    const int r = dvp.div(f);
                    const int hi = hi0 + r, wi = dvp.rem(f, r) - P;
                    okv[u] = chan_ok && f < total_st && (unsigned)hi < (unsigned)a.Hin && (unsigned)wi < (unsigned)a.Win;
                    const unsigned off = okv[u] ? __umul24(__mul24(hi, a.Win) + wi, (unsigned)a.in.ld) : 0u;
                    raw[u] = ld4_raw<T>(in0 + off + chs);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    if (f < total_st) {
                        float v[4];
                        V4<T>::unpack(raw[u], v);
                        bn_silu4(v, bs, bt);
                        tile[f * NCV + cv] = okv[u] ? V4<T>::pack(v) : V4<T>::zero();
                    }
                }
            }
        }
        __syncthreads();
        {
            const int total = nro * a.Wout;                 // flat walk: narrow planes still fill every pixel lane
            const i64 orow0 = ((i64)plane * a.Hout + ho0) * a.Wout;
            T* out0 = outp + orow0 * a.C + chan;
            const int wdiff = stride * Wp - stride * a.Wout;   // tile index of output i = (i*stride + oy*wdiff) (+ taps)
            for (int i = pl; i < total; i += LP) {
                const int oy = dvo.div(i);
                f2_t acc0 = f2_t{0.f, 0.f}, acc1 = f2_t{0.f, 0.f};
                const raw_t* tp = tile + (i * stride + __mul24(oy, wdiff)) * NCV + cv;
#pragma unroll
                for (int dy = 0; dy < KS; ++dy)
#pragma unroll
                    for (int dx = 0; dx < KS; ++dx) {
                        f2_t v0, v1;
                        unpack_pairs<T>(tp[(dy * Wp + dx) * NCV], v0, v1);
                        acc0 += f2_t{w[dy * KS + dx][0], w[dy * KS + dx][1]} * v0;
                        acc1 += f2_t{w[dy * KS + dx][2], w[dy * KS + dx][3]} * v1;
                    }
                if (chan_ok) {
                    const float acc[4] = {acc0.x, acc0.y, acc1.x, acc1.y};
                    const raw_t packed = V4<T>::pack(acc);
                    *reinterpret_cast<raw_t*>(out0 + __umul24((unsigned)i, (unsigned)a.C)) = packed;
                    float r[4];
                    V4<T>::unpack(packed, r);
#pragma unroll
                    for (int q = 0; q < 4; ++q) { st0[q] += r[q]; st1[q] += r[q] * r[q]; }
                }
            }
        }
        __syncthreads();
    }
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// ------------------------------------------------------------------------------------------------
// spatial forward, bf16 storage, 3x3, stride 1 or 2: x-pair-packed LDS tile + v_dot2c_f32_bf16.
//
// The activated input is staged as dwords holding two horizontally adjacent pixels of one channel,
// tile[row][xp][c] = (z[row][2xp][c], z[row][2xp+1][c])  (xs = wi + 1 is the zero-padded column index).
// A 3-tap row of the stencil is then 2 dot2 instructions on packed operands — dot2(P[j], (w0,w1)) +
// dot2(P[j+1], (w2,0)) for an even output column, dot2(P[j], (0,w0)) + dot2(P[j+1], (w1,w2)) for an odd one —
// instead of 3 bf16->fp32 unpacks + 1.5 packed FMAs per channel, and a thread's 4 channels of a pixel pair are
// one ds_read_b128.  Weights are rounded to bf16 (as the reference's autocast conv does); accumulation is fp32.
// ------------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ float dot2_bf16(unsigned a, unsigned b, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, a), __builtin_bit_cast(bf16x2_t, b), c, false);
}
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) { return pk_bf16(lo, hi); }

template <int ST, int NT>
__global__ __launch_bounds__(NT, 4) void dw_spatial_fwd_pair_kernel(const DwSpatialFwd a) {
    typedef bf16_t T;
    constexpr int NCV = 16, CS = 64, LP = NT / NCV, P = 1;
    constexpr int NWC = ST == 1 ? 4 : 2;                 // packed weight combinations per stencil row
    __shared__ float lstat[2 * CS];
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    __syncthreads();

    // packed weights per stencil row dy and channel: A = (w0,w1), B = (w2,0) [, C = (0,w0), D = (w1,w2)]
    unsigned wp[3][NWC][4];
    {
        float w[9][4];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            ldc4(a.w + (i64)k * a.C + chs, w[k]);
            if (!chan_ok) { w[k][0] = w[k][1] = w[k][2] = w[k][3] = 0.f; }
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                wp[dy][0][q] = pack_bf16x2(w[dy * 3 + 0][q], w[dy * 3 + 1][q]);
                wp[dy][1][q] = pack_bf16x2(w[dy * 3 + 2][q], 0.f);
                if constexpr (ST == 1) {
                    wp[dy][2][q] = pack_bf16x2(0.f, w[dy * 3 + 0][q]);
                    wp[dy][3][q] = pack_bf16x2(w[dy * 3 + 1][q], w[dy * 3 + 2][q]);
                }
            }
    }
    f2_t st0[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}}, st1[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};

    const int Wp = a.Win + 2 * P;
    const int Wpp = (Wp + 1) >> 1;                       // staged pixel pairs per row
    const int Wop = (a.Wout + 1) >> 1;                   // output pixel pairs per row
    const FastDiv dvpp(Wpp), dvop(Wop);
    const int nbands = (a.Hout + a.rows_band - 1) / a.rows_band;
    const int ntiles = a.planes * nbands;
    const T* inp = reinterpret_cast<const T*>(a.in.p);
    T* outp = reinterpret_cast<T*>(a.out);
    unsigned* tile = reinterpret_cast<unsigned*>(dyn_smem);          // [rows_in][Wpp][64] dwords
    // staging role: 8 channels x one pixel pair
    constexpr int SV = 8, LPS = NT / SV, NB = 4;
    const int scv = tid % SV, spl = tid / SV;
    const int sch = c0 + scv * 8;
    const bool sch_ok = sch < a.C;
    const int schs = sch_ok ? sch : 0;
    f2_t s8[4], t8[4];
    {
        float sf[8], tf[8];
        ldc4(a.in.v1 + schs, sf); ldc4(a.in.v1 + schs + 4, sf + 4);
        ldc4(a.in.v2 + schs, tf); ldc4(a.in.v2 + schs + 4, tf + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { s8[i] = f2_t{sf[2 * i], sf[2 * i + 1]}; t8[i] = f2_t{tf[2 * i], tf[2 * i + 1]}; }
    }
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int plane = tile_id / nbands, band = tile_id % nbands;
        const int ho0 = band * a.rows_band;
        const int nro = (a.Hout - ho0 < a.rows_band) ? a.Hout - ho0 : a.rows_band;
        const int hi0 = ho0 * ST - P;
        const int rows_in = (nro - 1) * ST + 3;
        const i64 plane_row0 = (i64)plane * a.Hin * a.Win;
        const int total_st = rows_in * Wpp;
        const T* in0 = inp + plane_row0 * a.in.ld + schs;
        for (int f0 = spl; f0 < total_st; f0 += NB * LPS) {
            uint4 ra[NB], rb[NB];
            unsigned msk[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int f = f0 + u * LPS;
                const int r = dvpp.div(f);
                const int xp = dvpp.rem(f, r);
                const int hi = hi0 + r, wi0 = 2 * xp - P;
                const bool rok = sch_ok && f < total_st && (unsigned)hi < (unsigned)a.Hin;
                const bool ok0 = rok && (unsigned)wi0 < (unsigned)a.Win, ok1 = rok && (unsigned)(wi0 + 1) < (unsigned)a.Win;
                const int rowpix = __mul24(hi, a.Win);
                ra[u] = *reinterpret_cast<const uint4*>(in0 + (ok0 ? __umul24((unsigned)(rowpix + wi0), (unsigned)a.in.ld) : 0u));
                rb[u] = *reinterpret_cast<const uint4*>(in0 + (ok1 ? __umul24((unsigned)(rowpix + wi0 + 1), (unsigned)a.in.ld) : 0u));
                msk[u] = (ok0 ? 0x0000ffffu : 0u) | (ok1 ? 0xffff0000u : 0u);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int f = f0 + u * LPS;
                if (f < total_st) {
                    const unsigned wa[4] = {ra[u].x, ra[u].y, ra[u].z, ra[u].w};
                    const unsigned wb[4] = {rb[u].x, rb[u].y, rb[u].z, rb[u].w};
                    unsigned o[8];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const f2_t ya = f2_t{__uint_as_float(wa[i] << 16), __uint_as_float(wa[i] & 0xffff0000u)};
                        const f2_t yb = f2_t{__uint_as_float(wb[i] << 16), __uint_as_float(wb[i] & 0xffff0000u)};
                        const f2_t ha = ya * s8[i] + t8[i], hb = yb * s8[i] + t8[i];
                        const f2_t za = ha * sigmoid2f_(ha);
                        const f2_t zb = hb * sigmoid2f_(hb);
                        o[2 * i] = pack_bf16x2(za.x, zb.x) & msk[u];
                        o[2 * i + 1] = pack_bf16x2(za.y, zb.y) & msk[u];
                    }
                    uint4* dst = reinterpret_cast<uint4*>(tile + f * CS + scv * 8);
                    dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
                    dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
                }
            }
        }
        __syncthreads();
        {
            const int total = nro * Wop;
            const i64 orow0 = ((i64)plane * a.Hout + ho0) * a.Wout;
            T* out0 = outp + orow0 * a.C + chan;
            const int rowdw = Wpp * CS;                  // dwords per staged row
            for (int i = pl; i < total; i += LP) {
                const int oy = dvop.div(i);
                const int j = dvop.rem(i, oy);
                const int ox0 = 2 * j;
                float acc0[4] = {0.f, 0.f, 0.f, 0.f}, acc1[4] = {0.f, 0.f, 0.f, 0.f};
                if constexpr (ST == 1) {
                    const unsigned* tp = tile + (__mul24(oy, Wpp) + j) * CS + cv * 4;
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const uint4 p0 = *reinterpret_cast<const uint4*>(tp + dy * rowdw);
                        const uint4 p1 = *reinterpret_cast<const uint4*>(tp + dy * rowdw + CS);
                        const unsigned a0[4] = {p0.x, p0.y, p0.z, p0.w}, a1[4] = {p1.x, p1.y, p1.z, p1.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            acc0[q] = dot2_bf16(a0[q], wp[dy][0][q], acc0[q]);
                            acc0[q] = dot2_bf16(a1[q], wp[dy][1][q], acc0[q]);
                            acc1[q] = dot2_bf16(a0[q], wp[dy][2][q], acc1[q]);
                            acc1[q] = dot2_bf16(a1[q], wp[dy][3][q], acc1[q]);
                        }
                    }
                } else {
                    // stride 2: output ox reads staged columns 2ox .. 2ox+2 = P[ox] and the low half of P[ox+1]
                    const int jp2 = (ox0 + 2 < Wpp) ? 2 : 1;      // P[ox0+2] only feeds the (possibly invalid) odd output
                    const unsigned* tp = tile + (__mul24(oy * 2, Wpp) + ox0) * CS + cv * 4;
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        const uint4 p0 = *reinterpret_cast<const uint4*>(tp + dy * rowdw);
                        const uint4 p1 = *reinterpret_cast<const uint4*>(tp + dy * rowdw + CS);
                        const uint4 p2 = *reinterpret_cast<const uint4*>(tp + dy * rowdw + jp2 * CS);
                        const unsigned a0[4] = {p0.x, p0.y, p0.z, p0.w}, a1[4] = {p1.x, p1.y, p1.z, p1.w};
                        const unsigned a2[4] = {p2.x, p2.y, p2.z, p2.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            acc0[q] = dot2_bf16(a0[q], wp[dy][0][q], acc0[q]);
                            acc0[q] = dot2_bf16(a1[q], wp[dy][1][q], acc0[q]);
                            acc1[q] = dot2_bf16(a1[q], wp[dy][0][q], acc1[q]);
                            acc1[q] = dot2_bf16(a2[q], wp[dy][1][q], acc1[q]);
                        }
                    }
                }
                if (chan_ok) {
                    const unsigned pix = (unsigned)(__mul24(oy, a.Wout) + ox0);
                    const uint2 pk0 = make_uint2(pack_bf16x2(acc0[0], acc0[1]), pack_bf16x2(acc0[2], acc0[3]));
                    T* dst = out0 + __umul24(pix, (unsigned)a.C);
                    *reinterpret_cast<uint2*>(dst) = pk0;
                    f2_t r0, r1;
                    unpack_pairs<T>(pk0, r0, r1);
                    st0[0] += r0; st0[1] += r1; st1[0] += r0 * r0; st1[1] += r1 * r1;
                    if (ox0 + 1 < a.Wout) {
                        const uint2 pk1 = make_uint2(pack_bf16x2(acc1[0], acc1[1]), pack_bf16x2(acc1[2], acc1[3]));
                        *reinterpret_cast<uint2*>(dst + a.C) = pk1;
                        unpack_pairs<T>(pk1, r0, r1);
                        st0[0] += r0; st0[1] += r1; st1[0] += r0 * r0; st1[1] += r1 * r1;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (a.stats) {
        const float s0[4] = {st0[0].x, st0[0].y, st0[1].x, st0[1].y}, s1[4] = {st1[0].x, st1[0].y, st1[1].x, st1[1].y};
        block_stats_flush<T>(lstat, s0, s1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    }
    DET_EXIT();
}

// ------------------------------------------------------------------------------------------------
// spatial backward: dh1 = (dwS^T dy2) * silu'(h1), dW, Σdh1, Σdh1·ŷ1
// ------------------------------------------------------------------------------------------------
template <typename T, int KS, int ST>
__global__ __launch_bounds__(DWS_BWD_THREADS, (ST == 1 ? DWS_BWD_MINB1 : 3)) void dw_spatial_bwd_kernel(const DwSpatialBwd a) {
    constexpr int NT = DWS_BWD_THREADS;
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = NT / NCV, P = KS / 2;
    constexpr int XB = 4;
    typedef typename SL<T>::raw_t raw_t;
    __shared__ float lstat[2 * CS];
    __shared__ __attribute__((aligned(16))) float lw[KS * KS * CS];      // stencil weights (broadcast reads), later dW
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    for (int i = tid; i < KS * KS * CS; i += NT) {
        int k = i / CS, c = c0 + i % CS;
        lw[i] = c < a.C ? a.w[(i64)k * a.C + c] : 0.f;
    }
    __syncthreads();

    f2_t dwp[KS * KS][2];
#pragma unroll
    for (int k = 0; k < KS * KS; ++k) { dwp[k][0] = f2_t{0.f, 0.f}; dwp[k][1] = f2_t{0.f, 0.f}; }
    float bs[4], bt[4], bm[4], bi[4];
    ldc4(a.y1.v1 + chs, bs); ldc4(a.y1.v2 + chs, bt); ldc4(a.y1.v3 + chs, bm); ldc4(a.y1.v4 + chs, bi);
    const f2_t bs2[2] = {f2_t{bs[0], bs[1]}, f2_t{bs[2], bs[3]}}, bt2[2] = {f2_t{bt[0], bt[1]}, f2_t{bt[2], bt[3]}};
    const f2_t bi2[2] = {f2_t{bi[0], bi[1]}, f2_t{bi[2], bi[3]}};
    const f2_t nbm2[2] = {f2_t{-bm[0] * bi[0], -bm[1] * bi[1]}, f2_t{-bm[2] * bi[2], -bm[3] * bi[3]}};   // yhat = y*bi + nbm
    f2_t sp0[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}}, sp1[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};

    const int Wq = a.Wout + 2;                      // staged columns wo = -1 .. Wout
    const FastDiv dvq(Wq), dvw(a.Win);
    const int nbands = (a.Hin + a.rows_band - 1) / a.rows_band;
    const int ntiles = a.planes * nbands;
    const int s = ST > 0 ? ST : a.stride;
    T* dhp = reinterpret_cast<T*>(a.dh1);
    const T* y1p = reinterpret_cast<const T*>(a.y1.p);
    const T* dpp = reinterpret_cast<const T*>(a.dy.p);
    const T* dqp = reinterpret_cast<const T*>(a.dy.q);
    raw_t* tile = reinterpret_cast<raw_t*>(dyn_smem);
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int plane = tile_id / nbands, band = tile_id % nbands;
        const int hi0 = band * a.rows_band;
        const int nri = (a.Hin - hi0 < a.rows_band) ? a.Hin - hi0 : a.rows_band;
        // output rows that touch input rows [hi0, hi0+nri): ho = (hi + P - dy) / s
        const int lo_num = hi0 + P - (KS - 1);
        const int ho_lo = lo_num >= 0 ? lo_num / s : -((-lo_num + s - 1) / s);
        const int ho_hi = (hi0 + nri - 1 + P) / s;
        const int rows_q = ho_hi - ho_lo + 1;
        const i64 orow0 = (i64)plane * a.Hout * a.Wout;
        // stage dL/dy2 = A1*dh2 + A2*y2 + A3 (BatchNorm backward) with zero padding; flat walk over the (row, column)
        // entries of the tile (flat index == tile index), 2*NB loads in flight per thread
        {
            constexpr int NB = 8;
            const int total_st = rows_q * Wq;
            // BN-backward coefficients: (re)loaded per tile so they do not occupy registers during the tap phase
            float a1[4], a2[4], a3[4];
            ldc4(a.dy.v1 + chs, a1); ldc4(a.dy.v2 + chs, a2); ldc4(a.dy.v3 + chs, a3);
            const f2_t a1v[2] = {f2_t{a1[0], a1[1]}, f2_t{a1[2], a1[3]}}, a2v[2] = {f2_t{a2[0], a2[1]}, f2_t{a2[2], a2[3]}};
            const f2_t a3v[2] = {f2_t{a3[0], a3[1]}, f2_t{a3[2], a3[3]}};
            const T* dp0 = dpp + orow0 * a.dy.ld + chs;
            const T* dq0 = dqp + orow0 * a.dy.ld + chs;
            for (int f0 = pl; f0 < total_st; f0 += NB * LP) {
                raw_t rp[NB], rq[NB];
                bool okv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    const int r = dvq.div(f);
                    const int ho = ho_lo + r, wo = dvq.rem(f, r) - 1;
                    okv[u] = chan_ok && f < total_st && (unsigned)ho < (unsigned)a.Hout && (unsigned)wo < (unsigned)a.Wout;
                    const unsigned off = okv[u] ? __umul24(__mul24(ho, a.Wout) + wo, (unsigned)a.dy.ld) : 0u;
                    rp[u] = ld4_raw<T>(dp0 + off);
                    rq[u] = ld4_raw<T>(dq0 + off);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    if (f < total_st) {
                        f2_t p0, p1, q0, q1;
                        unpack_pairs<T>(rp[u], p0, p1);
                        unpack_pairs<T>(rq[u], q0, q1);
                        p0 = a1v[0] * p0 + (a2v[0] * q0 + a3v[0]);
                        p1 = a1v[1] * p1 + (a2v[1] * q1 + a3v[1]);
                        const float p[4] = {p0.x, p0.y, p1.x, p1.y};
                        tile[f * NCV + cv] = okv[u] ? V4<T>::pack(p) : V4<T>::zero();
                    }
                }
            }
        }
        __syncthreads();
        {
            const i64 prow0 = (i64)plane * a.Hin * a.Win;
            // one tap: g = dL/dy2 at (ho, wo) from the LDS tile; dz += w*g; dW[tap] += z1*g   (channel pairs)
            auto tap_at = [&](const int k, const raw_t* tp, const f2_t* z1, f2_t* dz) {
                f2_t g0, g1;
                unpack_pairs<T>(*tp, g0, g1);
                const float4 wv = *reinterpret_cast<const float4*>(&lw[k * CS + cv * 4]);
                dz[0] += f2_t{wv.x, wv.y} * g0;
                dz[1] += f2_t{wv.z, wv.w} * g1;
                dwp[k][0] += z1[0] * g0;
                dwp[k][1] += z1[1] * g1;
            };
            auto tap = [&](const int k, const int ho, const int wo, const f2_t* z1, f2_t* dz) {
                tap_at(k, tile + ((ho - ho_lo) * Wq + wo + 1) * NCV + cv, z1, dz);
            };
            // everything after the taps: dh1 = dz * silu'(h1), store, BN-backward sums
            // per-plane base pointers + 32-bit in-plane offsets (24-bit multiplies): no 64-bit VALU address math
            T* dh0 = dhp + prow0 * a.C + chan;
            const T* y10 = y1p + prow0 * a.y1.ld + chs;
            auto finish_at = [&](const int pix, const f2_t* y, const f2_t* dsl, const f2_t* dz) {
                const f2_t d0 = dz[0] * dsl[0], d1 = dz[1] * dsl[1];
                float dh[4] = {d0.x, d0.y, d1.x, d1.y};
                const typename V4<T>::raw_t packed = V4<T>::pack(dh);
                *reinterpret_cast<typename V4<T>::raw_t*>(dh0 + __umul24((unsigned)pix, (unsigned)a.C)) = packed;
                f2_t r0, r1;
                unpack_pairs<T>(packed, r0, r1);              // statistics of the values as stored
                sp0[0] += r0; sp0[1] += r1;
                sp1[0] += r0 * (y[0] * bi2[0] + nbm2[0]);
                sp1[1] += r1 * (y[1] * bi2[1] + nbm2[1]);
            };
            auto finish = [&](const int hi, const int wi, const f2_t* y, const f2_t* dsl, const f2_t* dz) {
                finish_at(hi * a.Win + wi, y, dsl, dz);
            };
            auto activate = [&](const raw_t& raw, f2_t* y, f2_t* z1, f2_t* dsl) {
                unpack_pairs<T>(raw, y[0], y[1]);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const f2_t h = y[i] * bs2[i] + bt2[i];
                    const f2_t sg = sigmoid2f_(h);
                    z1[i] = h * sg;
                    dsl[i] = sg * (1.0f + h * (1.0f - sg));
                }
            };
            // Pixels are walked as ONE flat index space (rows x columns of the band / of a parity class), XB loads in
            // flight per thread, so narrow planes (W = 8..16) still fill all pixel lanes and every load batch.
            if constexpr (ST == 2 && KS == 3) {
                // stride 2: an input pixel receives 1, 2, 2 or 4 taps depending on the parity of (hi, wi): one pass per
                // parity class, taps known at compile time.
                auto run_class = [&](auto hp_c, auto px_c) {
                    constexpr int HP = decltype(hp_c)::value, PX = decltype(px_c)::value;
                    const int hfirst = hi0 + (((hi0 & 1) == HP) ? 0 : 1);
                    const int nr = (hi0 + nri - hfirst + 1) >> 1;
                    const int nc = (a.Win - PX + 1) >> 1;
                    const int total = nr > 0 ? nr * nc : 0;
                    // pixel (k, j) of the class: hi = hfirst + 2k, wi = PX + 2j.  Its taps read tile entries at
                    // workgroup-uniform offsets from entry (k, j): one index per pixel, uniform offsets per tap.
                    const int wdiff = Wq - nc;
                    const FastDiv dvc(nc > 0 ? nc : 1);
                    const int r_dn = ((hfirst + HP) >> 1) - ho_lo;          // row of (hi + HP) >> 1 at k = 0
                    const int o00 = (r_dn * Wq + 1) * NCV;                  // (hi+HP)>>1, (wi-PX)>>1 ... column j
                    const int o01 = o00 + NCV;                              // column j + 1
                    const int o10 = o00 - Wq * NCV, o11 = o01 - Wq * NCV;   // row (hi-1)>>1 (odd rows only)
                    for (int i0 = pl; i0 < total; i0 += XB * LP) {
                        raw_t ry[XB];
                        int ti[XB];
                        int gg[XB];
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            const int i = i0 + u * LP;
                            const bool ok = chan_ok && i < total;
                            const int iv = ok ? i : 0;
                            const int k = dvc.div(iv);
                            const int j = dvc.rem(iv, k);
                            ti[u] = (iv + __mul24(k, wdiff)) * NCV + cv;
                            gg[u] = __mul24(hfirst + 2 * k, a.Win) + (PX + 2 * j);
                            ry[u] = ld4_raw<T>(y10 + __umul24((unsigned)gg[u], (unsigned)a.y1.ld));
                        }
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            if (!chan_ok || i0 + u * LP >= total) continue;
                            f2_t y[2], z1[2], dsl[2], dz[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};
                            activate(ry[u], y, z1, dsl);
                            const raw_t* tp = tile + ti[u];
                            if constexpr (HP == 0 && PX == 0) {
                                tap_at(4, tp + o00, z1, dz);
                            } else if constexpr (HP == 0 && PX == 1) {
                                tap_at(3, tp + o01, z1, dz); tap_at(5, tp + o00, z1, dz);
                            } else if constexpr (HP == 1 && PX == 0) {
                                tap_at(1, tp + o00, z1, dz); tap_at(7, tp + o10, z1, dz);
                            } else {
                                tap_at(0, tp + o01, z1, dz); tap_at(2, tp + o00, z1, dz);
                                tap_at(6, tp + o11, z1, dz); tap_at(8, tp + o10, z1, dz);
                            }
                            finish_at(gg[u], y, dsl, dz);
                        }
                    }
                };
                run_class(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
                run_class(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
                run_class(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
                run_class(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
            } else {
                const int total = nri * a.Win;
                if constexpr (ST == 1) {
                    // stride 1: every tap is valid (the zero halo supplies the borders): branch-free.  The tile entry of
                    // tap (dy, dx) sits at a fixed offset from the pixel's own entry: one index per pixel, not per tap.
                    const int wdiff = Wq - a.Win;                // staged row is wider than the input row
                    const int rowstep = Wq * NCV;
                    const int grow0 = hi0 * a.Win;
                    for (int i0 = pl; i0 < total; i0 += XB * LP) {
                        raw_t ry[XB];
                        int ii[XB], ti[XB];
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            const int i = i0 + u * LP;
                            const bool ok = chan_ok && i < total;
                            ii[u] = ok ? i : 0;
                            const int iy = dvw.div(ii[u]);
                            ti[u] = (ii[u] + __mul24(iy, wdiff) + (P + 2 - KS)) * NCV + cv;
                            ry[u] = ld4_raw<T>(y10 + __umul24((unsigned)(grow0 + ii[u]), (unsigned)a.y1.ld));
                        }
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            if (!chan_ok || i0 + u * LP >= total) continue;
                            f2_t y[2], z1[2], dsl[2], dz[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};
                            activate(ry[u], y, z1, dsl);
                            const raw_t* tp = tile + ti[u];
#pragma unroll
                            for (int dy = 0; dy < KS; ++dy) {
                                const raw_t* tr = tp + (KS - 1 - dy) * rowstep;
#pragma unroll
                                for (int dx = 0; dx < KS; ++dx) tap_at(dy * KS + dx, tr + (KS - 1 - dx) * NCV, z1, dz);
                            }
                            finish_at(grow0 + ii[u], y, dsl, dz);
                        }
                    }
                } else {
                for (int i0 = pl; i0 < total; i0 += XB * LP) {
                    raw_t ry[XB];
                    int hh[XB], ww[XB];
#pragma unroll
                    for (int u = 0; u < XB; ++u) {
                        const int i = i0 + u * LP;
                        const bool ok = chan_ok && i < total;
                        const int iy = ok ? i / a.Win : 0;
                        hh[u] = hi0 + iy;
                        ww[u] = (ok ? i : 0) - iy * a.Win;
                        ry[u] = ld4_raw<T>(y10 + (ok ? (i64)hh[u] * a.Win + ww[u] : 0) * a.y1.ld);
                    }
#pragma unroll
                    for (int u = 0; u < XB; ++u) {
                        if (!chan_ok || i0 + u * LP >= total) continue;
                        const int hi = hh[u], wi = ww[u];
                        f2_t y[2], z1[2], dsl[2], dz[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};
                        activate(ry[u], y, z1, dsl);
#pragma unroll
                        for (int dy = 0; dy < KS; ++dy) {
                            const int nh = hi + P - dy;
                            if (nh < 0 || nh % s != 0) continue;
                            const int ho = nh / s;
                            if (ho > ho_hi) continue;
#pragma unroll
                            for (int dx = 0; dx < KS; ++dx) {
                                const int nw = wi + P - dx;
                                if (nw < 0 || nw % s != 0) continue;
                                const int wo = nw / s;
                                if (wo > a.Wout) continue;
                                tap(dy * KS + dx, ho, wo, z1, dz);
                            }
                        }
                        finish(hi, wi, y, dsl, dz);
                    }
                }
                }
            }
        }
        __syncthreads();
    }
    // weight gradient: reduce over the threads sharing a channel vector through LDS, then global fp32 atomics
    __syncthreads();
    for (int i = tid; i < KS * KS * CS; i += NT) lw[i] = 0.f;
    __syncthreads();
    DET_WAVES_BEGIN
    if (chan_ok) {
#pragma unroll
        for (int k = 0; k < KS * KS; ++k) {
            atomicAdd(&lw[k * CS + cv * 4 + 0], dwp[k][0].x);
            atomicAdd(&lw[k * CS + cv * 4 + 1], dwp[k][0].y);
            atomicAdd(&lw[k * CS + cv * 4 + 2], dwp[k][1].x);
            atomicAdd(&lw[k * CS + cv * 4 + 3], dwp[k][1].y);
        }
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
    for (int i = tid; i < KS * KS * CS; i += NT) {
        int k = i / CS, c = c0 + i % CS;
        if (c < a.C) atomicAdd(a.dw + (i64)c * (KS * KS) + k, lw[i]);
    }
    const float st0[4] = {sp0[0].x, sp0[0].y, sp0[1].x, sp0[1].y}, st1[4] = {sp1[0].x, sp1[0].y, sp1[1].x, sp1[1].y};
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// ------------------------------------------------------------------------------------------------
// temporal forward: y3[t] = sum_k w[k] z2[t + k - P]
// ------------------------------------------------------------------------------------------------
// ZOUT (eval mode): the output is z3 = SiLU(BN3(y3)) and the SqueezeExcite pooling sums ride along (see dwn.h)
template <typename T, int KT, bool ZOUT = false>
__global__ __launch_bounds__(256) void dw_temporal_fwd_kernel(const DwTemporalFwd a) {
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = SL<T>::LP, P = KT / 2;
    typedef typename SL<T>::raw_t raw_t;
    __shared__ float lstat[2 * CS];
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    __syncthreads();
    float w[KT][4], bs[4], bt[4];
#pragma unroll
    for (int k = 0; k < KT; ++k) ldc4(a.w + (i64)k * a.C + chs, w[k]);
    ldc4(a.in.v1 + chs, bs);
    ldc4(a.in.v2 + chs, bt);
    float st0[4] = {0.f, 0.f, 0.f, 0.f}, st1[4] = {0.f, 0.f, 0.f, 0.f};
    [[maybe_unused]] float zs[4], zt[4];
    if constexpr (ZOUT) { ldc4(a.z_scale + chs, zs); ldc4(a.z_shift + chs, zt); }

    const i64 npos = (i64)a.B * a.HW;
    const T* inp = reinterpret_cast<const T*>(a.in.p);
    T* outp = reinterpret_cast<T*>(a.out);
    const i64 tstride = (i64)a.HW * a.C;
    if (chan_ok) {
        // ZOUT: a workgroup takes a CONTIGUOUS run of positions, so its lanes stay inside one sample for many iterations and the
        // SqueezeExcite pooling sums wait in registers (pacc) until the sample changes: ~10x fewer atomics than a flush per
        // position (5 M eight-byte atomics on 40 K addresses per launch at the inference batch)
        i64 p_beg = (i64)blockIdx.x * LP + pl, p_end = npos, p_step = (i64)gridDim.x * LP;
        if constexpr (ZOUT) {
            const i64 per = ((npos + (i64)gridDim.x * LP - 1) / ((i64)gridDim.x * LP)) * LP;
            p_beg = (i64)blockIdx.x * per + pl;
            p_end = p_beg - pl + per < npos ? p_beg - pl + per : npos;
            p_step = LP;
        }
        [[maybe_unused]] float pacc[4] = {0.f, 0.f, 0.f, 0.f};
        [[maybe_unused]] i64 pacc_b = -1;
        // adds pacc into pooled[pacc_b] (64-bit fixed point, pool_fix: whatever the arrival order, the same total).  The wave's
        // pixel lanes that share a channel vector hold one sample almost always: then they are folded with xor-shuffles and
        // the first NCV lanes add 4 channels each.  Called by all lanes that are still in the loop (or by all, after it).
        [[maybe_unused]] auto pool_flush = [&]() {
            const int b0 = __builtin_amdgcn_readfirstlane((int)pacc_b);
            const bool uniform = __popcll(__ballot(1)) == 64 && __all((int)pacc_b == b0) && b0 >= 0;
            if (uniform) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int o = NCV; o < 64; o <<= 1) pacc[i] += __shfl_xor(pacc[i], o);
                if ((tid & 63) < NCV) {
                    unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.pooled) + (i64)b0 * a.C + chan;
#pragma unroll
                    for (int i = 0; i < 4; ++i) atomicAdd(dst + i, (unsigned long long)pool_fix(pacc[i]));
                }
            } else if (pacc_b >= 0) {
                unsigned long long* dst = reinterpret_cast<unsigned long long*>(a.pooled) + pacc_b * a.C + chan;
#pragma unroll
                for (int i = 0; i < 4; ++i) atomicAdd(dst + i, (unsigned long long)pool_fix(pacc[i]));
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) pacc[i] = 0.f;
        };
        for (i64 pos = p_beg; pos < p_end; pos += p_step) {
            const i64 b = pos / a.HW, hw = pos % a.HW;
            const T* ip = inp + (b * a.T * a.HW + hw) * a.C + chan;      // element (t = 0)
            T* op = outp + (b * a.T * a.HW + hw) * a.C + chan;
            // ring of KT slots, KT frames per unrolled batch: at step u of a batch z2(t + k - P) lives in slot (u + k) % KT — compile-time
            // indices, no register shifting (the shifting version spent 52 moves per 16 outputs)
            float win[KT][4];
            [[maybe_unused]] float ps[4] = {0.f, 0.f, 0.f, 0.f};         // ZOUT: this position's sums over t of the stored z3
#pragma unroll
            for (int k = 0; k < KT - 1; ++k) {
                int t = k - P;
                if (t >= 0 && t < a.T) { ld4<T>(ip + t * tstride, win[k]); bn_silu4(win[k], bs, bt); }
                else { win[k][0] = win[k][1] = win[k][2] = win[k][3] = 0.f; }
            }
            [[maybe_unused]] T* sp = op;                                  // KT > 5: frame t of the next store
            [[maybe_unused]] const T* lp = ip + P * tstride;           // KT > 5: frame t0 + u + P of the next load
            for (int t0 = 0; t0 < a.T; t0 += KT) {
                raw_t raw[KT];
#pragma unroll
                for (int u = 0; u < KT; ++u) {
                    int tl = t0 + u + P;
                    if constexpr (KT > 5) {
                        // sizes 7 and 9: the look-ahead pointer advances in vector registers; KT scalar offsets at once run the
                        // deterministic build out of scalar registers
                        raw[u] = ld4_raw<T>(tl < a.T ? lp : ip);
                        lp += tstride;
                    } else {
                        raw[u] = ld4_raw<T>(ip + (tl < a.T ? tl : 0) * tstride);
                    }
                }
#pragma unroll
                for (int u = 0; u < KT; ++u) {
                    int t = t0 + u;
                    if (t >= a.T) break;
                    const int sn = (u + KT - 1) % KT;                   // newest slot: frame t + P
                    if (t + P < a.T) { V4<T>::unpack(raw[u], win[sn]); bn_silu4(win[sn], bs, bt); }
                    else { win[sn][0] = win[sn][1] = win[sn][2] = win[sn][3] = 0.f; }
                    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < KT; ++k)
#pragma unroll
                        for (int i = 0; i < 4; ++i) acc[i] = fmaf(w[k][i], win[(u + k) % KT][i], acc[i]);
                    if constexpr (ZOUT) {
                        float z[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) z[i] = fmaf(round_t<T>(acc[i]), zs[i], zt[i]);     // BN3 + SiLU of the value a stored y3 holds
                        silu_n<4>(z);
#pragma unroll
                        for (int i = 0; i < 4; ++i) ps[i] += round_t<T>(z[i]);
                        st4<T>(KT > 5 ? sp : op + t * tstride, z);
                    } else {
                        st4<T>(KT > 5 ? sp : op + t * tstride, acc);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float r = round_t<T>(acc[i]);
                            st0[i] += r;
                            st1[i] += r * r;
                        }
                    }
                    if constexpr (KT > 5) sp += tstride;
                }
            }
            if constexpr (ZOUT) {
                if (a.pooled) {
                    if (__any(b != pacc_b)) { pool_flush(); pacc_b = b; }      // a lane entered another sample: everybody flushes
#pragma unroll
                    for (int i = 0; i < 4; ++i) pacc[i] += ps[i];
                }
            }
        }
        if constexpr (ZOUT) {
            if (a.pooled) pool_flush();
        }
    }
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// ------------------------------------------------------------------------------------------------
// temporal backward: dz2[t] = sum_k w[k] dy3[t - k + P];  dW[k] = sum z2[t] dy3[t - k + P];
//                    dh2 = dz2 * silu'(h2);  Σdh2, Σdh2·ŷ2
// dy3 is never materialised: DYK = LD_DY3 rebuilds it from (du, y3) — SE gate/gradient, SiLU' and the bn3
// backward affine — DYK = LD_AFFINE2 from (dh3, y3).
// ------------------------------------------------------------------------------------------------
template <typename T, int KT, int DYK, int TB>
__global__ __launch_bounds__(256, TB >= 8 ? 2 : 3) void dw_temporal_bwd_kernel(const DwTemporalBwd a) {
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = SL<T>::LP, P = KT / 2;
    typedef typename SL<T>::raw_t raw_t;
    __shared__ float lstat[2 * CS];
    __shared__ float lw[KT * CS];
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    for (int i = tid; i < KT * CS; i += 256) lw[i] = 0.f;
    __syncthreads();
    float w[KT][4], dwacc[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        ldc4(a.w + (i64)k * a.C + chs, w[k]);
        dwacc[k][0] = dwacc[k][1] = dwacc[k][2] = dwacc[k][3] = 0.f;
    }
    float bs[4], bt[4], bm[4], bi[4], a1[4], a2[4], a3[4], s3[4] = {0, 0, 0, 0}, t3[4] = {0, 0, 0, 0};
    ldc4(a.y2.v1 + chs, bs); ldc4(a.y2.v2 + chs, bt); ldc4(a.y2.v3 + chs, bm); ldc4(a.y2.v4 + chs, bi);
    ldc4(a.dy.v1 + chs, a1); ldc4(a.dy.v2 + chs, a2); ldc4(a.dy.v3 + chs, a3);
    if constexpr (DYK == LD_DY3) { ldc4(a.dy.v4 + chs, s3); ldc4(a.dy.v5 + chs, t3); }
    float st0[4] = {0.f, 0.f, 0.f, 0.f}, st1[4] = {0.f, 0.f, 0.f, 0.f};

    const i64 npos = (i64)a.B * a.HW;
    T* dhp = reinterpret_cast<T*>(a.dh2);
    const T* y2p = reinterpret_cast<const T*>(a.y2.p);
    const T* dpp = reinterpret_cast<const T*>(a.dy.p);
    const T* dqp = reinterpret_cast<const T*>(a.dy.q);
    const i64 tstride = (i64)a.HW * a.C;

    auto make_dy = [&](const raw_t& rp, const raw_t& rq, const float* g, const float* g2, float* o) {
        float p[4], q[4];
        V4<T>::unpack(rp, p);
        V4<T>::unpack(rq, q);
        [[maybe_unused]] float sp4[4];
        if constexpr (DYK == LD_DY3) {
            float h4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) h4[i] = fmaf(q[i], s3[i], t3[i]);
            silu_grad_n<4>(h4, sp4);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (DYK == LD_DY3) {
                float dh = fmaf(p[i], g[i], g2[i]) * sp4[i];
                o[i] = fmaf(a1[i], dh, fmaf(a2[i], q[i], a3[i]));
            } else {
                o[i] = fmaf(a1[i], p[i], fmaf(a2[i], q[i], a3[i]));
            }
        }
    };

    if (chan_ok) {
        for (i64 pos = (i64)blockIdx.x * LP + pl; pos < npos; pos += (i64)gridDim.x * LP) {
            const i64 b = pos / a.HW, hw = pos % a.HW;
            const i64 e0 = (b * a.T * a.HW + hw) * a.C + chan;
            float g[4] = {1.f, 1.f, 1.f, 1.f}, g2[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (DYK == LD_DY3) {
                ldc4(a.dy.gate + b * a.dy.gate_ld + chan, g);
                ldc4(a.dy.gate2 + b * a.dy.gate_ld + chan, g2);
            }
            float win[KT][4];                           // win[j] = dy3(t + j - P)
#pragma unroll
            for (int k = 0; k < KT - 1; ++k) {
                int t = k - P;
                if (t >= 0 && t < a.T) make_dy(ld4_raw<T>(dpp + e0 + t * tstride), ld4_raw<T>(dqp + e0 + t * tstride), g, g2, win[k]);
                else { win[k][0] = win[k][1] = win[k][2] = win[k][3] = 0.f; }
            }
            for (int t0 = 0; t0 < a.T; t0 += TB) {
                raw_t rp[TB], rq[TB], ry[TB];
#pragma unroll
                for (int u = 0; u < TB; ++u) {
                    int tl = t0 + u + P;
                    i64 off = e0 + (tl < a.T ? tl : 0) * tstride;
                    rp[u] = ld4_raw<T>(dpp + off);
                    rq[u] = ld4_raw<T>(dqp + off);
                    int ty = t0 + u;
                    ry[u] = ld4_raw<T>(y2p + e0 + (ty < a.T ? ty : 0) * tstride);
                }
#pragma unroll
                for (int u = 0; u < TB; ++u) {
                    int t = t0 + u;
                    if (t >= a.T) break;
                    if (t + P < a.T) make_dy(rp[u], rq[u], g, g2, win[KT - 1]);
                    else { win[KT - 1][0] = win[KT - 1][1] = win[KT - 1][2] = win[KT - 1][3] = 0.f; }
                    float y[4], dh[4];
                    V4<T>::unpack(ry[u], y);
                    float h4[4], sg4[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) h4[i] = fmaf(y[i], bs[i], bt[i]);
                    sigmoid_n<4>(h4, sg4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float h = h4[i], sg = sg4[i];
                        float z2 = h * sg;
                        float dz = 0.f;
#pragma unroll
                        for (int k = 0; k < KT; ++k) {
                            float gk = win[KT - 1 - k][i];
                            dz = fmaf(w[k][i], gk, dz);
                            dwacc[k][i] = fmaf(z2, gk, dwacc[k][i]);
                        }
                        dh[i] = dz * (sg * (1.0f + h * (1.0f - sg)));
                    }
                    st4<T>(dhp + e0 + t * tstride, dh);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float r = round_t<T>(dh[i]);
                        st0[i] += r;
                        st1[i] += r * (y[i] - bm[i]) * bi[i];
                    }
#pragma unroll
                    for (int k = 0; k < KT - 1; ++k)
#pragma unroll
                        for (int i = 0; i < 4; ++i) win[k][i] = win[k + 1][i];
                }
            }
        }
    }
    DET_WAVES_BEGIN
    if (chan_ok) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(&lw[k * CS + cv * 4 + i], dwacc[k][i]);
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
    for (int i = tid; i < KT * CS; i += 256) {
        int k = i / CS, c = c0 + i % CS;
        if (c < a.C) atomicAdd(a.dw + (i64)c * KT + k, lw[i]);
    }
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// persistent grids (dwn_launch.h): one full resident round of workgroups, `slices` of them per x index.  Fallback 2 workgroups per
// CU when the occupancy query fails: historical
template <typename K, typename A>
static int launch_dw(K kernel, int threads, size_t dyn_lds, int slices, i64 work, hipStream_t s, const A& a) {
    return launch_resident(kernel, threads, dyn_lds, 2, slices, work, false, s, a);
}
// The instantiation ladder of the banded spatial kernels: f gets the stride as a compile-time constant (1, 2, or 0 = read a.stride)
// and, forward, the workgroup size: 512 threads on planes of 512 pixels and more (`big`), else 256; the generic stride is built for 256
template <typename F>
static int by_stride(int stride, F f) {
    if (stride == 1) return f(std::integral_constant<int, 1>{});
    if (stride == 2) return f(std::integral_constant<int, 2>{});
    return f(std::integral_constant<int, 0>{});
}
template <typename F>
static int by_stride_threads(int stride, bool big, F f) {
    return by_stride(stride, [&](auto st) {
        if constexpr (st.value != 0) if (big) return f(st, std::integral_constant<int, 512>{});
        return f(st, std::integral_constant<int, 256>{});
    });
}

// ------------------------------------------------------------------------------------------------
// spatial kernel sizes 5 and 7 (P = KS/2 = 2, 3), both storage types, stride 1, 2 and generic.
//
// 25 / 49 taps of 4 channels do not fit a thread's registers next to anything else (100 / 196 floats of weights forward, as
// many weight-gradient accumulators backward), so neither is held per thread:
//   * stencil weights live in LDS as [tap][channel] floats and are read as one broadcast ds_read_b128 per tap, shared by the
//     XB pixels a thread has in flight (forward: XB outputs, backward: XB input pixels);
//   * the weight gradient is split by TAP ROW over the waves of the workgroup: wave v owns tap row v % KS for the whole
//     persistent kernel and keeps its KS accumulators (4 channels each) in registers; it needs z1 of pixels other threads
//     activated, so the data-gradient pass leaves z1 of the band in a second LDS tile (zero halo of P columns).
// Backward, per band of input rows:  stage g = dL/dy2 (true halo: ceil(P/s) columns each side, rows floor((hi0-P)/s) ..
// (hi0+nri-1+P)/s)  ->  pass A: dh1 = (W^T g) * SiLU'(h1), BatchNorm-backward sums, z1 -> LDS  ->  pass B: dW[dy][dx] +=
// sum over outputs (ho, wo) of g(ho, wo) * z1(s*ho - P + dy, s*wo - P + dx), the forward's own indexing: no parity cases, and
// every product is a real tap at any stride.
// ------------------------------------------------------------------------------------------------
#define DWS_KS_BWD_THREADS 512
// dynamic LDS the band choice may fill: two 512-thread workgroups per CU next to the static weight table
#define DWS_KS_LDS_BUDGET(static_bytes) (80 * 1024 - (int)(static_bytes) - 1024)

template <typename T, int KS, int ST, int NT>
__global__ __launch_bounds__(NT, 4) void dw_spatial_fwd_ks_kernel(const DwSpatialFwd a) {
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = NT / NCV, P = KS / 2;
    constexpr int XB = 4;                              // outputs per thread sharing one weight read per tap
    typedef typename SL<T>::raw_t raw_t;
    const int stride = ST > 0 ? ST : a.stride;
    __shared__ float lstat[2 * CS];
    __shared__ __attribute__((aligned(16))) float lw[KS * KS * CS];      // stencil weights [tap][channel] (broadcast reads)
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;               // safe channel for predicated loads
    if (tid < 2 * CS) lstat[tid] = 0.f;
    for (int i = tid; i < KS * KS * CS; i += NT) {
        const int k = i / CS, c = c0 + i % CS;
        lw[i] = c < a.C ? a.w[(i64)k * a.C + c] : 0.f;
    }
    __syncthreads();

    float bs[4], bt[4];
    ldc4(a.in.v1 + chs, bs);
    ldc4(a.in.v2 + chs, bt);
    f2_t st0[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}}, st1[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};

    const int Wp = a.Win + 2 * P;
    const FastDiv dvp(Wp), dvo(a.Wout);
    const int nbands = (a.Hout + a.rows_band - 1) / a.rows_band;
    const int ntiles = a.planes * nbands;
    const T* inp = reinterpret_cast<const T*>(a.in.p);
    T* outp = reinterpret_cast<T*>(a.out);
    raw_t* tile = reinterpret_cast<raw_t*>(dyn_smem);
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int plane = tile_id / nbands, band = tile_id % nbands;
        const int ho0 = band * a.rows_band;
        const int nro = (a.Hout - ho0 < a.rows_band) ? a.Hout - ho0 : a.rows_band;
        const int hi0 = ho0 * stride - P;
        const int rows_in = (nro - 1) * stride + KS;
        const i64 plane_row0 = (i64)plane * a.Hin * a.Win;
        // stage the activated input rows with their zero halo: flat (row, column) walk, flat index == tile index, NB loads in flight
        {
            constexpr int NB = 8;
            const int total_st = rows_in * Wp;
            const T* in0 = inp + plane_row0 * a.in.ld;
            for (int f0 = pl; f0 < total_st; f0 += NB * LP) {
                raw_t raw[NB];
                bool okv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    const int r = dvp.div(f);
                    const int hi = hi0 + r, wi = dvp.rem(f, r) - P;
                    okv[u] = chan_ok && f < total_st && (unsigned)hi < (unsigned)a.Hin && (unsigned)wi < (unsigned)a.Win;
                    const unsigned off = okv[u] ? __umul24(__mul24(hi, a.Win) + wi, (unsigned)a.in.ld) : 0u;
                    raw[u] = ld4_raw<T>(in0 + off + chs);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    if (f < total_st) {
                        float v[4];
                        V4<T>::unpack(raw[u], v);
                        bn_silu4(v, bs, bt);
                        tile[f * NCV + cv] = okv[u] ? V4<T>::pack(v) : V4<T>::zero();
                    }
                }
            }
        }
        __syncthreads();
        {
            const int total = nro * a.Wout;
            const i64 orow0 = ((i64)plane * a.Hout + ho0) * a.Wout;
            T* out0 = outp + orow0 * a.C + chan;
            const int wdiff = stride * Wp - stride * a.Wout;   // tile index of output i = i*stride + oy*wdiff (+ taps)
            const int rowstep = Wp * NCV;
            for (int i0 = pl; i0 < total; i0 += XB * LP) {
                int ti[XB];
                f2_t acc[XB][2];
#pragma unroll
                for (int u = 0; u < XB; ++u) {
                    const int i = i0 + u * LP;
                    const int iv = i < total ? i : 0;           // lanes past the band read output 0's taps and store nothing
                    const int oy = dvo.div(iv);
                    ti[u] = (iv * stride + __mul24(oy, wdiff)) * NCV + cv;
                    acc[u][0] = f2_t{0.f, 0.f}; acc[u][1] = f2_t{0.f, 0.f};
                }
                // a LOOP over tap rows (not unrolled): unrolled, the compiler hoists all KS*KS weight reads out of the pixel loop
                // and spills them; one row's KS weight vectors (4 channels each) is what a thread holds at a time
#pragma unroll 1
                for (int dy = 0; dy < KS; ++dy) {
                    const float* wr = &lw[dy * KS * CS + cv * 4];
                    const raw_t* tr = tile + dy * rowstep;
#pragma unroll
                    for (int dx = 0; dx < KS; ++dx) {
                        const float4 wv = *reinterpret_cast<const float4*>(wr + dx * CS);
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            f2_t v0, v1;
                            unpack_pairs<T>(tr[ti[u] + dx * NCV], v0, v1);
                            acc[u][0] += f2_t{wv.x, wv.y} * v0;
                            acc[u][1] += f2_t{wv.z, wv.w} * v1;
                        }
                        __builtin_amdgcn_sched_barrier(0);       // one tap's reads in flight: a whole row's would not fit the registers
                    }
                }
#pragma unroll
                for (int u = 0; u < XB; ++u) {
                    const int i = i0 + u * LP;
                    if (chan_ok && i < total) {
                        const float o[4] = {acc[u][0].x, acc[u][0].y, acc[u][1].x, acc[u][1].y};
                        const raw_t packed = V4<T>::pack(o);
                        *reinterpret_cast<raw_t*>(out0 + __umul24((unsigned)i, (unsigned)a.C)) = packed;
                        f2_t r0, r1;
                        unpack_pairs<T>(packed, r0, r1);              // statistics of the values as stored
                        st0[0] += r0; st0[1] += r1; st1[0] += r0 * r0; st1[1] += r1 * r1;
                    }
                }
            }
        }
        __syncthreads();
    }
    if (a.stats) {
        const float s0[4] = {st0[0].x, st0[0].y, st0[1].x, st0[1].y}, s1[4] = {st1[0].x, st1[0].y, st1[1].x, st1[1].y};
        block_stats_flush<T>(lstat, s0, s1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    }
    DET_EXIT();
}

template <typename T, int KS, int ST>
__global__ __launch_bounds__(DWS_KS_BWD_THREADS, DWS_KS_BWD_THREADS / 128) void dw_spatial_bwd_ks_kernel(const DwSpatialBwd a) {
    constexpr int NT = DWS_KS_BWD_THREADS, NW = NT / 64;
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = NT / NCV, PLW = 64 / NCV, P = KS / 2;
    constexpr int XB = 1;                              // input pixels per thread and batch (2 would share a weight read but spill)
    static_assert(NW >= KS, "every tap row needs a wave");
    typedef typename SL<T>::raw_t raw_t;
    __shared__ float lstat[2 * CS];
    __shared__ __attribute__((aligned(16))) float lw[KS * KS * CS];      // stencil weights (broadcast reads), later dW
    // BatchNorm-1 scale, shift, invstd, -mean*invstd per channel: read where a pixel is activated / finished instead of held
    // (16 registers that the tap-row accumulators need)
    __shared__ __attribute__((aligned(16))) float lbn[4 * CS];
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    const int s = ST > 0 ? ST : a.stride;
    const int HL = (P + s - 1) / s;                  // halo columns of the gradient tile, each side
    const int Wq = a.Wout + 2 * HL;                  // staged gradient columns wo = -HL .. Wout - 1 + HL
    const int Wz = a.Win + 2 * P;                    // z1 tile columns wi = -P .. Win - 1 + P (halo stays zero)
    const int rows_q_max = s == 1 ? a.rows_band + 2 * P : (a.rows_band - 1 + 2 * P) / s + 2;      // as the launcher sizes the tile
    raw_t* tile = reinterpret_cast<raw_t*>(dyn_smem);
    raw_t* zt = tile + rows_q_max * Wq * NCV;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    if (tid < CS) {                                  // yhat = y*invstd + nbm
        const int c = c0 + tid < a.C ? c0 + tid : 0;
        lbn[tid] = a.y1.v1[c]; lbn[CS + tid] = a.y1.v2[c]; lbn[2 * CS + tid] = a.y1.v4[c]; lbn[3 * CS + tid] = -a.y1.v3[c] * a.y1.v4[c];
    }
    // (the set-up loops stay rolled: unrolled, their loads push the values the main loop keeps into scratch)
#pragma unroll 1
    for (int i = tid; i < KS * KS * CS; i += NT) {
        const int k = i / CS, c = c0 + i % CS;
        lw[i] = c < a.C ? a.w[(i64)k * a.C + c] : 0.f;
    }
#pragma unroll 1
    for (int i = tid; i < a.rows_band * Wz * NCV; i += NT) zt[i] = V4<T>::zero();
    __syncthreads();

    // pass B role: this wave's tap row, its lane among the lanes of that row, and their number
    const int wave = tid >> 6;
    const int mydy = wave % KS;
    const int gl = (wave / KS) * PLW + (pl % PLW);
    const int gn = ((NW - mydy + KS - 1) / KS) * PLW;
    f2_t dwr[KS][2];
#pragma unroll
    for (int k = 0; k < KS; ++k) { dwr[k][0] = f2_t{0.f, 0.f}; dwr[k][1] = f2_t{0.f, 0.f}; }
    f2_t sp0[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}}, sp1[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};

    const FastDiv dvq(Wq), dvo(a.Wout);
    const int nbands = (a.Hin + a.rows_band - 1) / a.rows_band;
    const int ntiles = a.planes * nbands;
    T* dhp = reinterpret_cast<T*>(a.dh1);
    const T* y1p = reinterpret_cast<const T*>(a.y1.p);
    const T* dpp = reinterpret_cast<const T*>(a.dy.p);
    const T* dqp = reinterpret_cast<const T*>(a.dy.q);
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int plane = tile_id / nbands, band = tile_id % nbands;
        const int hi0 = band * a.rows_band;
        const int nri = (a.Hin - hi0 < a.rows_band) ? a.Hin - hi0 : a.rows_band;
        // output rows that touch input rows [hi0, hi0+nri): ho = (hi + P - dy) / s
        const int lo_num = hi0 - P;
        const int ho_lo = lo_num >= 0 ? lo_num / s : -((-lo_num + s - 1) / s);
        const int ho_hi = (hi0 + nri - 1 + P) / s;
        const int rows_q = ho_hi - ho_lo + 1;
        const i64 orow0 = (i64)plane * a.Hout * a.Wout;
        // stage dL/dy2 = A1*dh2 + A2*y2 + A3 (BatchNorm backward) with zero padding; flat walk, 2*NB loads in flight per thread
        {
            constexpr int NB = 2;
            const int total_st = rows_q * Wq;
            float a1[4], a2[4], a3[4];
            ldc4(a.dy.v1 + chs, a1); ldc4(a.dy.v2 + chs, a2); ldc4(a.dy.v3 + chs, a3);
            const f2_t a1v[2] = {f2_t{a1[0], a1[1]}, f2_t{a1[2], a1[3]}}, a2v[2] = {f2_t{a2[0], a2[1]}, f2_t{a2[2], a2[3]}};
            const f2_t a3v[2] = {f2_t{a3[0], a3[1]}, f2_t{a3[2], a3[3]}};
            const T* dp0 = dpp + orow0 * a.dy.ld + chs;
            const T* dq0 = dqp + orow0 * a.dy.ld + chs;
            for (int f0 = pl; f0 < total_st; f0 += NB * LP) {
                raw_t rp[NB], rq[NB];
                bool okv[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    const int r = dvq.div(f);
                    const int ho = ho_lo + r, wo = dvq.rem(f, r) - HL;
                    okv[u] = chan_ok && f < total_st && (unsigned)ho < (unsigned)a.Hout && (unsigned)wo < (unsigned)a.Wout;
                    const unsigned off = okv[u] ? __umul24(__mul24(ho, a.Wout) + wo, (unsigned)a.dy.ld) : 0u;
                    rp[u] = ld4_raw<T>(dp0 + off);
                    rq[u] = ld4_raw<T>(dq0 + off);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    if (f < total_st) {
                        f2_t p0, p1, q0, q1;
                        unpack_pairs<T>(rp[u], p0, p1);
                        unpack_pairs<T>(rq[u], q0, q1);
                        p0 = a1v[0] * p0 + (a2v[0] * q0 + a3v[0]);
                        p1 = a1v[1] * p1 + (a2v[1] * q1 + a3v[1]);
                        const float p[4] = {p0.x, p0.y, p1.x, p1.y};
                        tile[f * NCV + cv] = okv[u] ? V4<T>::pack(p) : V4<T>::zero();
                    }
                }
            }
        }
        __syncthreads();
        // ---- pass A: data gradient, SiLU', BatchNorm-backward sums; z1 of the band -> zt
        {
            const i64 prow0 = (i64)plane * a.Hin * a.Win;
            T* dh0 = dhp + prow0 * a.C + chan;
            const T* y10 = y1p + prow0 * a.y1.ld + chs;
            // activation of one pixel: z1 goes to the LDS tile, y / SiLU' stay for the epilogue
            auto activate = [&](const raw_t& raw, const int zi, f2_t* y, f2_t* dsl) {
                unpack_pairs<T>(raw, y[0], y[1]);
                const float4 s4 = *reinterpret_cast<const float4*>(&lbn[cv * 4]), t4 = *reinterpret_cast<const float4*>(&lbn[CS + cv * 4]);
                const f2_t bs2[2] = {f2_t{s4.x, s4.y}, f2_t{s4.z, s4.w}}, bt2[2] = {f2_t{t4.x, t4.y}, f2_t{t4.z, t4.w}};
                f2_t z1[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const f2_t h = y[i] * bs2[i] + bt2[i];
                    const f2_t sg = sigmoid2f_(h);
                    z1[i] = h * sg;
                    dsl[i] = sg * (1.0f + h * (1.0f - sg));
                }
                const float z[4] = {z1[0].x, z1[0].y, z1[1].x, z1[1].y};
                zt[zi * NCV + cv] = V4<T>::pack(z);
            };
            auto finish_at = [&](const int pix, const f2_t* y, const f2_t* dsl, const f2_t* dz) {
                const f2_t d0 = dz[0] * dsl[0], d1 = dz[1] * dsl[1];
                const float dh[4] = {d0.x, d0.y, d1.x, d1.y};
                const raw_t packed = V4<T>::pack(dh);
                *reinterpret_cast<raw_t*>(dh0 + __umul24((unsigned)pix, (unsigned)a.C)) = packed;
                f2_t r0, r1;
                unpack_pairs<T>(packed, r0, r1);              // statistics of the values as stored
                const float4 i4 = *reinterpret_cast<const float4*>(&lbn[2 * CS + cv * 4]), n4 = *reinterpret_cast<const float4*>(&lbn[3 * CS + cv * 4]);
                const f2_t bi2[2] = {f2_t{i4.x, i4.y}, f2_t{i4.z, i4.w}}, nbm2[2] = {f2_t{n4.x, n4.y}, f2_t{n4.z, n4.w}};
                sp0[0] += r0; sp0[1] += r1;
                sp1[0] += r0 * (y[0] * bi2[0] + nbm2[0]);
                sp1[1] += r1 * (y[1] * bi2[1] + nbm2[1]);
            };
            if constexpr (ST == 1 || ST == 2) {
                // Input pixels of one parity class (hi % ST, wi % ST) = (HP, PX) receive the taps dy = dy0 + ST*m, dx = dx0 + ST*n
                // (dy0 = (HP + P) % ST: hi + P - dy divisible by ST), all of them inside the zero-padded tile: branch-free, the
                // tap set known at compile time from KS, ST and the class.  Pixel (k, j) of the class is hi = hfirst + ST*k,
                // wi = PX + ST*j; tap (m, n) reads tile entry (r0 + k - m, q0 + j - n): one index per pixel, uniform offsets per tap.
                auto run_class = [&](auto hp_c, auto px_c) {
                    constexpr int HP = decltype(hp_c)::value, PX = decltype(px_c)::value;
                    constexpr int DY0 = (HP + P) % ST, DX0 = (PX + P) % ST;
                    const int hfirst = hi0 + ((hi0 % ST) == HP ? 0 : 1);
                    const int nr = (hi0 + nri - hfirst + ST - 1) / ST;
                    const int nc = (a.Win - PX + ST - 1) / ST;
                    const int total = (nr > 0 && nc > 0) ? nr * nc : 0;
                    const FastDiv dvc(nc > 0 ? nc : 1);
                    const int r0 = (hfirst + P - DY0) / ST - ho_lo;
                    const int q0 = (PX + P - DX0) / ST + HL;
                    const int base = (r0 * Wq + q0) * NCV + cv;
                    const int wdiff = Wq - nc;
                    const int rowstep = Wq * NCV;
                    for (int i0 = pl; i0 < total; i0 += XB * LP) {
                        raw_t ry[XB];
                        int gg[XB];
                        int ti[XB];
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            const int i = i0 + u * LP;
                            const int iv = (chan_ok && i < total) ? i : 0;
                            const int k = dvc.div(iv);
                            const int j = dvc.rem(iv, k);
                            ti[u] = (iv + __mul24(k, wdiff)) * NCV + base;
                            gg[u] = __mul24(hfirst + ST * k, a.Win) + (PX + ST * j);
                            ry[u] = ld4_raw<T>(y10 + __umul24((unsigned)gg[u], (unsigned)a.y1.ld));
                        }
                        // the taps run first, on the tile alone: the y1 loads land behind them, and y / SiLU' (8 registers per
                        // pixel) are not live next to a tap row's weights
                        f2_t dz[XB][2];
#pragma unroll
                        for (int u = 0; u < XB; ++u) { dz[u][0] = f2_t{0.f, 0.f}; dz[u][1] = f2_t{0.f, 0.f}; }
                        // a loop over the class's tap rows (not unrolled, as in the forward): one row of weights held at a time
#pragma unroll 1
                        for (int m = 0; m < (KS - DY0 + ST - 1) / ST; ++m) {
                            const float* wr = &lw[(DY0 + ST * m) * KS * CS + cv * 4];
                            const raw_t* tr = tile - m * rowstep;
#pragma unroll
                            for (int dx = DX0; dx < KS; dx += ST) {
                                const float4 wv = *reinterpret_cast<const float4*>(wr + dx * CS);
#pragma unroll
                                for (int u = 0; u < XB; ++u) {
                                    f2_t g0, g1;
                                    unpack_pairs<T>(tr[ti[u] - ((dx - DX0) / ST) * NCV], g0, g1);
                                    dz[u][0] += f2_t{wv.x, wv.y} * g0;
                                    dz[u][1] += f2_t{wv.z, wv.w} * g1;
                                }
                                __builtin_amdgcn_sched_barrier(0);   // as in the forward
                            }
                        }
#pragma unroll
                        for (int u = 0; u < XB; ++u) {
                            const int i = i0 + u * LP;
                            if (chan_ok && i < total) {
                                const int k = dvc.div(i);
                                const int j = dvc.rem(i, k);
                                f2_t y[2], dsl[2];
                                activate(ry[u], (hfirst - hi0 + ST * k) * Wz + (PX + ST * j) + P, y, dsl);
                                finish_at(gg[u], y, dsl, dz[u]);
                            }
                        }
                    }
                };
                run_class(std::integral_constant<int, 0>{}, std::integral_constant<int, 0>{});
                if constexpr (ST == 2) {
                    run_class(std::integral_constant<int, 0>{}, std::integral_constant<int, 1>{});
                    run_class(std::integral_constant<int, 1>{}, std::integral_constant<int, 0>{});
                    run_class(std::integral_constant<int, 1>{}, std::integral_constant<int, 1>{});
                }
            } else {
                // generic stride: taps tested per pixel
                const int total = nri * a.Win;
                for (int i = pl; i < total; i += LP) {
                    if (!chan_ok) continue;
                    const int iy = i / a.Win;
                    const int hi = hi0 + iy, wi = i - iy * a.Win;
                    f2_t y[2], dsl[2], dz[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};
                    activate(ld4_raw<T>(y10 + (i64)(hi * a.Win + wi) * a.y1.ld), iy * Wz + wi + P, y, dsl);
#pragma unroll 1
                    for (int dy = 0; dy < KS; ++dy) {
                        const int nh = hi + P - dy;
                        if (nh < 0 || nh % s != 0) continue;
                        const int ho = nh / s;
#pragma unroll 1
                        for (int dx = 0; dx < KS; ++dx) {
                            const int nw = wi + P - dx;
                            if (nw < 0 || nw % s != 0) continue;
                            const int wo = nw / s;
                            f2_t g0, g1;
                            unpack_pairs<T>(tile[((ho - ho_lo) * Wq + wo + HL) * NCV + cv], g0, g1);
                            const float4 wv = *reinterpret_cast<const float4*>(&lw[(dy * KS + dx) * CS + cv * 4]);
                            dz[0] += f2_t{wv.x, wv.y} * g0;
                            dz[1] += f2_t{wv.z, wv.w} * g1;
                        }
                    }
                    finish_at(hi * a.Win + wi, y, dsl, dz);
                }
            }
        }
        __syncthreads();
        // ---- pass B: this wave's tap row of dW over the outputs whose input row s*ho - P + mydy lies in the band
        {
            const int num = hi0 + P - mydy;                                   // s*ho >= num
            const int numl = hi0 + nri - 1 + P - mydy;                        // s*ho <= numl
            const int ho_f = num > 0 ? (num + s - 1) / s : 0;
            int ho_l = numl >= 0 ? numl / s : -1;
            if (ho_l > a.Hout - 1) ho_l = a.Hout - 1;
            const int total = ho_l >= ho_f ? (ho_l - ho_f + 1) * a.Wout : 0;
            const int zr0 = s * ho_f - num;                                   // band row of output row ho_f under this tap row
            const raw_t* gp0 = tile + ((ho_f - ho_lo) * Wq + HL) * NCV + cv;
            const raw_t* zp0 = zt + zr0 * Wz * NCV + cv;
            const int gdiff = Wq - a.Wout, zdiff = s * Wz - s * a.Wout;
            for (int i = gl; i < total; i += gn) {
                const int rr = dvo.div(i);
                f2_t g0, g1;
                unpack_pairs<T>(gp0[(i + __mul24(rr, gdiff)) * NCV], g0, g1);
                const raw_t* zp = zp0 + (i * s + __mul24(rr, zdiff)) * NCV;
#pragma unroll
                for (int dx = 0; dx < KS; ++dx) {
                    f2_t z0, z1;
                    unpack_pairs<T>(zp[dx * NCV], z0, z1);
                    dwr[dx][0] += z0 * g0;
                    dwr[dx][1] += z1 * g1;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        __syncthreads();
    }
    // weight gradient: reduce over the threads sharing a tap row and channel vector through LDS, then global fp32 atomics
    __syncthreads();
#pragma unroll 1
    for (int i = tid; i < KS * KS * CS; i += NT) lw[i] = 0.f;
    __syncthreads();
    DET_WAVES_BEGIN
    if (chan_ok) {
#pragma unroll
        for (int dx = 0; dx < KS; ++dx) {
            float* d = &lw[(mydy * KS + dx) * CS + cv * 4];
            atomicAdd(d + 0, dwr[dx][0].x);
            atomicAdd(d + 1, dwr[dx][0].y);
            atomicAdd(d + 2, dwr[dx][1].x);
            atomicAdd(d + 3, dwr[dx][1].y);
        }
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
#pragma unroll 1
    for (int i = tid; i < KS * KS * CS; i += NT) {
        const int k = i / CS, c = c0 + i % CS;
        if (c < a.C) atomicAdd(a.dw + (i64)c * (KS * KS) + k, lw[i]);
    }
    const float st0[4] = {sp0[0].x, sp0[0].y, sp0[1].x, sp0[1].y}, st1[4] = {sp1[0].x, sp1[0].y, sp1[1].x, sp1[1].y};
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// launchers of the two kernels above: tile bytes from P, the band from plan_bands; the LDS limit and its error as for 3x3
template <typename T, int KS>
static int spatial_fwd_ks_t(DwSpatialFwd a, hipStream_t s) {
    constexpr int CS = SL<T>::CS, P = KS / 2;
    constexpr size_t STATIC = (size_t)(KS * KS + 2) * CS * sizeof(float);
    const int Wp = a.Win + 2 * P;
    const size_t fwd = (size_t)DWS_FWD_LDS_BUDGET, ksb = (size_t)DWS_KS_LDS_BUDGET(STATIC), budget = fwd < ksb ? fwd : ksb;
    const BandPlan bp = plan_bands(a.Hout, [&](int rb) { return (size_t)((rb - 1) * a.stride + KS) * Wp * 128; }, budget,
                                   156 * 1024 - STATIC, 1, a.rows_band);
    if (!bp.ok) return dwn_set_error(-5, "dw_spatial: plane too wide for the LDS tile");
    a.rows_band = bp.rows;
    const int slices = (a.C + CS - 1) / CS;
    const i64 work = (i64)a.planes * bp.nbands;
    return by_stride_threads(a.stride, a.Hin * a.Win >= 512, [&](auto st, auto nt) {
        return launch_dw(dw_spatial_fwd_ks_kernel<T, KS, st.value, nt.value>, nt.value, bp.lds, slices, work, s, a);
    });
}

template <typename T, int KS>
static int spatial_bwd_ks_t(DwSpatialBwd a, hipStream_t s) {
    constexpr int CS = SL<T>::CS, P = KS / 2;
    constexpr size_t STATIC = (size_t)(KS * KS + 6) * CS * sizeof(float);
    const int HL = (P + a.stride - 1) / a.stride;
    const int Wq = a.Wout + 2 * HL, Wz = a.Win + 2 * P;
    auto rows_q = [&](int rb) { return a.stride == 1 ? rb + 2 * P : (rb - 1 + 2 * P) / a.stride + 2; };   // staged output rows (bound)
    const BandPlan bp = plan_bands(a.Hin, [&](int rb) { return ((size_t)rows_q(rb) * Wq + (size_t)rb * Wz) * 128; },      // gradient tile + z1 tile
                                   (size_t)DWS_KS_LDS_BUDGET(STATIC), 156 * 1024 - STATIC, 1, a.rows_band);
    if (!bp.ok) return dwn_set_error(-5, "dw_spatial_bwd: plane too wide for the LDS tile");
    a.rows_band = bp.rows;
    const int slices = (a.C + CS - 1) / CS;
    const i64 work = (i64)a.planes * bp.nbands;
    return by_stride(a.stride, [&](auto st) {
        return launch_dw(dw_spatial_bwd_ks_kernel<T, KS, st.value>, DWS_KS_BWD_THREADS, bp.lds, slices, work, s, a);
    });
}

#define DWS_KS_BUILT "dw_spatial: spatial_kernel must be 3, 5 or 7 (the built set)"

template <typename T>
static int spatial_fwd_t(DwSpatialFwd a, hipStream_t s) {
    constexpr int CS = SL<T>::CS;
    if (a.ks != 3 && a.ks != 5 && a.ks != 7) return dwn_set_error(-4, DWS_KS_BUILT);
    if (a.C % 8) return dwn_set_error(-2, "dw_spatial: C must be a multiple of 8");
    if (a.ks == 5) return spatial_fwd_ks_t<T, 5>(a, s);
    if (a.ks == 7) return spatial_fwd_ks_t<T, 7>(a, s);
    const int Wp = a.Win + 2;
    // bf16, stride 1/2: x-pair-packed tile (dot2 kernel), rows of ceil(Wp/2) pairs x 256 bytes
    const bool pair = TT<T>::IS_BF16 && (a.stride == 1 || a.stride == 2);
    const size_t row_bytes = pair ? (size_t)((Wp + 1) / 2) * 256 : (size_t)Wp * 128;
    const BandPlan bp = plan_bands(a.Hout, [&](int rb) { return (size_t)((rb - 1) * a.stride + 3) * row_bytes; },
                                   (size_t)DWS_FWD_LDS_BUDGET, 156 * 1024, 1, a.rows_band);
    if (!bp.ok) return dwn_set_error(-5, "dw_spatial: plane too wide for the LDS tile");
    a.rows_band = bp.rows;
    const int slices = (a.C + CS - 1) / CS;
    const i64 work = (i64)a.planes * bp.nbands;
    // 512-thread workgroups (twice the waves per LDS tile) pay off on large planes; tiny planes prefer 256
    return by_stride_threads(a.stride, a.Hin * a.Win >= 512, [&](auto st, auto nt) {
        if constexpr (TT<T>::IS_BF16 && st.value != 0)       // == pair: the generic kernel is not built for bf16 at strides 1, 2
            return launch_dw(dw_spatial_fwd_pair_kernel<st.value, nt.value>, nt.value, bp.lds, slices, work, s, a);
        else
            return launch_dw(dw_spatial_fwd_kernel<T, 3, st.value, nt.value>, nt.value, bp.lds, slices, work, s, a);
    });
}
bool dw_spatial_fwd_walk_supported(const DwSpatialFwd& a, int dtype);
int launch_dw_spatial_fwd_walk(const DwSpatialFwd& a, hipStream_t s);
int launch_dw_spatial_fwd(const DwSpatialFwd& a, int dtype, hipStream_t s) {
    if (a.a0 && !dw_spatial_fwd_walk_supported(a, dtype))
        return dwn_set_error(-3, "dw_spatial_fwd: rebuilt-input mode (a0 != NULL) is built into the chained row-walk kernels only (dwn_dw_spatial_fwd_rc_supported)");
    if (dw_spatial_fwd_walk_supported(a, dtype)) return launch_dw_spatial_fwd_walk(a, s);     // row-walk kernels (dwn_dwfwd.hip)
    return dtype == DWN_BF16 ? spatial_fwd_t<bf16_t>(a, s) : spatial_fwd_t<float>(a, s);
}

// ------------------------------------------------------------------------------------------------
// spatial backward, bf16 storage, 3x3, stride 1: x-pair-packed gradient tile + v_dot2c_f32_bf16.
//
// The staged gradient g = dL/dy2 (BatchNorm-backward affine applied, zero halo; column index xq = wo + 1) is
// packed as G[k] = (g[2k], g[2k+1]) per channel.  A thread owns the input pixel pair (2j, 2j+1) of a row:
//   dz[2j]   = dot2(G[j], (w2,w1)) + dot2(G[j+1], (w0,0))         dz[2j+1] = dot2(G[j], (0,w2)) + dot2(G[j+1], (w1,w0))
//   dW[.,2] += dot2(Z, G[j])      dW[.,0] += dot2(Z, G[j+1])      dW[.,1] += dot2(Z, (G[j].hi, G[j+1].lo))
// with Z = (z1[2j], z1[2j+1]) rounded to bf16 (the reference's autocast stores z1 in bf16): 8 VALU ops per stencil row,
// channel and pixel pair instead of 6 unpacks + 6 packed FMAs.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DWS_BWD_THREADS, DWS_BWD_PAIR_MINW) void dw_spatial_bwd_pair_kernel(const DwSpatialBwd a) {
    typedef bf16_t T;
    constexpr int NT = DWS_BWD_THREADS, NCV = 16, CS = 64, LP = NT / NCV, KS = 3, P = 1;
    __shared__ float lstat[2 * CS];
    __shared__ __attribute__((aligned(16))) float lw[KS * KS * CS];          // dW reduction at the end
    __shared__ __attribute__((aligned(16))) unsigned lwp[3 * 4 * CS];        // packed weights [dy][combo][channel]
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    for (int i = tid; i < 3 * CS; i += NT) {
        const int dy = i / CS, cc = i % CS, c = c0 + cc;
        float w0 = 0.f, w1 = 0.f, w2 = 0.f;
        if (c < a.C) { w0 = a.w[(i64)(dy * 3 + 0) * a.C + c]; w1 = a.w[(i64)(dy * 3 + 1) * a.C + c]; w2 = a.w[(i64)(dy * 3 + 2) * a.C + c]; }
        lwp[(dy * 4 + 0) * CS + cc] = pack_bf16x2(w2, w1);
        lwp[(dy * 4 + 1) * CS + cc] = pack_bf16x2(w0, 0.f);
        lwp[(dy * 4 + 2) * CS + cc] = pack_bf16x2(0.f, w2);
        lwp[(dy * 4 + 3) * CS + cc] = pack_bf16x2(w1, w0);
    }
    __syncthreads();

    float dwp[KS * KS][4];
#pragma unroll
    for (int k = 0; k < KS * KS; ++k) { dwp[k][0] = dwp[k][1] = dwp[k][2] = dwp[k][3] = 0.f; }
    float bs[4], bt[4], bm[4], bi[4];
    ldc4(a.y1.v1 + chs, bs); ldc4(a.y1.v2 + chs, bt); ldc4(a.y1.v3 + chs, bm); ldc4(a.y1.v4 + chs, bi);
    const f2_t bs2[2] = {f2_t{bs[0], bs[1]}, f2_t{bs[2], bs[3]}}, bt2[2] = {f2_t{bt[0], bt[1]}, f2_t{bt[2], bt[3]}};
    const f2_t bi2[2] = {f2_t{bi[0], bi[1]}, f2_t{bi[2], bi[3]}};
    const f2_t nbm2[2] = {f2_t{-bm[0] * bi[0], -bm[1] * bi[1]}, f2_t{-bm[2] * bi[2], -bm[3] * bi[3]}};   // yhat = y*bi + nbm
    f2_t sp0[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}}, sp1[2] = {f2_t{0.f, 0.f}, f2_t{0.f, 0.f}};

    const int Wq = a.Wout + 2;                       // staged columns wo = -1 .. Wout
    const int Wqp = (Wq + 1) >> 1;                   // ... as pairs
    const int Wip = (a.Win + 1) >> 1;                // input pixel pairs per row
    const FastDiv dvq(Wqp), dvw(Wip);
    const int nbands = (a.Hin + a.rows_band - 1) / a.rows_band;
    const int ntiles = a.planes * nbands;
    T* dhp = reinterpret_cast<T*>(a.dh1);
    const T* y1p = reinterpret_cast<const T*>(a.y1.p);
    const T* dpp = reinterpret_cast<const T*>(a.dy.p);
    const T* dqp = reinterpret_cast<const T*>(a.dy.q);
    unsigned* tile = reinterpret_cast<unsigned*>(dyn_smem);      // [rows_q][Wqp][64] dwords
    const int rowdw = Wqp * CS;
    for (int tile_id = blockIdx.x; tile_id < ntiles; tile_id += gridDim.x) {
        const int plane = tile_id / nbands, band = tile_id % nbands;
        const int hi0 = band * a.rows_band;
        const int nri = (a.Hin - hi0 < a.rows_band) ? a.Hin - hi0 : a.rows_band;
        const int ho_lo = hi0 - 1;                   // stride 1: rows ho = hi - 1 .. hi + 1
        const int rows_q = nri + 2;
        const i64 orow0 = (i64)plane * a.Hout * a.Wout;
        {
            constexpr int NB = 4;
            const int total_st = rows_q * Wqp;
            float a1[4], a2[4], a3[4];
            ldc4(a.dy.v1 + chs, a1); ldc4(a.dy.v2 + chs, a2); ldc4(a.dy.v3 + chs, a3);
            const f2_t a1v[2] = {f2_t{a1[0], a1[1]}, f2_t{a1[2], a1[3]}}, a2v[2] = {f2_t{a2[0], a2[1]}, f2_t{a2[2], a2[3]}};
            const f2_t a3v[2] = {f2_t{a3[0], a3[1]}, f2_t{a3[2], a3[3]}};
            const T* dp0 = dpp + orow0 * a.dy.ld + chs;
            const T* dq0 = dqp + orow0 * a.dy.ld + chs;
            for (int f0 = pl; f0 < total_st; f0 += NB * LP) {
                uint2 rp[NB][2], rq[NB][2];
                unsigned msk[NB];
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    const int r = dvq.div(f);
                    const int xp = dvq.rem(f, r);
                    const int ho = ho_lo + r, wo0 = 2 * xp - 1;
                    const bool rok = chan_ok && f < total_st && (unsigned)ho < (unsigned)a.Hout;
                    const bool ok0 = rok && (unsigned)wo0 < (unsigned)a.Wout, ok1 = rok && (unsigned)(wo0 + 1) < (unsigned)a.Wout;
                    const int rowpix = __mul24(ho, a.Wout);
                    const unsigned off0 = ok0 ? __umul24((unsigned)(rowpix + wo0), (unsigned)a.dy.ld) : 0u;
                    const unsigned off1 = ok1 ? __umul24((unsigned)(rowpix + wo0 + 1), (unsigned)a.dy.ld) : 0u;
                    rp[u][0] = ld4_raw<T>(dp0 + off0); rq[u][0] = ld4_raw<T>(dq0 + off0);
                    rp[u][1] = ld4_raw<T>(dp0 + off1); rq[u][1] = ld4_raw<T>(dq0 + off1);
                    msk[u] = (ok0 ? 0x0000ffffu : 0u) | (ok1 ? 0xffff0000u : 0u);
                }
#pragma unroll
                for (int u = 0; u < NB; ++u) {
                    const int f = f0 + u * LP;
                    if (f < total_st) {
                        f2_t g[2][2];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            f2_t p0, p1, q0, q1;
                            unpack_pairs<T>(rp[u][h], p0, p1);
                            unpack_pairs<T>(rq[u][h], q0, q1);
                            g[h][0] = a1v[0] * p0 + (a2v[0] * q0 + a3v[0]);
                            g[h][1] = a1v[1] * p1 + (a2v[1] * q1 + a3v[1]);
                        }
                        const uint4 o = make_uint4(pack_bf16x2(g[0][0].x, g[1][0].x) & msk[u], pack_bf16x2(g[0][0].y, g[1][0].y) & msk[u],
                                                   pack_bf16x2(g[0][1].x, g[1][1].x) & msk[u], pack_bf16x2(g[0][1].y, g[1][1].y) & msk[u]);
                        *reinterpret_cast<uint4*>(tile + f * CS + cv * 4) = o;
                    }
                }
            }
        }
        __syncthreads();
        {
            const i64 prow0 = (i64)plane * a.Hin * a.Win;
            T* dh0 = dhp + prow0 * a.C + chan;
            const T* y10 = y1p + prow0 * a.y1.ld + chs;
            const int total = nri * Wip;
            const int grow0 = hi0 * a.Win;
            constexpr int XB = DWS_BWD_PAIR_XB;      // pixel pairs in flight per thread
            for (int i0 = pl; i0 < total; i0 += XB * LP) {
                uint2 ry[XB][2];
                int jj[XB], iyv[XB];
                bool v1[XB];
#pragma unroll
                for (int u = 0; u < XB; ++u) {
                    const int i = i0 + u * LP;
                    const bool ok = chan_ok && i < total;
                    const int iv = ok ? i : 0;
                    iyv[u] = dvw.div(iv);
                    jj[u] = dvw.rem(iv, iyv[u]);
                    const int pix = grow0 + __mul24(iyv[u], a.Win) + 2 * jj[u];
                    v1[u] = 2 * jj[u] + 1 < a.Win;
                    ry[u][0] = ld4_raw<T>(y10 + __umul24((unsigned)pix, (unsigned)a.y1.ld));
                    ry[u][1] = ld4_raw<T>(y10 + __umul24((unsigned)(pix + (v1[u] ? 1 : 0)), (unsigned)a.y1.ld));
                }
#pragma unroll
                for (int u = 0; u < XB; ++u) {
                    if (!chan_ok || i0 + u * LP >= total) continue;
                    f2_t y[2][2], z1[2][2], dsl[2][2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        unpack_pairs<T>(ry[u][h], y[h][0], y[h][1]);
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const f2_t hh = y[h][q] * bs2[q] + bt2[q];
                            const f2_t sg = sigmoid2f_(hh);
                            z1[h][q] = hh * sg;
                            dsl[h][q] = sg * (1.0f + hh * (1.0f - sg));
                        }
                    }
                    if (!v1[u]) { z1[1][0] = f2_t{0.f, 0.f}; z1[1][1] = f2_t{0.f, 0.f}; }
                    const unsigned Z[4] = {pack_bf16x2(z1[0][0].x, z1[1][0].x), pack_bf16x2(z1[0][0].y, z1[1][0].y),
                                           pack_bf16x2(z1[0][1].x, z1[1][1].x), pack_bf16x2(z1[0][1].y, z1[1][1].y)};
                    float dz0[4] = {0.f, 0.f, 0.f, 0.f}, dz1[4] = {0.f, 0.f, 0.f, 0.f};
                    const unsigned* tp = tile + (__mul24(iyv[u], Wqp) + jj[u]) * CS + cv * 4;
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy) {
                        // tile row iy + (2 - dy): output row ho = hi + 1 - dy
                        const uint4 G0 = *reinterpret_cast<const uint4*>(tp + (2 - dy) * rowdw);
                        const uint4 G1 = *reinterpret_cast<const uint4*>(tp + (2 - dy) * rowdw + CS);
                        const uint4 Wa = *reinterpret_cast<const uint4*>(&lwp[(dy * 4 + 0) * CS + cv * 4]);
                        const uint4 Wb = *reinterpret_cast<const uint4*>(&lwp[(dy * 4 + 1) * CS + cv * 4]);
                        const uint4 Wc = *reinterpret_cast<const uint4*>(&lwp[(dy * 4 + 2) * CS + cv * 4]);
                        const uint4 Wd = *reinterpret_cast<const uint4*>(&lwp[(dy * 4 + 3) * CS + cv * 4]);
                        const unsigned g0[4] = {G0.x, G0.y, G0.z, G0.w}, g1[4] = {G1.x, G1.y, G1.z, G1.w};
                        const unsigned wa[4] = {Wa.x, Wa.y, Wa.z, Wa.w}, wb[4] = {Wb.x, Wb.y, Wb.z, Wb.w};
                        const unsigned wc[4] = {Wc.x, Wc.y, Wc.z, Wc.w}, wd[4] = {Wd.x, Wd.y, Wd.z, Wd.w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            dz0[q] = dot2_bf16(g0[q], wa[q], dz0[q]);
                            dz0[q] = dot2_bf16(g1[q], wb[q], dz0[q]);
                            dz1[q] = dot2_bf16(g0[q], wc[q], dz1[q]);
                            dz1[q] = dot2_bf16(g1[q], wd[q], dz1[q]);
                            const unsigned gm = __builtin_amdgcn_alignbit(g1[q], g0[q], 16);      // (G0.hi, G1.lo)
                            dwp[dy * 3 + 2][q] = dot2_bf16(Z[q], g0[q], dwp[dy * 3 + 2][q]);
                            dwp[dy * 3 + 1][q] = dot2_bf16(Z[q], gm, dwp[dy * 3 + 1][q]);
                            dwp[dy * 3 + 0][q] = dot2_bf16(Z[q], g1[q], dwp[dy * 3 + 0][q]);
                        }
                    }
                    const int pix = grow0 + __mul24(iyv[u], a.Win) + 2 * jj[u];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        if (h == 1 && !v1[u]) break;
                        const float* dz = h == 0 ? dz0 : dz1;
                        const f2_t d0 = f2_t{dz[0], dz[1]} * dsl[h][0], d1 = f2_t{dz[2], dz[3]} * dsl[h][1];
                        const uint2 packed = make_uint2(pack_bf16x2(d0.x, d0.y), pack_bf16x2(d1.x, d1.y));
                        *reinterpret_cast<uint2*>(dh0 + __umul24((unsigned)(pix + h), (unsigned)a.C)) = packed;
                        f2_t r0, r1;
                        unpack_pairs<T>(packed, r0, r1);
                        sp0[0] += r0; sp0[1] += r1;
                        sp1[0] += r0 * (y[h][0] * bi2[0] + nbm2[0]);
                        sp1[1] += r1 * (y[h][1] * bi2[1] + nbm2[1]);
                    }
                }
            }
        }
        __syncthreads();
    }
    // weight gradient: reduce over the threads sharing a channel vector through LDS, then global fp32 atomics
    for (int i = tid; i < KS * KS * CS; i += NT) lw[i] = 0.f;
    __syncthreads();
    DET_WAVES_BEGIN
    if (chan_ok) {
#pragma unroll
        for (int k = 0; k < KS * KS; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) atomicAdd(&lw[k * CS + cv * 4 + q], dwp[k][q]);
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
    for (int i = tid; i < KS * KS * CS; i += NT) {
        const int k = i / CS, c = c0 + i % CS;
        if (c < a.C) atomicAdd(&a.dw[(i64)c * (KS * KS) + k], lw[i]);
    }
    if (a.stats) {
        const float s0[4] = {sp0[0].x, sp0[0].y, sp0[1].x, sp0[1].y}, s1[4] = {sp1[0].x, sp1[0].y, sp1[1].x, sp1[1].y};
        block_stats_flush<T>(lstat, s0, s1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    }
    DET_EXIT();
}

template <typename T>
static int spatial_bwd_t(DwSpatialBwd a, hipStream_t s) {
    constexpr int CS = SL<T>::CS;
    if (a.ks != 3 && a.ks != 5 && a.ks != 7) return dwn_set_error(-4, DWS_KS_BUILT);
    if (a.C % 8) return dwn_set_error(-2, "dw_spatial: C must be a multiple of 8");
    if (a.ks == 5) return spatial_bwd_ks_t<T, 5>(a, s);
    if (a.ks == 7) return spatial_bwd_ks_t<T, 7>(a, s);
    const int Wq = a.Wout + 2;
    auto rows_q = [&](int rb) { return (rb - 1 + 2) / a.stride + 2; };   // upper bound on staged output rows
    // bf16, stride 1: x-pair-packed gradient tile (dot2 kernel), rows of ceil(Wq/2) pairs x 256 bytes
    const bool pair = TT<T>::IS_BF16 && a.stride == 1;
    const size_t row_bytes = pair ? (size_t)((Wq + 1) / 2) * 256 : (size_t)Wq * 128;
    const BandPlan bp = plan_bands(a.Hin, [&](int rb) { return (size_t)rows_q(rb) * row_bytes; }, (size_t)DWS_BWD_LDS_BUDGET,
                                   150 * 1024, 1, a.rows_band);
    if (!bp.ok) return dwn_set_error(-5, "dw_spatial_bwd: plane too wide for the LDS tile");
    a.rows_band = bp.rows;
    const int slices = (a.C + CS - 1) / CS;
    const i64 work = (i64)a.planes * bp.nbands;
    return by_stride(a.stride, [&](auto st) {
        if constexpr (TT<T>::IS_BF16 && st.value == 1)       // == pair: the generic kernel is not built for bf16 at stride 1
            return launch_dw(dw_spatial_bwd_pair_kernel, DWS_BWD_THREADS, bp.lds, slices, work, s, a);
        else
            return launch_dw(dw_spatial_bwd_kernel<T, 3, st.value>, DWS_BWD_THREADS, bp.lds, slices, work, s, a);
    });
}
bool dw_spatial_bwd_walk_supported(const DwSpatialBwd& a, int dtype);
int launch_dw_spatial_bwd_walk(const DwSpatialBwd& a, hipStream_t s);
int launch_dw_spatial_bwd(const DwSpatialBwd& a, int dtype, hipStream_t s) {
    if (a.a0 && !dw_spatial_bwd_walk_supported(a, dtype))
        return dwn_set_error(-3, "dw_spatial_bwd: rebuilt-y1 mode (a0 != NULL) is built into the row-walk kernels only (dwn_dw_spatial_bwd_rc_supported)");
    if (dw_spatial_bwd_walk_supported(a, dtype)) return launch_dw_spatial_bwd_walk(a, s);     // row-walk kernels (dwn_dwbwd.hip)
    return dtype == DWN_BF16 ? spatial_bwd_t<bf16_t>(a, s) : spatial_bwd_t<float>(a, s);
}

template <typename T>
static int temporal_fwd_t(const DwTemporalFwd& a, hipStream_t s) {
    constexpr int CS = SL<T>::CS, LP = SL<T>::LP;
    if (a.C % 8) return dwn_set_error(-2, "dw_temporal: C must be a multiple of 8");
    const int slices = (a.C + CS - 1) / CS;
    const i64 work = ((i64)a.B * a.HW + LP - 1) / LP;
    const bool zout = a.z_scale != nullptr;
    if (zout && (!a.z_shift || a.stats)) return dwn_set_error(-2, "dw_temporal: the z3 epilogue needs z_shift and no statistics (eval mode)");
    auto go = [&](auto plain, auto z3) { return zout ? launch_dw(z3, 256, 0, slices, work, s, a) : launch_dw(plain, 256, 0, slices, work, s, a); };
    switch (a.kt) {        // 7 and 9 arrive through launch_dw_temporal_wide_fwd, which refuses first what those sizes refuse
        case 3: return go(dw_temporal_fwd_kernel<T, 3>, dw_temporal_fwd_kernel<T, 3, true>);
        case 5: return go(dw_temporal_fwd_kernel<T, 5>, dw_temporal_fwd_kernel<T, 5, true>);
        case 7: return go(dw_temporal_fwd_kernel<T, 7>, dw_temporal_fwd_kernel<T, 7, true>);
        case 9: return go(dw_temporal_fwd_kernel<T, 9>, dw_temporal_fwd_kernel<T, 9, true>);
    }
    return dwn_set_error(-4, "dw_temporal: only temporal_kernel 3 or 5 is built");
}
int launch_dw_temporal_fwd(const DwTemporalFwd& a, int dtype, hipStream_t s) {
    if (a.kt == 7 || a.kt == 9) return launch_dw_temporal_wide_fwd(a, dtype, s);       // dw_temporal_wide_check first
    return dtype == DWN_BF16 ? temporal_fwd_t<bf16_t>(a, s) : temporal_fwd_t<float>(a, s);
}
int launch_dw_temporal_wide_fwd(const DwTemporalFwd& a, int dtype, hipStream_t s) {
    if (int rc = dw_temporal_wide_check(a.kt, a.C, LD_PLAIN)) return rc;
    return dtype == DWN_BF16 ? temporal_fwd_t<bf16_t>(a, s) : temporal_fwd_t<float>(a, s);
}

// ------------------------------------------------------------------------------------------------
// temporal backward without reading y3 (dy_kind == LD_PLAIN: dy.p = dh3, dy.v1..v3 = bn3-backward A1, A2, A3).
// dy3 = A1*dh3 + A2*y3 + A3 needs y3 = sum_j w[j] z2[t + j - P], and z2 = SiLU(BN2(y2)) is computed here anyway (for dW
// and SiLU'): y3 is recomputed from a (2P+1)-deep window of z2 that runs 2P frames ahead of the output frame.
// Three passes over the E-wide tensors (dh3, y2 in; dh2 out) instead of four; 5 extra FMAs per element.
// ------------------------------------------------------------------------------------------------
template <typename T, int KT>
__global__ __launch_bounds__(256, DWT_RC_MINW) void dw_temporal_bwd_rc_kernel(const DwTemporalBwd a) {
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = SL<T>::LP, P = KT / 2, NW = 2 * P + 1;
    constexpr int TB = NW;            // frames per unrolled batch == window length: ring indices are compile-time, no shifting
    static_assert(NW == KT, "ring rotation below assumes an odd kernel: window length == kernel length");
    typedef typename SL<T>::raw_t raw_t;
    __shared__ float lstat[2 * CS];
    __shared__ float lw[KT * CS];
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    for (int i = tid; i < KT * CS; i += 256) lw[i] = 0.f;
    __syncthreads();
    float w[KT][4], dwacc[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        ldc4(a.w + (i64)k * a.C + chs, w[k]);
        dwacc[k][0] = dwacc[k][1] = dwacc[k][2] = dwacc[k][3] = 0.f;
    }
    float bs[4], bt[4], bm[4], bi[4], a1[4], a2[4], a3[4];
    ldc4(a.y2.v1 + chs, bs); ldc4(a.y2.v2 + chs, bt); ldc4(a.y2.v3 + chs, bm); ldc4(a.y2.v4 + chs, bi);
    ldc4(a.dy.v1 + chs, a1); ldc4(a.dy.v2 + chs, a2); ldc4(a.dy.v3 + chs, a3);
    float st0[4] = {0.f, 0.f, 0.f, 0.f}, st1[4] = {0.f, 0.f, 0.f, 0.f};

    const i64 npos = (i64)a.B * a.HW;
    T* dhp = reinterpret_cast<T*>(a.dh2);
    const T* y2p = reinterpret_cast<const T*>(a.y2.p);
    const T* dpp = reinterpret_cast<const T*>(a.dy.p);
    const i64 tstride = (i64)a.HW * a.C;

    if (chan_ok) {
        for (i64 pos = (i64)blockIdx.x * LP + pl; pos < npos; pos += (i64)gridDim.x * LP) {
            const i64 b = pos / a.HW, hw = pos % a.HW;
            const i64 e0 = (b * a.T * a.HW + hw) * a.C + chan;
            // rings of NW = KT slots: at unrolled step u of a batch, frame t + j of (y2, z2, SiLU') lives in slot
            // (u + j) % NW and dy3(t + k - P) in win[(u + k) % KT].  Frames outside [0, T) are zero slots.
            float yw[NW][4], zw[NW][4], dsw[NW][4], win[KT][4];
#pragma unroll
            for (int j = 0; j < NW; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) { yw[j][i] = 0.f; zw[j][i] = 0.f; dsw[j][i] = 0.f; }
#pragma unroll
            for (int k = 0; k < KT; ++k) win[k][0] = win[k][1] = win[k][2] = win[k][3] = 0.f;
            auto activate = [&](const raw_t& raw, float* y, float* z, float* ds) {
                V4<T>::unpack(raw, y);
                float h4[4], sg4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) h4[i] = fmaf(y[i], bs[i], bt[i]);
                sigmoid_n<4>(h4, sg4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float h = h4[i], sg = sg4[i];
                    z[i] = h * sg;
                    ds[i] = sg * (1.0f + h * (1.0f - sg));
                }
            };
            // at virtual frame t = -P the window covers frames -P .. P-1: load frames 0 .. P-1 into slots P .. 2P-1
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (j < a.T) activate(ld4_raw<T>(y2p + e0 + j * tstride), yw[P + j], zw[P + j], dsw[P + j]);
            for (int t0 = -P; t0 < a.T; t0 += TB) {
                raw_t rp[TB], ry[TB];
                // load issue at raised priority: a streaming kernel's next loads should leave before the other waves' arithmetic gets
                // the issue slot (measured: 240 -> 227 us per launch in the step; the forward kernel and se_pool, whose vector ALUs are half as busy, gain nothing)
                __builtin_amdgcn_s_setprio(DWT_PRIO);
#pragma unroll
                for (int u = 0; u < TB; ++u) {
                    const int td = t0 + u + P, ty = t0 + u + 2 * P;          // frames of dh3 / y2 fetched for output frame t0+u
                    rp[u] = ld4_raw<T>(dpp + e0 + (td < a.T ? td : 0) * tstride);
                    ry[u] = ld4_raw<T>(y2p + e0 + (ty < a.T ? ty : 0) * tstride);
                }
                __builtin_amdgcn_s_setprio(0);
#pragma unroll
                for (int u = 0; u < TB; ++u) {
                    const int t = t0 + u;
                    if (t >= a.T) break;
                    // newest window slot: frame t + 2P
                    const int sn = (u + NW - 1) % NW;                   // newest slot (frame t + 2P)
                    if (t + 2 * P < a.T) activate(ry[u], yw[sn], zw[sn], dsw[sn]);
                    else { for (int i = 0; i < 4; ++i) { yw[sn][i] = 0.f; zw[sn][i] = 0.f; dsw[sn][i] = 0.f; } }
                    const int s0 = u % NW;                              // slot of the output frame t
                    // dy3(t + P) from dh3 and the recomputed y3(t + P) = sum_j w[j] z2(t + j)
                    if (t + P < a.T) {
                        float p[4];
                        V4<T>::unpack(rp[u], p);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float y3 = 0.f;
#pragma unroll
                            for (int j = 0; j < KT; ++j) y3 = fmaf(w[j][i], zw[(u + j) % NW][i], y3);
                            win[sn][i] = fmaf(a1[i], p[i], fmaf(a2[i], round_t<T>(y3), a3[i]));
                        }
                    } else { win[sn][0] = win[sn][1] = win[sn][2] = win[sn][3] = 0.f; }
                    if (t >= 0) {
                        float dh[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            float dz = 0.f;
#pragma unroll
                            for (int k = 0; k < KT; ++k) {
                                const float gk = win[(u + KT - 1 - k) % KT][i];
                                dz = fmaf(w[k][i], gk, dz);
                                dwacc[k][i] = fmaf(zw[s0][i], gk, dwacc[k][i]);
                            }
                            dh[i] = dz * dsw[s0][i];
                        }
                        st4<T>(dhp + e0 + t * tstride, dh);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float r = round_t<T>(dh[i]);
                            st0[i] += r;
                            st1[i] = fmaf(r, yw[s0][i], st1[i]);          // raw sum(dh2 * y2): normalised once, below
                        }
                    }
                }
            }
        }
    }
    // sum(dh2 * (y2 - mean) * invstd) = invstd * (sum(dh2 * y2) - mean * sum(dh2)): two VALU operations per element less in
    // a kernel that is VALU-bound (as in the spatial backward kernels and the dh3 GEMM epilogue)
#pragma unroll
    for (int i = 0; i < 4; ++i) st1[i] = bi[i] * fmaf(-bm[i], st0[i], st1[i]);
    DET_WAVES_BEGIN
    if (chan_ok) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(&lw[k * CS + cv * 4 + i], dwacc[k][i]);
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
    for (int i = tid; i < KT * CS; i += 256) {
        int k = i / CS, c = c0 + i % CS;
        if (c < a.C) atomicAdd(a.dw + (i64)c * KT + k, lw[i]);
    }
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// ------------------------------------------------------------------------------------------------
// temporal kernel sizes 7 and 9: the y3-recomputing backward with another register plan.
//
// dw_temporal_bwd_rc_kernel holds, per thread, the weights, the weight-gradient accumulators and four rings of [KT][4] floats:
// 24*KT registers before the loads in flight (216 at KT = 9), which does not fit the 256 of two waves per SIMD.  Here
//   * the weights are an LDS table [tap][channel], one broadcast ds_read_b128 per tap and output frame, read through a volatile
//     pointer so that the reads of the unrolled tap loop stay where they are used (hoisted, they are the 4*KT registers again);
//   * there is no SiLU' ring and the y2 ring is in LDS, in storage form, a column per thread (KT * 2 or 4 KB per workgroup, one
//     write and one read per frame): both serve the output frame only, so y2(t) is unpacked and its sigmoid taken a second
//     time there, 2P frames after the first.  Only frames inside [0, T) are ever read back, so the ring has no zero slots;
//   * the loads are not issued a batch of KT frames at a time but D frames ahead of their use, rolling through the unrolled
//     batch: D + 1 raw frames of each tensor are live instead of KT.
// What remains is the z2 ring, the dy3 ring and the weight gradient, 12*KT registers.  The arithmetic is that of the rc kernel
// (y3 rounded to storage as a stored y3 would read back, the same sums), with one difference in order: the newest tap of dz2,
// the one that waits for the frame's own dy3, is added last.
// ------------------------------------------------------------------------------------------------
typedef float dwt_f4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) dwt_f4_t dwt_lds_f4_t;      // an LDS pointer by type: a volatile read through a generic one is a flat load

template <typename T, int KT>
__global__ __launch_bounds__(256, DWT_RC_MINW) void dw_temporal_bwd_wide_kernel(const DwTemporalBwd a) {
    constexpr int NCV = SL<T>::NCV, CS = SL<T>::CS, LP = SL<T>::LP, P = KT / 2, NW = 2 * P + 1;
    constexpr int TB = NW;            // frames per unrolled batch == window length: ring indices are compile-time, no shifting
    constexpr int D = TT<T>::IS_BF16 ? 4 : (KT > 7 ? 2 : 3);     // frames a load is issued ahead of its use
    static_assert(NW == KT && D < TB, "odd kernel: window length == kernel length; the look-ahead stays inside one batch");
    typedef typename SL<T>::raw_t raw_t;
    __shared__ float lstat[2 * CS];
    __shared__ float lw[KT * CS];
    __shared__ __attribute__((aligned(16))) float lwt[KT * CS];       // weights [tap][channel of the slice]
    __shared__ raw_t lyr[NW * 256];                                   // y2 ring [slot][thread], as stored
    const int tid = threadIdx.x;
    const int cv = tid % NCV, pl = tid / NCV;
    const int c0 = blockIdx.y * CS;
    const int chan = c0 + cv * 4;
    const bool chan_ok = chan < a.C;
    const int chs = chan_ok ? chan : 0;
    if (tid < 2 * CS) lstat[tid] = 0.f;
    for (int i = tid; i < KT * CS; i += 256) {
        const int k = i / CS, c = c0 + i % CS;
        lw[i] = 0.f;
        lwt[i] = c < a.C ? a.w[(i64)k * a.C + c] : 0.f;
    }
    __syncthreads();
    const volatile dwt_lds_f4_t* wtab = (const volatile dwt_lds_f4_t*)lwt + cv;      // tap k: wtab[k * NCV]
    raw_t* const yr = lyr + tid;            // a thread's own column: no barrier; a slot is written before the step that reads it
    float dwacc[KT][4];
#pragma unroll
    for (int k = 0; k < KT; ++k) dwacc[k][0] = dwacc[k][1] = dwacc[k][2] = dwacc[k][3] = 0.f;
    float bs[4], bt[4], a1[4], a2[4], a3[4];
    ldc4(a.y2.v1 + chs, bs); ldc4(a.y2.v2 + chs, bt);
    ldc4(a.dy.v1 + chs, a1); ldc4(a.dy.v2 + chs, a2); ldc4(a.dy.v3 + chs, a3);
    float st0[4] = {0.f, 0.f, 0.f, 0.f}, st1[4] = {0.f, 0.f, 0.f, 0.f};

    const i64 npos = (i64)a.B * a.HW;
    T* dhp = reinterpret_cast<T*>(a.dh2);
    const T* y2p = reinterpret_cast<const T*>(a.y2.p);
    const T* dpp = reinterpret_cast<const T*>(a.dy.p);
    const i64 tstride = (i64)a.HW * a.C;

    if (chan_ok) {
        for (i64 pos = (i64)blockIdx.x * LP + pl; pos < npos; pos += (i64)gridDim.x * LP) {
            const i64 b = pos / a.HW, hw = pos % a.HW;
            const i64 e0 = (b * a.T * a.HW + hw) * a.C + chan;
            // rings of NW = KT slots: at unrolled step u of a batch, frame t + j of (y2 as stored, z2) lives in slot (u + j) % NW
            // and dy3(t + k - P) in win[(u + k) % KT].  Frames outside [0, T) are zero slots.
            float zw[NW][4], win[KT][4];
#pragma unroll
            for (int j = 0; j < NW; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i) { zw[j][i] = 0.f; win[j][i] = 0.f; }
            }
            // z2 of a stored y2 frame; with ds also SiLU' (the output frame's second visit)
            auto activate = [&](const raw_t& raw, float* y, float* z, float* ds) {
                V4<T>::unpack(raw, y);
                float h4[4], sg4[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) h4[i] = fmaf(y[i], bs[i], bt[i]);
                sigmoid_n<4>(h4, sg4);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float h = h4[i], sg = sg4[i];
                    z[i] = h * sg;
                    if (ds) ds[i] = sg * (1.0f + h * (1.0f - sg));
                }
            };
            // the frames fetched for the output frame t: dh3(t + P) and y2(t + 2P), clamped inside the tensor (unused past T)
            auto fetch = [&](int t, raw_t& rp, raw_t& ry) {
                const int td = t + P, ty = t + 2 * P;
                rp = ld4_raw<T>(dpp + e0 + (td < a.T ? td : 0) * tstride);
                ry = ld4_raw<T>(y2p + e0 + (ty < a.T ? ty : 0) * tstride);
            };
            // at virtual frame t = -P the window covers frames -P .. P-1: load frames 0 .. P-1 into slots P .. 2P-1
#pragma unroll
            for (int j = 0; j < P; ++j)
                if (j < a.T) {
                    float y[4];
                    const raw_t r = ld4_raw<T>(y2p + e0 + j * tstride);
                    yr[(P + j) * 256] = r;
                    activate(r, y, zw[P + j], nullptr);
                }
            raw_t rp[TB], ry[TB];                       // slot u: the frames of step u; D + 1 of them are live at a time
#pragma unroll
            for (int u = 0; u < D; ++u) fetch(-P + u, rp[u], ry[u]);
            for (int t0 = -P; t0 < a.T; t0 += TB) {
#pragma unroll
                for (int u = 0; u < TB; ++u) {
                    const int t = t0 + u;
                    if (t >= a.T) break;
                    fetch(t + D, rp[(u + D) % TB], ry[(u + D) % TB]);
                    const int sn = (u + NW - 1) % NW;                   // newest slot (frame t + 2P)
                    const int s0 = u % NW;                              // slot of the output frame t
                    if (t + 2 * P < a.T) {
                        float y[4];
                        yr[sn * 256] = ry[u];
                        activate(ry[u], y, zw[sn], nullptr);
                    } else {
                        zw[sn][0] = zw[sn][1] = zw[sn][2] = zw[sn][3] = 0.f;
                    }
                    const bool dy_ok = t + P < a.T;
                    float p[4];
                    V4<T>::unpack(rp[u], p);
                    if (u >= P || t >= 0) {
                        // one pass over the taps: y3(t + P) = sum_j w[j] z2(t + j), and of dz2(t) = sum_k w[k] dy3(t + P - k) and
                        // dW[k] += z2(t) dy3(t + P - k) the taps k >= 1, whose dy3 the ring already holds
                        float y3[4] = {0.f, 0.f, 0.f, 0.f}, dz[4] = {0.f, 0.f, 0.f, 0.f}, w0[4];
#pragma unroll
                        for (int k = 0; k < KT; ++k) {
                            const dwt_f4_t wk = wtab[k * NCV];
#pragma unroll
                            for (int i = 0; i < 4; ++i) {
                                y3[i] = fmaf(wk[i], zw[(u + k) % NW][i], y3[i]);
                                if (k == 0) w0[i] = wk[i];
                                else {
                                    const float gk = win[(u + KT - 1 - k) % KT][i];
                                    dz[i] = fmaf(wk[i], gk, dz[i]);
                                    dwacc[k][i] = fmaf(zw[s0][i], gk, dwacc[k][i]);
                                }
                            }
                        }
                        float y[4], z[4], ds[4], dh[4];
                        activate(yr[s0 * 256], y, z, ds);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float g0 = dy_ok ? fmaf(a1[i], p[i], fmaf(a2[i], round_t<T>(y3[i]), a3[i])) : 0.f;
                            win[sn][i] = g0;
                            dz[i] = fmaf(w0[i], g0, dz[i]);
                            dwacc[0][i] = fmaf(zw[s0][i], g0, dwacc[0][i]);
                            dh[i] = dz[i] * ds[i];
                        }
                        st4<T>(dhp + e0 + t * tstride, dh);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const float r = round_t<T>(dh[i]);
                            st0[i] += r;
                            st1[i] = fmaf(r, y[i], st1[i]);              // raw sum(dh2 * y2): normalised once, below
                        }
                    } else {
                        // the P frames before frame 0: only dy3(t + P) is due
#pragma unroll
                        for (int i = 0; i < 4; ++i) win[sn][i] = 0.f;
                        if (dy_ok) {
                            float y3[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int k = 0; k < KT; ++k) {
                                const dwt_f4_t wk = wtab[k * NCV];
#pragma unroll
                                for (int i = 0; i < 4; ++i) y3[i] = fmaf(wk[i], zw[(u + k) % NW][i], y3[i]);
                            }
#pragma unroll
                            for (int i = 0; i < 4; ++i) win[sn][i] = fmaf(a1[i], p[i], fmaf(a2[i], round_t<T>(y3[i]), a3[i]));
                        }
                    }
                }
            }
        }
    }
    // sum(dh2 * (y2 - mean) * invstd) = invstd * (sum(dh2 * y2) - mean * sum(dh2)), as in the rc kernel; mean and invstd are
    // fetched here, not held through the loop
    {
        float bm[4], bi[4];
        ldc4(a.y2.v3 + chs, bm); ldc4(a.y2.v4 + chs, bi);
#pragma unroll
        for (int i = 0; i < 4; ++i) st1[i] = bi[i] * fmaf(-bm[i], st0[i], st1[i]);
    }
    DET_WAVES_BEGIN
    if (chan_ok) {
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) atomicAdd(&lw[k * CS + cv * 4 + i], dwacc[k][i]);
    }
    DET_WAVES_END
    __syncthreads();
    DET_ENTER();
    for (int i = tid; i < KT * CS; i += 256) {
        int k = i / CS, c = c0 + i % CS;
        if (c < a.C) atomicAdd(a.dw + (i64)c * KT + k, lw[i]);
    }
    if (a.stats) block_stats_flush<T>(lstat, st0, st1, cv, c0, a.C, a.stats, blockIdx.x % DWN_NREP);
    DET_EXIT();
}

// what launch_dw_temporal_wide_fwd / _bwd refuse, in this order; host only, so the C entries ask it before they enter the device
int dw_temporal_wide_check(int kt, int C, int dy_kind) {
    if (kt != 7 && kt != 9) return dwn_set_error(-4, "dw_temporal_wide: only temporal_kernel 7 or 9 is built (3 and 5: dwn_dw_temporal_fwd / _bwd)");
    if (C % 8) return dwn_set_error(-2, "dw_temporal_wide: C must be a multiple of 8");
    if (dy_kind != LD_PLAIN)
        return dwn_set_error(-3, "dw_temporal_wide_bwd: the stored-y3 loaders (LD_AFFINE2, LD_DY3) are built for temporal_kernel 3 and 5 only");
    return 0;
}

// temporal backward, every size and loader (the forward's launcher stands behind its kernel, above)
template <typename T>
static int temporal_bwd_t(const DwTemporalBwd& a, hipStream_t s) {
    constexpr int CS = SL<T>::CS, LP = SL<T>::LP;
    if (a.C % 8) return dwn_set_error(-2, "dw_temporal: C must be a multiple of 8");
    const int slices = (a.C + CS - 1) / CS;
    const i64 work = ((i64)a.B * a.HW + LP - 1) / LP;
    auto go = [&](auto kernel) { return launch_dw(kernel, 256, 0, slices, work, s, a); };
    if (a.dy_kind == LD_PLAIN) {       // dy.p = dh3 only: y3 is recomputed from y2 (three passes instead of four)
        switch (a.kt) {                // 7 and 9 arrive through launch_dw_temporal_wide_bwd, which refuses the other loaders first
            case 3: return go(dw_temporal_bwd_rc_kernel<T, 3>);
            case 5: return go(dw_temporal_bwd_rc_kernel<T, 5>);
            case 7: return go(dw_temporal_bwd_wide_kernel<T, 7>);
            case 9: return go(dw_temporal_bwd_wide_kernel<T, 9>);
        }
        return dwn_set_error(-4, "dw_temporal: only temporal_kernel 3 or 5 is built");
    }
    const bool dy3 = a.dy_kind == LD_DY3;
    if (!dy3 && a.dy_kind != LD_AFFINE2) return dwn_set_error(-3, "dw_temporal_bwd: unsupported dy loader");
    if (a.kt == 5) return dy3 ? go(dw_temporal_bwd_kernel<T, 5, LD_DY3, 4>) : go(dw_temporal_bwd_kernel<T, 5, LD_AFFINE2, 4>);
    if (a.kt == 3) return dy3 ? go(dw_temporal_bwd_kernel<T, 3, LD_DY3, 4>) : go(dw_temporal_bwd_kernel<T, 3, LD_AFFINE2, 4>);
    return dwn_set_error(-4, "dw_temporal: only temporal_kernel 3 or 5 is built");
}
int launch_dw_temporal_wide_bwd(const DwTemporalBwd& a, int dtype, hipStream_t s) {
    if (int rc = dw_temporal_wide_check(a.kt, a.C, a.dy_kind)) return rc;
    return dtype == DWN_BF16 ? temporal_bwd_t<bf16_t>(a, s) : temporal_bwd_t<float>(a, s);
}
int launch_dw_temporal_bwd(const DwTemporalBwd& a, int dtype, hipStream_t s) {
    if (a.kt == 7 || a.kt == 9) return launch_dw_temporal_wide_bwd(a, dtype, s);       // dw_temporal_wide_check first
    return dtype == DWN_BF16 ? temporal_bwd_t<bf16_t>(a, s) : temporal_bwd_t<float>(a, s);
}


// Regularised MEI synthesis (include/dwn.h dwn_blur3d_args, dwn_clip_moments_args, dwn_mei_update_args): the
// smoothness prior and the luminance / contrast projection of the pixel-space ascent.
//
//   blur3d    two launches.  blur_plane_kernel: one workgroup per (clip, frame, BL_TH x BL_TW tile of the window); the tile and its
//             halo go to LDS with zeros outside the window, the x axis is filtered LDS -> LDS over the tile's rows and halo rows,
//             the y axis LDS -> workspace.  blur_time_kernel: one thread per 4 (or 1) pixels of the destination channel; the
//             2 Rt + 1 frames of the workspace it needs are read through the cache (a thread's taps are a pixel column: the
//             neighbouring frames of a workgroup re-read the same lines), taps outside [0, T) are skipped, pixels outside the
//             window are written with 0 and read nothing.  Every sum starts from its first product and continues with fmaf in
//             ascending tap order: the same expression in both builds, and 1.0f * x on an axis of radius 0.
//   moments   moments_partial_kernel: one workgroup per (clip, chunk of DWN_MOMENTS_CHUNK window elements); the chunk stays in
//             registers, so the chunk mean and the centred sum about it cost one read.  moments_fold_kernel: one wave per clip,
//             mean = (sum of sums) / n and M2 = sum_c (M2_c + n_c (mean_c - mean)^2), every term non-negative.  Float64, a fixed
//             butterfly inside the wave and a fixed order over waves and chunks.  The element -> thread assignment does not depend
//             on the load width, so an offset view gives the bits of the aligned tensor.
//   update    one thread per 4 (or 1) window elements; the per-clip coefficient is recomputed by every thread from the [B][4]
//             table (uniform loads), the element is evaluated in float64 and rounded once.
// The taps, the statistics and lr are read from device memory at run time: a captured graph follows their schedules.  No address
// depends on a tensor value; no atomics; every grid is a function of the geometry alone.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"

namespace {

constexpr int BL_NT = 256;
constexpr int BL_R = DWN_BLUR_MAX_RADIUS;
constexpr int BL_TS = DWN_BLUR_TAPS_STRIDE;
constexpr int BL_TH = 16, BL_TW = 64;                          // outputs per tile
constexpr int BL_IH = BL_TH + 2 * BL_R, BL_IW = BL_TW + 2 * BL_R;   // with the largest halo: 48 x 96

constexpr int MO_NT = 256;
constexpr int MO_PER = DWN_MOMENTS_CHUNK / MO_NT;              // 16 elements per thread: 4 groups of 4 consecutive ones
constexpr int MO_WAVES = MO_NT / 64;
static_assert(MO_PER == 16, "the partial kernel holds 4 x 4 elements per thread");

struct Window { int y0, x0, wh, ww; };

template <typename A>
inline Window window_of(const A& a) {
    const bool whole = a.wh == 0 && a.ww == 0;
    return Window{whole ? 0 : a.y0, whole ? 0 : a.x0, whole ? a.H : a.wh, whole ? a.W : a.ww};
}

// ---- blur: x then y, inside one frame
__global__ __launch_bounds__(BL_NT) void blur_plane_kernel(const float* __restrict__ src, float* __restrict__ ws,
                                                           const float* __restrict__ taps, int Cin, int c, int T, int H, int W,
                                                           int Rh, int Rw, Window wd, int tiles_y, int tiles_x) {
    __shared__ float tin[BL_IH * BL_IW];
    __shared__ float mid[BL_IH * BL_TW];
    __shared__ float kh[BL_TS], kw[BL_TS];
    const int tid = threadIdx.x;
    i64 item = blockIdx.x;                                     // ((b * T + t) * tiles_y + ty) * tiles_x + tx
    const int tx = (int)(item % tiles_x); item /= tiles_x;
    const int ty = (int)(item % tiles_y); item /= tiles_y;
    const int t = (int)(item % T);
    const i64 b = item / T;
    const i64 HW = (i64)H * W;
    const float* s = src + ((b * Cin + c) * T + t) * HW;
    float* o = ws + (b * T + t) * HW;
    const int wy0 = ty * BL_TH, wx0 = tx * BL_TW;              // tile origin, window coordinates
    const int th = min(BL_TH, wd.wh - wy0), tw = min(BL_TW, wd.ww - wx0);
    const int ih = th + 2 * Rh, iw = tw + 2 * Rw;
    if (tid < BL_TS) { kh[tid] = taps[BL_TS + tid]; kw[tid] = taps[2 * BL_TS + tid]; }
    for (int i = tid; i < ih * iw; i += BL_NT) {
        const int r = i / iw, q = i - r * iw;
        const int wy = wy0 - Rh + r, wx = wx0 - Rw + q;
        const bool inside = (unsigned)wy < (unsigned)wd.wh && (unsigned)wx < (unsigned)wd.ww;
        tin[r * BL_IW + q] = inside ? s[(i64)(wd.y0 + wy) * W + (wd.x0 + wx)] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < ih * tw; i += BL_NT) {
        const int r = i / tw, q = i - r * tw;
        const float* row = tin + r * BL_IW + q;
        float acc = kw[0] * row[0];
        for (int k = 1; k <= 2 * Rw; ++k) acc = fmaf(kw[k], row[k], acc);
        mid[r * BL_TW + q] = acc;
    }
    __syncthreads();
    for (int i = tid; i < th * tw; i += BL_NT) {
        const int r = i / tw, q = i - r * tw;
        const float* col = mid + r * BL_TW + q;
        float acc = kh[0] * col[0];
        for (int j = 1; j <= 2 * Rh; ++j) acc = fmaf(kh[j], col[j * BL_TW], acc);
        o[(i64)(wd.y0 + wy0 + r) * W + (wd.x0 + wx0 + q)] = acc;
    }
}

// ---- blur: t, from the workspace into the destination channel (the whole plane: 0 outside the window)
template <int VEC>
__global__ __launch_bounds__(BL_NT) void blur_time_kernel(const float* __restrict__ ws, float* __restrict__ dst,
                                                          const float* __restrict__ taps, int Cin, int c, int T, int H, int W,
                                                          int Rt, Window wd, i64 units) {
    const i64 u = (i64)blockIdx.x * BL_NT + threadIdx.x;
    if (u >= units) return;
    const int Wq = W / VEC;
    i64 r = u;
    const int x = (int)(r % Wq) * VEC; r /= Wq;
    const int y = (int)(r % H); r /= H;
    const int t = (int)(r % T);
    const i64 b = r / T;
    const i64 HW = (i64)H * W;
    const float* in = ws + (b * T * HW + (i64)y * W + x);      // frame 0 of this pixel
    float* out = dst + (((b * Cin + c) * T + t) * HW + (i64)y * W + x);
    const bool row_in = (unsigned)(y - wd.y0) < (unsigned)wd.wh;
    const int lo = max(0, Rt - t), hi = min(2 * Rt, Rt + T - 1 - t);     // taps whose frame t + i - Rt is in [0, T): lo <= Rt <= hi
    float acc[VEC];
    if constexpr (VEC == 4) {
        if (row_in && x >= wd.x0 && x + 3 < wd.x0 + wd.ww) {
            const float4 v0 = *reinterpret_cast<const float4*>(in + (i64)(t + lo - Rt) * HW);
            const float k0 = taps[lo];
            acc[0] = k0 * v0.x; acc[1] = k0 * v0.y; acc[2] = k0 * v0.z; acc[3] = k0 * v0.w;
            for (int i = lo + 1; i <= hi; ++i) {
                const float4 v = *reinterpret_cast<const float4*>(in + (i64)(t + i - Rt) * HW);
                const float k = taps[i];
                acc[0] = fmaf(k, v.x, acc[0]); acc[1] = fmaf(k, v.y, acc[1]);
                acc[2] = fmaf(k, v.z, acc[2]); acc[3] = fmaf(k, v.w, acc[3]);
            }
            *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        acc[e] = 0.f;
        if (row_in && (unsigned)(x + e - wd.x0) < (unsigned)wd.ww) {
            float a = taps[lo] * in[(i64)(t + lo - Rt) * HW + e];
            for (int i = lo + 1; i <= hi; ++i) a = fmaf(taps[i], in[(i64)(t + i - Rt) * HW + e], a);
            acc[e] = a;
        }
    }
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(out) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    else out[0] = acc[0];
}

// ---- moments (the sums: dwn_reduce.h, a fixed butterfly inside each wave, then the waves in order)
// address of window element i of a clip's channel (i = (t * wh + wy) * ww + wx)
__device__ __forceinline__ i64 window_offset(int i, const Window& wd, int W, i64 HW) {
    const int per = wd.wh * wd.ww;
    const int t = i / per, rem = i - t * per;
    const int wy = rem / wd.ww, wx = rem - wy * wd.ww;
    return (i64)t * HW + (i64)(wd.y0 + wy) * W + (wd.x0 + wx);
}

// thread tid holds elements chunk * CHUNK + (k * NT + tid) * 4 + e, k, e = 0..3, whatever the load width.  VEC: the window is the
// whole plane (the channel block is contiguous), n % 4 == 0 and the base is 16-byte aligned.
template <bool VEC>
__device__ __forceinline__ void load_chunk(const float* __restrict__ base, int first, int n, const Window& wd, int W, i64 HW,
                                           float (&v)[MO_PER], bool (&on)[MO_PER]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i0 = first + (k * MO_NT + (int)threadIdx.x) * 4;
        if (VEC) {
            const bool in = i0 < n;
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in) q = *reinterpret_cast<const float4*>(base + i0);
            v[k * 4 + 0] = q.x; v[k * 4 + 1] = q.y; v[k * 4 + 2] = q.z; v[k * 4 + 3] = q.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) on[k * 4 + e] = in;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = i0 + e < n;
                on[k * 4 + e] = in;
                v[k * 4 + e] = in ? base[window_offset(i0 + e, wd, W, HW)] : 0.f;
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(MO_NT) void moments_partial_kernel(const float* __restrict__ x, double* __restrict__ part, int Cin,
                                                                int c, int T, int H, int W, Window wd, int n, int nchunk) {
    __shared__ double red[MO_WAVES];
    const i64 b = blockIdx.x / nchunk;
    const int chunk = (int)(blockIdx.x - b * nchunk);
    const i64 HW = (i64)H * W;
    const float* base = x + (b * Cin + c) * T * HW;
    const int first = chunk * DWN_MOMENTS_CHUNK;
    const int nc = min(DWN_MOMENTS_CHUNK, n - first);
    float v[MO_PER];
    bool on[MO_PER];
    load_chunk<VEC>(base, first, n, wd, W, HW, v, on);
    double s = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < MO_PER; ++k)
        if (on[k]) { const double d = (double)v[k]; s += d; s2 += d * d; }
    s = wg_wave_sum<MO_NT>(s, red);
    s2 = wg_wave_sum<MO_NT>(s2, red);
    const double mean = s / (double)nc;
    double m2 = 0.0;
#pragma unroll
    for (int k = 0; k < MO_PER; ++k)
        if (on[k]) { const double d = (double)v[k] - mean; m2 += d * d; }
    m2 = wg_wave_sum<MO_NT>(m2, red);
    if (threadIdx.x == 0) {
        double* p = part + (i64)blockIdx.x * 3;
        p[0] = s; p[1] = m2; p[2] = s2;
    }
}

// one wave per clip
__global__ __launch_bounds__(64) void moments_fold_kernel(const double* __restrict__ part, double* __restrict__ stat, int n,
                                                          int nchunk) {
    const i64 b = blockIdx.x;
    const double* p = part + b * nchunk * 3;
    double s = 0.0, s2 = 0.0;
    for (int ch = threadIdx.x; ch < nchunk; ch += 64) { s += p[ch * 3]; s2 += p[ch * 3 + 2]; }
    s = wave_sum(s);
    s2 = wave_sum(s2);
    const double mean = s / (double)n;
    double m2 = 0.0;
    for (int ch = threadIdx.x; ch < nchunk; ch += 64) {
        const double nc = (double)min(DWN_MOMENTS_CHUNK, n - ch * DWN_MOMENTS_CHUNK);
        const double d = p[ch * 3] / nc - mean;
        m2 += p[ch * 3 + 1] + nc * (d * d);
    }
    m2 = wave_sum(m2);
    if (threadIdx.x == 0) {
        double* o = stat + b * 4;
        o[0] = (double)n; o[1] = mean; o[2] = m2; o[3] = s2;
    }
}

// ---- update
struct MeiCoef {
    int mode, has_mean, has_contrast, contrast_mode;
    float lo, hi;
    double mean_target, contrast;
};

template <bool VEC>
__global__ __launch_bounds__(MO_NT) void mei_update_kernel(float* __restrict__ x, const float* __restrict__ g,
                                                           const double* __restrict__ stat, const float* __restrict__ lr, int Cin,
                                                           int c, int Cin_g, int c_g, int T, int H, int W, Window wd, int n,
                                                           int nblk, MeiCoef k) {
    constexpr int PER = VEC ? 4 : 1;
    const i64 b = blockIdx.x / nblk;
    const int blk = (int)(blockIdx.x - b * nblk);
    const int i0 = (blk * MO_NT + (int)threadIdx.x) * PER;
    if (i0 >= n) return;
    const i64 HW = (i64)H * W;
    const i64 off = VEC ? (i64)i0 : window_offset(i0, wd, W, HW);
    float* px = x + (b * Cin + c) * T * HW + off;
    const double* st = stat + b * 4;
    const double cnt = st[0], mu = st[1], M2 = st[2], S2 = st[3];
    float v[PER];
    if constexpr (VEC) { const float4 q = *reinterpret_cast<const float4*>(px); v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
    else v[0] = px[0];
    if (k.mode == DWN_MEI_STEP) {
        if (!is_finite(S2)) {
#pragma unroll
            for (int e = 0; e < PER; ++e) v[e] = qnan_f();
        } else {
            if (S2 == 0.0) return;                             // the whole clip: no step
            const float* pg = g + (b * Cin_g + c_g) * T * HW + off;
            float gv[PER];
            if constexpr (VEC) { const float4 q = *reinterpret_cast<const float4*>(pg); gv[0] = q.x; gv[1] = q.y; gv[2] = q.z; gv[3] = q.w; }
            else gv[0] = pg[0];
            const double a = (double)*lr * (1.0 / sqrt(S2 / cnt));
#pragma unroll
            for (int e = 0; e < PER; ++e) v[e] = (float)((double)v[e] + a * (double)gv[e]);
        }
    } else {
        if (!(is_finite(mu) && is_finite(M2))) {
#pragma unroll
            for (int e = 0; e < PER; ++e) v[e] = qnan_f();
        } else {
            const double sd = sqrt(M2 / cnt);
            const double m = k.has_mean ? k.mean_target : mu;
            double s = 1.0;
            if (k.has_contrast) {
                if (k.contrast_mode == DWN_MEI_CONTRAST_FIXED) s = sd == 0.0 ? 0.0 : k.contrast / sd;
                else s = sd == 0.0 ? 1.0 : fmin(1.0, k.contrast / sd);
            }
            const bool binds = !(s == 1.0 && m == mu);
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const float r = binds ? (float)(m + s * ((double)v[e] - mu)) : v[e];
                v[e] = fminf(fmaxf(r, k.lo), k.hi);
            }
        }
    }
    if constexpr (VEC) *reinterpret_cast<float4*>(px) = make_float4(v[0], v[1], v[2], v[3]);
    else px[0] = v[0];
}

inline int moments_nchunk(i64 n) { return (int)((n + DWN_MOMENTS_CHUNK - 1) / DWN_MOMENTS_CHUNK); }

}  // namespace

size_t k_blur3d_ws_bytes(const dwn_blur3d_args& a) { return (size_t)a.B * a.T * a.H * a.W * sizeof(float); }

int k_blur3d(const dwn_blur3d_args& a, hipStream_t s) {
    const Window wd = window_of(a);
    const int tiles_y = (wd.wh + BL_TH - 1) / BL_TH, tiles_x = (wd.ww + BL_TW - 1) / BL_TW;
    const i64 items = (i64)a.B * a.T * tiles_y * tiles_x;
    float* ws = (float*)a.ws;
    hipLaunchKernelGGL(blur_plane_kernel, dim3((unsigned)items), dim3(BL_NT), 0, s, a.src, ws, a.taps, a.Cin_src, a.c_src, a.T, a.H, a.W,
                       a.Rh, a.Rw, wd, tiles_y, tiles_x);
    DWN_CHECK_LAUNCH();
    const bool vec = (a.W % 4) == 0 && aligned16(ws) && aligned16(a.dst);
    const i64 units = (i64)a.B * a.T * a.H * (a.W / (vec ? 4 : 1));
    const dim3 grid((unsigned)((units + BL_NT - 1) / BL_NT));
    if (vec) hipLaunchKernelGGL(blur_time_kernel<4>, grid, dim3(BL_NT), 0, s, ws, a.dst, a.taps, a.Cin_dst, a.c_dst, a.T, a.H, a.W, a.Rt, wd, units);
    else hipLaunchKernelGGL(blur_time_kernel<1>, grid, dim3(BL_NT), 0, s, ws, a.dst, a.taps, a.Cin_dst, a.c_dst, a.T, a.H, a.W, a.Rt, wd, units);
    DWN_CHECK_LAUNCH();
    return 0;
}

size_t k_clip_moments_ws_bytes(const dwn_clip_moments_args& a) {
    const Window wd = window_of(a);
    return (size_t)a.B * moments_nchunk((i64)a.T * wd.wh * wd.ww) * 3 * sizeof(double);
}

int k_clip_moments(const dwn_clip_moments_args& a, hipStream_t s) {
    const Window wd = window_of(a);
    const int n = a.T * wd.wh * wd.ww;
    const int nchunk = moments_nchunk(n);
    const bool whole = wd.wh == a.H && wd.ww == a.W;
    const bool vec = whole && (n % 4) == 0 && aligned16(a.x);
    double* part = (double*)a.ws;
    const dim3 grid((unsigned)((i64)a.B * nchunk));
    if (vec) hipLaunchKernelGGL(moments_partial_kernel<true>, grid, dim3(MO_NT), 0, s, a.x, part, a.Cin, a.c, a.T, a.H, a.W, wd, n, nchunk);
    else hipLaunchKernelGGL(moments_partial_kernel<false>, grid, dim3(MO_NT), 0, s, a.x, part, a.Cin, a.c, a.T, a.H, a.W, wd, n, nchunk);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(moments_fold_kernel, dim3((unsigned)a.B), dim3(64), 0, s, part, a.stat, n, nchunk);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_mei_update(const dwn_mei_update_args& a, hipStream_t s) {
    const Window wd = window_of(a);
    const int n = a.T * wd.wh * wd.ww;
    const bool whole = wd.wh == a.H && wd.ww == a.W;
    const bool vec = whole && (n % 4) == 0 && aligned16(a.x) && (a.mode != DWN_MEI_STEP || aligned16(a.g));
    const int per = MO_NT * (vec ? 4 : 1);
    const int nblk = (n + per - 1) / per;
    MeiCoef k;
    k.mode = a.mode; k.has_mean = a.has_mean; k.has_contrast = a.has_contrast; k.contrast_mode = a.contrast_mode;
    k.lo = a.lo; k.hi = a.hi; k.mean_target = a.mean_target; k.contrast = a.contrast;
    const dim3 grid((unsigned)((i64)a.B * nblk));
    if (vec) hipLaunchKernelGGL(mei_update_kernel<true>, grid, dim3(MO_NT), 0, s, a.x, a.g, a.stat, a.lr, a.Cin, a.c, a.Cin_g, a.c_g, a.T, a.H, a.W, wd, n, nblk, k);
    else hipLaunchKernelGGL(mei_update_kernel<false>, grid, dim3(MO_NT), 0, s, a.x, a.g, a.stat, a.lr, a.Cin, a.c, a.Cin_g, a.c_g, a.T, a.H, a.W, wd, n, nblk, k);
    DWN_CHECK_LAUNCH();
    return 0;
}

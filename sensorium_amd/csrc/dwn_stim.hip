// In-silico stimuli (include/dwn.h dwn_gabor_args): a drifting Gabor rendered straight into the NCDHW fp32 model
// input, and the reduction of the input gradient to the eight Gabor parameters of each clip.
//
//   forward   one launch over all B*Cin*T planes, as the gaze shifter's stream: the copied channels move with 16-byte accesses
//             where the plane size and the alignment allow, the video channel is computed per pixel.  The carrier's phase is kept
//             in CYCLES and reduced with q - rint(q) before sincospif: the reduction is exact, so the error of the carrier is the
//             rounding of q itself and does not grow with the number of cycles beyond that.
//   backward  one workgroup per (clip, frame, chunk of GB_CHUNK window pixels): per-pixel products in fp32, eight float64 sums per
//             thread, a fixed butterfly inside each wave and a fixed order over the waves.  The partials go to the caller's
//             workspace; one workgroup per clip folds them in a fixed order and applies the per-clip factors in float64.
// gabor_pixel() is the one place that evaluates the stimulus: the backward decides the clamp mask from its own recomputation of
// `raw`, with contraction switched off inside the function, so the two passes see the same bits.
// No parameter is ever converted to an integer and no address depends on one: any bit pattern in `params` is safe.  No atomics;
// the grids of the backward depend on the geometry alone (not on the build, not on the occupancy the runtime reports).
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_launch.h"
#include "dwn_philox.h"
#include "dwn_reduce.h"

namespace {

constexpr int GB_NT = 256;
constexpr int GB_PIX = 4;                      // window pixels per thread of the backward
constexpr int GB_CHUNK = GB_NT * GB_PIX;       // window pixels per workgroup of the backward
constexpr int GB_NSUM = 8;                     // float64 sums per partial (below)
constexpr int GB_WAVES = GB_NT / 64;

struct GaborGeom {
    int y0, x0, wh, ww;                        // the window, resolved (whole plane: 0, 0, H, W)
    int clamp;
    float background, lo, hi, pad;
};

struct GaborClip {
    float cy, cx, ct, st, sf, tf, phc, amp, k2;    // cos / sin theta, phase in cycles, 1 / (2 sigma^2)
    bool ok;
};

struct GaborPix {
    float dyp, dxp, u, r2, ec, es, raw;            // ec = envelope * cos, es = envelope * sin
};

__device__ __forceinline__ GaborClip gabor_clip(const float* __restrict__ p, bool gauss) {
    GaborClip g;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 8; ++k) fin = fin && fabsf(p[k]) <= FLT_MAX;      // false for NaN and Inf
    const float sigma = p[2];
    g.ok = fin && (!gauss || sigma > 0.f);
    g.cy = p[0]; g.cx = p[1]; g.sf = p[4]; g.tf = p[5]; g.amp = p[7];
    sincosf(p[3], &g.st, &g.ct);
    g.phc = p[6] * 0.15915494309189535f;
    // a sigma whose square underflows: the factor stays finite, so the centre pixel (r2 == 0) is 0 * finite, not 0 * Inf
    g.k2 = gauss ? fminf(0.5f / (sigma * sigma), FLT_MAX) : 0.f;
    return g;
}

// The stimulus at pixel (y, x) of frame t (ft = (float)t).  Every operation is rounded on its own: the forward and the backward
// inline this function into different loops, and a product contracted into an FMA in one of them only would move `raw` by an ulp.
template <bool GAUSS>
__device__ __forceinline__ GaborPix gabor_pixel(const GaborClip& g, float ft, int y, int x, float background) {
#pragma clang fp contract(off)
    GaborPix p;
    p.dyp = (float)y - g.cy;
    p.dxp = (float)x - g.cx;
    p.u = p.dxp * g.ct + p.dyp * g.st;
    const float q = (g.sf * p.u - g.tf * ft) + g.phc;
    const float r = q - rintf(q);                  // exact (Sterbenz): |r| <= 1/2
    float s, c;
    sincospif(2.f * r, &s, &c);
    p.r2 = p.dxp * p.dxp + p.dyp * p.dyp;
    const float e = GAUSS ? expf(-(p.r2 * g.k2)) : 1.f;
    p.ec = e * c;
    p.es = e * s;
    p.raw = background + g.amp * p.ec;
    return p;
}

__device__ __forceinline__ void copy_plane(const float* __restrict__ src, float* __restrict__ dst, int HW, int vec) {
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int i = threadIdx.x; i < (HW >> 2); i += GB_NT) d4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < HW; i += GB_NT) dst[i] = src[i];
    }
}

// plane p = (b * Cin + c) * T + t
template <bool GAUSS>
__global__ __launch_bounds__(GB_NT) void gabor_stream_kernel(const float* __restrict__ in, const float* __restrict__ params,
                                                             float* __restrict__ out, i64 planes, int Cin, int T, int H, int W,
                                                             int vc, GaborGeom gm, int vec) {
    const int HW = H * W;
    const UDiv32 divW((unsigned)W);
    for (i64 p = blockIdx.x; p < planes; p += gridDim.x) {
        const i64 bc = p / T;
        const int t = (int)(p - bc * T);
        const i64 b = bc / Cin;
        const int c = (int)(bc - b * Cin);
        float* dst = out + p * HW;
        if (c != vc) {
            copy_plane(in + p * HW, dst, HW, vec);
            continue;
        }
        const GaborClip g = gabor_clip(params + b * 8, GAUSS);
        const float ft = (float)t, bad = qnan_f();
        for (int i = threadIdx.x; i < HW; i += GB_NT) {
            const int y = (int)divW.div((unsigned)i), x = i - y * W;
            const bool inside = (unsigned)(y - gm.y0) < (unsigned)gm.wh && (unsigned)(x - gm.x0) < (unsigned)gm.ww;
            float o = gm.pad;
            if (inside) {
                o = gabor_pixel<GAUSS>(g, ft, y, x, gm.background).raw;
                if (gm.clamp) o = fminf(fmaxf(o, gm.lo), gm.hi);
                o = g.ok ? o : bad;
            }
            dst[i] = o;
        }
    }
}

// Partial sums of one (clip, frame, chunk), with g = dout where the clamp passes and 0 elsewhere:
//   0 sum g ec   1 sum g es   2 sum g es u   3 sum g es v   4 sum g ec r2   5 sum g ec dyp   6 sum g ec dxp   7 t * (sum g es)
// u = dxp cos + dyp sin, v = du / dtheta = dyp cos - dxp sin.  The products are fp32, the sums float64.
template <bool GAUSS>
__global__ __launch_bounds__(GB_NT) void gabor_partial_kernel(const float* __restrict__ params, const float* __restrict__ dout,
                                                              double* __restrict__ part, int Cin, int T, int H, int W, int vc,
                                                              GaborGeom gm, int nchunk) {
    __shared__ double red[GB_WAVES][GB_NSUM];
    const i64 item = blockIdx.x;                   // (b * T + t) * nchunk + chunk
    const i64 f = item / nchunk;
    const int chunk = (int)(item - f * nchunk);
    const i64 b = f / T;
    const int t = (int)(f - b * T);
    const float* d = dout + ((b * Cin + vc) * T + t) * ((i64)H * W);
    const GaborClip g = gabor_clip(params + b * 8, GAUSS);
    const float ft = (float)t;
    const int npix = gm.wh * gm.ww;
    const UDiv32 divW((unsigned)gm.ww);
    double acc[GB_NSUM];
#pragma unroll
    for (int k = 0; k < GB_NSUM; ++k) acc[k] = 0.0;
#pragma unroll
    for (int k = 0; k < GB_PIX; ++k) {
        const int i = chunk * GB_CHUNK + k * GB_NT + (int)threadIdx.x;
        if (i < npix) {
            const int wy = (int)divW.div((unsigned)i), wx = i - wy * gm.ww;
            const int y = gm.y0 + wy, x = gm.x0 + wx;
            const GaborPix p = gabor_pixel<GAUSS>(g, ft, y, x, gm.background);
            const bool pass = !gm.clamp || (p.raw >= gm.lo && p.raw <= gm.hi);
            const float gd = pass ? d[(i64)y * W + x] : 0.f;
            const float gc = gd * p.ec, gs = gd * p.es;
            const float v = p.dyp * g.ct - p.dxp * g.st;
            acc[0] += (double)gc;
            acc[1] += (double)gs;
            acc[2] += (double)(gs * p.u);
            acc[3] += (double)(gs * v);
            acc[4] += (double)(gc * p.r2);
            acc[5] += (double)(gc * p.dyp);
            acc[6] += (double)(gc * p.dxp);
        }
    }
    // fixed butterfly inside the wave, then the waves in order
#pragma unroll
    for (int k = 0; k < GB_NSUM - 1; ++k) acc[k] = wave_sum(acc[k]);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < GB_NSUM - 1; ++k) red[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < GB_NSUM) {
        const int k = threadIdx.x;
        double s = 0.0;
        if (k < GB_NSUM - 1) {
            for (int w = 0; w < GB_WAVES; ++w) s += red[w][k];
        } else {
            for (int w = 0; w < GB_WAVES; ++w) s += red[w][1];
            s *= (double)t;
        }
        part[item * GB_NSUM + k] = s;
    }
}

// One workgroup per clip: the T * nchunk partials summed thread-strided (32 threads per sum) and by a fixed tree, then
//   dcy = A (S5 / sigma^2 + 2 pi sf sin S1)   dcx = A (S6 / sigma^2 + 2 pi sf cos S1)   dsigma = A S4 / sigma^3
//   dtheta = -2 pi A sf S3   dsf = -2 pi A S2   dtf = 2 pi A S7   dphase = -A S1   damplitude = S0
// in float64 (envelope none: the sigma terms are dropped, dsigma is exactly 0).
template <bool GAUSS>
__global__ __launch_bounds__(GB_NT) void gabor_finalize_kernel(const float* __restrict__ params, const double* __restrict__ part,
                                                               float* __restrict__ dparams, int nper) {
    __shared__ double red[GB_NT / GB_NSUM][GB_NSUM];
    const i64 b = blockIdx.x;
    const int k = threadIdx.x & (GB_NSUM - 1), l = threadIdx.x / GB_NSUM;     // 32 strided lanes per sum
    const double* src = part + b * (i64)nper * GB_NSUM;
    double s = 0.0;
    for (int i = l; i < nper; i += GB_NT / GB_NSUM) s += src[(i64)i * GB_NSUM + k];
    red[l][k] = s;
    __syncthreads();
    for (int h = GB_NT / GB_NSUM / 2; h > 0; h >>= 1) {
        if (l < h) red[l][k] += red[l + h][k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float* p = params + b * 8;
        const GaborClip g = gabor_clip(p, GAUSS);
        const double tau = 6.283185307179586476925286766559;
        const double S0 = red[0][0], S1 = red[0][1], S2 = red[0][2], S3 = red[0][3], S4 = red[0][4], S5 = red[0][5],
                     S6 = red[0][6], S7 = red[0][7];
        const double sigma = (double)p[2], sf = (double)p[4], A = (double)p[7];
        const double ct = cos((double)p[3]), st = sin((double)p[3]);
        double o[8];
        o[0] = A * tau * sf * st * S1;
        o[1] = A * tau * sf * ct * S1;
        o[2] = 0.0;
        if (GAUSS) {
            const double s2 = sigma * sigma;
            o[0] += A * S5 / s2;
            o[1] += A * S6 / s2;
            o[2] = A * S4 / (s2 * sigma);
        }
        o[3] = -tau * A * sf * S3;
        o[4] = -tau * A * S2;
        o[5] = tau * A * S7;
        o[6] = -A * S1;
        o[7] = S0;
        const float bad = qnan_f();
#pragma unroll
        for (int j = 0; j < 8; ++j) dparams[b * 8 + j] = g.ok ? (float)o[j] : bad;
    }
}

// ---- noise stimulus (include/dwn.h dwn_noise_args): every cell of every frame is one word of a Philox4x32-10 block
// addressed by (cell >> 2, frame / hold, clip number), so a clip is a function of (seed, clip number) alone.  The block is
// recomputed by each pixel of a cell (ten rounds of two 32 x 32 -> 64 multiplies): the kernel stays a single store stream.
struct NoiseGeom {
    int y0, x0, wh, ww, cell, hold, gw, sparse;
    float v_lo, v_mid, v_hi, pad;              // background - contrast, background, background + contrast: formed once on the host
    unsigned k0, k1, thr, clip0;               // key, floor(density 2^31), first clip number
};

__global__ __launch_bounds__(GB_NT) void noise_stream_kernel(const float* __restrict__ in, float* __restrict__ out, i64 planes, int Cin,
                                                             int T, int H, int W, int vc, NoiseGeom gm, int vec) {
    const int HW = H * W;
    const UDiv32 divW((unsigned)W), divC((unsigned)gm.cell);
    for (i64 p = blockIdx.x; p < planes; p += gridDim.x) {
        const i64 bc = p / T;
        const int t = (int)(p - bc * T);
        const i64 b = bc / Cin;
        const int c = (int)(bc - b * Cin);
        float* dst = out + p * HW;
        if (c != vc) {
            copy_plane(in + p * HW, dst, HW, vec);
            continue;
        }
        const unsigned step = (unsigned)(t / gm.hold), clip = gm.clip0 + (unsigned)b;     // first_clip + B <= 2^32: no wrap
        for (int i = threadIdx.x; i < HW; i += GB_NT) {
            const int y = (int)divW.div((unsigned)i), x = i - y * W;
            const bool inside = (unsigned)(y - gm.y0) < (unsigned)gm.wh && (unsigned)(x - gm.x0) < (unsigned)gm.ww;
            float o = gm.pad;
            if (inside) {
                const unsigned q = divC.div((unsigned)(y - gm.y0)) * (unsigned)gm.gw + divC.div((unsigned)(x - gm.x0));
                const unsigned w = philox_word(q >> 2, step, clip, 0u, gm.k0, gm.k1, (int)(q & 3u));
                if (gm.sparse) o = w < gm.thr ? gm.v_lo : (gm.thr != 0u && w >= 0u - gm.thr) ? gm.v_hi : gm.v_mid;
                else o = (w >> 31) ? gm.v_hi : gm.v_lo;
            }
            dst[i] = o;
        }
    }
}

inline GaborGeom gabor_geom(const dwn_gabor_args& a) {
    GaborGeom gm;
    const bool whole = a.wh == 0 && a.ww == 0;
    gm.y0 = whole ? 0 : a.y0; gm.x0 = whole ? 0 : a.x0;
    gm.wh = whole ? a.H : a.wh; gm.ww = whole ? a.W : a.ww;
    gm.clamp = a.clamp; gm.background = a.background; gm.lo = a.lo; gm.hi = a.hi; gm.pad = a.pad;
    return gm;
}

inline int gabor_nchunk(const GaborGeom& gm) { return (int)(((i64)gm.wh * gm.ww + GB_CHUNK - 1) / GB_CHUNK); }

}  // namespace

size_t k_gabor_ws_bytes(const dwn_gabor_args& a) {
    return (size_t)a.B * a.T * gabor_nchunk(gabor_geom(a)) * GB_NSUM * sizeof(double);
}

int k_gabor_forward(const dwn_gabor_args& a, hipStream_t s) {
    const i64 planes = (i64)a.B * a.Cin * a.T;
    const int vec = (((i64)a.H * a.W) % 4 == 0 && aligned16(a.x) && aligned16(a.out)) ? 1 : 0;
    const GaborGeom gm = gabor_geom(a);
    if (a.envelope == DWN_GABOR_GAUSSIAN)
        return launch_resident(gabor_stream_kernel<true>, GB_NT, 0, 4, 1, planes, false, s, a.x, a.params, a.out, planes, a.Cin, a.T,
                               a.H, a.W, a.video_channel, gm, vec);
    return launch_resident(gabor_stream_kernel<false>, GB_NT, 0, 4, 1, planes, false, s, a.x, a.params, a.out, planes, a.Cin, a.T,
                           a.H, a.W, a.video_channel, gm, vec);
}

int k_noise_forward(const dwn_noise_args& a, hipStream_t s) {
    const i64 planes = (i64)a.B * a.Cin * a.T;
    const int vec = (((i64)a.H * a.W) % 4 == 0 && aligned16(a.x) && aligned16(a.out)) ? 1 : 0;
    NoiseGeom gm;
    gm.y0 = a.y0; gm.x0 = a.x0; gm.wh = a.wh; gm.ww = a.ww; gm.cell = a.cell; gm.hold = a.hold; gm.gw = a.ww / a.cell;
    gm.sparse = a.kind == DWN_NOISE_SPARSE;
    gm.v_lo = a.background - a.contrast; gm.v_mid = a.background; gm.v_hi = a.background + a.contrast; gm.pad = a.pad;
    gm.k0 = (unsigned)(a.seed & 0xffffffffull); gm.k1 = (unsigned)(a.seed >> 32);
    gm.thr = (unsigned)floor((double)a.density * 2147483648.0);
    gm.clip0 = (unsigned)a.first_clip;
    return launch_resident(noise_stream_kernel, GB_NT, 0, 4, 1, planes, false, s, a.x, a.out, planes, a.Cin, a.T, a.H, a.W,
                           a.video_channel, gm, vec);
}

int k_gabor_backward(const dwn_gabor_args& a, hipStream_t s) {
    const GaborGeom gm = gabor_geom(a);
    const int nchunk = gabor_nchunk(gm);
    const i64 items = (i64)a.B * a.T * nchunk;
    const int nper = a.T * nchunk;
    double* part = (double*)a.ws;
    const bool gauss = a.envelope == DWN_GABOR_GAUSSIAN;
    if (gauss) hipLaunchKernelGGL(gabor_partial_kernel<true>, dim3((unsigned)items), dim3(GB_NT), 0, s, a.params, a.dout, part, a.Cin, a.T, a.H, a.W, a.video_channel, gm, nchunk);
    else hipLaunchKernelGGL(gabor_partial_kernel<false>, dim3((unsigned)items), dim3(GB_NT), 0, s, a.params, a.dout, part, a.Cin, a.T, a.H, a.W, a.video_channel, gm, nchunk);
    DWN_CHECK_LAUNCH();
    if (gauss) hipLaunchKernelGGL(gabor_finalize_kernel<true>, dim3((unsigned)a.B), dim3(GB_NT), 0, s, a.params, part, a.dparams, nper);
    else hipLaunchKernelGGL(gabor_finalize_kernel<false>, dim3((unsigned)a.B), dim3(GB_NT), 0, s, a.params, part, a.dparams, nper);
    DWN_CHECK_LAUNCH();
    return 0;
}

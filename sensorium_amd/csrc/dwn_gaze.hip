// Gaze shifter (include/dwn.h dwn_gaze_args): a per-frame translation of one channel of the NCDHW fp32 model input,
// resampled bilinearly, with its two gradients, and the per-plane mean that turns the pupil planes into one gaze per frame.
//
// A pure translation has four weights per FRAME, not per pixel, so every pass is a stream over [H][W] planes:
//   forward   one launch over all B*Cin*T planes: the copied channels move with 16-byte accesses where the plane size and the
//             alignment allow, the resampled channel reads its two source rows (4-byte accesses at the shifted column);
//   backward  dx: the same stream over dout (the adjoint of a translation is again a gather: no atomics);
//             dshift: one workgroup per frame, float64 partial sums per thread and a fixed-order tree.
// Out-of-frame taps are handled by address clamp + select (no predicated loads), the float -> int
// conversion of floor(shift) goes through a clamp (any finite shift is legal, NaN included in the conversion), and nothing
// here uses an atomic: results are bit-reproducible in the product and the -DDWN_DETERMINISTIC builds alike.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"
#include "dwn_launch.h"
#include <float.h>

namespace {

constexpr int GZ_NT = 256;

struct GazeFrame {            // one frame's translation
    int iy, ix;               // floor(dy), floor(dx), clamped to +-(size + 2): beyond that every tap is outside anyway
    float fy, fx;
    float w00, w01, w10, w11; // (1-fy)(1-fx), (1-fy)fx, fy(1-fx), fy fx
    bool finite;              // false: NaN / Inf shift
};

__device__ __forceinline__ int floor_to_int(float fl, int lim) {
    // fmaxf / fminf return the other operand for a NaN: the conversion below always sees a value in [-lim, lim]
    return (int)fminf(fmaxf(fl, -(float)lim), (float)lim);
}

__device__ __forceinline__ GazeFrame gaze_frame(const float* __restrict__ sh, int H, int W) {
    GazeFrame g;
    const float dy = sh[0], dx = sh[1];
    g.finite = fabsf(dy) <= FLT_MAX && fabsf(dx) <= FLT_MAX;
    const float fly = floorf(dy), flx = floorf(dx);
    g.iy = floor_to_int(fly, H + 2);
    g.ix = floor_to_int(flx, W + 2);
    g.fy = g.finite ? dy - fly : 0.f;
    g.fx = g.finite ? dx - flx : 0.f;
    const float ay = 1.f - g.fy, ax = 1.f - g.fx;
    g.w00 = ay * ax; g.w01 = ay * g.fx; g.w10 = g.fy * ax; g.w11 = g.fy * g.fx;
    return g;
}

// value of the plane extended by `fill` at (r, c): the load is always inside the plane (clamped address), the select decides;
// `any` collects whether a tap of this pixel was inside the frame
__device__ __forceinline__ float tap(const float* __restrict__ p, int r, int c, int H, int W, float fill, bool& any) {
    const bool in = (unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W;
    const int rr = min(max(r, 0), H - 1), cc = min(max(c, 0), W - 1);
    const float v = p[(i64)rr * W + cc];
    any = any || in;
    return in ? v : fill;
}

__device__ __forceinline__ void copy_plane(const float* __restrict__ src, float* __restrict__ dst, int HW, int vec) {
    if (vec) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int i = threadIdx.x; i < (HW >> 2); i += GZ_NT) d4[i] = s4[i];
    } else {
        for (int i = threadIdx.x; i < HW; i += GZ_NT) dst[i] = src[i];
    }
}

// plane p = (b * Cin + c) * T + t
__device__ __forceinline__ void plane_decode(i64 p, int Cin, int T, int& b, int& c, int& t) {
    const i64 bc = p / T;
    t = (int)(p - bc * T);
    b = (int)(bc / Cin);
    c = (int)(bc - (i64)b * Cin);
}

// ADJ = false: out = resample(x) on the video channel, copy elsewhere.
// ADJ = true:  dx  = adjoint gather of dout on the video channel (fill = 0: terms outside the frame are dropped), copy elsewhere.
template <bool ADJ>
__global__ __launch_bounds__(GZ_NT) void gaze_stream_kernel(const float* __restrict__ in, const float* __restrict__ shift,
                                                            float* __restrict__ out, i64 planes, int Cin, int T, int H, int W,
                                                            int vc, float fill, int vec) {
    const int HW = H * W;
    const UDiv32 divW((unsigned)W);
    for (i64 p = blockIdx.x; p < planes; p += gridDim.x) {
        int b, c, t;
        plane_decode(p, Cin, T, b, c, t);
        const float* src = in + p * HW;
        float* dst = out + p * HW;
        if (c != vc) {
            copy_plane(src, dst, HW, vec);
            continue;
        }
        const GazeFrame g = gaze_frame(shift + ((i64)b * T + t) * 2, H, W);
        const float bad = ADJ ? 0.f : qnan_f();
        for (int i = threadIdx.x; i < HW; i += GZ_NT) {
            const int y = (int)divW.div((unsigned)i), x = i - y * W;
            float v00, v01, v10, v11;
            bool any = false;
            if (ADJ) {        // out[y-iy-a][x-ix-b] reads this pixel with weight w_ab
                const int r = y - g.iy, q = x - g.ix;
                v00 = tap(src, r, q, H, W, 0.f, any);     v01 = tap(src, r, q - 1, H, W, 0.f, any);
                v10 = tap(src, r - 1, q, H, W, 0.f, any); v11 = tap(src, r - 1, q - 1, H, W, 0.f, any);
            } else {
                const int r = y + g.iy, q = x + g.ix;
                v00 = tap(src, r, q, H, W, fill, any);     v01 = tap(src, r, q + 1, H, W, fill, any);
                v10 = tap(src, r + 1, q, H, W, fill, any); v11 = tap(src, r + 1, q + 1, H, W, fill, any);
            }
            // a tap of weight 0 contributes nothing, whatever it holds (0 * Inf, 0 * NaN, a non-finite fill); a tap of weight 1
            // (shift 0; a fraction that rounds to 1, as for -1e-9) gives the bits of the source, -0.0 and Inf included.  The
            // conditions are uniform over the frame.
            v00 = g.w00 != 0.f ? v00 : 0.f; v01 = g.w01 != 0.f ? v01 : 0.f;
            v10 = g.w10 != 0.f ? v10 : 0.f; v11 = g.w11 != 0.f ? v11 : 0.f;
            float o = g.w00 * v00 + g.w01 * v01 + g.w10 * v10 + g.w11 * v11;
            o = g.w00 == 1.f ? v00 : g.w01 == 1.f ? v01 : g.w10 == 1.f ? v10 : g.w11 == 1.f ? v11 : o;
            o = any ? o : fill;                      // no tap inside the frame: the fill itself, not fill * (sum of the weights)
            dst[i] = g.finite ? o : bad;
        }
    }
}

// dshift[b][t] = sum_{y,x} dout * d out / d (dy, dx), iy / ix held constant; one workgroup per frame
__global__ __launch_bounds__(GZ_NT) void gaze_dshift_kernel(const float* __restrict__ x, const float* __restrict__ shift,
                                                            const float* __restrict__ dout, float* __restrict__ dshift,
                                                            i64 frames, int Cin, int T, int H, int W, int vc, float fill) {
    __shared__ double red[2][GZ_NT];
    const int HW = H * W;
    const UDiv32 divW((unsigned)W);
    for (i64 f = blockIdx.x; f < frames; f += gridDim.x) {
        const i64 b = f / T;
        const int t = (int)(f - b * T);
        const i64 off = ((b * Cin + vc) * T + t) * HW;
        const float* v = x + off;
        const float* d = dout + off;
        const GazeFrame g = gaze_frame(shift + f * 2, H, W);
        const float ay = 1.f - g.fy, ax = 1.f - g.fx;
        double sum[2] = {0.0, 0.0};                   // sy, sx
        for (int i = threadIdx.x; i < HW; i += GZ_NT) {
            const int y = (int)divW.div((unsigned)i), xx = i - y * W;
            const int r = y + g.iy, q = xx + g.ix;
            bool any = false;
            const float v00 = tap(v, r, q, H, W, fill, any),     v01 = tap(v, r, q + 1, H, W, fill, any);
            const float v10 = tap(v, r + 1, q, H, W, fill, any), v11 = tap(v, r + 1, q + 1, H, W, fill, any);
            // as in the forward: a difference whose coefficient is 0 contributes nothing, whatever its pixels hold
            const float gy = (ax != 0.f ? ax * (v10 - v00) : 0.f) + (g.fx != 0.f ? g.fx * (v11 - v01) : 0.f);
            const float gx = (ay != 0.f ? ay * (v01 - v00) : 0.f) + (g.fy != 0.f ? g.fy * (v11 - v10) : 0.f);
            const double dd = (double)d[i];
            sum[0] += dd * (double)gy;
            sum[1] += dd * (double)gx;
        }
        wg_tree_sum(sum, red);                         // dwn_reduce.h: the fixed tree, two values per thread
        if (threadIdx.x == 0) {
            const float bad = qnan_f();
            dshift[f * 2] = g.finite ? (float)sum[0] : bad;
            dshift[f * 2 + 1] = g.finite ? (float)sum[1] : bad;
        }
    }
}

// mean[b][t][k] over the H x W plane of channel c0 + k; one workgroup per plane.  The accumulators start at -0.0, the identity
// of the addition, so that a plane of -0.0 sums to -0.0.
__global__ __launch_bounds__(GZ_NT) void plane_mean_kernel(const float* __restrict__ x, float* __restrict__ mean, i64 nplanes,
                                                           int Cin, int T, int HW, int c0, int nc, int vec) {
    __shared__ double red[GZ_NT];
    for (i64 f = blockIdx.x; f < nplanes; f += gridDim.x) {
        const i64 bt = f / nc;
        const int k = (int)(f - bt * nc);
        const i64 b = bt / T;
        const int t = (int)(bt - b * T);
        const float* p = x + ((b * Cin + c0 + k) * T + t) * HW;
        double s0 = -0.0, s1 = -0.0;
        if (vec) {
            const float4* p4 = reinterpret_cast<const float4*>(p);
            for (int i = threadIdx.x; i < (HW >> 2); i += GZ_NT) {
                const float4 q = p4[i];
                s0 += (double)q.x; s1 += (double)q.y; s0 += (double)q.z; s1 += (double)q.w;
            }
        } else {
            for (int i = threadIdx.x; i < HW; i += GZ_NT) s0 += (double)p[i];
        }
        const double tot = wg_tree_sum(s0 + s1, red);
        if (threadIdx.x == 0) mean[f] = (float)(tot / (double)HW);
    }
}

}  // namespace

int k_gaze_forward(const dwn_gaze_args& a, hipStream_t s) {
    const i64 planes = (i64)a.B * a.Cin * a.T;
    const int vec = (((i64)a.H * a.W) % 4 == 0 && aligned16(a.x) && aligned16(a.out)) ? 1 : 0;
    return launch_resident(gaze_stream_kernel<false>, GZ_NT, 0, 4, 1, planes, false, s, a.x, a.shift, a.out, planes, a.Cin, a.T,
                           a.H, a.W, a.video_channel, a.fill, vec);
}

int k_gaze_backward(const dwn_gaze_args& a, hipStream_t s) {
    if (a.dx) {
        const i64 planes = (i64)a.B * a.Cin * a.T;
        const int vec = (((i64)a.H * a.W) % 4 == 0 && aligned16(a.dout) && aligned16(a.dx)) ? 1 : 0;
        const int rc = launch_resident(gaze_stream_kernel<true>, GZ_NT, 0, 4, 1, planes, false, s, a.dout, a.shift, a.dx, planes,
                                       a.Cin, a.T, a.H, a.W, a.video_channel, 0.f, vec);
        if (rc != 0) return rc;
    }
    if (a.dshift) {
        const i64 frames = (i64)a.B * a.T;
        return launch_resident(gaze_dshift_kernel, GZ_NT, 0, 4, 1, frames, false, s, a.x, a.shift, a.dout, a.dshift, frames,
                               a.Cin, a.T, a.H, a.W, a.video_channel, a.fill);
    }
    return 0;
}

int k_plane_mean(const float* x, int B, int Cin, int T, int H, int W, int c0, int nc, float* mean, hipStream_t s) {
    const i64 nplanes = (i64)B * T * nc;
    const int vec = (((i64)H * W) % 4 == 0 && aligned16(x)) ? 1 : 0;
    return launch_resident(plane_mean_kernel, GZ_NT, 0, 4, 1, nplanes, false, s, x, mean, nplanes, Cin, T, H * W, c0, nc, vec);
}

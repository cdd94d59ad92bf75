// Behaviour modulator (include/dwn.h dwn_modulator_args): a per-neuron gain on the readout's output,
//   a = c[n] + sum_k h[b,t,k] u[n,k],   gain = exp(m tanh(a)),   out[b,n,t] = y[b,n,t] gain
// with its four gradients.  y, out, dout, dy are [B][N][T] (T contiguous), h [B][T][K], u [N][K], c [N].
//
// Tiling, forward and backward alike: a workgroup owns MD_TN = 128 neurons x TT = min(T, 64) frames of one sample.  Its 256
// threads are NG = 256 / TT groups of TT lanes: a thread keeps ONE frame (its h row in registers, K padded with zeros to the
// template's KP, which adds exact zeros to the FMA chain) and walks the neurons ng, ng + NG, ...; u and c of the tile are in LDS
// and are read as broadcasts.  With T = 32 a wave covers two adjacent neurons: 256 contiguous bytes per access.
//
// Backward: the pass that writes dy leaves s = dout y gain m sech^2(a) of the tile in LDS, and the two reductions read it in their
// own directions:
//   du / dc   a thread per (neuron, k) sums over the tile's frames, t ascending, and goes on over the MD_RB samples of its batch
//             group in registers: one float64 partial per (batch group, frame chunk, neuron, k);
//   dh        a thread per (frame, k) sums over the tile's neurons, n ascending: one float64 partial per (neuron tile, b, t, k).
// A finaliser sums the partials in ascending order and rounds to fp32 once.  Products are fp32, sums float64, nothing is atomic and
// the grids depend on the geometry alone: the same inputs give the same bits, in the product and the -DDWN_DETERMINISTIC builds.
// sech^2 is 4 e / (1 + e)^2 with e = exp(-2 |a|): no cancellation (1 - tanh^2 is exactly 0 in fp32 from |a| ~ 9).
// A frame whose h row holds a NaN or an Inf gives NaN in that frame of out / dy / s (an infinite a would otherwise saturate the
// gain to a finite e^+-m); other frames are untouched.  A null output is skipped with its partials.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_launch.h"
#include "dwn_gain.h"
#include "dwn_reduce.h"

namespace {

constexpr int MD_NT = 256;
constexpr int MD_TN = 128;         // neurons per tile
constexpr int MD_TTMAX = 64;       // frames per tile: min(T, 64)
constexpr int MD_U = 4;            // neurons per thread whose loads are issued together
constexpr int MD_RB = 2;           // samples per batch group (du / dc partials accumulate over them in registers)

struct ModGeom {
    int B, N, T, K;
    int TT, nTc, nNt, G;           // frames per tile, frame chunks, neuron tiles, batch groups
    int ST;                        // row stride of the LDS tiles over frames: TT + 1 (odd: no bank conflicts down a column)
    float m;
};

inline ModGeom mod_geom(const dwn_modulator_args& a) {
    ModGeom g;
    g.B = a.B; g.N = a.N; g.T = a.T; g.K = a.K; g.m = a.max_log_gain;
    g.TT = a.T < MD_TTMAX ? a.T : MD_TTMAX;
    g.nTc = (a.T + g.TT - 1) / g.TT;
    g.nNt = (a.N + MD_TN - 1) / MD_TN;
    g.G = (a.B + MD_RB - 1) / MD_RB;
    g.ST = g.TT + 1;
    return g;
}

// mod_gain, mod_sech2: dwn_gain.h (shared with the retinotopic readout gain); is_finite, qnan_f: dwn_reduce.h

// u and c of the neuron tile into LDS: us [MD_TN][KP] (zero beyond K and beyond N), cs [MD_TN]
template <int KP>
__device__ __forceinline__ void load_uc(const float* __restrict__ u, const float* __restrict__ c, float* us, float* cs, int n0,
                                        int ncnt, int K) {
    for (int i = threadIdx.x; i < MD_TN * KP; i += MD_NT) {
        const int nl = i / KP, k = i - nl * KP;
        us[i] = (nl < ncnt && k < K) ? u[(i64)(n0 + nl) * K + k] : 0.f;
    }
    for (int i = threadIdx.x; i < MD_TN; i += MD_NT) cs[i] = i < ncnt ? c[n0 + i] : 0.f;
}

// the thread's h row into registers (zero beyond K); returns whether every entry is finite
template <int KP>
__device__ __forceinline__ bool load_h(const float* __restrict__ hrow, int K, float (&hr)[KP]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < KP; ++k) {
        hr[k] = k < K ? hrow[k] : 0.f;
        ok = ok && is_finite(hr[k]);
    }
    return ok;
}

template <int KP>
__device__ __forceinline__ float mod_a(const float (&hr)[KP], const float* urow, float c) {
    float a = c;
#pragma unroll
    for (int k = 0; k < KP; k += 4) {
        const float4 q = *reinterpret_cast<const float4*>(urow + k);
        a = fmaf(hr[k], q.x, a); a = fmaf(hr[k + 1], q.y, a); a = fmaf(hr[k + 2], q.z, a); a = fmaf(hr[k + 3], q.w, a);
    }
    return a;
}

// work item -> (neuron tile, frame chunk, b): b fastest within a tile so that neighbours share u
template <int KP>
__global__ __launch_bounds__(MD_NT) void modulator_fwd_kernel(const float* __restrict__ y, const float* __restrict__ h,
                                                              const float* __restrict__ u, const float* __restrict__ c,
                                                              float* __restrict__ out, ModGeom g) {
    __shared__ __attribute__((aligned(16))) float us[MD_TN * KP];
    __shared__ float cs[MD_TN];
    const i64 item = blockIdx.x;
    const int b = (int)(item % g.B);
    const i64 r = item / g.B;
    const int tc = (int)(r % g.nTc), nt = (int)(r / g.nTc);
    const int n0 = nt * MD_TN, ncnt = min(MD_TN, g.N - n0);
    const int t0 = tc * g.TT, tcnt = min(g.TT, g.T - t0);
    load_uc<KP>(u, c, us, cs, n0, ncnt, g.K);
    __syncthreads();
    const int NG = MD_NT / g.TT;
    const int tl = threadIdx.x % g.TT, ng = threadIdx.x / g.TT;
    if (ng >= NG || tl >= tcnt) return;
    float hr[KP];
    const bool ok = load_h<KP>(h + ((i64)b * g.T + t0 + tl) * g.K, g.K, hr);
    const float bad = qnan_f();
    const i64 base = ((i64)b * g.N + n0) * g.T + t0 + tl;
    // MD_U loads in flight per thread (one per iteration left the pass bound by the latency of its loads); a neuron past the
    // tile's end is loaded from the last one (an address inside the tensor) and not stored
    for (int nl0 = ng; nl0 < ncnt; nl0 += MD_U * NG) {
        float yv[MD_U];
#pragma unroll
        for (int j = 0; j < MD_U; ++j) yv[j] = y[base + (i64)min(nl0 + j * NG, ncnt - 1) * g.T];
#pragma unroll
        for (int j = 0; j < MD_U; ++j) {
            const int nl = nl0 + j * NG;
            if (nl < ncnt) {
                const float a = mod_a<KP>(hr, us + nl * KP, cs[nl]);
                const float o = yv[j] * mod_gain(a, g.m);
                out[base + (i64)nl * g.T] = ok ? o : bad;
            }
        }
    }
}

constexpr int md_nacc(int KP) { return (MD_TN * (KP + 1) + MD_NT - 1) / MD_NT; }

// dynamic LDS: hs [KP][ST] | ss [MD_TN][ST]   (floats), behind the static u / c tiles
template <int KP>
__global__ __launch_bounds__(MD_NT) void modulator_bwd_kernel(const float* __restrict__ y, const float* __restrict__ h,
                                                              const float* __restrict__ u, const float* __restrict__ c,
                                                              const float* __restrict__ dout, float* __restrict__ dy,
                                                              double* __restrict__ pdu, double* __restrict__ pdc,
                                                              double* __restrict__ pdh, ModGeom g) {
    __shared__ __attribute__((aligned(16))) float us[MD_TN * KP];
    __shared__ float cs[MD_TN];
    extern __shared__ float dyn[];
    float* hs = dyn;
    float* ss = dyn + KP * g.ST;
    constexpr int NACC = md_nacc(KP);

    const i64 item = blockIdx.x;
    const int grp = (int)(item % g.G);
    const i64 r = item / g.G;
    const int tc = (int)(r % g.nTc), nt = (int)(r / g.nTc);
    const int n0 = nt * MD_TN, ncnt = min(MD_TN, g.N - n0);
    const int t0 = tc * g.TT, tcnt = min(g.TT, g.T - t0);
    const bool red = pdu || pdc || pdh;
    load_uc<KP>(u, c, us, cs, n0, ncnt, g.K);

    const int NG = MD_NT / g.TT;
    const int tl = threadIdx.x % g.TT, ng = threadIdx.x / g.TT;
    const bool active = ng < NG && tl < tcnt;
    const int K = g.K;
    const int KO = (pdu ? K : 0) + (pdc ? 1 : 0);      // reduced outputs per neuron: du's K columns, then dc
    const int nout = ncnt * KO;
    double acc[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j) acc[j] = 0.0;
    const float bad = qnan_f();

    const int b_end = min(g.B, (grp + 1) * MD_RB);
    for (int b = grp * MD_RB; b < b_end; ++b) {
        __syncthreads();                               // u / c loaded; the previous sample's tiles are no longer read
        if (active) {
            float hr[KP];
            const bool ok = load_h<KP>(h + ((i64)b * g.T + t0 + tl) * K, K, hr);
            if (red && ng == 0) {
#pragma unroll
                for (int k = 0; k < KP; ++k) hs[k * g.ST + tl] = hr[k];
            }
            const i64 base = ((i64)b * g.N + n0) * g.T + t0 + tl;
            for (int nl0 = ng; nl0 < ncnt; nl0 += MD_U * NG) {       // as in the forward: MD_U loads of each stream in flight
                float dv[MD_U], yv[MD_U];
#pragma unroll
                for (int j = 0; j < MD_U; ++j) {
                    const i64 idx = base + (i64)min(nl0 + j * NG, ncnt - 1) * g.T;
                    dv[j] = dout[idx];
                    yv[j] = red ? y[idx] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < MD_U; ++j) {
                    const int nl = nl0 + j * NG;
                    if (nl < ncnt) {
                        const float a = mod_a<KP>(hr, us + nl * KP, cs[nl]);
                        const float gain = mod_gain(a, g.m);
                        if (dy) dy[base + (i64)nl * g.T] = ok ? dv[j] * gain : bad;
                        if (red) {
                            const float s = dv[j] * yv[j] * gain * g.m * mod_sech2(a);
                            ss[nl * g.ST + tl] = ok ? s : bad;
                        }
                    }
                }
            }
        }
        if (!red) continue;
        __syncthreads();
        // du / dc: output o of the tile = (neuron o / KO, column o % KO), summed over the frames in ascending order
        if (KO) {
#pragma unroll
            for (int j = 0; j < NACC; ++j) {
                const int o = threadIdx.x + j * MD_NT;
                if (o < nout) {
                    const int nl = o / KO, kk = o - nl * KO;
                    const float* srow = ss + nl * g.ST;
                    double sum = 0.0;
                    if (pdu && kk < K) {
                        const float* hrow = hs + kk * g.ST;
                        for (int t = 0; t < tcnt; ++t) sum += (double)(srow[t] * hrow[t]);
                    } else {
                        for (int t = 0; t < tcnt; ++t) sum += (double)srow[t];
                    }
                    acc[j] += sum;
                }
            }
        }
        // dh: output o = (frame o / K, column o % K), summed over the tile's neurons in ascending order
        if (pdh) {
            double* dst = pdh + ((i64)nt * g.B + b) * g.T * K + (i64)t0 * K;
            for (int o = threadIdx.x; o < tcnt * K; o += MD_NT) {
                const int t = o / K, k = o - t * K;
                double sum = 0.0;
                for (int nl = 0; nl < ncnt; ++nl) sum += (double)(ss[nl * g.ST + t] * us[nl * KP + k]);
                dst[o] = sum;
            }
        }
    }
    if (KO) {
        const i64 p = (i64)grp * g.nTc + tc;           // partial index of this (batch group, frame chunk)
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
            const int o = threadIdx.x + j * MD_NT;
            if (o < nout) {
                const int nl = o / KO, kk = o - nl * KO;
                if (pdu && kk < K) pdu[(p * g.N + n0 + nl) * K + kk] = acc[j];
                else pdc[p * g.N + n0 + nl] = acc[j];
            }
        }
    }
}

// one thread per reduced output: du [N][K] and dc [N] over the P = G nTc partials, dh [B][T][K] over the nNt neuron tiles,
// each in ascending order in float64, rounded once
__global__ __launch_bounds__(MD_NT) void modulator_finalize_kernel(const double* __restrict__ pdu, const double* __restrict__ pdc,
                                                                   const double* __restrict__ pdh, float* __restrict__ du,
                                                                   float* __restrict__ dc, float* __restrict__ dh, i64 nu, i64 nc,
                                                                   i64 nh, int P, int nNt) {
    const i64 i = (i64)blockIdx.x * MD_NT + threadIdx.x;
    if (i < nu) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += pdu[(i64)p * nu + i];
        du[i] = (float)s;
    } else if (i < nu + nc) {
        const i64 j = i - nu;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += pdc[(i64)p * nc + j];
        dc[j] = (float)s;
    } else if (i < nu + nc + nh) {
        const i64 j = i - nu - nc;
        double s = 0.0;
        for (int p = 0; p < nNt; ++p) s += pdh[(i64)p * nh + j];
        dh[j] = (float)s;
    }
}

struct ModWs { size_t du, dc, dh, total; };      // offsets in doubles
inline ModWs mod_ws(const ModGeom& g) {
    ModWs w;
    const size_t P = (size_t)g.G * g.nTc;
    w.du = 0;
    w.dc = w.du + P * g.N * g.K;
    w.dh = w.dc + P * g.N;
    w.total = w.dh + (size_t)g.nNt * g.B * g.T * g.K;
    return w;
}

template <int KP>
int mod_forward(const dwn_modulator_args& a, const ModGeom& g, hipStream_t s) {
    const i64 items = (i64)g.nNt * g.nTc * g.B;
    hipLaunchKernelGGL(modulator_fwd_kernel<KP>, dim3((unsigned)items), dim3(MD_NT), 0, s, a.y, a.h, a.u, a.c, a.out, g);
    DWN_CHECK_LAUNCH();
    return 0;
}

template <int KP>
int mod_backward(const dwn_modulator_args& a, const ModGeom& g, hipStream_t s) {
    const ModWs w = mod_ws(g);
    double* base = (double*)a.ws;
    double* pdu = a.du ? base + w.du : nullptr;
    double* pdc = a.dc ? base + w.dc : nullptr;
    double* pdh = a.dh ? base + w.dh : nullptr;
    const bool red = pdu || pdc || pdh;
    const i64 items = (i64)g.nNt * g.nTc * g.G;
    const size_t dyn = red ? (size_t)(KP + MD_TN) * g.ST * sizeof(float) : 0;
    hipLaunchKernelGGL(modulator_bwd_kernel<KP>, dim3((unsigned)items), dim3(MD_NT), dyn, s, a.y, a.h, a.u, a.c, a.dout, a.dy, pdu,
                       pdc, pdh, g);
    DWN_CHECK_LAUNCH();
    if (red) {
        const i64 nu = pdu ? (i64)g.N * g.K : 0, nc = pdc ? (i64)g.N : 0, nh = pdh ? (i64)g.B * g.T * g.K : 0;
        const i64 blocks = (nu + nc + nh + MD_NT - 1) / MD_NT;
        hipLaunchKernelGGL(modulator_finalize_kernel, dim3((unsigned)blocks), dim3(MD_NT), 0, s, pdu, pdc, pdh, a.du, a.dc, a.dh,
                           nu, nc, nh, g.G * g.nTc, g.nNt);
        DWN_CHECK_LAUNCH();
    }
    return 0;
}

}  // namespace

size_t k_modulator_ws_bytes(const dwn_modulator_args& a) { return mod_ws(mod_geom(a)).total * sizeof(double); }

int k_modulator_forward(const dwn_modulator_args& a, hipStream_t s) {
    const ModGeom g = mod_geom(a);
    if (a.K <= 4) return mod_forward<4>(a, g, s);
    if (a.K <= 8) return mod_forward<8>(a, g, s);
    if (a.K <= 16) return mod_forward<16>(a, g, s);
    return mod_forward<32>(a, g, s);
}

int k_modulator_backward(const dwn_modulator_args& a, hipStream_t s) {
    const ModGeom g = mod_geom(a);
    if (a.K <= 4) return mod_backward<4>(a, g, s);
    if (a.K <= 8) return mod_backward<8>(a, g, s);
    if (a.K <= 16) return mod_backward<16>(a, g, s);
    return mod_backward<32>(a, g, s);
}

// Receptive-field mapping by reverse correlation (include/dwn.h dwn_sta_args): the lagged cross-sums of a batch of
// responses with the cell means of any stimulus, into a float64 state, and the maps that state gives.
//
//   cross      the hot path: for one lag l, Cuv[:, l, :] += U^T V_l with the samples (b, t) as the K dimension, on the fp32-input
//              matrix instruction (mfma_f32_32x32x2f32: exact fp32 products, a k-ordered fma chain).  One workgroup per
//              (RF_TM neurons, RF_TG cells, lag); its four waves own one 32 x 32 tile each.  The samples are taken RF_KT at a time,
//              flattened over (b, t) so that no chunk is padded but the last: u = r - r0 (RF_KT x RF_TM) and v = cell mean - s0 of
//              frame t - l (RF_KT x RF_TG) are formed while they are staged into LDS, both stored sample-major so that the 32 lanes
//              of an operand read consecutive words.  Rows past N, columns past G and samples past the end are staged as zeros
//              in BOTH operands (0 * NaN never meets a stored element).  The accumulators stay in registers over the whole call,
//              are converted once and added to the state by their only owner.  Two variants were measured and not kept
//              (DESIGN.md 12q): a 128 x 64 workgroup tile with two tiles per wave sharing the stimulus operand (slower), and a
//              register prefetch of the next chunk (within 3 %).
//   moments    U1 / U2: one wave per neuron, lanes strided over the samples, float64, fixed butterfly.  V1 / V2: one thread per
//              (lag, cell), the samples in order, float64.
//   finalize   V1 / K and var_v once into the workspace; then one wave per neuron: cov, z and the energy of every lag in one
//              sweep, the peak cell, the thresholded centroid and its spread in three more over the peak lag (from cache).
// sta_cell() is the one place that evaluates v; contraction is off in it and in the finaliser, so a multiply and a subtract are
// two roundings here as they are in the float64 checker (tests/rf_reference.py).
// No atomics, no scratch; no grid depends on anything but the geometry, and the file does not read DWN_DETERMINISTIC: the same
// inputs give the same bits on every launch and in both builds.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"

namespace {

// the whole file: a multiply and the add that follows are two roundings (the matrix instruction is not affected)
#pragma clang fp contract(off)

constexpr int RF_NT = 256;
constexpr int RF_WAVE = 64;
constexpr int RF_TM = 64;              // neurons per workgroup of the cross term
constexpr int RF_TG = 64;              // cells per workgroup
constexpr int RF_KT = 32;              // samples per staged chunk
constexpr int RF_LD = RF_TM + 2;       // LDS row pitch (words): the four k-groups of a staging wave land in different banks
constexpr int RF_PER = RF_KT * RF_TM / RF_NT;      // staged elements per thread and operand
constexpr int RF_TILE = RF_NT / RF_WAVE;           // neurons per workgroup of the one-wave-per-neuron kernels
static_assert(RF_TM == RF_TG && RF_PER * RF_NT == RF_KT * RF_TM && RF_KT % 2 == 0, "staging layout");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct StaGeom {
    int B, Cin, T, H, W, N, channel, y0, x0, gh, gw, cell, L, t0, Tv;      // Tv = T - t0 valid frames per clip
    float s0, inv;                                                          // inv = 1 / cell^2, formed once on the host
};

// v of the cell whose first pixel is (py, px) in `plane` (one frame of the stimulus channel)
__device__ __forceinline__ float sta_cell(const float* __restrict__ plane, int W, int py, int px, int cell, float inv, float s0) {
    float s = 0.f;
    for (int dy = 0; dy < cell; ++dy) {
        const float* row = plane + (i64)(py + dy) * W + px;
        for (int dx = 0; dx < cell; ++dx) s += row[dx];
    }
    const float m = s * inv;
    return m - s0;
}

__device__ __forceinline__ const float* sta_plane(const float* __restrict__ x, const StaGeom& g, int b, int t) {
    return x + (((i64)b * g.Cin + g.channel) * g.T + t) * ((i64)g.H * g.W);
}

__global__ __launch_bounds__(RF_NT) void sta_cross_kernel(const float* __restrict__ x, const float* __restrict__ r,
                                                          const float* __restrict__ r0, double* __restrict__ Cuv, StaGeom g) {
    __shared__ float As[RF_KT][RF_LD];
    __shared__ float Bs[RF_KT][RF_LD];
    const int n0 = blockIdx.x * RF_TM, g0 = blockIdx.y * RF_TG, l = blockIdx.z;
    const int G = g.gh * g.gw, Ktot = g.B * g.Tv;
    const int tid = threadIdx.x, lane = tid & (RF_WAVE - 1), wave = tid / RF_WAVE;
    const int wm = (wave >> 1) * 32, wg = (wave & 1) * 32;
    const UDiv32 divT((unsigned)g.Tv);
    // A: thread -> neuron an, RF_PER consecutive samples (consecutive frames of one row of r while they stay in one clip)
    const int an = tid / (RF_KT / RF_PER), ak = (tid % (RF_KT / RF_PER)) * RF_PER;
    const int n = n0 + an;
    const bool n_ok = n < g.N;
    const float c0 = (n_ok && r0) ? r0[n] : 0.f;
    // B: thread -> cell bg (consecutive lanes: consecutive cells of a grid row), RF_PER consecutive samples
    const int bg = tid % RF_TG, bk = (tid / RF_TG) * RF_PER;
    const int cg = g0 + bg;
    const bool g_ok = cg < G;
    int py = 0, px = 0;
    if (g_ok) {
        const int gy = cg / g.gw, gx = cg - gy * g.gw;
        py = g.y0 + gy * g.cell; px = g.x0 + gx * g.cell;
    }
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < Ktot; k0 += RF_KT) {
#pragma unroll
        for (int j = 0; j < RF_PER; ++j) {
            const int k = k0 + ak + j;
            float u = 0.f;
            if (n_ok && k < Ktot) {
                const int b = (int)divT.div((unsigned)k), t = g.t0 + (k - b * g.Tv);
                u = r[((i64)b * g.N + n) * g.T + t] - c0;
            }
            As[ak + j][an] = u;
        }
#pragma unroll
        for (int j = 0; j < RF_PER; ++j) {
            const int k = k0 + bk + j;
            float v = 0.f;
            if (g_ok && k < Ktot) {
                const int b = (int)divT.div((unsigned)k), t = g.t0 + (k - b * g.Tv) - l;      // t0 >= L - 1: never negative
                v = sta_cell(sta_plane(x, g, b, t), g.W, py, px, g.cell, g.inv, g.s0);
            }
            Bs[bk + j][bg] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < RF_KT; kk += 2) {
            const int kr = kk + (lane >> 5);                 // operand maps: A[i = lane & 31][k = lane >> 5], B[k][j = lane & 31]
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kr][wm + (lane & 31)], Bs[kr][wg + (lane & 31)], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    // C/D map: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int col = g0 + wg + (lane & 31);
    if (col < G) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = n0 + wm + (q & 3) + 8 * (q >> 2) + 4 * (lane >> 5);
            if (row < g.N) {
                double* dst = Cuv + ((i64)row * g.L + l) * G + col;
                *dst += (double)acc[q];
            }
        }
    }
}

__global__ __launch_bounds__(RF_NT) void sta_umom_kernel(const float* __restrict__ r, const float* __restrict__ r0,
                                                         double* __restrict__ U1, double* __restrict__ U2, StaGeom g) {
    const int lane = threadIdx.x & (RF_WAVE - 1);
    const int j = blockIdx.x * RF_TILE + (int)(threadIdx.x / RF_WAVE);
    if (j >= g.N) return;                                     // a whole wave: the kernel has no barrier
    const float c0 = r0 ? r0[j] : 0.f;
    const int Ktot = g.B * g.Tv;
    const UDiv32 divT((unsigned)g.Tv);
    double s1 = 0.0, s2 = 0.0;
    for (int k = lane; k < Ktot; k += RF_WAVE) {
        const int b = (int)divT.div((unsigned)k), t = g.t0 + (k - b * g.Tv);
        const double u = (double)(r[((i64)b * g.N + j) * g.T + t] - c0);
        s1 += u; s2 += u * u;
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    if (lane == 0) { U1[j] += s1; U2[j] += s2; }
}

__global__ __launch_bounds__(RF_NT) void sta_vmom_kernel(const float* __restrict__ x, double* __restrict__ V1, double* __restrict__ V2,
                                                         StaGeom g) {
    const int G = g.gh * g.gw;
    const i64 i = (i64)blockIdx.x * RF_NT + threadIdx.x;      // (l, cell)
    if (i >= (i64)g.L * G) return;
    const int l = (int)(i / G), cg = (int)(i - (i64)l * G);
    const int gy = cg / g.gw, gx = cg - gy * g.gw;
    const int py = g.y0 + gy * g.cell, px = g.x0 + gx * g.cell;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < g.B; ++b) {
        for (int t = g.t0 - l; t < g.T - l; ++t) {
            const double v = (double)sta_cell(sta_plane(x, g, b, t), g.W, py, px, g.cell, g.inv, g.s0);
            s1 += v; s2 += v * v;
        }
    }
    V1[i] += s1; V2[i] += s2;
}

// ws: mv [L G] = V1 / K, then vv [L G] = var_v
__global__ __launch_bounds__(RF_NT) void sta_vstat_kernel(const double* __restrict__ V1, const double* __restrict__ V2, i64 LG, double K,
                                                          double* __restrict__ ws) {
    const i64 i = (i64)blockIdx.x * RF_NT + threadIdx.x;
    if (i >= LG) return;
    const double a = V1[i], m = a / K;
    ws[i] = m;
    ws[LG + i] = (V2[i] - a * m) / K;
}

__global__ __launch_bounds__(RF_NT) void sta_finalize_kernel(const double* __restrict__ state, const double* __restrict__ ws, int N, int L,
                                                             int gh, int gw, double K, double rel, float* __restrict__ cov,
                                                             float* __restrict__ z, double* __restrict__ summary) {
    const int lane = threadIdx.x & (RF_WAVE - 1);
    const i64 j = (i64)blockIdx.x * RF_TILE + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / RF_WAVE));
    if (j >= N) return;                                       // a whole wave: the kernel has no barrier
    const int G = gh * gw;
    const i64 LG = (i64)L * G;
    const double* C = state + j * LG;
    const double U1 = state[(i64)N * LG + j], U2 = state[(i64)N * LG + N + j];
    const double* mv = ws;
    const double* vv = ws + LG;
    const double var_u = (U2 - U1 * (U1 / K)) / K, sqrtK = sqrt(K);
    auto cov_at = [&](i64 i) { return (C[i] - U1 * mv[i]) / K; };
    auto z_at = [&](i64 i, double c) {
        const double v = vv[i];
        return (var_u > 0.0 && v > 0.0) ? c * sqrtK / sqrt(var_u * v) : 0.0;
    };
    double etot = 0.0, ebest = 0.0;
    int lbest = 0;
    for (int l = 0; l < L; ++l) {
        double e = 0.0;
        for (int c = lane; c < G; c += RF_WAVE) {
            const i64 i = (i64)l * G + c;
            const double v = cov_at(i);
            e += v * v;
            cov[j * LG + i] = (float)v;
            if (z) z[j * LG + i] = (float)z_at(i, v);
        }
        e = wave_sum(e);                                      // the same bits in every lane: the branch below is uniform
        etot += e;
        if (e > ebest) { ebest = e; lbest = l; }
    }
    double* out = summary + j * DWN_STA_SUMMARY;
    const double nan = qnan_d();
    if (!(etot > 0.0)) {
        if (lane == 0) { out[0] = 0.0; out[1] = 0.0; out[2] = out[3] = out[4] = out[5] = nan; out[6] = 0.0; out[7] = 0.0; }
        return;
    }
    const i64 base = (i64)lbest * G;
    double amax = -1.0;
    int imax = G;
    for (int c = lane; c < G; c += RF_WAVE) {
        const double a = fabs(cov_at(base + c));
        if (a > amax) { amax = a; imax = c; }
    }
#pragma unroll
    for (int m = RF_WAVE / 2; m > 0; m >>= 1) {
        const double oa = __shfl_xor(amax, m, RF_WAVE);
        const int oi = __shfl_xor(imax, m, RF_WAVE);
        if (oa > amax || (oa == amax && oi < imax)) { amax = oa; imax = oi; }
    }
    const double thr = rel * amax;
    double sw = 0.0, swy = 0.0, swx = 0.0, cnt = 0.0;
    for (int c = lane; c < G; c += RF_WAVE) {
        const double v = cov_at(base + c);
        if (fabs(v) >= thr) {
            const int gy = c / gw, gx = c - gy * gw;
            const double w = v * v;
            sw += w; swy += w * (double)gy; swx += w * (double)gx; cnt += 1.0;
        }
    }
    sw = wave_sum(sw); swy = wave_sum(swy); swx = wave_sum(swx); cnt = wave_sum(cnt);
    const double cy = swy / sw, cx = swx / sw;
    double qy = 0.0, qx = 0.0;
    for (int c = lane; c < G; c += RF_WAVE) {
        const double v = cov_at(base + c);
        if (fabs(v) >= thr) {
            const int gy = c / gw, gx = c - gy * gw;
            const double w = v * v, dy = (double)gy - cy, dx = (double)gx - cx;
            qy += w * (dy * dy); qx += w * (dx * dx);
        }
    }
    qy = wave_sum(qy); qx = wave_sum(qx);
    if (lane == 0) {
        out[0] = (double)lbest;
        out[1] = imax < G ? z_at(base + imax, cov_at(base + imax)) : 0.0;
        out[2] = cy; out[3] = cx;
        out[4] = sqrt(qy / sw); out[5] = sqrt(qx / sw);
        out[6] = ebest / etot;
        out[7] = cnt;
    }
}

inline StaGeom sta_geom(const dwn_sta_args& a) {
    StaGeom g;
    g.B = a.B; g.Cin = a.Cin; g.T = a.T; g.H = a.H; g.W = a.W; g.N = a.N; g.channel = a.channel;
    g.y0 = a.y0; g.x0 = a.x0; g.cell = a.cell; g.gh = a.wh / a.cell; g.gw = a.ww / a.cell;
    g.L = a.lags; g.t0 = a.skip > a.lags - 1 ? a.skip : a.lags - 1; g.Tv = a.T - g.t0;
    g.s0 = a.s0; g.inv = 1.0f / (float)(a.cell * a.cell);
    return g;
}

inline size_t sta_cells(const dwn_sta_args& a) { return (size_t)(a.wh / a.cell) * (size_t)(a.ww / a.cell); }

}  // namespace

size_t k_sta_state_bytes(const dwn_sta_args& a) {
    const size_t LG = (size_t)a.lags * sta_cells(a);
    return ((size_t)a.N * LG + 2 * (size_t)a.N + 2 * LG) * sizeof(double);
}

size_t k_sta_ws_bytes(const dwn_sta_args& a) { return 2 * (size_t)a.lags * sta_cells(a) * sizeof(double); }

int k_sta_accumulate(const dwn_sta_args& a, hipStream_t s) {
    const StaGeom g = sta_geom(a);
    const i64 G = (i64)g.gh * g.gw, LG = (i64)g.L * G;
    double* Cuv = a.state;
    double* U1 = Cuv + (i64)a.N * LG;
    double* U2 = U1 + a.N;
    double* V1 = U2 + a.N;
    double* V2 = V1 + LG;
    const dim3 grid((unsigned)((a.N + RF_TM - 1) / RF_TM), (unsigned)((G + RF_TG - 1) / RF_TG), (unsigned)g.L);
    hipLaunchKernelGGL(sta_cross_kernel, grid, dim3(RF_NT), 0, s, a.x, a.r, a.r0, Cuv, g);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sta_umom_kernel, dim3((unsigned)((a.N + RF_TILE - 1) / RF_TILE)), dim3(RF_NT), 0, s, a.r, a.r0, U1, U2, g);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sta_vmom_kernel, dim3((unsigned)((LG + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, s, a.x, V1, V2, g);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_sta_finalize(const dwn_sta_args& a, hipStream_t s) {
    const int gh = a.wh / a.cell, gw = a.ww / a.cell;
    const i64 LG = (i64)a.lags * gh * gw;
    const double* V1 = a.state + (i64)a.N * LG + 2 * (i64)a.N;
    double* ws = (double*)a.ws;
    hipLaunchKernelGGL(sta_vstat_kernel, dim3((unsigned)((LG + RF_NT - 1) / RF_NT)), dim3(RF_NT), 0, s, V1, V1 + LG, LG,
                       (double)a.samples, ws);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(sta_finalize_kernel, dim3((unsigned)((a.N + RF_TILE - 1) / RF_TILE)), dim3(RF_NT), 0, s, a.state, ws, a.N, a.lags,
                       gh, gw, (double)a.samples, a.rel_threshold, a.cov, a.z, a.summary);
    DWN_CHECK_LAUNCH();
    return 0;
}

// Correlation objective (include/dwn.h dwn_corr_args): per-neuron Pearson correlation of one mouse over the
// (sample, frame) values of the rows whose mouse weight is not zero, the loss share * red_j (1 - r_j) and its gradient.
//
//   moments   one workgroup per tile of DWN_CORR_TILE neurons.  For a fixed row b the tile is ONE contiguous run of tile * T floats,
//             so a row is read by consecutive lanes (16-byte accesses when T % 4 == 0 and the pointers allow).  The run is cut into
//             units of VEC floats; `lpr` lanes (64, 128 or 256) cover a row and the 256 / lpr lane groups take the counted rows
//             round robin.  Means in a first sweep, centred sums in a second sweep of the same workgroup, float64 throughout.  Each
//             thread's partial goes to LDS and ONE thread per neuron adds them in the order (lane group, unit): no atomics, the
//             same bits on every launch and in both builds.  Rows of weight 0 are not read.
//   finalize  r and the two gradient coefficients per neuron; sum_j (1 - r_j) as one partial per workgroup (fixed tree) and a
//             one-workgroup launch that folds the partials in order and adds share * rho * sum to the caller's accumulator.
//   backward  one stream over pred / target -> dpred, the per-element expression in float64, rounded once.
// Nothing here depends on the occupancy the runtime reports: every grid is a function of the shapes alone.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"

namespace {

constexpr int CR_NT = 256;
constexpr int CR_TILE = DWN_CORR_TILE;
constexpr int CR_ROWS = 4;            // rows in flight per lane group

template <int VEC> struct CorrVec;
template <> struct CorrVec<1> {
    float v[1];
    __device__ __forceinline__ void load(const float* p) { v[0] = *p; }
};
template <> struct CorrVec<4> {
    float v[4];
    __device__ __forceinline__ void load(const float* p) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    }
};

// One sweep over the counted rows of this workgroup's tile.  CENTRED = false: acc = (sum p, sum t).  CENTRED = true:
// acc = (sum dp^2, sum dt^2, sum dp dt) with dp = p - mean_s[0][j], dt = t - mean_s[1][j].  The per-neuron totals end in
// tot[] of thread j < tn; returns the number of counted rows (the same in every thread).
template <int VEC, bool CENTRED>
__device__ __forceinline__ int corr_sweep(const float* __restrict__ p0, const float* __restrict__ t0, const float* __restrict__ w,
                                          i64 w_stride, int B, i64 row_stride, int T, int tn, int lpr,
                                          double (*part)[CR_NT], const double (*mean_s)[CR_TILE], double* tot) {
    constexpr int NA = CENTRED ? 3 : 2;
    const int tid = threadIdx.x;
    const int rgs = CR_NT / lpr;                  // lane groups: 1, 2 or 4
    const int rg = tid / lpr, lane = tid - rg * lpr;
    const int upn = T / VEC;                      // units per neuron (VEC == 4 only with T % 4 == 0)
    const int units = tn * upn;
    const int rounds = (units + lpr - 1) / lpr;
    int nrows = 0;
#pragma unroll
    for (int q = 0; q < NA; ++q) tot[q] = 0.0;
    for (int k = 0; k < rounds; ++k) {
        const int u = k * lpr + lane;
        const bool on = u < units;
        const i64 off = (i64)u * VEC;
        double mp = 0.0, mt = 0.0;
        if (CENTRED && on) { const int j = u / upn; mp = mean_s[0][j]; mt = mean_s[1][j]; }
        double acc[NA];
#pragma unroll
        for (int q = 0; q < NA; ++q) acc[q] = 0.0;
        int b = 0, ord = 0;
        // the next counted row of this lane group, or -1 (wave-uniform: lpr is a multiple of the wave)
        auto next = [&]() -> int {
            while (b < B) {
                const int bb = b++;
                if (w[(i64)bb * w_stride] == 0.f) continue;
                const bool mine = (ord & (rgs - 1)) == rg;
                ++ord;
                if (mine) return bb;
            }
            return -1;
        };
        for (;;) {
            int r[CR_ROWS];
#pragma unroll
            for (int q = 0; q < CR_ROWS; ++q) r[q] = next();
            if (r[0] < 0) break;
            CorrVec<VEC> xv[CR_ROWS], yv[CR_ROWS];
#pragma unroll
            for (int q = 0; q < CR_ROWS; ++q)
                if (on && r[q] >= 0) { xv[q].load(p0 + (i64)r[q] * row_stride + off); yv[q].load(t0 + (i64)r[q] * row_stride + off); }
#pragma unroll
            for (int q = 0; q < CR_ROWS; ++q)
                if (on && r[q] >= 0) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        if (CENTRED) {
                            const double dp = (double)xv[q].v[e] - mp, dt = (double)yv[q].v[e] - mt;
                            acc[0] += dp * dp; acc[1] += dt * dt; acc[NA - 1] += dp * dt;
                        } else {
                            acc[0] += (double)xv[q].v[e]; acc[1] += (double)yv[q].v[e];
                        }
                    }
                }
            if (r[CR_ROWS - 1] < 0) break;
        }
        nrows = ord;
#pragma unroll
        for (int q = 0; q < NA; ++q) part[q][tid] = acc[q];
        __syncthreads();
        if (tid < tn) {                           // the units of neuron tid that fall into this round, lane group by lane group
            const int lo = max(tid * upn, k * lpr) - k * lpr, hi = min((tid + 1) * upn, (k + 1) * lpr) - k * lpr;
            for (int g = 0; g < rgs; ++g)
                for (int l = lo; l < hi; ++l) {
#pragma unroll
                    for (int q = 0; q < NA; ++q) tot[q] += part[q][g * lpr + l];
                }
        }
        __syncthreads();
    }
    return nrows;
}

template <int VEC>
__global__ __launch_bounds__(CR_NT) void corr_moments_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                             const float* __restrict__ w, i64 w_stride, int B, int N, int T,
                                                             int lpr, double* __restrict__ stat, double* __restrict__ count) {
    __shared__ double part[3][CR_NT];
    __shared__ double mean_s[2][CR_TILE];
    const int j0 = blockIdx.x * CR_TILE;
    const int tn = min(CR_TILE, N - j0);
    const i64 row_stride = (i64)N * T;
    const float* p0 = pred + (i64)j0 * T;
    const float* t0 = target + (i64)j0 * T;
    const int tid = threadIdx.x;
    double s[2], c[3];
    const int nrows = corr_sweep<VEC, false>(p0, t0, w, w_stride, B, row_stride, T, tn, lpr, part, mean_s, s);
    const double n = (double)nrows * (double)T;
    if (tid < tn) {
        mean_s[0][tid] = nrows > 0 ? s[0] / n : 0.0;
        mean_s[1][tid] = nrows > 0 ? s[1] / n : 0.0;
    }
    __syncthreads();
    corr_sweep<VEC, true>(p0, t0, w, w_stride, B, row_stride, T, tn, lpr, part, mean_s, c);
    if (tid < tn) {
        const i64 j = j0 + tid;
        stat[j] = mean_s[0][tid];
        stat[(i64)N + j] = mean_s[1][tid];
        stat[2 * (i64)N + j] = c[0];
        stat[3 * (i64)N + j] = c[1];
        stat[4 * (i64)N + j] = c[2];
    }
    if (blockIdx.x == 0 && tid == 0) *count = n;
}

__global__ __launch_bounds__(CR_NT) void corr_finalize_kernel(double* __restrict__ stat, const double* __restrict__ count, int N,
                                                              double eps, double* __restrict__ partial) {
    __shared__ double red[CR_NT];
    const i64 j = (i64)blockIdx.x * CR_NT + threadIdx.x;
    const double n = *count;
    double term = 0.0;
    if (j < N) {
        double r = 0.0, c1 = 0.0, c2 = 0.0;
        if (n > 0.0) {
            const double sd_p = sqrt(stat[2 * (i64)N + j] / n), sd_t = sqrt(stat[3 * (i64)N + j] / n);
            const double a = sd_p + eps, c = sd_t + eps;
            r = (stat[4 * (i64)N + j] / n) / (a * c);
            c1 = 1.0 / (n * a * c);
            c2 = sd_p > 0.0 ? r / (n * sd_p * a) : 0.0;      // the kink of sqrt at a constant prediction: defined as 0
            term = 1.0 - r;
        }
        stat[5 * (i64)N + j] = r;
        stat[6 * (i64)N + j] = c1;
        stat[7 * (i64)N + j] = c2;
    }
    const double tot = wg_tree_sum(term, red);         // dwn_reduce.h: the fixed tree
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// one workgroup: loss_acc += share * rho * (partial[0] + partial[1] + ...), thread-strided then the fixed tree
__global__ __launch_bounds__(CR_NT) void corr_fold_kernel(const double* __restrict__ partial, int nparts, const float* __restrict__ share,
                                                          double rho, double* __restrict__ loss_acc) {
    __shared__ double red[CR_NT];
    double a = 0.0;
    for (int i = threadIdx.x; i < nparts; i += CR_NT) a += partial[i];
    const double tot = wg_tree_sum(a, red);
    if (threadIdx.x == 0) *loss_acc += (double)*share * (rho * tot);
}

template <int VEC>
__global__ __launch_bounds__(CR_NT) void corr_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                         const float* __restrict__ w, i64 w_stride, const double* __restrict__ stat,
                                                         const float* __restrict__ share, const float* __restrict__ gscale,
                                                         double rho, int N, int T, int per_sample, int chunks, i64 items,
                                                         float* __restrict__ dpred) {
    const double gs = -(double)(gscale ? *gscale : 1.0f) * (double)*share * rho;
    for (i64 item = blockIdx.x; item < items; item += gridDim.x) {
        const i64 b = item / chunks;
        const int ch = (int)(item - b * chunks);
        const int i = (ch * CR_NT + (int)threadIdx.x) * VEC;
        if (i >= per_sample) continue;
        const i64 at = b * (i64)per_sample + i;
        const bool counted = w[b * w_stride] != 0.f;         // uniform over the workgroup
        float o[VEC];
        if (counted) {
            const i64 j = (unsigned)i / (unsigned)T;        // VEC == 4 only with T % 4 == 0: the four elements share the neuron
            const double mp = stat[j], mt = stat[(i64)N + j], c1 = stat[6 * (i64)N + j], c2 = stat[7 * (i64)N + j];
            CorrVec<VEC> xv, yv;
            xv.load(pred + at); yv.load(target + at);
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = (float)(gs * (c1 * ((double)yv.v[e] - mt) - c2 * ((double)xv.v[e] - mp)));
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e) o[e] = 0.f;
        }
        if constexpr (VEC == 4) *reinterpret_cast<float4*>(dpred + at) = make_float4(o[0], o[1], o[2], o[3]);
        else dpred[at] = o[0];
    }
}

}  // namespace

size_t k_corr_ws_bytes(int N) { return (size_t)((N + CR_NT - 1) / CR_NT) * sizeof(double); }

int k_corr_moments(const dwn_corr_args& a, hipStream_t s) {
    const bool vec = (a.T % 4) == 0 && aligned16(a.pred) && aligned16(a.target);
    const i64 units = (i64)CR_TILE * a.T / (vec ? 4 : 1);
    const int lpr = units <= 64 ? 64 : units <= 128 ? 128 : 256;
    const dim3 grid((unsigned)((a.N + CR_TILE - 1) / CR_TILE));
    if (vec) hipLaunchKernelGGL(corr_moments_kernel<4>, grid, dim3(CR_NT), 0, s, a.pred, a.target, a.w, (i64)a.w_stride, a.B, a.N, a.T, lpr, a.stat, a.count);
    else hipLaunchKernelGGL(corr_moments_kernel<1>, grid, dim3(CR_NT), 0, s, a.pred, a.target, a.w, (i64)a.w_stride, a.B, a.N, a.T, lpr, a.stat, a.count);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_corr_finalize(const dwn_corr_args& a, hipStream_t s) {
    const int nparts = (a.N + CR_NT - 1) / CR_NT;
    double* partial = (double*)a.ws;
    hipLaunchKernelGGL(corr_finalize_kernel, dim3((unsigned)nparts), dim3(CR_NT), 0, s, a.stat, a.count, a.N, a.eps, partial);
    DWN_CHECK_LAUNCH();
    const double rho = a.reduction == DWN_CORR_SUM ? 1.0 : 1.0 / (double)a.N;
    hipLaunchKernelGGL(corr_fold_kernel, dim3(1), dim3(CR_NT), 0, s, partial, nparts, a.share, rho, a.loss_acc);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_corr_backward(const dwn_corr_args& a, hipStream_t s) {
    const int per_sample = a.N * a.T;
    const bool vec = (a.T % 4) == 0 && aligned16(a.pred) && aligned16(a.target) && aligned16(a.dpred);
    const int chunks = (per_sample + CR_NT * (vec ? 4 : 1) - 1) / (CR_NT * (vec ? 4 : 1));
    const i64 items = (i64)a.B * chunks;
    const dim3 grid((unsigned)(items < 4096 ? items : 4096));
    const double rho = a.reduction == DWN_CORR_SUM ? 1.0 : 1.0 / (double)a.N;
    if (vec) hipLaunchKernelGGL(corr_bwd_kernel<4>, grid, dim3(CR_NT), 0, s, a.pred, a.target, a.w, (i64)a.w_stride, a.stat, a.share, a.gscale, rho, a.N, a.T, per_sample, chunks, items, a.dpred);
    else hipLaunchKernelGGL(corr_bwd_kernel<1>, grid, dim3(CR_NT), 0, s, a.pred, a.target, a.w, (i64)a.w_stride, a.stat, a.share, a.gscale, rho, a.N, a.T, per_sample, chunks, items, a.dpred);
    DWN_CHECK_LAUNCH();
    return 0;
}

// Population structure (include/dwn.h dwn_pair_args): the N x N centred co-moments of one mouse over whole trials
// (total, signal and noise sample sets), the correlation matrices they give and the comparison of two such matrices.
//
//   stage     one workgroup per ST_TN neurons for the whole launch, so the running mean has one owner.  A wave owns ST_Q neurons;
//             its lanes run along the frames (consecutive lanes read consecutive fp32 of one row, 4-byte loads only).  Per chunk:
//             sweep 1 the chunk mean (lane-strided float64 sums closed by an xor butterfly: every lane ends with the same bits),
//             sweep 2 the centred values, transposed through LDS so that Z is written k-major with the neurons contiguous; then
//             the merge column sqrt(na nb / (na + nb)) (mb - ma), the zero columns up to the k-step, and the mean's advance.
//             Z Z^T is then exactly the pairwise (Chan) merge of the chunks: nothing is ever formed from a raw sum.
//   syrk      C += Z Z^T on v_mfma_f64_16x16x4_f64.  One workgroup per 64 x 64 tile with ti >= tj, four waves of 32 x 32 (2 x 2
//             MFMA tiles each); the operands pass through LDS in blocks of SY_KB columns (double-buffered, rows padded so that the
//             16 lanes of a k-slice read consecutive doubles and the four slices of a half-wave fall on different banks).  An
//             accumulator starts from C and walks every column in ascending order; K is never split, so the bits do not depend
//             on how the chunks were cut into launches.  The owner writes the mirror; on a diagonal tile the sub-block above the
//             diagonal is neither computed nor written and a diagonal sub-block writes its lower triangle: one owner per element.
//             C/D lane map of THIS instruction: col = lane & 15, row = (lane >> 4) + 4 * reg (not the f32 forms' 4 * (lane >> 4)
//             + reg); A: lane holds A[row = lane & 15][k = lane >> 4], B: B[k = lane >> 4][col = lane & 15].
//   finalize  element-wise; compare: one wave per selected row, two sweeps, then a one-workgroup merge in row order.
// No atomics, no scratch, no grid that depends on anything but the sizes: the same inputs give the same bits on every launch and in
// both builds (the file does not read DWN_DETERMINISTIC).
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"

namespace {

constexpr int PW_NT = 256;
constexpr int PW_WAVE = 64;
constexpr int PW_KSTEP = DWN_PAIR_KSTEP;
constexpr int ST_TN = 32;                  // neurons per stage workgroup
constexpr int ST_Q = ST_TN / (PW_NT / PW_WAVE);   // neurons per wave
constexpr int ST_TF = PW_WAVE;             // frames per LDS tile
constexpr int SY_T = DWN_PAIR_TILE;        // syrk tile edge
constexpr int SY_KB = 16;                  // columns per LDS block
constexpr int SY_LD = SY_T + 16;           // LDS row stride in doubles: 160 dwords, so consecutive k-slices start 32 banks apart
constexpr int CMP_ROWS = PW_NT / PW_WAVE;  // compare: rows per workgroup
static_assert(SY_T % ST_TN == 0 && SY_KB % PW_KSTEP == 0 && PW_KSTEP == 4, "tile geometry");

typedef double d4 __attribute__((ext_vector_type(4)));

// the average over the R repeats of frame f of one neuron's rows (repeats in table order, float64, one division)
__device__ __forceinline__ double repeat_mean(const dwn_pair_seg* sg, int R, i64 i, int f) {
    double s = 0.0;
    for (int r = 0; r < R; ++r) s += (double)sg[r].x[i * sg[r].ld + sg[r].first + f];
    return s / (double)R;
}

__global__ __launch_bounds__(PW_NT) void pair_stage_kernel(const dwn_pair_seg* __restrict__ segs, const dwn_trial_group* __restrict__ groups,
                                                           int n_segs, int n_groups, int max_repeats, int max_frames, int N, int kind,
                                                           double na, int cols, i64 ldz, double* __restrict__ mean,
                                                           double* __restrict__ Z) {
    __shared__ double tile[ST_TF][ST_TN + 1];
    const int tid = threadIdx.x, lane = tid & (PW_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / PW_WAVE);
    const i64 i0 = (i64)blockIdx.x * ST_TN, iw = i0 + wave * ST_Q;        // iw: the wave's first neuron
    const int nl = tid & (ST_TN - 1), fl = tid / ST_TN;                   // the write-out role: neuron, first frame of the tile
    double ma[ST_Q], mb[ST_Q];
#pragma unroll
    for (int q = 0; q < ST_Q; ++q) ma[q] = iw + q < N ? mean[iw + q] : 0.0;
    i64 col = 0;
    for (int g = 0; g < n_groups; ++g) {
        const dwn_trial_group G = groups[g];
        const int R = min(G.repeats, max_repeats), K = min(G.frames, max_frames), t0 = G.first_trial;
        if (R < 1 || K < 1 || t0 < 0 || t0 > n_segs - R) continue;        // not followed (dwn.h): the caller validates its tables
        if (kind != DWN_PAIR_TOTAL && R < 2) continue;
        const int nchunks = kind == DWN_PAIR_TOTAL ? R : 1;
        for (int c = 0; c < nchunks; ++c) {
            const dwn_pair_seg* sg = segs + t0 + c;                        // total: the chunk's trial; else the group's first
            const int vrows = kind == DWN_PAIR_NOISE ? R : 1;
            const i64 nvals = (i64)vrows * K, ccols = (nvals + 1 + PW_KSTEP - 1) / PW_KSTEP * PW_KSTEP;
            if (col + ccols > cols) { g = n_groups; break; }               // the same decision in every thread: Z is never passed
            // sweep 1: the chunk's mean
#pragma unroll
            for (int q = 0; q < ST_Q; ++q) {
                const i64 i = iw + q;
                double s = 0.0;
                if (i < N) {
                    for (int f = lane; f < K; f += PW_WAVE) {
                        if (kind == DWN_PAIR_TOTAL) s += (double)sg[0].x[i * sg[0].ld + sg[0].first + f];
                        else {
                            const double yb = repeat_mean(sg, R, i, f);
                            if (kind == DWN_PAIR_SIGNAL) s += yb;
                            else for (int r = 0; r < R; ++r) s += (double)sg[r].x[i * sg[r].ld + sg[r].first + f] - yb;
                        }
                    }
                }
                mb[q] = wave_sum(s) / (double)nvals;
            }
            // sweep 2: the centred values, ST_TF frames of ST_TN neurons at a time through LDS
            for (int f0 = 0; f0 < K; f0 += ST_TF) {
                const int f = f0 + lane;
                double yb[ST_Q];
#pragma unroll
                for (int q = 0; q < ST_Q; ++q)
                    yb[q] = (kind != DWN_PAIR_TOTAL && iw + q < N && f < K) ? repeat_mean(sg, R, iw + q, f) : 0.0;
                for (int vr = 0; vr < vrows; ++vr) {
#pragma unroll
                    for (int q = 0; q < ST_Q; ++q) {
                        const i64 i = iw + q;
                        double v = 0.0;
                        if (i < N && f < K) {
                            if (kind == DWN_PAIR_SIGNAL) v = yb[q] - mb[q];
                            else {
                                const double x = (double)sg[vr].x[i * sg[vr].ld + sg[vr].first + f];
                                v = kind == DWN_PAIR_TOTAL ? x - mb[q] : (x - yb[q]) - mb[q];
                            }
                        }
                        tile[lane][wave * ST_Q + q] = v;
                    }
                    __syncthreads();
                    double* zc = Z + (col + (i64)vr * K + f0) * ldz + i0 + nl;
                    for (int ff = fl; ff < ST_TF && f0 + ff < K; ff += PW_NT / ST_TN) zc[(i64)ff * ldz] = tile[ff][nl];
                    __syncthreads();
                }
            }
            // the merge column, the zero columns up to the k-step, and the mean's advance
            const double nb = (double)nvals, n = na + nb;
            const double coef = na > 0.0 ? sqrt(na * nb / n) : 0.0, w = nb / n;
#pragma unroll
            for (int q = 0; q < ST_Q; ++q) {
                const double d = mb[q] - ma[q];
                const double mcol = (na > 0.0 && iw + q < N) ? coef * d : 0.0;
                ma[q] = na > 0.0 ? ma[q] + d * w : mb[q];
                if (lane == 0) {
                    double* zc = Z + (col + nvals) * ldz + iw + q;
                    zc[0] = mcol;
                    for (i64 p = nvals + 1; p < ccols; ++p) zc[(p - nvals) * ldz] = 0.0;
                }
            }
            col += ccols;
            na = n;
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < ST_Q; ++q)
            if (iw + q < N) mean[iw + q] = ma[q];
    }
}

__global__ __launch_bounds__(PW_NT) void pair_syrk_kernel(const double* __restrict__ Z, int cols, i64 ldz, int N, double* __restrict__ C) {
    __shared__ __attribute__((aligned(16))) double As[2][SY_KB][SY_LD];
    __shared__ __attribute__((aligned(16))) double Bs[2][SY_KB][SY_LD];
    const int tid = threadIdx.x, lane = tid & (PW_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / PW_WAVE);
    // the tile (ti, tj), ti >= tj, of the linear index ti (ti + 1) / 2 + tj
    const i64 t = blockIdx.x;
    i64 ti = (i64)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    while (ti * (ti + 1) / 2 > t) --ti;
    const i64 tj = t - ti * (ti + 1) / 2;
    const i64 i0 = ti * SY_T, j0 = tj * SY_T;
    const int wr = wave >> 1, wc = wave & 1;
    const bool diag = ti == tj;
    const bool skip = diag && wr < wc;          // above the diagonal: the mirror of sub-block (wc, wr), which writes it
    const int l15 = lane & 15, l4 = lane >> 4;
    d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const i64 row = i0 + wr * 32 + a * 16 + l4 + 4 * r, cl = j0 + wc * 32 + b * 16 + l15;
                acc[a][b][r] = (!skip && row < N && cl < N) ? C[row * N + cl] : 0.0;
            }
    // the loader's role: two rows of the block, two doubles each
    const int kr = tid >> 5, c2 = (tid & 31) * 2;
    double2 ra[2], rb[2];
    auto gload = [&](int kb) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const i64 k = (i64)kb * SY_KB + kr + 8 * p;
            if (k < cols) {
                ra[p] = *reinterpret_cast<const double2*>(Z + k * ldz + i0 + c2);
                rb[p] = *reinterpret_cast<const double2*>(Z + k * ldz + j0 + c2);
            } else {
                ra[p] = make_double2(0.0, 0.0); rb[p] = make_double2(0.0, 0.0);
            }
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            *reinterpret_cast<double2*>(&As[buf][kr + 8 * p][c2]) = ra[p];
            *reinterpret_cast<double2*>(&Bs[buf][kr + 8 * p][c2]) = rb[p];
        }
    };
    const int nkb = (cols + SY_KB - 1) / SY_KB;
    gload(0);
    sstore(0);
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const int cur = kb & 1;
        if (kb + 1 < nkb) gload(kb + 1);
        const int steps = min(SY_KB, cols - kb * SY_KB) / PW_KSTEP;        // only real columns: no step is ever made up
        if (!skip) {
            for (int s = 0; s < steps; ++s) {
                const int kk = s * PW_KSTEP + l4;
                const double a0 = As[cur][kk][wr * 32 + l15], a1 = As[cur][kk][wr * 32 + 16 + l15];
                const double b0 = Bs[cur][kk][wc * 32 + l15], b1 = Bs[cur][kk][wc * 32 + 16 + l15];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        if (kb + 1 < nkb) sstore(cur ^ 1);
        __syncthreads();
    }
    if (skip) return;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const i64 row = i0 + wr * 32 + a * 16 + l4 + 4 * r, cl = j0 + wc * 32 + b * 16 + l15;
                if (row < N && cl < N && (!diag || row >= cl)) {
                    C[row * N + cl] = acc[a][b][r];
                    if (row != cl) C[cl * N + row] = acc[a][b][r];
                }
            }
}

__global__ __launch_bounds__(PW_NT) void pair_corr_kernel(const double* __restrict__ C, int N, double n, double eps, int out_f32,
                                                          void* __restrict__ out) {
    const i64 j = (i64)blockIdx.x * PW_NT + threadIdx.x, i = blockIdx.y;
    if (j >= N) return;
    double v = qnan_d();
    if (n > 0.0) v = (C[i * N + j] / n) / ((sqrt(C[i * N + i] / n) + eps) * (sqrt(C[j * N + j] / n) + eps));
    if (out_f32) ((float*)out)[i * N + j] = (float)v;
    else ((double*)out)[i * N + j] = v;
}

// one wave per selected row: count, mean_a, mean_b, Maa, Mbb, Cab, sum |a - b|, sum (a - b)^2 into stats, the score into per_neuron
__global__ __launch_bounds__(PW_NT) void pair_compare_rows_kernel(const double* __restrict__ A, const double* __restrict__ B, i64 lda,
                                                                  i64 ldb, int N, int M, const int* __restrict__ sel, double eps,
                                                                  double* __restrict__ per_neuron, double* __restrict__ stats) {
    const int lane = threadIdx.x & (PW_WAVE - 1);
    const int m = blockIdx.x * CMP_ROWS + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / PW_WAVE));
    if (m >= M) return;                                   // a whole wave: the kernel has no barrier
    const int i = sel ? sel[m] : m;
    const bool rowok = i >= 0 && i < N;
    double sa = 0.0, sb = 0.0, cnt = 0.0;
    bool bad = !rowok;
    for (int q = lane; q < M; q += PW_WAVE) {
        const int j = sel ? sel[q] : q;
        if (q == m) continue;
        if (j < 0 || j >= N) { bad = true; continue; }
        if (rowok) { sa += A[(i64)i * lda + j]; sb += B[(i64)i * ldb + j]; cnt += 1.0; }
    }
    cnt = wave_sum(cnt);
    const double ma = wave_sum(sa) / cnt, mb = wave_sum(sb) / cnt;
    double Maa = 0.0, Mbb = 0.0, Cab = 0.0, s1 = 0.0, s2 = 0.0;
    for (int q = lane; q < M; q += PW_WAVE) {
        const int j = sel ? sel[q] : q;
        if (q == m || j < 0 || j >= N || !rowok) continue;
        const double a = A[(i64)i * lda + j], b = B[(i64)i * ldb + j];
        const double da = a - ma, db = b - mb, e = a - b;
        Maa += da * da; Mbb += db * db; Cab += da * db; s1 += fabs(e); s2 += e * e;
    }
    Maa = wave_sum(Maa); Mbb = wave_sum(Mbb); Cab = wave_sum(Cab); s1 = wave_sum(s1); s2 = wave_sum(s2);
    const double anybad = wave_sum(bad ? 1.0 : 0.0);
    if (lane == 0) {
        double* st = stats + (i64)m * DWN_PAIR_ROW_STATS;
        const double nan = qnan_d();
        if (anybad > 0.0 || !(cnt > 0.0)) {
            per_neuron[m] = nan;
            st[0] = cnt; st[1] = st[2] = st[3] = st[4] = st[5] = st[6] = st[7] = nan;
        } else {
            per_neuron[m] = (Cab / cnt) / ((sqrt(Maa / cnt) + eps) * (sqrt(Mbb / cnt) + eps));
            st[0] = cnt; st[1] = ma; st[2] = mb; st[3] = Maa; st[4] = Mbb; st[5] = Cab; st[6] = s1; st[7] = s2;
        }
    }
}

struct PairMoments { double n, ma, mb, Maa, Mbb, Cab, s1, s2; };

// pairwise merge of b (b.n > 0) into a (a may be empty: copied, not divided by)
__device__ __forceinline__ void pair_merge(PairMoments& a, const PairMoments& b) {
    if (a.n == 0.0 && b.n > 0.0) { a = b; return; }
    const double n = a.n + b.n, f = b.n / n, cross = a.n * f;
    const double da = b.ma - a.ma, db = b.mb - a.mb;
    a.ma += da * f; a.mb += db * f;
    a.Maa = a.Maa + b.Maa + da * da * cross;
    a.Mbb = a.Mbb + b.Mbb + db * db * cross;
    a.Cab = a.Cab + b.Cab + da * db * cross;
    a.s1 += b.s1; a.s2 += b.s2;
    a.n = n;
}

// one workgroup: thread t merges its contiguous block of rows in row order, thread 0 merges the 256 partials in thread order
__global__ __launch_bounds__(PW_NT) void pair_compare_fold_kernel(const double* __restrict__ stats, int M, double eps,
                                                                  double* __restrict__ summary) {
    __shared__ PairMoments part[PW_NT];
    __shared__ int empty_row[PW_NT];                     // a row without a pair: the summary is NaN
    const int per = (M + PW_NT - 1) / PW_NT;
    PairMoments acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int poisoned = 0;
    for (int m = threadIdx.x * per; m < min(M, ((int)threadIdx.x + 1) * per); ++m) {
        const double* st = stats + (i64)m * DWN_PAIR_ROW_STATS;
        const PairMoments row = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        if (row.n == 0.0) { poisoned = 1; continue; }
        pair_merge(acc, row);
    }
    part[threadIdx.x] = acc;
    empty_row[threadIdx.x] = poisoned;
    __syncthreads();
    if (threadIdx.x != 0) return;
    PairMoments tot = part[0];
    for (int q = 1; q < PW_NT; ++q) {
        poisoned |= empty_row[q];
        if (part[q].n > 0.0) pair_merge(tot, part[q]);
    }
    const double nan = qnan_d();
    summary[0] = tot.n;
    if (poisoned || !(tot.n > 0.0) || tot.Cab != tot.Cab || tot.s1 != tot.s1) {      // a NaN entry on either side: all of it
        for (int q = 1; q < DWN_PAIR_SUMMARY; ++q) summary[q] = nan;
        return;
    }
    const double sda = sqrt(tot.Maa / tot.n), sdb = sqrt(tot.Mbb / tot.n);
    summary[1] = (tot.Cab / tot.n) / ((sda + eps) * (sdb + eps));
    summary[2] = tot.ma; summary[3] = tot.mb; summary[4] = sda; summary[5] = sdb;
    summary[6] = tot.s1 / tot.n; summary[7] = sqrt(tot.s2 / tot.n);
}

}  // namespace

long long k_pair_ldz(int N) { return ((long long)N + SY_T - 1) / SY_T * SY_T; }
size_t k_pair_compare_ws_bytes(int M) { return (size_t)M * DWN_PAIR_ROW_STATS * sizeof(double); }

int k_pair_stage(const dwn_pair_args& a, hipStream_t s) {
    const i64 ldz = k_pair_ldz(a.N);
    double* C = a.state;
    hipLaunchKernelGGL(pair_stage_kernel, dim3((unsigned)(ldz / ST_TN)), dim3(PW_NT), 0, s, a.segs, a.groups, a.n_segs, a.n_groups,
                       a.max_repeats, a.max_frames, a.N, a.kind, (double)a.n, a.cols, ldz, C + (i64)a.N * a.N, (double*)a.ws);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_pair_syrk(const dwn_pair_args& a, hipStream_t s) {
    const i64 ldz = k_pair_ldz(a.N), nt = ldz / SY_T;
    hipLaunchKernelGGL(pair_syrk_kernel, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(PW_NT), 0, s, (const double*)a.ws, a.cols, ldz, a.N,
                       a.state);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_pair_corr_finalize(const dwn_pair_args& a, hipStream_t s) {
    hipLaunchKernelGGL(pair_corr_kernel, dim3((unsigned)((a.N + PW_NT - 1) / PW_NT), (unsigned)a.N), dim3(PW_NT), 0, s, a.state, a.N,
                       (double)a.n, a.eps, a.out_f32, a.out);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_pair_compare(const dwn_pair_compare_args& a, hipStream_t s) {
    double* stats = (double*)a.ws;
    hipLaunchKernelGGL(pair_compare_rows_kernel, dim3((unsigned)((a.M + CMP_ROWS - 1) / CMP_ROWS)), dim3(PW_NT), 0, s, a.A, a.B, a.lda,
                       a.ldb, a.N, a.M, a.sel, a.eps, a.per_neuron, stats);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(pair_compare_fold_kernel, dim3(1), dim3(PW_NT), 0, s, stats, a.M, a.eps, a.summary);
    DWN_CHECK_LAUNCH();
    return 0;
}

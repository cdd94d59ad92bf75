// Trial-level evaluation (include/dwn.h dwn_trial_score_args): per-neuron centred moments over whole trials of
// different length, with a second level over the repeats of a video, and the scores they give.
//
//   moments   one WAVE per neuron for the whole launch (TS_TILE waves per workgroup, no LDS, no barrier), so the merge into the
//             running state is race-free.  The lanes run along the frames of a group and loop over its repeats: consecutive lanes
//             read consecutive fp32 of one row (4-byte loads only: a row start has no more alignment than that), and the average
//             over repeats, the within-frame variance and the leave-one-out terms of a frame stay inside one lane.  Per group:
//               sweep 1   sum p, sum y                                          -> the group means mp, my
//               sweep 2   per frame t (TS_U frames per lane at a time): pbar_t, ybar_t (first loop over the repeats), then the
//                         deviations from them (second loop: W.. = sum_r d^2, SSres), and the deviations of the frame means from
//                         the group means (B.. = sum_t).
//             Sweep 2 reads what sweep 1 read: a group of one neuron is 2 R K floats (20 KB at R = 10, K = 250), which the cache
//             still holds; an LDS copy would cap R K per wave.  (What limits the kernel is the chain of dependent load rounds of
//             one wave walking its groups, not bytes: profiles/trial_score_time.txt.)  Every group moment follows exactly from
//             the within-frame and the between-frame sums:
//               M2y = Wyy + R Byy,  M2p, C alike;   M2ybar = Byy;   SSwithin = Wyy / (R - 1);
//               loo_rt - ybar_t = -(y_rt - ybar_t) / (R - 1)  =>  M2loo = Wyy / (R - 1)^2 + R Byy,  C_y_loo = -Wyy / (R - 1) + R Byy
//             so nothing is ever formed from a raw sum of squares.  The lanes' partials are added by an xor butterfly (every lane
//             ends with the same bits), the groups are merged in table order with the pairwise (Chan) formulas.
//   finalize  the five scores per neuron; the summary sums as one partial per workgroup (fixed tree) and a one-workgroup fold.
// No atomics and no grid that depends on anything but N: the same inputs give the same bits on every launch and in both builds
// (the file does not read DWN_DETERMINISTIC).
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"

namespace {

constexpr int TS_NT = 256;
constexpr int TS_WAVE = 64;
constexpr int TS_TILE = DWN_TRIAL_TILE;
constexpr int TS_U = 4;                // frames per lane in flight
constexpr int TS_CHUNK = TS_U * TS_WAVE;
constexpr int TS_PARTS = 5;           // summary partials per workgroup: sum r1, sum r2, sum r4, sum of the masked feve, mask count
static_assert(TS_TILE * TS_WAVE == TS_NT, "one wave per neuron of the tile");

// pairwise merge of (mean_a, mean_b, M2a, M2b, Cab) with counts na (state s..) and nb > 0 (new); an empty state is replaced
__device__ __forceinline__ void chan5(double na, double nb, double& s_ma, double& s_mb, double& s_M2a, double& s_M2b, double& s_C,
                                      double ma, double mb, double M2a, double M2b, double Cab) {
    if (na == 0.0) { s_ma = ma; s_mb = mb; s_M2a = M2a; s_M2b = M2b; s_C = Cab; return; }
    const double n = na + nb, f = nb / n, cross = na * f;
    const double da = ma - s_ma, db = mb - s_mb;
    s_ma += da * f; s_mb += db * f;
    s_M2a = s_M2a + M2a + da * da * cross;
    s_M2b = s_M2b + M2b + db * db * cross;
    s_C = s_C + Cab + da * db * cross;
}

__global__ __launch_bounds__(TS_NT) void trial_moments_kernel(const dwn_trial_desc* __restrict__ trials,
                                                              const dwn_trial_group* __restrict__ groups, int n_trials, int n_groups,
                                                              int max_repeats, int max_frames, int N, double n_all, double n_rep,
                                                              double n_gf, double* __restrict__ state) {
    const int lane = threadIdx.x & (TS_WAVE - 1);
    // the wave index as a SCALAR: every row address below is then scalar arithmetic plus the lane's frame offset
    const i64 j = (i64)blockIdx.x * TS_TILE + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / TS_WAVE));
    if (j >= N) return;                                 // a whole wave: the kernel has no barrier
    // the 17 rows of this neuron (dwn.h), as scalars: sets A, B, C, D
    double* sj = state + j;
    const i64 n64 = N;
    double a_mp = sj[0], a_my = sj[n64], a_M2p = sj[2 * n64], a_M2y = sj[3 * n64], a_C = sj[4 * n64];
    double b_my = sj[5 * n64], b_M2y = sj[6 * n64], b_res = sj[7 * n64], b_ssw = sj[8 * n64];
    double c_mp = sj[9 * n64], c_my = sj[10 * n64], c_M2p = sj[11 * n64], c_M2y = sj[12 * n64], c_C = sj[13 * n64];
    double d_m = sj[14 * n64], d_M2 = sj[15 * n64], d_C = sj[16 * n64];
    for (int g = 0; g < n_groups; ++g) {
        const dwn_trial_group G = groups[g];
        const int R = min(G.repeats, max_repeats), K = min(G.frames, max_frames), t0 = G.first_trial;
        if (R < 1 || K < 1 || t0 < 0 || t0 > n_trials - R) continue;      // not followed (dwn.h): the caller validates its tables
        const dwn_trial_desc* tr = trials + t0;
        // sweep 1: the group means
        double sp = 0.0, sy = 0.0;
        for (int r = 0; r < R; ++r) {
            const float* p = tr[r].pred + j * tr[r].ld_pred + tr[r].first;
            const float* y = tr[r].target + j * tr[r].ld_target + tr[r].first;
            for (int c0 = 0; c0 < K; c0 += TS_CHUNK) {
                float xp[TS_U], xy[TS_U];
#pragma unroll
                for (int u = 0; u < TS_U; ++u) {
                    const int t = c0 + u * TS_WAVE + lane;
                    xp[u] = t < K ? p[t] : 0.f; xy[u] = t < K ? y[t] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < TS_U; ++u) { sp += (double)xp[u]; sy += (double)xy[u]; }
            }
        }
        const double ng = (double)R * (double)K;
        const double mp = wave_sum(sp) / ng, my = wave_sum(sy) / ng;
        if (R == 1) {
            const float* p = tr[0].pred + j * tr[0].ld_pred + tr[0].first;
            const float* y = tr[0].target + j * tr[0].ld_target + tr[0].first;
            double a0 = 0.0, a1 = 0.0, a2 = 0.0;
            for (int c0 = 0; c0 < K; c0 += TS_CHUNK) {
                float xp[TS_U], xy[TS_U];
#pragma unroll
                for (int u = 0; u < TS_U; ++u) {
                    const int t = c0 + u * TS_WAVE + lane;
                    xp[u] = t < K ? p[t] : 0.f; xy[u] = t < K ? y[t] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < TS_U; ++u) {
                    if (c0 + u * TS_WAVE + lane < K) {
                        const double dp = (double)xp[u] - mp, dy = (double)xy[u] - my;
                        a0 += dp * dp; a1 += dy * dy; a2 += dp * dy;
                    }
                }
            }
            a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
            chan5(n_all, ng, a_mp, a_my, a_M2p, a_M2y, a_C, mp, my, a0, a1, a2);
            n_all += ng;
            continue;
        }
        // sweep 2, TS_U frames per lane at a time: within-frame (W) and between-frame (B) sums
        const double rR = (double)R;
        double Wpp = 0.0, Wyy = 0.0, Wpy = 0.0, Bpp = 0.0, Byy = 0.0, Bpy = 0.0, res = 0.0;
        for (int c0 = 0; c0 < K; c0 += TS_CHUNK) {
            double fp[TS_U], fy[TS_U];
#pragma unroll
            for (int u = 0; u < TS_U; ++u) fp[u] = fy[u] = 0.0;
            for (int r = 0; r < R; ++r) {
                const float* p = tr[r].pred + j * tr[r].ld_pred + tr[r].first;
                const float* y = tr[r].target + j * tr[r].ld_target + tr[r].first;
#pragma unroll
                for (int u = 0; u < TS_U; ++u) {
                    const int t = c0 + u * TS_WAVE + lane;
                    if (t < K) { fp[u] += (double)p[t]; fy[u] += (double)y[t]; }
                }
            }
#pragma unroll
            for (int u = 0; u < TS_U; ++u) { fp[u] /= rR; fy[u] /= rR; }      // pbar_t, ybar_t
            for (int r = 0; r < R; ++r) {
                const float* p = tr[r].pred + j * tr[r].ld_pred + tr[r].first;
                const float* y = tr[r].target + j * tr[r].ld_target + tr[r].first;
#pragma unroll
                for (int u = 0; u < TS_U; ++u) {
                    const int t = c0 + u * TS_WAVE + lane;
                    if (t < K) {
                        const double xp = (double)p[t], xy = (double)y[t];
                        const double dp = xp - fp[u], dy = xy - fy[u], e = xy - xp;
                        Wpp += dp * dp; Wyy += dy * dy; Wpy += dp * dy; res += e * e;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < TS_U; ++u) {
                if (c0 + u * TS_WAVE + lane < K) {
                    const double bp = fp[u] - mp, by = fy[u] - my;
                    Bpp += bp * bp; Byy += by * by; Bpy += bp * by;
                }
            }
        }
        Wpp = wave_sum(Wpp); Wyy = wave_sum(Wyy); Wpy = wave_sum(Wpy); res = wave_sum(res);
        Bpp = wave_sum(Bpp); Byy = wave_sum(Byy); Bpy = wave_sum(Bpy);
        const double r1 = rR - 1.0, kf = (double)K;
        const double M2y = Wyy + rR * Byy;
        chan5(n_all, ng, a_mp, a_my, a_M2p, a_M2y, a_C, mp, my, Wpp + rR * Bpp, M2y, Wpy + rR * Bpy);       // set A
        chan5(n_gf, kf, c_mp, c_my, c_M2p, c_M2y, c_C, mp, my, Bpp, Byy, Bpy);                               // set C
        // sets B and D share mean_y / M2y (rows 5, 6); mean_loo (row 14) follows the same arithmetic as mean_y
        chan5(n_rep, ng, b_my, d_m, b_M2y, d_M2, d_C, my, my, M2y, Wyy / (r1 * r1) + rR * Byy, -Wyy / r1 + rR * Byy);
        if (n_rep == 0.0) { b_res = res; b_ssw = Wyy / r1; }
        else { b_res += res; b_ssw += Wyy / r1; }
        n_all += ng; n_rep += ng; n_gf += kf;
    }
    if (lane == 0) {
        sj[0] = a_mp; sj[n64] = a_my; sj[2 * n64] = a_M2p; sj[3 * n64] = a_M2y; sj[4 * n64] = a_C;
        sj[5 * n64] = b_my; sj[6 * n64] = b_M2y; sj[7 * n64] = b_res; sj[8 * n64] = b_ssw;
        sj[9 * n64] = c_mp; sj[10 * n64] = c_my; sj[11 * n64] = c_M2p; sj[12 * n64] = c_M2y; sj[13 * n64] = c_C;
        sj[14 * n64] = d_m; sj[15 * n64] = d_M2; sj[16 * n64] = d_C;
    }
}

__device__ __forceinline__ double pearson(double Ma, double Mb, double Cab, double n, double eps) {
    if (!(n > 0.0)) return qnan_d();
    return (Cab / n) / ((sqrt(Ma / n) + eps) * (sqrt(Mb / n) + eps));
}

__global__ __launch_bounds__(TS_NT) void trial_finalize_kernel(const double* __restrict__ state, int N, double n_all, double n_rep,
                                                               double n_gf, double eps, double thr, double* __restrict__ scores,
                                                               double* __restrict__ partial) {
    __shared__ double red[TS_NT];
    const i64 j = (i64)blockIdx.x * TS_NT + threadIdx.x;
    const double nan = qnan_d();
    double v[TS_PARTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (j < N) {
        auto S = [&](int q) { return state[(i64)q * N + j]; };
        const double r1 = pearson(S(2), S(3), S(4), n_all, eps);
        const double r2 = pearson(S(11), S(12), S(13), n_gf, eps);
        const double r4 = pearson(S(6), S(15), S(16), n_rep, eps);
        double fev = nan, feve = nan;
        if (n_rep > 1.0 && n_gf > 0.0) {
            const double TV = S(6) / (n_rep - 1.0), NV = S(8) / n_gf, MSE = S(7) / n_rep;
            if (TV > 0.0 && TV - NV > 0.0) { fev = (TV - NV) / TV; feve = 1.0 - (MSE - NV) / (TV - NV); }
        }
        scores[j] = r1; scores[(i64)N + j] = r2; scores[2 * (i64)N + j] = fev; scores[3 * (i64)N + j] = feve;
        scores[4 * (i64)N + j] = r4;
        v[0] = r1; v[1] = r2; v[2] = r4;
        if (fev >= thr) { v[3] = feve; v[4] = 1.0; }
    }
#pragma unroll
    for (int q = 0; q < TS_PARTS; ++q) {
        const double tot = wg_tree_sum(v[q], red);     // dwn_reduce.h: the fixed tree
        if (threadIdx.x == 0) partial[(i64)blockIdx.x * TS_PARTS + q] = tot;
    }
}

// one workgroup: the partials thread-strided in ascending order, then the fixed tree
__global__ __launch_bounds__(TS_NT) void trial_fold_kernel(const double* __restrict__ partial, int nparts, int N, double n_all,
                                                           double n_rep, double n_gf, double* __restrict__ summary) {
    __shared__ double red[TS_NT];
    double tot[TS_PARTS];
#pragma unroll
    for (int q = 0; q < TS_PARTS; ++q) {
        double a = 0.0;
        for (int i = threadIdx.x; i < nparts; i += TS_NT) a += partial[(i64)i * TS_PARTS + q];
        tot[q] = wg_tree_sum(a, red);
    }
    if (threadIdx.x == 0) {
        summary[0] = tot[0] / (double)N; summary[1] = tot[1] / (double)N; summary[2] = tot[2] / (double)N;
        summary[3] = tot[4] > 0.0 ? tot[3] / tot[4] : qnan_d();
        summary[4] = tot[4];
        summary[5] = n_all; summary[6] = n_rep; summary[7] = n_gf;
    }
}

}  // namespace

size_t k_trial_score_ws_bytes(int N) { return (size_t)((N + TS_NT - 1) / TS_NT) * TS_PARTS * sizeof(double); }

int k_trial_moments(const dwn_trial_score_args& a, hipStream_t s) {
    const dim3 grid((unsigned)((a.N + TS_TILE - 1) / TS_TILE));
    hipLaunchKernelGGL(trial_moments_kernel, grid, dim3(TS_NT), 0, s, a.trials, a.groups, a.n_trials, a.n_groups, a.max_repeats,
                       a.max_frames, a.N, (double)a.n_all, (double)a.n_repeat, (double)a.n_group_frames, a.state);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_trial_score_finalize(const dwn_trial_score_args& a, hipStream_t s) {
    const int nparts = (a.N + TS_NT - 1) / TS_NT;
    double* partial = (double*)a.ws;
    hipLaunchKernelGGL(trial_finalize_kernel, dim3((unsigned)nparts), dim3(TS_NT), 0, s, a.state, a.N, (double)a.n_all,
                       (double)a.n_repeat, (double)a.n_group_frames, a.eps, a.fev_threshold, a.scores, partial);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(trial_fold_kernel, dim3(1), dim3(TS_NT), 0, s, partial, nparts, a.N, (double)a.n_all, (double)a.n_repeat,
                       (double)a.n_group_frames, a.summary);
    DWN_CHECK_LAUNCH();
    return 0;
}

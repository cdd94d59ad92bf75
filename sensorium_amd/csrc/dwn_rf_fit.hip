// Parametric receptive-field fits (include/dwn.h dwn_gauss2d_args): an elliptical Gaussian per map by
// Levenberg-Marquardt, and the temporal profile of a lagged map on the fitted spatial shape.
//
//   fit        one wave per map, four maps per workgroup, one launch for all of them.  Lane i owns the cells i, i + 64, ...: it
//              stages them once (fp32, into the wave's slice of LDS, or reads them from global memory through L2: the host picks
//              by GF_STAGE below) and is the only lane that ever reads them back, so the kernel has no barrier and no cross-lane
//              memory traffic.  Every pass over the cells (start statistics, the normal equations, a trial's S) accumulates in
//              float64 per lane, cells ascending, and is closed by a fixed xor butterfly: all 64 lanes hold the same bits, so the
//              7 x 7 Cholesky solve, the clamps and every accept / reject decision are taken redundantly and uniformly in
//              registers.  The system is held in arrays that are only ever indexed by fully unrolled loops (a dynamically indexed
//              register array would become scratch).
//   profile    one wave per neuron: per lag two passes over the cells (the five sums of the 2 x 2 system, then SSE and SStot
//              about the solution), same ownership and butterfly.
// Contraction is off for the whole file: a multiply and the add that follows are two roundings here as they are in the float64
// checker (tests/rf_fit_reference.py), which differs only in the order of the sums and in the last bits of exp / log.
// No atomics, no scratch; a row depends on its map and the options alone, and the file does not read DWN_DETERMINISTIC: the same
// inputs give the same bits for any M, any row table, every launch and both builds.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_reduce.h"

namespace {

#pragma clang fp contract(off)

constexpr int GF_NT = 256;
constexpr int GF_WAVE = 64;
constexpr int GF_TILE = GF_NT / GF_WAVE;          // maps per workgroup
constexpr int GF_NP = DWN_GAUSS_PARAMS;
constexpr int GF_NA = GF_NP * (GF_NP + 1) / 2;    // packed upper triangle of JtJ
constexpr int GF_TRIES = 16;
#ifndef DWN_GF_STAGE
#define DWN_GF_STAGE 1                            // 1: stage the map in LDS; 0: read it through L2 on every pass (the variant that was
#endif                                            // measured against it, tools/rf_fit_time.py --variant-lib)
constexpr bool GF_STAGE = DWN_GF_STAGE != 0;
static_assert(GF_NP == 7 && DWN_GAUSS_TABLE == 16, "table layout");

struct GfArgs {
    int R, gh, gw, M, fit_b, max_iter;
    double rel, xtol, ftol;
};

// the cells of one map as their owner lane sees them
template <bool STAGE>
struct GfMap {
    const float* g;            // global row
    const float* l;            // the wave's LDS slice (STAGE)
    __device__ __forceinline__ double at(int c) const { return (double)(STAGE ? l[c] : g[c]); }
};

// one pass over the cells at parameters p: S = sum r^2 and, with NORMAL, the packed upper triangle of JtJ and Jt r
template <bool NORMAL, bool STAGE>
__device__ __forceinline__ double gf_pass(const GfMap<STAGE>& m, int G, int gw, const UDiv32& dgw, int lane, const double (&p)[GF_NP],
                                          bool fit_b, double (&A)[GF_NA], double (&g)[GF_NP]) {
    const double b = p[0], a = p[1], cy = p[2], cx = p[3], l11 = exp(p[4]), l21 = p[5], l22 = exp(p[6]);
    const double j0 = fit_b ? 1.0 : 0.0;
    double S = 0.0;
    if (NORMAL) {
#pragma unroll
        for (int i = 0; i < GF_NA; ++i) A[i] = 0.0;
#pragma unroll
        for (int i = 0; i < GF_NP; ++i) g[i] = 0.0;
    }
    for (int c0 = 0; c0 < G; c0 += GF_WAVE) {
        const int c = c0 + lane;
        if (c < G) {
            const int y = (int)dgw.div((unsigned)c), x = c - y * gw;
            const double dx = (double)x - cx, dy = (double)y - cy;
            const double u = l11 * dx, v = l21 * dx + l22 * dy;
            const double q = u * u + v * v;
            const double e = exp(-0.5 * q);
            const double ae = a * e;
            const double r = m.at(c) - (b + ae);
            S += r * r;
            if (NORMAL) {
                double J[GF_NP];
                J[0] = j0;
                J[1] = e;
                J[2] = ae * (v * l22);
                J[3] = ae * (u * l11 + v * l21);
                J[4] = -(ae * (u * u));
                J[5] = -(ae * (v * dx));
                J[6] = -(ae * (v * (l22 * dy)));
                int k = 0;
#pragma unroll
                for (int i = 0; i < GF_NP; ++i) {
#pragma unroll
                    for (int j = i; j < GF_NP; ++j) A[k++] += J[i] * J[j];
                    g[i] += J[i] * r;
                }
            }
        }
    }
    S = wave_sum(S);
    if (NORMAL) {
#pragma unroll
        for (int i = 0; i < GF_NA; ++i) A[i] = wave_sum(A[i]);
#pragma unroll
        for (int i = 0; i < GF_NP; ++i) g[i] = wave_sum(g[i]);
        if (!fit_b) A[0] = 1.0;            // the baseline is held: row and column 0 are zero but for this pivot
    }
    return S;
}

// Cholesky factor of A + lam diag(A) (packed upper triangle in, lower factor out); false when a pivot is not positive
__device__ __forceinline__ bool gf_chol(const double (&A)[GF_NA], double lam, double (&Lf)[GF_NP][GF_NP]) {
    double Mx[GF_NP][GF_NP];
    int k = 0;
#pragma unroll
    for (int i = 0; i < GF_NP; ++i) {
#pragma unroll
        for (int j = i; j < GF_NP; ++j) { Mx[j][i] = A[k]; ++k; }
    }
#pragma unroll
    for (int i = 0; i < GF_NP; ++i) Mx[i][i] = Mx[i][i] + lam * Mx[i][i];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < GF_NP; ++j) {
        double d = Mx[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) d -= Lf[j][q] * Lf[j][q];
        ok = ok && (d > 0.0) && is_finite(d);
        const double piv = sqrt(d);
        Lf[j][j] = piv;
#pragma unroll
        for (int i = j + 1; i < GF_NP; ++i) {
            double s = Mx[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) s -= Lf[i][q] * Lf[j][q];
            Lf[i][j] = s / piv;
        }
    }
    return ok;
}

// x = (L L^T)^-1 rhs
__device__ __forceinline__ void gf_solve(const double (&Lf)[GF_NP][GF_NP], const double (&rhs)[GF_NP], double (&x)[GF_NP]) {
    double z[GF_NP];
#pragma unroll
    for (int i = 0; i < GF_NP; ++i) {
        double s = rhs[i];
#pragma unroll
        for (int q = 0; q < i; ++q) s -= Lf[i][q] * z[q];
        z[i] = s / Lf[i][i];
    }
#pragma unroll
    for (int i = GF_NP - 1; i >= 0; --i) {
        double s = z[i];
#pragma unroll
        for (int q = i + 1; q < GF_NP; ++q) s -= Lf[q][i] * x[q];
        x[i] = s / Lf[i][i];
    }
}

__device__ __forceinline__ double gf_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <bool STAGE>
__global__ __launch_bounds__(GF_NT) void gauss2d_fit_kernel(const float* __restrict__ maps, const int* __restrict__ sel,
                                                            double* __restrict__ params, double* __restrict__ table,
                                                            double* __restrict__ start, GfArgs o) {
    extern __shared__ float gf_lds[];
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / GF_WAVE));
    const int i = blockIdx.x * GF_TILE + wave;
    if (i >= o.M) return;                                     // a whole wave: the kernel has no barrier
    const int G = o.gh * o.gw, gw = o.gw;
    const UDiv32 dgw((unsigned)gw);
    const bool fit_b = o.fit_b != 0;
    const double nan = qnan_d();
    double* prow = params + (i64)i * GF_NP;
    double* trow = table + (i64)i * DWN_GAUSS_TABLE;
    double* srow = start + (i64)i * 8;
    const int row = sel ? sel[i] : i;

    double p[GF_NP];
    // a row with no fit: baseline and sse as given, amplitude 0, NaN geometry
    auto no_fit = [&](double base, double sse) {
        if (lane == 0) {
            prow[0] = base; prow[1] = 0.0;
#pragma unroll
            for (int k = 2; k < GF_NP; ++k) prow[k] = nan;
            trow[0] = 2.0; trow[1] = 0.0; trow[2] = base; trow[3] = 0.0;
#pragma unroll
            for (int k = 4; k < 9; ++k) trow[k] = nan;
            trow[9] = sse; trow[10] = 0.0; trow[11] = nan; trow[12] = nan; trow[13] = nan; trow[14] = 0.0; trow[15] = (double)row;
#pragma unroll
            for (int k = 0; k < 8; ++k) srow[k] = nan;
        }
    };
    if (row < 0 || row >= o.R) { no_fit(nan, nan); return; }  // never read outside maps

    GfMap<STAGE> m;
    m.g = maps + (i64)row * G;
    m.l = gf_lds + wave * G;
    if (STAGE) {
        float* dst = gf_lds + wave * G;
        for (int c = lane; c < G; c += GF_WAVE) dst[c] = m.g[c];          // read back by this lane only
    }

    // ---- start: perimeter mean, peak, thresholded centroid and spread
    double nbad = 0.0, psum = 0.0, tsum = 0.0, mn = 0.0, mx = 0.0;
    bool first = true;
    for (int c = lane; c < G; c += GF_WAVE) {
        const double v = m.at(c);
        const int y = (int)dgw.div((unsigned)c), x = c - y * gw;
        if (!is_finite(v)) nbad += 1.0;
        if (y == 0 || y == o.gh - 1 || x == 0 || x == gw - 1) psum += v;
        tsum += v;
        if (first) { mn = v; mx = v; first = false; }
        else { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
    }
    // G >= 9 and lanes past G hold no cell: take lane 0's range for them (lane 0 always owns cell 0)
    {
        const double mn0 = __shfl(mn, 0, GF_WAVE), mx0 = __shfl(mx, 0, GF_WAVE);
        if (first) { mn = mn0; mx = mx0; }
    }
    nbad = wave_sum(nbad); psum = wave_sum(psum); tsum = wave_sum(tsum);
#pragma unroll
    for (int s = GF_WAVE / 2; s > 0; s >>= 1) {
        const double on = __shfl_xor(mn, s, GF_WAVE), ox = __shfl_xor(mx, s, GF_WAVE);
        mn = on < mn ? on : mn; mx = ox > mx ? ox : mx;
    }
    const double b0 = fit_b ? psum / (double)(2 * o.gh + 2 * gw - 4) : 0.0;
    const double mean = tsum / (double)G;
    double amax = -1.0, dpk = 0.0, sstot = 0.0, sd2 = 0.0;
    int imax = G;
    for (int c = lane; c < G; c += GF_WAVE) {
        const double v = m.at(c);
        const double d = v - b0, a = fabs(d), t = v - mean;
        sstot += t * t; sd2 += d * d;
        if (a > amax) { amax = a; imax = c; dpk = d; }
    }
    sstot = wave_sum(sstot); sd2 = wave_sum(sd2);
#pragma unroll
    for (int s = GF_WAVE / 2; s > 0; s >>= 1) {
        const double oa = __shfl_xor(amax, s, GF_WAVE), od = __shfl_xor(dpk, s, GF_WAVE);
        const int oi = __shfl_xor(imax, s, GF_WAVE);
        if (oa > amax || (oa == amax && oi < imax)) { amax = oa; imax = oi; dpk = od; }
    }
    const double a0 = dpk;
    if (nbad > 0.0 || mn == mx || a0 == 0.0) {
        no_fit(is_finite(b0) ? b0 : nan, is_finite(sd2) ? sd2 : nan);
        return;
    }
    const double thr = o.rel * fabs(a0);
    double sw = 0.0, swy = 0.0, swx = 0.0;
    for (int c = lane; c < G; c += GF_WAVE) {
        const double d = m.at(c) - b0;
        if (fabs(d) >= thr) {
            const int y = (int)dgw.div((unsigned)c), x = c - y * gw;
            const double w = d * d;
            sw += w; swy += w * (double)y; swx += w * (double)x;
        }
    }
    sw = wave_sum(sw); swy = wave_sum(swy); swx = wave_sum(swx);
    const double cy0 = swy / sw, cx0 = swx / sw;
    double qy = 0.0, qx = 0.0;
    for (int c = lane; c < G; c += GF_WAVE) {
        const double d = m.at(c) - b0;
        if (fabs(d) >= thr) {
            const int y = (int)dgw.div((unsigned)c), x = c - y * gw;
            const double w = d * d, ey = (double)y - cy0, ex = (double)x - cx0;
            qy += w * (ey * ey); qx += w * (ex * ex);
        }
    }
    qy = wave_sum(qy); qx = wave_sum(qx);
    double sy = sqrt(qy / sw), sx = sqrt(qx / sw);
    sy = sy > 0.5 ? sy : 0.5; sx = sx > 0.5 ? sx : 0.5;
    p[0] = b0; p[1] = a0; p[2] = cy0; p[3] = cx0; p[4] = -log(sx); p[5] = 0.0; p[6] = -log(sy);

    // ---- Levenberg-Marquardt
    const int gmax = o.gh > gw ? o.gh : gw;
    const double ulo = -log(2.0 * (double)gmax), uhi = -log(0.3);
    const double cyhi = (double)o.gh, cxhi = (double)gw;
    double A[GF_NA], g[GF_NP];
    double S = gf_pass<true, STAGE>(m, G, gw, dgw, lane, p, fit_b, A, g);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < GF_NP; ++k) srow[k] = p[k];
        srow[7] = S;
    }
    double lam = 1e-3;
    int status = 1, iters = 0;
    for (int it = 1; it <= o.max_iter; ++it) {
        iters = it;
        bool accepted = false, conv_x = false;
        double dec = 0.0;
        for (int t = 0; t < GF_TRIES; ++t) {
            double Lf[GF_NP][GF_NP], dp[GF_NP], pn[GF_NP];
            const bool ok = gf_chol(A, lam, Lf);
            if (!ok) { lam *= 10.0; continue; }
            gf_solve(Lf, g, dp);
#pragma unroll
            for (int k = 0; k < GF_NP; ++k) pn[k] = p[k] + dp[k];
            if (!fit_b) pn[0] = p[0];
            pn[2] = gf_clamp(pn[2], -1.0, cyhi); pn[3] = gf_clamp(pn[3], -1.0, cxhi);
            pn[4] = gf_clamp(pn[4], ulo, uhi);   pn[6] = gf_clamp(pn[6], ulo, uhi);
            const double sa = o.xtol * fabs(p[1]);
            bool small = true;
#pragma unroll
            for (int k = 0; k < GF_NP; ++k) small = small && (fabs(pn[k] - p[k]) < (k < 2 ? sa : o.xtol));
            if (small) { conv_x = true; break; }
            double An[GF_NA], gn[GF_NP];
            (void)An; (void)gn;
            const double Sn = gf_pass<false, STAGE>(m, G, gw, dgw, lane, pn, fit_b, An, gn);
            if (is_finite(Sn) && Sn < S) {
                dec = S - Sn;
#pragma unroll
                for (int k = 0; k < GF_NP; ++k) p[k] = pn[k];
                S = Sn;
                lam = lam / 10.0; lam = lam > 1e-12 ? lam : 1e-12;
                accepted = true;
                break;
            }
            lam *= 10.0;
        }
        if (conv_x) { status = 0; break; }
        if (!accepted) break;                                  // out of tries
        (void)gf_pass<true, STAGE>(m, G, gw, dgw, lane, p, fit_b, A, g);
        if (dec <= o.ftol * S) { status = 0; break; }
    }

    // ---- derived columns at the solution (A, g hold the normal equations at p)
    const double l11 = exp(p[4]), l21 = p[5], l22 = exp(p[6]);
    const double pxx = l11 * l11 + l21 * l21, pxy = l21 * l22, pyy = l22 * l22;
    const double det = (l11 * l22) * (l11 * l22);
    const double cxx = pyy / det, cyy = pxx / det, cxy = (0.0 - pxy) / det;
    const double hd = 0.5 * (cxx - cyy);
    const double lmaj = 0.5 * (cxx + cyy) + sqrt(hd * hd + cxy * cxy);
    const double lmin = (1.0 / det) / lmaj;
    double theta = 0.5 * atan2(2.0 * cxy, cxx - cyy);
    const double half_pi = 1.5707963267948966;
    if (theta <= -half_pi) theta += 2.0 * half_pi;
    double se[3] = {nan, nan, nan};
    {
        double Lf[GF_NP][GF_NP];
        if (gf_chol(A, 0.0, Lf)) {
            const double s2 = S / (double)(G - (fit_b ? GF_NP : GF_NP - 1));
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int col = q == 0 ? 2 : (q == 1 ? 3 : 1);          // cy, cx, amplitude
                double rhs[GF_NP], x[GF_NP];
#pragma unroll
                for (int k = 0; k < GF_NP; ++k) rhs[k] = k == col ? 1.0 : 0.0;
                gf_solve(Lf, rhs, x);
                double cii = 0.0;
#pragma unroll
                for (int k = 0; k < GF_NP; ++k) cii = k == col ? x[k] : cii;
                se[q] = sqrt(cii * s2);
            }
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < GF_NP; ++k) prow[k] = p[k];
        trow[0] = (double)status; trow[1] = (double)iters; trow[2] = p[0]; trow[3] = p[1]; trow[4] = p[2]; trow[5] = p[3];
        trow[6] = sqrt(lmaj); trow[7] = sqrt(lmin); trow[8] = theta; trow[9] = S;
        trow[10] = sstot > 0.0 ? 1.0 - S / sstot : 0.0;
        trow[11] = se[0]; trow[12] = se[1]; trow[13] = se[2]; trow[14] = lam; trow[15] = (double)row;
    }
}

__global__ __launch_bounds__(GF_NT) void gauss2d_profile_kernel(const double* __restrict__ params, const float* __restrict__ maps,
                                                                double* __restrict__ profile, double* __restrict__ sep, int N, int L,
                                                                int gh, int gw, int fit_b) {
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const int j = blockIdx.x * GF_TILE + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / GF_WAVE));
    if (j >= N) return;                                       // a whole wave: the kernel has no barrier
    const int G = gh * gw;
    const UDiv32 dgw((unsigned)gw);
    const double* p = params + (i64)j * GF_NP;
    const double nan = qnan_d();
    bool bad = false;
#pragma unroll
    for (int k = 0; k < GF_NP; ++k) bad = bad || !is_finite(p[k]);
    if (bad) {
        for (int l = lane; l < L; l += GF_WAVE) profile[(i64)j * L + l] = nan;
        if (lane == 0) sep[j] = nan;
        return;
    }
    const double cy = p[2], cx = p[3], l11 = exp(p[4]), l21 = p[5], l22 = exp(p[6]);
    auto shape = [&](int c) {
        const int y = (int)dgw.div((unsigned)c), x = c - y * gw;
        const double dx = (double)x - cx, dy = (double)y - cy;
        const double u = l11 * dx, v = l21 * dx + l22 * dy;
        const double q = u * u + v * v;
        return exp(-0.5 * q);
    };
    double se1 = 0.0, se2 = 0.0;
    for (int c = lane; c < G; c += GF_WAVE) { const double e = shape(c); se1 += e; se2 += e * e; }
    se1 = wave_sum(se1); se2 = wave_sum(se2);
    const double Gd = (double)G;
    const double det = Gd * se2 - se1 * se1;
    double sse_all = 0.0, sst_all = 0.0;
    for (int l = 0; l < L; ++l) {
        const float* mp = maps + ((i64)j * L + l) * G;
        double sm = 0.0, sme = 0.0;
        for (int c = lane; c < G; c += GF_WAVE) { const double v = (double)mp[c]; sm += v; sme += v * shape(c); }
        sm = wave_sum(sm); sme = wave_sum(sme);
        double al, bl, mu;
        if (fit_b) {
            al = det > 0.0 ? (Gd * sme - se1 * sm) / det : 0.0;
            bl = (sm - al * se1) / Gd;
            mu = sm / Gd;
        } else {
            al = se2 > 0.0 ? sme / se2 : 0.0;
            bl = 0.0; mu = 0.0;
        }
        double sse = 0.0, sst = 0.0;
        for (int c = lane; c < G; c += GF_WAVE) {
            const double v = (double)mp[c];
            const double r = v - (bl + al * shape(c)), t = v - mu;
            sse += r * r; sst += t * t;
        }
        sse = wave_sum(sse); sst = wave_sum(sst);
        sse_all += sse; sst_all += sst;
        if (lane == 0) profile[(i64)j * L + l] = al;
    }
    if (lane == 0) sep[j] = sst_all > 0.0 ? 1.0 - sse_all / sst_all : 0.0;
}

}  // namespace

size_t k_gauss2d_ws_bytes(const dwn_gauss2d_args& a) { return (size_t)a.M * 8 * sizeof(double); }

int k_gauss2d_fit(const dwn_gauss2d_args& a, hipStream_t s) {
    GfArgs o;
    o.R = a.R; o.gh = a.gh; o.gw = a.gw; o.M = a.M; o.fit_b = a.fit_baseline ? 1 : 0; o.max_iter = a.max_iter;
    o.rel = a.rel_threshold; o.xtol = a.xtol; o.ftol = a.ftol;
    const dim3 grid((unsigned)((a.M + GF_TILE - 1) / GF_TILE));
    const size_t lds = GF_STAGE ? (size_t)GF_TILE * a.gh * a.gw * sizeof(float) : 0;      // <= 64 KiB: G <= 4096
    hipLaunchKernelGGL(gauss2d_fit_kernel<GF_STAGE>, grid, dim3(GF_NT), lds, s, a.maps, a.sel, a.params, a.table, (double*)a.ws, o);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_gauss2d_profile(const dwn_gauss2d_profile_args& a, hipStream_t s) {
    hipLaunchKernelGGL(gauss2d_profile_kernel, dim3((unsigned)((a.N + GF_TILE - 1) / GF_TILE)), dim3(GF_NT), 0, s, a.params, a.maps,
                       a.profile, a.separability, a.N, a.L, a.gh, a.gw, a.fit_baseline ? 1 : 0);
    DWN_CHECK_LAUNCH();
    return 0;
}

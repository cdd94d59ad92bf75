// Retinotopic readout gain (include/dwn.h dwn_spatial_gain_args): every neuron reads the core map at its own learned
// position and turns what it finds there into a bounded gain on the readout's output,
//   samp[b,n,t,:] = bilinear sample of G[b,t,:,:,:] at pos[n]     (grid_sample: bilinear, border, align_corners)
//   a = bias[n] + weight[n,:] . samp,   gain = exp(m tanh(a)),   out[b,n,t] = y[b,n,t] gain
// with its five gradients.  y, out, dout, dy are [B][N][T] (T contiguous), G is [B][T][Hf][Wf][K] in fp32 or bf16, dG the same shape
// in fp32, pos [N][2] = (x, y), weight [N][K], bias [N].  It generalises dwn_modulator.hip: the feature row is per neuron.
//
// ONE DECISION PER NEURON.  sp_decide() turns pos[n] into the four cell indices, the four fp32 weights and three flags (non-finite,
// x live, y live).  The forward is a single pass and derives it inline; the backward's prep launch writes it into the workspace and
// every later pass (element pass, dG pass, finaliser) reads that table: no two passes can put a neuron on a cell boundary into
// different cells.  Every product of sp_decide is an explicit single rounding, so both uses give the same bits.
//
// ELEMENT PASS (forward, and backward with BWD): a workgroup of 128 threads owns 128 neurons x min(T, 32) frames of one sample
// (backward: of the SP_RB samples of its batch group).  The y / dout tile goes through LDS so that global traffic runs along T while
// a THREAD OWNS A NEURON: its weight row sits in registers, and for each frame it reads its four corner rows of G (16-byte loads
// when K is a multiple of 8; all threads of the workgroup read the same frame, a few KB that stay in the vector cache) into the
// four corner dots d00 .. d11 (K FMAs each, k ascending, from 0), then a = bias + w00 d00 + w01 d01 + w10 d10 + w11 d11 (4 FMAs).
// The corner dots also give the position slopes: da/dfx = (1 - fy)(d01 - d00) + fy (d11 - d10), da/dfy likewise.
// Backward: dy = dout gain, s = dout y gain m sech^2(a) (sech^2 = 4e / (1 + e)^2), and per thread float64 sums over the frames of
//   dbias += s,  dfx += s da/dfx,  dfy += s da/dfy,  dweight[k] += s samp[k]   (a second sweep over the corner rows, cache hot)
// stored as one partial per (batch group, frame chunk); s itself goes to the workspace as [B][N][T] fp32 when dG is asked for.
// dG PASS: a stable bucketing first (one workgroup per cell walks the per-neuron table in index order and lists the neurons one of
// whose corners is this cell, with that corner's weight: ballot + prefix counts keep the index order; non-finite neurons are left
// out).  Then one wave per (sample, cell, 32 frames) stages its bucket's s rows times the corner weight and their weight rows in LDS
// and adds s w_c weight[n,k] into a register tile of float64 FMAs, neurons ascending (the product of two fp32 numbers is exact in
// float64).  Every cell is written; a cell no neuron touches gets exact zeros.
// FINALISER: sums the partials in ascending order, scales dfx, dfy by (Wf - 1) / 2, (Hf - 1) / 2 in float64 and rounds to fp32
// once; a clamped coordinate (strictly outside [-1, 1]) and a one-cell axis get exactly 0, a non-finite neuron NaN.
// Nothing is atomic and every grid depends on the geometry alone: the same inputs give the same bits, in the product and the
// -DDWN_DETERMINISTIC builds.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_launch.h"
#include "dwn_gain.h"
#include "dwn_reduce.h"

namespace {

constexpr int SP_NT = 128;         // threads per workgroup of the element pass = neurons per tile
constexpr int SP_TT = 32;          // frames per tile: min(T, 32)
constexpr int SP_ST = SP_TT + 1;   // row stride of the LDS tiles (odd: a thread per row reads down a column without bank conflicts)
constexpr int SP_RB = 2;           // samples per batch group (the backward's partial sums go on over them in registers)
constexpr int SP_LB = 64;        // dG pass: neurons of a bucket staged at a time
constexpr int SP_TG = 32;          // dG pass: frames per wave
constexpr int SP_BAD = 1, SP_LIVE_X = 2, SP_LIVE_Y = 4;

struct SpEnt {                     // one neuron's decision (48 bytes)
    int c00, c01, c10, c11;        // cell indices y * Wf + x of the four corners
    float w00, w01, w10, w11;      // their bilinear weights
    float fx, fy;
    int flags, pad_;
};

struct SpGeom {
    int B, N, T, Hf, Wf, K, HW;
    int TT, nTc, nNt, G;           // frames per tile, frame chunks, neuron tiles, batch groups
    int vec;                       // K % 8 == 0 and G 16-byte aligned: corner rows are read 8 features per 16-byte load (2 for fp32)
    float m;
};

inline SpGeom sp_geom(const dwn_spatial_gain_args& a) {
    SpGeom g;
    g.B = a.B; g.N = a.N; g.T = a.T; g.Hf = a.Hf; g.Wf = a.Wf; g.K = a.K; g.HW = a.Hf * a.Wf; g.m = a.max_log_gain;
    g.TT = a.T < SP_TT ? a.T : SP_TT;
    g.nTc = (a.T + g.TT - 1) / g.TT;
    g.nNt = (a.N + SP_NT - 1) / SP_NT;
    g.G = (a.B + SP_RB - 1) / SP_RB;
    g.vec = (a.K % 8 == 0) && aligned16(a.g);
    return g;
}

// one axis: clamp, pixel coordinate, base cell, fraction (exact: v in [i0, i0 + 1]), neighbour
__device__ __forceinline__ void sp_axis(float v, int n, int& i0, int& i1, float& f) {
    const float c = fminf(fmaxf(v, -1.f), 1.f);
    const float p = __fmul_rn((c + 1.f) * 0.5f, (float)(n - 1));
    i0 = min((int)floorf(p), max(n - 2, 0));
    f = __fsub_rn(p, (float)i0);
    i1 = min(i0 + 1, n - 1);
}

__device__ __forceinline__ SpEnt sp_decide(float x, float y, int Hf, int Wf) {
    SpEnt e;
    const bool bad = !is_finite(x) || !is_finite(y);
    e.flags = (bad ? SP_BAD : 0) | ((!bad && x >= -1.f && x <= 1.f && Wf > 1) ? SP_LIVE_X : 0) |
              ((!bad && y >= -1.f && y <= 1.f && Hf > 1) ? SP_LIVE_Y : 0);
    if (bad) { x = 0.f; y = 0.f; }                       // indices stay inside the map; the flag decides what is written
    int x0, x1, y0, y1;
    sp_axis(x, Wf, x0, x1, e.fx);
    sp_axis(y, Hf, y0, y1, e.fy);
    const float gx = __fsub_rn(1.f, e.fx), gy = __fsub_rn(1.f, e.fy);
    e.w00 = __fmul_rn(gy, gx); e.w01 = __fmul_rn(gy, e.fx); e.w10 = __fmul_rn(e.fy, gx); e.w11 = __fmul_rn(e.fy, e.fx);
    e.c00 = y0 * Wf + x0; e.c01 = y0 * Wf + x1; e.c10 = y1 * Wf + x0; e.c11 = y1 * Wf + x1;
    e.pad_ = 0;
    return e;
}

__global__ __launch_bounds__(256) void spatial_prep_kernel(const float* __restrict__ pos, SpEnt* __restrict__ table, int N, int Hf,
                                                           int Wf) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n < N) table[n] = sp_decide(pos[2 * (i64)n], pos[2 * (i64)n + 1], Hf, Wf);
}

// 8 features kc .. kc + 7 of the row that starts at element e of G (zero beyond K)
template <bool BF16>
__device__ __forceinline__ void sp_load8(const void* __restrict__ g, i64 e, int kc, int K, bool vec, float (&r)[8]) {
    if (vec) {
        if (BF16) {
            const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const bf16_t*>(g) + e + kc);
            r[0] = __uint_as_float(q.x << 16); r[1] = __uint_as_float(q.x & 0xffff0000u);
            r[2] = __uint_as_float(q.y << 16); r[3] = __uint_as_float(q.y & 0xffff0000u);
            r[4] = __uint_as_float(q.z << 16); r[5] = __uint_as_float(q.z & 0xffff0000u);
            r[6] = __uint_as_float(q.w << 16); r[7] = __uint_as_float(q.w & 0xffff0000u);
        } else {
            const float4* p = reinterpret_cast<const float4*>(reinterpret_cast<const float*>(g) + e + kc);
            const float4 u = p[0], v = p[1];
            r[0] = u.x; r[1] = u.y; r[2] = u.z; r[3] = u.w; r[4] = v.x; r[5] = v.y; r[6] = v.z; r[7] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float v = 0.f;
            if (kc + i < K) v = BF16 ? bf2f(reinterpret_cast<const bf16_t*>(g)[e + kc + i]) : reinterpret_cast<const float*>(g)[e + kc + i];
            r[i] = v;
        }
    }
}

// coalesced copy between a [ncnt][tcnt] piece of a [B][N][T] tensor and an LDS tile
__device__ __forceinline__ void sp_tile_in(const float* __restrict__ src, float* tile, i64 base, int ncnt, int tcnt, int T) {
    for (int i = threadIdx.x; i < ncnt * tcnt; i += SP_NT) {
        const int nl = i / tcnt, tl = i - nl * tcnt;
        tile[nl * SP_ST + tl] = src[base + (i64)nl * T + tl];
    }
}
__device__ __forceinline__ void sp_tile_out(float* __restrict__ dst, const float* tile, i64 base, int ncnt, int tcnt, int T) {
    for (int i = threadIdx.x; i < ncnt * tcnt; i += SP_NT) {
        const int nl = i / tcnt, tl = i - nl * tcnt;
        dst[base + (i64)nl * T + tl] = tile[nl * SP_ST + tl];
    }
}

// work item -> (neuron tile, frame chunk, sample or batch group): the last fastest, so that neighbours share the weights
template <int KP, bool BF16, bool BWD>
__global__ __launch_bounds__(SP_NT) void spatial_elem_kernel(const float* __restrict__ y, const void* __restrict__ g,
                                                             const float* __restrict__ pos, const float* __restrict__ weight,
                                                             const float* __restrict__ bias, float* __restrict__ out,
                                                             const float* __restrict__ dout, float* __restrict__ dy,
                                                             float* __restrict__ sws, const SpEnt* __restrict__ table,
                                                             double* __restrict__ pdw, double* __restrict__ pdb,
                                                             double* __restrict__ pdx, double* __restrict__ pdy, SpGeom q) {
    __shared__ float yt[SP_NT * SP_ST];                  // y, then out (forward) or s (backward)
    __shared__ float dt[BWD ? SP_NT * SP_ST : 1];        // dout, then dy
    const int groups = BWD ? q.G : q.B, rb = BWD ? SP_RB : 1;
    const i64 item = blockIdx.x;
    const int grp = (int)(item % groups);
    const i64 r = item / groups;
    const int tc = (int)(r % q.nTc), nt = (int)(r / q.nTc);
    const int n0 = nt * SP_NT, ncnt = min(SP_NT, q.N - n0);
    const int t0 = tc * q.TT, tcnt = min(q.TT, q.T - t0);
    const int nl = threadIdx.x, n = n0 + nl, K = q.K;
    const bool valid = nl < ncnt, vec = q.vec != 0;
    const bool red = BWD && (pdw || pdb || pdx || pdy || sws);      // s is needed
    const bool part = BWD && (pdw || pdb || pdx || pdy);

    SpEnt e = {};
    float wr[KP], bn = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) wr[k] = 0.f;
    if (valid) {
        e = BWD ? table[n] : sp_decide(pos[2 * (i64)n], pos[2 * (i64)n + 1], q.Hf, q.Wf);
#pragma unroll
        for (int k = 0; k < KP; ++k)
            if (k < K) wr[k] = weight[(i64)n * K + k];
        bn = bias[n];
    }
    const bool isbad = (e.flags & SP_BAD) != 0;
    const i64 e00 = (i64)e.c00 * K, e01 = (i64)e.c01 * K, e10 = (i64)e.c10 * K, e11 = (i64)e.c11 * K;
    const float bad = qnan_f();
    double dW[BWD ? KP : 1], dB = 0.0, dX = 0.0, dY = 0.0;
#pragma unroll
    for (int k = 0; k < (BWD ? KP : 1); ++k) dW[k] = 0.0;

    const int b_end = min(q.B, (grp + 1) * rb);
    for (int b = grp * rb; b < b_end; ++b) {
        const i64 base = ((i64)b * q.N + n0) * q.T + t0;
        __syncthreads();                                 // the previous sample's tiles have been stored
        if (!BWD || red) sp_tile_in(y, yt, base, ncnt, tcnt, q.T);
        if (BWD) sp_tile_in(dout, dt, base, ncnt, tcnt, q.T);
        __syncthreads();
        if (valid) {
#pragma unroll 2
            for (int tl = 0; tl < tcnt; ++tl) {                       // two frames' corner rows in flight
                const i64 row = ((i64)b * q.T + t0 + tl) * q.HW * K;
                float d00 = 0.f, d01 = 0.f, d10 = 0.f, d11 = 0.f;
#pragma unroll
                for (int kc = 0; kc < KP; kc += 8) {
                    if (kc < K) {
                        float r0[8], r1[8], r2[8], r3[8];
                        sp_load8<BF16>(g, row + e00, kc, K, vec, r0);
                        sp_load8<BF16>(g, row + e01, kc, K, vec, r1);
                        sp_load8<BF16>(g, row + e10, kc, K, vec, r2);
                        sp_load8<BF16>(g, row + e11, kc, K, vec, r3);
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            d00 = fmaf(r0[i], wr[kc + i], d00); d01 = fmaf(r1[i], wr[kc + i], d01);
                            d10 = fmaf(r2[i], wr[kc + i], d10); d11 = fmaf(r3[i], wr[kc + i], d11);
                        }
                    }
                }
                const float a = fmaf(e.w11, d11, fmaf(e.w10, d10, fmaf(e.w01, d01, fmaf(e.w00, d00, bn))));
                const float gain = mod_gain(a, q.m);
                const int ti = nl * SP_ST + tl;
                if (!BWD) {
                    yt[ti] = isbad ? bad : yt[ti] * gain;
                } else {
                    const float dv = dt[ti];
                    dt[ti] = isbad ? bad : dv * gain;
                    if (red) {
                        const float s = isbad ? bad : dv * yt[ti] * gain * q.m * mod_sech2(a);
                        yt[ti] = s;
                        if (part) {
                            dB += (double)s;
                            const float hx = __fsub_rn(d01, d00), lx = __fsub_rn(d11, d10);
                            const float hy = __fsub_rn(d10, d00), ly = __fsub_rn(d11, d01);
                            const float ax = fmaf(e.fy, lx, __fmul_rn(__fsub_rn(1.f, e.fy), hx));
                            const float ay = fmaf(e.fx, ly, __fmul_rn(__fsub_rn(1.f, e.fx), hy));
                            dX += (double)__fmul_rn(s, ax);
                            dY += (double)__fmul_rn(s, ay);
                        }
                        if (pdw) {
#pragma unroll
                            for (int kc = 0; kc < KP; kc += 8) {
                                if (kc < K) {
                                    float r0[8], r1[8], r2[8], r3[8];
                                    sp_load8<BF16>(g, row + e00, kc, K, vec, r0);
                                    sp_load8<BF16>(g, row + e01, kc, K, vec, r1);
                                    sp_load8<BF16>(g, row + e10, kc, K, vec, r2);
                                    sp_load8<BF16>(g, row + e11, kc, K, vec, r3);
#pragma unroll
                                    for (int i = 0; i < 8; ++i) {
                                        const float samp = fmaf(e.w11, r3[i], fmaf(e.w10, r2[i], fmaf(e.w01, r1[i], __fmul_rn(e.w00, r0[i]))));
                                        dW[BWD ? kc + i : 0] += (double)__fmul_rn(s, samp);
                                    }
                                }
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (!BWD) {
            sp_tile_out(out, yt, base, ncnt, tcnt, q.T);
        } else {
            if (dy) sp_tile_out(dy, dt, base, ncnt, tcnt, q.T);
            if (sws) sp_tile_out(sws, yt, base, ncnt, tcnt, q.T);
        }
    }
    if (BWD && valid) {
        const i64 p = (i64)grp * q.nTc + tc;             // partial index of this (batch group, frame chunk)
        if (pdw) {
#pragma unroll
            for (int k = 0; k < KP; ++k)
                if (k < K) pdw[(p * q.N + n) * K + k] = dW[BWD ? k : 0];
        }
        if (pdb) pdb[p * q.N + n] = dB;
        if (pdx) { pdx[p * q.N + n] = dX; pdy[p * q.N + n] = dY; }
    }
}

// The bucket of a cell: the neurons one of whose corners is this cell, in ascending index, each with the weight of that corner.
// One workgroup per cell walks the table in index order; a ballot per wave and the waves' counts keep the order (a stable
// bucketing: the dG pass then adds in ascending neuron order whatever the launch).  Non-finite neurons are left out.
struct SpItem { int n; float w; };

__global__ __launch_bounds__(256) void spatial_bucket_kernel(const SpEnt* __restrict__ table, SpItem* __restrict__ lists,
                                                             int* __restrict__ counts, int N) {
    __shared__ int wcnt[4];
    const int cell = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    SpItem* dst = lists + (i64)cell * N;
    int running = 0;
    for (int nb = 0; nb < N; nb += 256) {
        const int n = nb + threadIdx.x;
        bool match = false;
        float wsel = 0.f;
        if (n < N) {
            const SpEnt e = table[n];
            if (!(e.flags & SP_BAD)) {
                match = e.c00 == cell || e.c01 == cell || e.c10 == cell || e.c11 == cell;
                // corners coincide only on a one-cell axis, where the second one's weight is exactly 0
                wsel = (e.c00 == cell ? e.w00 : 0.f) + (e.c01 == cell ? e.w01 : 0.f) + (e.c10 == cell ? e.w10 : 0.f) +
                       (e.c11 == cell ? e.w11 : 0.f);
            }
        }
        const unsigned long long mask = __ballot(match);
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int off = running;
        for (int w = 0; w < wave; ++w) off += wcnt[w];
        if (match) {
            SpItem it;
            it.n = n; it.w = wsel;
            dst[off + __popcll(mask & ((1ull << lane) - 1ull))] = it;
        }
        running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (threadIdx.x == 0) counts[cell] = running;
}

// dG: one wave per (cell, frame chunk of 32, sample), cells fastest.  Lane = (feature quad kq, frame group tq); a lane owns
// TI = KP / 8 frames x 4 features.  The cell's bucket is staged SP_LB neurons at a time: their s rows times the corner weight (one
// fp32 rounding) and their weight rows; the products with the weights are exact in float64 and the sum runs in ascending neuron order.
template <int KP>
__global__ __launch_bounds__(64) void spatial_dg_kernel(const float* __restrict__ sws, const float* __restrict__ weight,
                                                        const SpItem* __restrict__ lists, const int* __restrict__ counts,
                                                        float* __restrict__ dg, SpGeom q, int nTg) {
    constexpr int KQ = KP / 4, TQ = 64 / KQ, TI = SP_TG / TQ;
    __shared__ __attribute__((aligned(16))) float srow[SP_LB * SP_TG];
    __shared__ __attribute__((aligned(16))) float wrow[SP_LB * KP];
    __shared__ int ln[SP_LB];
    __shared__ float lw[SP_LB];
    const i64 item = blockIdx.x;
    const int cell = (int)(item % q.HW);
    const i64 r = item / q.HW;
    const int tg = (int)(r % nTg), b = (int)(r / nTg);
    const int t0 = tg * SP_TG, tcnt = min(SP_TG, q.T - t0);
    const int lane = threadIdx.x, kq = lane % KQ, tq = lane / KQ;
    const int K = q.K;
    const SpItem* src = lists + (i64)cell * q.N;
    const int count = counts[cell];
    // 16-byte loads where the rows allow them (s sits 16-byte aligned in the workspace; weight is checked)
    const bool vec_t = q.T % 4 == 0, vec_k = K % 4 == 0 && ((size_t)weight & 15) == 0;
    double acc[TI][4];
#pragma unroll
    for (int i = 0; i < TI; ++i)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[i][c] = 0.0;

    for (int j0 = 0; j0 < count; j0 += SP_LB) {
        const int cnt = min(SP_LB, count - j0);
        __syncthreads();                                 // the previous batch has been read
        for (int i = lane; i < cnt; i += 64) {
            const SpItem it = src[j0 + i];
            ln[i] = it.n; lw[i] = it.w;
        }
        __syncthreads();
        // independent loads, eight in flight per lane: a single wave has nothing else to hide their latency with
        if (vec_t) {
#pragma unroll 8
            for (int i = lane; i < cnt * (SP_TG / 4); i += 64) {
                const int j = i / (SP_TG / 4), tl = (i - j * (SP_TG / 4)) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (tl < tcnt) v = *reinterpret_cast<const float4*>(sws + ((i64)b * q.N + ln[j]) * q.T + t0 + tl);
                const float w = lw[j];
                v.x = __fmul_rn(v.x, w); v.y = __fmul_rn(v.y, w); v.z = __fmul_rn(v.z, w); v.w = __fmul_rn(v.w, w);
                *reinterpret_cast<float4*>(srow + j * SP_TG + tl) = v;
            }
        } else {
#pragma unroll 8
            for (int i = lane; i < cnt * SP_TG; i += 64) {
                const int j = i / SP_TG, tl = i - j * SP_TG;
                srow[i] = tl < tcnt ? __fmul_rn(sws[((i64)b * q.N + ln[j]) * q.T + t0 + tl], lw[j]) : 0.f;
            }
        }
        if (vec_k) {
#pragma unroll 8
            for (int i = lane; i < cnt * KQ; i += 64) {
                const int j = i / KQ, k = (i - j * KQ) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < K) v = *reinterpret_cast<const float4*>(weight + (i64)ln[j] * K + k);
                *reinterpret_cast<float4*>(wrow + j * KP + k) = v;
            }
        } else {
#pragma unroll 8
            for (int i = lane; i < cnt * KP; i += 64) {
                const int j = i / KP, k = i - j * KP;
                wrow[i] = k < K ? weight[(i64)ln[j] * K + k] : 0.f;
            }
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float4 wv = *reinterpret_cast<const float4*>(wrow + j * KP + kq * 4);
            const double wd[4] = {(double)wv.x, (double)wv.y, (double)wv.z, (double)wv.w};
#pragma unroll
            for (int i = 0; i < TI; ++i) {
                const double sd = (double)srow[j * SP_TG + tq * TI + i];
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[i][c] = fma(sd, wd[c], acc[i][c]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < TI; ++i) {
        const int tl = tq * TI + i;
        if (tl < tcnt) {
            float* dst = dg + (((i64)b * q.T + t0 + tl) * q.HW + cell) * K;
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (kq * 4 + c < K) dst[kq * 4 + c] = (float)acc[i][c];
        }
    }
}

// one thread per reduced output: dweight [N][K], dbias [N], dpos [N][2] over the P = G nTc partials in ascending order
__global__ __launch_bounds__(256) void spatial_finalize_kernel(const double* __restrict__ pdw, const double* __restrict__ pdb,
                                                               const double* __restrict__ pdx, const double* __restrict__ pdy,
                                                               const SpEnt* __restrict__ table, float* __restrict__ dweight,
                                                               float* __restrict__ dbias, float* __restrict__ dpos, i64 nw, i64 nb,
                                                               i64 np, int P, int N, int Hf, int Wf) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += pdw[(i64)p * nw + i];
        dweight[i] = (float)s;
    } else if (i < nw + nb) {
        const i64 j = i - nw;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += pdb[(i64)p * N + j];
        dbias[j] = (float)s;
    } else if (i < nw + nb + np) {
        const i64 j = i - nw - nb;
        const int n = (int)(j >> 1), c = (int)(j & 1);
        const double* src = c ? pdy : pdx;
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += src[(i64)p * N + n];
        const int flags = table[n].flags;
        const double scale = 0.5 * (double)((c ? Hf : Wf) - 1);
        float v = 0.f;                                   // clamped, or a one-cell axis: exactly 0
        if (flags & SP_BAD) v = qnan_f();
        else if (flags & (c ? SP_LIVE_Y : SP_LIVE_X)) v = (float)(s * scale);
        dpos[j] = v;
    }
}

struct SpWs { size_t dw, db, dx, dy, table, counts, lists, s, total; };       // offsets in bytes
inline SpWs sp_ws(const SpGeom& g) {
    SpWs w;
    const size_t P = (size_t)g.G * g.nTc, N = (size_t)g.N;
    w.dw = 0;
    w.db = w.dw + P * N * g.K * sizeof(double);
    w.dx = w.db + P * N * sizeof(double);
    w.dy = w.dx + P * N * sizeof(double);
    w.table = (w.dy + P * N * sizeof(double) + 15) & ~(size_t)15;
    w.counts = w.table + N * sizeof(SpEnt);
    w.lists = (w.counts + (size_t)g.HW * sizeof(int) + 15) & ~(size_t)15;
    w.s = (w.lists + (size_t)g.HW * N * sizeof(SpItem) + 15) & ~(size_t)15;
    w.total = (w.s + (size_t)g.B * N * g.T * sizeof(float) + 15) & ~(size_t)15;
    return w;
}

template <int KP, bool BF16>
int sp_forward(const dwn_spatial_gain_args& a, const SpGeom& g, hipStream_t s) {
    const i64 items = (i64)g.nNt * g.nTc * g.B;
    hipLaunchKernelGGL((spatial_elem_kernel<KP, BF16, false>), dim3((unsigned)items), dim3(SP_NT), 0, s, a.y, a.g, a.pos, a.weight,
                       a.bias, a.out, (const float*)nullptr, (float*)nullptr, (float*)nullptr, (const SpEnt*)nullptr,
                       (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, g);
    DWN_CHECK_LAUNCH();
    return 0;
}

template <int KP>
int sp_dg(const dwn_spatial_gain_args& a, const SpGeom& g, const float* sws, const SpEnt* table, SpItem* lists, int* counts,
          hipStream_t s) {
    hipLaunchKernelGGL(spatial_bucket_kernel, dim3((unsigned)g.HW), dim3(256), 0, s, table, lists, counts, g.N);
    DWN_CHECK_LAUNCH();
    const int nTg = (g.T + SP_TG - 1) / SP_TG;
    const i64 items = (i64)g.B * nTg * g.HW;
    hipLaunchKernelGGL(spatial_dg_kernel<KP>, dim3((unsigned)items), dim3(64), 0, s, sws, a.weight, (const SpItem*)lists,
                       (const int*)counts, a.dg, g, nTg);
    DWN_CHECK_LAUNCH();
    return 0;
}

template <int KP, bool BF16>
int sp_backward(const dwn_spatial_gain_args& a, const SpGeom& g, hipStream_t s) {
    const SpWs w = sp_ws(g);
    char* base = (char*)a.ws;
    double* pdw = a.dweight ? (double*)(base + w.dw) : nullptr;
    double* pdb = a.dbias ? (double*)(base + w.db) : nullptr;
    double* pdx = a.dpos ? (double*)(base + w.dx) : nullptr;
    double* pdy = a.dpos ? (double*)(base + w.dy) : nullptr;
    SpEnt* table = (SpEnt*)(base + w.table);
    float* sws = a.dg ? (float*)(base + w.s) : nullptr;
    hipLaunchKernelGGL(spatial_prep_kernel, dim3((unsigned)((g.N + 255) / 256)), dim3(256), 0, s, a.pos, table, g.N, g.Hf, g.Wf);
    DWN_CHECK_LAUNCH();
    const i64 items = (i64)g.nNt * g.nTc * g.G;
    hipLaunchKernelGGL((spatial_elem_kernel<KP, BF16, true>), dim3((unsigned)items), dim3(SP_NT), 0, s, a.y, a.g, a.pos, a.weight,
                       a.bias, (float*)nullptr, a.dout, a.dy, sws, (const SpEnt*)table, pdw, pdb, pdx, pdy, g);
    DWN_CHECK_LAUNCH();
    if (a.dg) {
        const int rc = sp_dg<KP>(a, g, sws, table, (SpItem*)(base + w.lists), (int*)(base + w.counts), s);
        if (rc != 0) return rc;
    }
    if (pdw || pdb || pdx) {
        const i64 nw = pdw ? (i64)g.N * g.K : 0, nb = pdb ? (i64)g.N : 0, np = pdx ? 2 * (i64)g.N : 0;
        const i64 blocks = (nw + nb + np + 255) / 256;
        hipLaunchKernelGGL(spatial_finalize_kernel, dim3((unsigned)blocks), dim3(256), 0, s, pdw, pdb, pdx, pdy, (const SpEnt*)table,
                           a.dweight, a.dbias, a.dpos, nw, nb, np, g.G * g.nTc, g.N, g.Hf, g.Wf);
        DWN_CHECK_LAUNCH();
    }
    return 0;
}

template <int KP>
int sp_forward_t(const dwn_spatial_gain_args& a, const SpGeom& g, hipStream_t s) {
    return a.g_dtype == DWN_BF16 ? sp_forward<KP, true>(a, g, s) : sp_forward<KP, false>(a, g, s);
}
template <int KP>
int sp_backward_t(const dwn_spatial_gain_args& a, const SpGeom& g, hipStream_t s) {
    return a.g_dtype == DWN_BF16 ? sp_backward<KP, true>(a, g, s) : sp_backward<KP, false>(a, g, s);
}

}  // namespace

size_t k_spatial_gain_ws_bytes(const dwn_spatial_gain_args& a) { return sp_ws(sp_geom(a)).total; }

int k_spatial_gain_forward(const dwn_spatial_gain_args& a, hipStream_t s) {
    const SpGeom g = sp_geom(a);
    if (a.K <= 8) return sp_forward_t<8>(a, g, s);
    if (a.K <= 16) return sp_forward_t<16>(a, g, s);
    if (a.K <= 32) return sp_forward_t<32>(a, g, s);
    return sp_forward_t<64>(a, g, s);
}

int k_spatial_gain_backward(const dwn_spatial_gain_args& a, hipStream_t s) {
    const SpGeom g = sp_geom(a);
    if (a.K <= 8) return sp_backward_t<8>(a, g, s);
    if (a.K <= 16) return sp_backward_t<16>(a, g, s);
    if (a.K <= 32) return sp_backward_t<32>(a, g, s);
    return sp_backward_t<64>(a, g, s);
}

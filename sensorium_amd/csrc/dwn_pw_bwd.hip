// ------------------------------------------------------------------------------------------------
// conv_pw backward of the 64-channel blocks (Cin = 64, E = 448) and, further down, of the 128-channel blocks (Cin = 128, E = 896):
// ONE pass over dh1, and y1 is not read at all.
// dy1 = A1*dh1 + A2*y1 + A3 (BatchNorm-1 backward) is linear and y1 = a0 . W1^T, so both products fold (reference math:
// backward of dwiseneuro.py:90-93):
//   da0 = dy1 . W1    = [dh1 | a0] . [diag(A1) W1 ; G] + r3,   G = W1^T diag(A2) W1, r3 = A3 . W1   (Bp / r3: k_pw_bwd_prep)
//   dW1 = dy1^T . a0  = diag(A1) (dh1^T a0) + diag(A2) W1 (a0^T a0) + A3 (1^T a0)                    (k_pw_wgrad_fold)
// The kernel therefore multiplies RAW tiles — no per-element BatchNorm arithmetic, no second E-wide tensor: per 128-row tile
// it streams the seven 64-column chunks of dh1 through LDS, da0 += chunk . Bp (row-major fragments, Bp resident in LDS) and
// T1[chunk] += chunk^T . a0 (ds_read_tr16_b64 fragments), plus once per tile da0 += a0 . G, Ga += a0^T a0 and s += 1^T a0.
// T1 / Ga / s leave as fp32 atomics into tacc [(E + Cin + 8)][Cin] (rows: T1, Ga, s), one flush per workgroup.
// 512 threads, one workgroup per CU (145 KB of LDS), persistent over the tiles; the NEXT tile's seven chunks are already in
// flight in registers while this tile multiplies (112 KB per CU: the version that fetched one chunk ahead ran at the pace of
// one memory latency per chunk and gained 20 % from halving its bytes).  The prefetch loads are unconditional and returned by
// value: a conditional load is waited for and copied at once, a pointer-filled array went to scratch.
// ------------------------------------------------------------------------------------------------
#include "dwn_gemm_nn.h"                                   // MFMA vector types, nn_lds_barrier

static __device__ __forceinline__ unsigned pwb_pack2(float a, float b) { return pk_bf16(a, b); }
namespace pwb {
constexpr int CIN = 64, BM = 128;
constexpr int RS = 160;                       // LDS row stride of the [128][64] bf16 tiles (128 B + 32 B shift)
template <int NKC> struct Cfg {               // NKC = E / 64: 7 (expansion 7) or 6 (the distillation student's expansion 6)
    static constexpr int E = NKC * 64, KCAT = E + CIN;
    static constexpr int WRS = KCAT * 2 + 16;            // row stride of the resident Bp [64][E + 64]
    static constexpr int SW_BYTES = CIN * WRS, SD_BYTES = BM * RS, SX_BYTES = BM * RS;
    static constexpr int MAP_INTS = 512;      // staged inverse nearest maps of the gathered shortcut form: Hin + Win entries
    static constexpr int LDS_BYTES = SW_BYTES + 2 * SD_BYTES + 2 * SX_BYTES + 7 * CIN * 4 + MAP_INTS * 4;   // + r3 [64], residual coefficients [<= 3][128], maps
};
}  // namespace pwb
// The shortcut branch's gradient in the kernel's epilogue (res != NULL), two forms:
//   identity map (stride-1 block; gq.hinv == NULL): its x terms are already in G / r3 (k_pw_bwd_prep), the epilogue adds
//     sum_j A1sc[n + 64 j] * res[m][n + 64 j];
//   gathered rows (stride-2 block; gq.hinv / gq.winv = inverse nearest maps, -1 = row not sampled): a row m = (bt, hi, wi) that the
//     shortcut samples adds sum_j (A1sc * res[rout][n + 64 j] + A2sc * a0[m][n] + A3sc) with rout = (bt * Hout + ho) * Wout + wo;
//     the other rows add nothing (so nothing can be folded into G / r3).  res_coef = [3][res_n * 64] (A1sc, A2sc, A3sc).
struct PwbGather { const int* hinv; const int* winv; int Hin, Win, Hout, Wout; };
template <int NKC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_bwd_fused_kernel(const bf16_t* __restrict__ dh1, const bf16_t* __restrict__ a0,
                                                       const bf16_t* __restrict__ bp, const float* __restrict__ r3,
                                                       bf16_t* __restrict__ da0, float* __restrict__ tacc, int M,
                                                       const bf16_t* __restrict__ res, const float* __restrict__ res_coef, int res_n,
                                                       const PwbGather gq) {
    using namespace pwb;
    constexpr int E = Cfg<NKC>::E, KCAT = Cfg<NKC>::KCAT, WRS = Cfg<NKC>::WRS;
    constexpr int SW_BYTES = Cfg<NKC>::SW_BYTES, SD_BYTES = Cfg<NKC>::SD_BYTES, SX_BYTES = Cfg<NKC>::SX_BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char pwb_smem[];
    unsigned char* const smem = pwb_smem;
    unsigned char* sW = smem;
    unsigned char* sD = smem + SW_BYTES;
    unsigned char* sX = sD + 2 * SD_BYTES;
    float* sR3 = reinterpret_cast<float*>(sX + 2 * SX_BYTES);      // r3 [64], then the residual coefficients [res_n * 64]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const int wm = wave & 3, wn = wave >> 2;
    if (tid < CIN) sR3[tid] = r3[tid];
    const bool gather = res && gq.hinv;
    if (res) for (int i = tid; i < (gather ? 3 : 1) * res_n * CIN; i += 512) sR3[CIN + i] = res_coef[i];
    // the inverse nearest maps, staged once (the epilogue's row decode must not wait for two dependent global loads per tile)
    int* sMap = reinterpret_cast<int*>(sR3 + 7 * CIN);
    if (gather) for (int i = tid; i < gq.Hin + gq.Win; i += 512) sMap[i] = i < gq.Hin ? gq.hinv[i] : gq.winv[i - gq.Hin];
    const RasterIdx ridx(gather ? gq.Hin : 1, gather ? gq.Win : 1);
    // resident Bp: [n][k], 16-byte chunks
    for (int c = tid; c < CIN * (KCAT / 8); c += 512) {
        const int n = c / (KCAT / 8), kc8 = c % (KCAT / 8);
        *reinterpret_cast<uint4*>(sW + n * WRS + kc8 * 16) = *reinterpret_cast<const uint4*>(bp + (size_t)n * KCAT + kc8 * 8);
    }
    f32x4_t acc_dw[NKC][2], acc_ga[2], acc_s[2];
#pragma unroll
    for (int k = 0; k < NKC; ++k) { acc_dw[k][0] = f32x4_t{0, 0, 0, 0}; acc_dw[k][1] = f32x4_t{0, 0, 0, 0}; }
    acc_ga[0] = acc_ga[1] = acc_s[0] = acc_s[1] = f32x4_t{0, 0, 0, 0};
    const int ntiles = M / BM;
    const int ch = tid & 7;                   // this thread's 16-byte column chunk inside a 64-column chunk (fixed)
    const int row_a = tid >> 3;               // rows row_a and row_a + 64
    struct Pair { uint4 lo, hi; };            // rows row_a and row_a + 64 of one 64-column chunk (values, never addressed: registers)
    Pair rd[NKC], rx;
    auto fetch_a0 = [&](int tile) {
        const bf16_t* src = a0 + ((size_t)tile * BM + row_a) * CIN + ch * 8;
        return Pair{*reinterpret_cast<const uint4*>(src), *reinterpret_cast<const uint4*>(src + (size_t)64 * CIN)};
    };
    auto fetch_chunk = [&](int tile, int kc) {
        const bf16_t* src = dh1 + ((size_t)tile * BM + row_a) * E + kc * 64 + ch * 8;
        return Pair{*reinterpret_cast<const uint4*>(src), *reinterpret_cast<const uint4*>(src + (size_t)64 * E)};
    };
    int tile = blockIdx.x;
    {
        const int t0 = tile < ntiles ? tile : 0;          // ntiles >= 1 (launcher): unconditional loads
        rx = fetch_a0(t0);
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) rd[kc] = fetch_chunk(t0, kc);
    }
    __syncthreads();
    const int q = lr >> 2, p = lr & 3;         // transposed-fragment lane roles (ds_read_tr16_b64)
    const bf16x8_t ones = {(short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80};
    int tpar = 0, step = 0;                  // step: running chunk counter (LDS buffer parity continues across tiles)
    for (; tile < ntiles; tile += gridDim.x, tpar ^= 1) {
        const size_t m0 = (size_t)tile * BM;
        // the prefetch target: the next tile of this workgroup, or (last round) this tile again — unconditional loads, so that
        // the values land in the ring registers themselves (a conditional load is waited for and copied at once)
        const int ntile = tile + (int)gridDim.x < ntiles ? tile + (int)gridDim.x : tile;
        unsigned char* sXt = sX + tpar * SX_BYTES;
        *reinterpret_cast<uint4*>(sXt + row_a * RS + ch * 16) = rx.lo;
        *reinterpret_cast<uint4*>(sXt + (row_a + 64) * RS + ch * 16) = rx.hi;
        rx = fetch_a0(ntile);
        f32x4_t acc_da[2][2];
        uint2 rres[2][2][2];
        bool rgat[2] = {true, true};            // gather form: is this lane's row i sampled by the shortcut?
#pragma unroll
        for (int i = 0; i < 2; ++i) { acc_da[i][0] = f32x4_t{0, 0, 0, 0}; acc_da[i][1] = f32x4_t{0, 0, 0, 0}; }
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            unsigned char* sDk = sD + ((step + kc) & 1) * SD_BYTES;
            *reinterpret_cast<uint4*>(sDk + row_a * RS + ch * 16) = rd[kc].lo;
            *reinterpret_cast<uint4*>(sDk + (row_a + 64) * RS + ch * 16) = rd[kc].hi;
            nn_lds_barrier();      // LDS hand-off only: the next tile's loads stay in flight across it
            rd[kc] = fetch_chunk(ntile, kc);                     // this chunk of the NEXT tile: a whole tile of loads in flight
            if (kc == NKC - 3 && res) {                          // the epilogue's residual values: in flight under the last three chunks
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    size_t rrow = m0 + wm * 32 + i * 16 + lr;
                    if (gather) {
                        unsigned bt; int hi, wi;
                        ridx.decode((unsigned)rrow, bt, hi, wi);
                        const int ho = sMap[hi], wo = sMap[gq.Hin + wi];
                        rgat[i] = ho >= 0 && wo >= 0;
                        rrow = rgat[i] ? ((size_t)bt * gq.Hout + ho) * gq.Wout + wo : 0;
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const bf16_t* rp_ = res + rrow * (size_t)(res_n * CIN) + wn * 32 + j * 16 + 4 * lg;
                        rres[i][j][0] = *reinterpret_cast<const uint2*>(rp_);
                        rres[i][j][1] = *reinterpret_cast<const uint2*>(rp_ + (res_n > 1 ? CIN : 0));
                    }
                }
            }
            // ---- data gradient: acc_da[m][n] += sum_k dh1[m][k] Bp[n][k]   (swapped roles: lanes own 4 consecutive n)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                bf16x8_t af[2], wf[2];
#pragma unroll
                for (int i = 0; i < 2; ++i)
                    af[i] = *reinterpret_cast<const bf16x8_t*>(sDk + (wm * 32 + i * 16 + lr) * RS + (kb * 4 + lg) * 16);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    wf[j] = *reinterpret_cast<const bf16x8_t*>(sW + (wn * 32 + j * 16 + lr) * WRS + (kc * 64 + kb * 32 + lg * 8) * 2);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc_da[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc_da[i][j], 0, 0, 0);
            }
            // ---- T1[kc][e][c] += sum_rows dh1[row][e] a0[row][c]   (transposed fragments)
#pragma unroll
            for (int kb = 0; kb < BM / 32; ++kb) {
                const int rb = kb * 32 + 8 * lg + q;
                bf16x8_t ef, cf[2];
                {
                    const int colb = (wm * 16 + 4 * p) * 2;
                    auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sDk + rb * RS + colb));
                    auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sDk + (rb + 4) * RS + colb));
                    ef = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int colb = (wn * 32 + j * 16 + 4 * p) * 2;
                    auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sXt + rb * RS + colb));
                    auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sXt + (rb + 4) * RS + colb));
                    cf[j] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc_dw[kc][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ef, cf[j], acc_dw[kc][j], 0, 0, 0);
            }
            if (kc == 0) {
                // ---- once per tile, on the a0 tile alone (complete since the barrier above): da0 += a0 . G, Ga += a0^T a0, s += 1^T a0
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    bf16x8_t af[2], wf[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
                        af[i] = *reinterpret_cast<const bf16x8_t*>(sXt + (wm * 32 + i * 16 + lr) * RS + (kb * 4 + lg) * 16);
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        wf[j] = *reinterpret_cast<const bf16x8_t*>(sW + (wn * 32 + j * 16 + lr) * WRS + (E + kb * 32 + lg * 8) * 2);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            acc_da[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc_da[i][j], 0, 0, 0);
                }
#pragma unroll
                for (int kb = 0; kb < BM / 32; ++kb) {
                    const int rb = kb * 32 + 8 * lg + q;
                    bf16x8_t ef, cf[2];
                    {
                        const int colb = (wm * 16 + 4 * p) * 2;
                        auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sXt + rb * RS + colb));
                        auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sXt + (rb + 4) * RS + colb));
                        ef = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int colb = (wn * 32 + j * 16 + 4 * p) * 2;
                        auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sXt + rb * RS + colb));
                        auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sXt + (rb + 4) * RS + colb));
                        cf[j] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        acc_ga[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ef, cf[j], acc_ga[j], 0, 0, 0);
                        if (wm == 0) acc_s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, cf[j], acc_s[j], 0, 0, 0);
                    }
                }
            }
        }
        step += NKC;
        // da0 tile: acc_da[i][j][r] = da0[m = wm*32 + i*16 + lr][n = wn*32 + j*16 + 4*lg + r]
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const size_t m = m0 + wm * 32 + i * 16 + lr;
                const int n = wn * 32 + j * 16 + 4 * lg;
                const float4 b4 = *reinterpret_cast<const float4*>(sR3 + n);
                float o[4] = {acc_da[i][j][0] + b4.x, acc_da[i][j][1] + b4.y, acc_da[i][j][2] + b4.z, acc_da[i][j][3] + b4.w};
                if (res) {       // + the shortcut branch's gradient: sum_j coef[n + 64 j] * res[m][n + 64 j]   (dwn.h)
                    const int rc = res_n * CIN;
                    float x4[4] = {0.f, 0.f, 0.f, 0.f};
                    if (gather) {
                        const uint2 xv = *reinterpret_cast<const uint2*>(sXt + (wm * 32 + i * 16 + lr) * RS + n * 2);
                        x4[0] = __uint_as_float(xv.x << 16); x4[1] = __uint_as_float(xv.x & 0xffff0000u);
                        x4[2] = __uint_as_float(xv.y << 16); x4[3] = __uint_as_float(xv.y & 0xffff0000u);
                    }
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        if (jj >= res_n || !rgat[i]) break;
                        const uint2 rv = rres[i][j][jj];
                        const float4 c4 = *reinterpret_cast<const float4*>(sR3 + CIN + jj * CIN + n);
                        float t[4] = {c4.x * __uint_as_float(rv.x << 16), c4.y * __uint_as_float(rv.x & 0xffff0000u),
                                      c4.z * __uint_as_float(rv.y << 16), c4.w * __uint_as_float(rv.y & 0xffff0000u)};
                        if (gather) {
                            const float4 a2 = *reinterpret_cast<const float4*>(sR3 + CIN + rc + jj * CIN + n);
                            const float4 a3 = *reinterpret_cast<const float4*>(sR3 + CIN + 2 * rc + jj * CIN + n);
                            t[0] += fmaf(a2.x, x4[0], a3.x); t[1] += fmaf(a2.y, x4[1], a3.y);
                            t[2] += fmaf(a2.z, x4[2], a3.z); t[3] += fmaf(a2.w, x4[3], a3.w);
                        }
                        o[0] += t[0]; o[1] += t[1]; o[2] += t[2]; o[3] += t[3];
                    }
                }
                uint2 v = make_uint2(pwb_pack2(o[0], o[1]), pwb_pack2(o[2], o[3]));
                *reinterpret_cast<uint2*>(da0 + m * CIN + n) = v;
            }
    }
    // acc_dw[kc][j][r] = T1[e = kc*64 + wm*16 + 4*lg + r][c = wn*32 + j*16 + lr]; Ga likewise at rows E + ...; s at row E + CIN
    DET_ENTER();
#pragma unroll
    for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                atomicAdd(tacc + (size_t)(kc * 64 + wm * 16 + 4 * lg + r) * CIN + wn * 32 + j * 16 + lr, acc_dw[kc][j][r]);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            atomicAdd(tacc + (size_t)(E + wm * 16 + 4 * lg + r) * CIN + wn * 32 + j * 16 + lr, acc_ga[j][r]);
        if (wm == 0 && lg == 0) atomicAdd(tacc + (size_t)KCAT * CIN + wn * 32 + j * 16 + lr, acc_s[j][0]);
    }
    DET_EXIT();
}


// ------------------------------------------------------------------------------------------------
// The same one pass at 128 input channels (Cin = 128, E = 896: blocks 4-6), split by COLUMNS of a0.  The 64-channel layout does
// not scale: a resident Bp [128][1024] is 256 KB and T1 [896][128] is 224 accumulator registers per thread.  Two workgroups
// therefore share a 64-row tile: each owns 64 of the 128 da0 columns and the matching 64 columns of T1 / Ga / s (112 + 16 + 1
// accumulator registers), both stream all fourteen chunks of dh1.  da0's columns are disjoint: no partial sums, no new atomics.
//   * the two halves of a tile are workgroups of ONE XCD, dispatched next to each other (the wk_block map of the stencils: linear
//     id b, xcd = b & 7, half = (b >> 3) & 1), so dh1 crosses the fabric once and its second read finds it in that L2;
//   * LDS per workgroup (154 KB of 160): Bp half resident with its G columns [64][1024] (129 KB), two dh1 chunk buffers
//     [64][64] (20 KB), coefficients and maps (5 KB).  The a0 tile [64][128] (18 KB) has no room of its own: it is staged through the
//     two chunk buffers at the top of a tile, where its whole use happens — a0 . G, Ga, s, and its transposed fragments for T1,
//     which then stay in 16 registers for the fourteen chunks (the 64-channel kernel re-reads them from LDS per chunk);
//   * the load schedule is the 64-channel kernel's, unconditional loads returned by value, at HALF its depth: seven chunks (56 KB
//     per CU) and the next tile's a0 rows are in flight in registers (28 + 8) while this tile multiplies.  A whole tile ahead
//     (56 registers) spilled 36 registers to scratch; seven divides fourteen, so the ring slot kc % 7 stays a compile-time constant.
// ------------------------------------------------------------------------------------------------
namespace pwb128 {
constexpr int CT = 128, CH = 64, BM = 64;     // channels of a0, columns per workgroup, rows per tile
constexpr int RS = 160;                       // LDS row stride of a dh1 chunk [64][64] bf16 (128 B + 32 B shift)
constexpr int XRS = 288;                      // ... of the a0 tile [64][128] bf16 (256 B + 32 B shift)
template <int NKC> struct Cfg {               // NKC = E / 64
    static constexpr int E = NKC * 64, KCAT = E + CT;
    static constexpr int WRS = KCAT * 2 + 16;            // row stride of the resident Bp half [64][E + 128]
    static constexpr int SW_BYTES = CH * WRS, SD_BYTES = BM * RS, SX_BYTES = BM * XRS;
    static_assert(SX_BYTES <= 2 * SD_BYTES, "the a0 tile is staged through the two chunk buffers");
    static constexpr int COEF_FLOATS = CH + 3 * 2 * CT;  // r3 [64], residual coefficients [<= 3][<= 256]
    static constexpr int MAP_INTS = 512;                 // staged inverse nearest maps: Hin + Win entries
    static constexpr int LDS_BYTES = SW_BYTES + 2 * SD_BYTES + COEF_FLOATS * 4 + MAP_INTS * 4;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS of one CU");
};
}  // namespace pwb128
// grid (gx, 2), gx % 8 == 0: see the XCD map above.  Residual forms and res_coef layout as pw_bwd_fused_kernel, rows 128 * res_n wide.
template <int NKC>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(2, 2))) void pw_bwd_fused128_kernel(const bf16_t* __restrict__ dh1, const bf16_t* __restrict__ a0,
                                                       const bf16_t* __restrict__ bp, const float* __restrict__ r3,
                                                       bf16_t* __restrict__ da0, float* __restrict__ tacc, int M,
                                                       const bf16_t* __restrict__ res, const float* __restrict__ res_coef, int res_n,
                                                       const PwbGather gq) {
    using namespace pwb128;
    constexpr int E = Cfg<NKC>::E, KCAT = Cfg<NKC>::KCAT, WRS = Cfg<NKC>::WRS;
    constexpr int SW_BYTES = Cfg<NKC>::SW_BYTES, SD_BYTES = Cfg<NKC>::SD_BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char pwb_smem[];
    unsigned char* const smem = pwb_smem;
    unsigned char* sW = smem;
    unsigned char* sD = smem + SW_BYTES;
    unsigned char* sX = sD;                                        // the a0 tile: alive only at the top of a tile
    float* sR3 = reinterpret_cast<float*>(sD + 2 * SD_BYTES);      // r3 [64] of this half, then the residual coefficients
    float* sCoef = sR3 + CH;
    int* sMap = reinterpret_cast<int*>(sR3 + Cfg<NKC>::COEF_FLOATS);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int lr = lane & 15, lg = lane >> 4;
    const int wm = wave & 3, wn = wave >> 2;
    // the two halves of a row tile on one XCD, next to each other in dispatch order
    const int gx = (int)gridDim.x;
    const int bl = (int)blockIdx.y * gx + (int)blockIdx.x;
    const int half = (bl >> 3) & 1, wx = (bl >> 4) * 8 + (bl & 7);
    const int c0 = half * CH;                                      // first of this workgroup's 64 columns
    if (tid < CH) sR3[tid] = r3[c0 + tid];
    const bool gather = res && gq.hinv;
    if (res) for (int i = tid; i < (gather ? 3 : 1) * res_n * CT; i += 512) sCoef[i] = res_coef[i];
    if (gather) for (int i = tid; i < gq.Hin + gq.Win; i += 512) sMap[i] = i < gq.Hin ? gq.hinv[i] : gq.winv[i - gq.Hin];
    const RasterIdx ridx(gather ? gq.Hin : 1, gather ? gq.Win : 1);
    // resident Bp half: rows n = c0 .. c0 + 63, [n][k], 16-byte chunks
    for (int c = tid; c < CH * (KCAT / 8); c += 512) {
        const int n = c / (KCAT / 8), kc8 = c % (KCAT / 8);
        *reinterpret_cast<uint4*>(sW + n * WRS + kc8 * 16) = *reinterpret_cast<const uint4*>(bp + (size_t)(c0 + n) * KCAT + kc8 * 8);
    }
    f32x4_t acc_dw[NKC][2], acc_ga[2][2];
    float acc_s = 0.f;                               // s: one column per lane of the waves wm < 2 (the ones-product's rows are all equal)
#pragma unroll
    for (int k = 0; k < NKC; ++k) { acc_dw[k][0] = f32x4_t{0, 0, 0, 0}; acc_dw[k][1] = f32x4_t{0, 0, 0, 0}; }
    acc_ga[0][0] = acc_ga[0][1] = acc_ga[1][0] = acc_ga[1][1] = f32x4_t{0, 0, 0, 0};
    const int ntiles = M / BM;
    const int ch = tid & 7, row_a = tid >> 3;        // dh1 chunk [64][64]: one 16-byte piece per thread
    const int chx = tid & 15, row_x = tid >> 4;      // a0 tile [64][128]: rows row_x and row_x + 32
    struct Pair { uint4 lo, hi; };                   // values, never addressed: registers
    constexpr int NPF = NKC / 2;                     // prefetch distance in chunks: half a tile (the ring slot kc % NPF stays a constant)
    static_assert(NKC % 2 == 0, "ring slots are compile-time constants only with an even chunk count");
    uint4 rd[NPF];
    Pair rx;
    auto fetch_a0 = [&](int tile) {
        const bf16_t* src = a0 + ((size_t)tile * BM + row_x) * CT + chx * 8;
        return Pair{*reinterpret_cast<const uint4*>(src), *reinterpret_cast<const uint4*>(src + (size_t)32 * CT)};
    };
    auto fetch_chunk = [&](int tile, int kc) {
        return *reinterpret_cast<const uint4*>(dh1 + ((size_t)tile * BM + row_a) * E + kc * 64 + ch * 8);
    };
    int tile = wx;
    {
        const int t0 = tile < ntiles ? tile : 0;          // ntiles >= 1 (launcher): unconditional loads
        rx = fetch_a0(t0);
#pragma unroll
        for (int kc = 0; kc < NPF; ++kc) rd[kc] = fetch_chunk(t0, kc);
    }
    __syncthreads();
    const int q = lr >> 2, p = lr & 3;         // transposed-fragment lane roles (ds_read_tr16_b64)
    const bf16x8_t ones = {(short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80, (short)0x3F80};
    auto read_tr = [&](const unsigned char* base, int rb, int rs, int colb) {
        auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + rb * rs + colb));
        auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(base + (rb + 4) * rs + colb));
        return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    for (; tile < ntiles; tile += gx) {
        const size_t m0 = (size_t)tile * BM;
        // the prefetch target: the next tile of this workgroup, or (last round) this tile again — unconditional loads
        const int ntile = tile + gx < ntiles ? tile + gx : tile;
        // ---- top of the tile, on the a0 tile alone: da0 = a0 . G, Ga += a0^T a0, s += 1^T a0, and a0's transposed fragments
        nn_lds_barrier();                          // every wave is past the previous tile's last chunk: its buffers become the a0 tile
        *reinterpret_cast<uint4*>(sX + row_x * XRS + chx * 16) = rx.lo;
        *reinterpret_cast<uint4*>(sX + (row_x + 32) * XRS + chx * 16) = rx.hi;
        nn_lds_barrier();
        rx = fetch_a0(ntile);
        f32x4_t acc_da[2] = {f32x4_t{0, 0, 0, 0}, f32x4_t{0, 0, 0, 0}};
        // gathered shortcut: is this lane's row m sampled, and by which output row?  Its a0 terms (A2sc * a0 + A3sc) start the
        // accumulator here, where the a0 tile is at hand; the A1sc * res term waits for the epilogue
        bool rgat = true;
        unsigned rrow = (unsigned)m0 + wm * 16 + lr;
        if (gather) {
            unsigned bt; int hi, wi;
            ridx.decode(rrow, bt, hi, wi);
            const int ho = sMap[hi], wo = sMap[gq.Hin + wi];
            rgat = ho >= 0 && wo >= 0;
            rrow = rgat ? (bt * gq.Hout + ho) * gq.Wout + wo : 0u;
            if (rgat) {
                const int rc = res_n * CT;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ng = c0 + wn * 32 + j * 16 + 4 * lg;
                    const uint2 xv = *reinterpret_cast<const uint2*>(sX + (wm * 16 + lr) * XRS + ng * 2);
                    const float x4[4] = {__uint_as_float(xv.x << 16), __uint_as_float(xv.x & 0xffff0000u),
                                         __uint_as_float(xv.y << 16), __uint_as_float(xv.y & 0xffff0000u)};
                    for (int jj = 0; jj < res_n; ++jj) {
                        const float4 a2 = *reinterpret_cast<const float4*>(sCoef + rc + jj * CT + ng);
                        const float4 a3 = *reinterpret_cast<const float4*>(sCoef + 2 * rc + jj * CT + ng);
                        acc_da[j][0] += fmaf(a2.x, x4[0], a3.x); acc_da[j][1] += fmaf(a2.y, x4[1], a3.y);
                        acc_da[j][2] += fmaf(a2.z, x4[2], a3.z); acc_da[j][3] += fmaf(a2.w, x4[3], a3.w);
                    }
                }
            }
        }
        bf16x8_t cf[2][2];                         // a0^T fragments of this workgroup's columns: [32-row block][j]
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int j = 0; j < 2; ++j) cf[kb][j] = read_tr(sX, kb * 32 + 8 * lg + q, XRS, (c0 + wn * 32 + j * 16 + 4 * p) * 2);
#pragma unroll
        for (int kb = 0; kb < CT / 32; ++kb) {
            const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(sX + (wm * 16 + lr) * XRS + (kb * 4 + lg) * 16);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const bf16x8_t wf = *reinterpret_cast<const bf16x8_t*>(sW + (wn * 32 + j * 16 + lr) * WRS + (E + kb * 32 + lg * 8) * 2);
                acc_da[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc_da[j], 0, 0, 0);
            }
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {          // Ga rows c' = g * 64 + wm * 16 + ...
                const bf16x8_t ef = read_tr(sX, kb * 32 + 8 * lg + q, XRS, (g * 64 + wm * 16 + 4 * p) * 2);
#pragma unroll
                for (int j = 0; j < 2; ++j) acc_ga[g][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ef, cf[kb][j], acc_ga[g][j], 0, 0, 0);
            }
            if (wm < 2) {                          // s: wave wm sums the columns of j = wm
                const bf16x8_t cs = wm == 0 ? cf[kb][0] : cf[kb][1];
                acc_s += __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, cs, f32x4_t{0, 0, 0, 0}, 0, 0, 0)[0];
            }
        }
        nn_lds_barrier();                          // the a0 tile is dead: chunk 0 goes into its place
        uint2 rres[2][2];
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
            unsigned char* sDk = sD + (kc & 1) * SD_BYTES;
            *reinterpret_cast<uint4*>(sDk + row_a * RS + ch * 16) = rd[kc % NPF];
            nn_lds_barrier();      // LDS hand-off only: the next tile's loads stay in flight across it
            rd[kc % NPF] = kc < NPF ? fetch_chunk(tile, kc + NPF) : fetch_chunk(ntile, kc - NPF);      // half a tile ahead
            if (kc == NKC - 3 && res) {                          // the epilogue's residual values: in flight under the last three chunks
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int ng = c0 + wn * 32 + j * 16 + 4 * lg;
                    const bf16_t* rp_ = res + (size_t)rrow * (size_t)(res_n * CT) + ng;
                    rres[j][0] = *reinterpret_cast<const uint2*>(rp_);
                    rres[j][1] = *reinterpret_cast<const uint2*>(rp_ + (res_n > 1 ? CT : 0));
                }
            }
            // ---- data gradient: acc_da[n] += sum_k dh1[m][k] Bp[n][k]   (swapped roles: lanes own 4 consecutive n)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const bf16x8_t af = *reinterpret_cast<const bf16x8_t*>(sDk + (wm * 16 + lr) * RS + (kb * 4 + lg) * 16);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const bf16x8_t wf = *reinterpret_cast<const bf16x8_t*>(sW + (wn * 32 + j * 16 + lr) * WRS + (kc * 64 + kb * 32 + lg * 8) * 2);
                    acc_da[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc_da[j], 0, 0, 0);
                }
            }
            // ---- T1[kc][e][c] += sum_rows dh1[row][e] a0[row][c]   (transposed fragments; a0's are in registers)
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                const bf16x8_t ef = read_tr(sDk, kb * 32 + 8 * lg + q, RS, (wm * 16 + 4 * p) * 2);
#pragma unroll
                for (int j = 0; j < 2; ++j) acc_dw[kc][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ef, cf[kb][j], acc_dw[kc][j], 0, 0, 0);
            }
        }
        // da0 tile: acc_da[j][r] = da0[m = wm*16 + lr][n = c0 + wn*32 + j*16 + 4*lg + r]
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const size_t m = m0 + wm * 16 + lr;
            const int n = wn * 32 + j * 16 + 4 * lg, ng = c0 + n;
            const float4 b4 = *reinterpret_cast<const float4*>(sR3 + n);
            float o[4] = {acc_da[j][0] + b4.x, acc_da[j][1] + b4.y, acc_da[j][2] + b4.z, acc_da[j][3] + b4.w};
            if (res && rgat) {       // + the shortcut branch's gradient (see pw_bwd_fused_kernel)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    if (jj >= res_n) break;
                    const uint2 rv = rres[j][jj];
                    const float4 c4 = *reinterpret_cast<const float4*>(sCoef + jj * CT + ng);
                    o[0] = fmaf(c4.x, __uint_as_float(rv.x << 16), o[0]); o[1] = fmaf(c4.y, __uint_as_float(rv.x & 0xffff0000u), o[1]);
                    o[2] = fmaf(c4.z, __uint_as_float(rv.y << 16), o[2]); o[3] = fmaf(c4.w, __uint_as_float(rv.y & 0xffff0000u), o[3]);
                }
            }
            *reinterpret_cast<uint2*>(da0 + m * CT + ng) = make_uint2(pwb_pack2(o[0], o[1]), pwb_pack2(o[2], o[3]));
        }
    }
    // acc_dw[kc][j][r] = T1[e = kc*64 + wm*16 + 4*lg + r][c = c0 + wn*32 + j*16 + lr]; Ga[g] likewise at rows E + g*64 + ...; s at row E + 128
    DET_ENTER();
    if (wx < ntiles) {                             // (a workgroup past the work holds zeros; it still passes the ticket)
        float* tc = tacc + c0 + wn * 32 + lr;
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    atomicAdd(tc + (size_t)(kc * 64 + wm * 16 + 4 * lg + r) * CT + j * 16, acc_dw[kc][j][r]);
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    atomicAdd(tc + (size_t)(E + g * 64 + wm * 16 + 4 * lg + r) * CT + j * 16, acc_ga[g][j][r]);
        if (wm < 2 && lg == 0) atomicAdd(tc + (size_t)KCAT * CT + wm * 16, acc_s);
    }
    DET_EXIT();
}

// M % 128 at both widths (the 128-channel kernel's own tile is 64 rows: the predicate keeps one row condition for callers)
bool pw_bwd_fused_supported(int dtype, long long M, int E, int Cin) {
    const bool shape = (Cin == pwb::CIN && (E == 448 || E == 384)) || (Cin == pwb128::CT && E == 896);
    return dtype == DWN_BF16 && shape && M > 0 && M % pwb::BM == 0 && M <= 0x7fffffffLL;
}
template <int NKC>
static int launch_pw_bwd_fused_t(const void* dh1, const void* a0, const void* bp, const float* r3, void* da0, float* tacc,
                                 long long M, const void* res, const float* res_coef, int res_n, const PwbGather& gq, hipStream_t s) {
    auto kern = pw_bwd_fused_kernel<NKC>;
    {   // > 64 KB of dynamic LDS needs the opt-in; per device, so it is (cheaply) repeated on every call
        hipError_t e = lds_opt_in(kern, pwb::Cfg<NKC>::LDS_BYTES);
        if (e != hipSuccess) return dwn_set_error((int)e, hipGetErrorString(e));
    }
    int grid = 256;
    if (grid > (int)(M / pwb::BM)) grid = (int)(M / pwb::BM);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), pwb::Cfg<NKC>::LDS_BYTES, s, (const bf16_t*)dh1, (const bf16_t*)a0,
                       (const bf16_t*)bp, r3, (bf16_t*)da0, tacc, (int)M, (const bf16_t*)res, res_coef, res_n, gq);
    DWN_CHECK_LAUNCH();
    return 0;
}
// 128 channels: grid (gx, 2) — gx row-tile owners, a multiple of 8 (the kernel's XCD map), times the two column halves; one
// workgroup per CU, so one resident round is 128 tiles
template <int NKC>
static int launch_pw_bwd_fused128_t(const void* dh1, const void* a0, const void* bp, const float* r3, void* da0, float* tacc,
                                    long long M, const void* res, const float* res_coef, int res_n, const PwbGather& gq, hipStream_t s) {
    auto kern = pw_bwd_fused128_kernel<NKC>;
    {
        hipError_t e = lds_opt_in(kern, pwb128::Cfg<NKC>::LDS_BYTES);
        if (e != hipSuccess) return dwn_set_error((int)e, hipGetErrorString(e));
    }
    const int gx = (int)resident_grid_x(1, 2, M / pwb128::BM, true);
    hipLaunchKernelGGL(kern, dim3(gx, 2), dim3(512), pwb128::Cfg<NKC>::LDS_BYTES, s, (const bf16_t*)dh1, (const bf16_t*)a0,
                       (const bf16_t*)bp, r3, (bf16_t*)da0, tacc, (int)M, (const bf16_t*)res, res_coef, res_n, gq);
    DWN_CHECK_LAUNCH();
    return 0;
}
// res / res_coef / res_n (+ hinv, winv, Hin, Win, Hout, Wout for the gathered form): the shortcut branch's gradient in the epilogue
// (see PwbGather above); res rows are res_n * Cin wide
int launch_pw_bwd_fused(const void* dh1, const void* a0, const void* bp, const float* r3, void* da0, float* tacc,
                        long long M, int E, int Cin, int dtype, const void* res, const float* res_coef, int res_n,
                        const int* hinv, const int* winv, int Hin, int Win, int Hout, int Wout, hipStream_t s) {
    PwbGather gq; gq.hinv = hinv; gq.winv = winv; gq.Hin = Hin; gq.Win = Win; gq.Hout = Hout; gq.Wout = Wout;
    if (res && hinv && (!winv || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || M % ((long long)Hin * Win) || Hin + Win > 512))
        return dwn_set_error(-2, "pw_bwd_fused: the gathered shortcut form needs both inverse maps, M = frames * Hin * Win and Hin + Win <= 512");
    if (!pw_bwd_fused_supported(dtype, M, E, Cin))
        return dwn_set_error(-3, "pw_bwd_fused: built for bf16, (Cin, E) = (64, 448), (64, 384) or (128, 896), M % 128 == 0 only");
    if (res && (!res_coef || res_n < 1 || res_n > 2)) return dwn_set_error(-3, "pw_bwd_fused: the residual term needs res_coef and res_n in {1, 2}");
    if (Cin == pwb128::CT) return launch_pw_bwd_fused128_t<14>(dh1, a0, bp, r3, da0, tacc, M, res, res_coef, res_n, gq, s);
    return E == 448 ? launch_pw_bwd_fused_t<7>(dh1, a0, bp, r3, da0, tacc, M, res, res_coef, res_n, gq, s)
                    : launch_pw_bwd_fused_t<6>(dh1, a0, bp, r3, da0, tacc, M, res, res_coef, res_n, gq, s);
}

// ------------------------------------------------------------------------------------------------
// Gram pass of the y1-free training forward: raw products [a0 | 1]^T a0 of the block input, the sums BatchNorm-1's batch
// statistics are made of (k_bn1_gram_finalize, dwn_elementwise.hip).  Until this kernel the pass ran as gemm_tn with
// P = [a0 | 1] and Q = a0: every a0 tile went through a CU's load path twice, a workgroup summed a whole M-split of several
// thousand rows in fp32, and some 500 workgroups added (Cin + 8) * Cin doubles each to the SAME addresses.  Here
//   * a row tile of a0 is loaded ONCE, staged in LDS and read back transposed (ds_read_b64_tr_b16, as gemm_tn reads its P
//     fragments): lane (c, g) of a wave holds channel 16 b + c of rows 8 g .. 8 g + 7 of a 32-row step — which is the A fragment of
//     v_mfma_f32_16x16x32_bf16 for output rows 16 b .. and the B fragment for output columns 16 b .. alike, so the four fragments
//     of a step serve all the products; G is symmetric, so only the ten 16 x 16 tiles with tile row <= tile column are computed
//     (the finaliser mirrors them), and 1^T a0 is the product of an all-ones A fragment with the same B fragments;
//   * every wave streams its own contiguous range of rows through its own LDS tile: no workgroup barrier in the loop, and
//     GRAM_SETS x four 16-byte loads per lane in flight ahead of the MFMAs (addresses clamped, loads unconditional; what lies
//     past the range is zeroed on the way to LDS: rows past M contribute nothing, to the ones row either);
//   * the matrix cores sum at most GRAM_FOLD_ROWS rows in fp32, then the tile is folded into fp64 accumulators in registers;
//   * the waves of a workgroup add their fp64 tiles in wave order through LDS, and the workgroup flushes ONE partial with fp64
//     atomics into replica blockIdx.x % GRAM_NREP: with one 512-thread workgroup per CU that is 256 / GRAM_NREP adders per
//     address instead of ~500 (same-address atomics at a kernel's end are a serial queue per address: DESIGN.md section 8).
// Layout of a replica: today's [(Cin + 8)][Cin] doubles, rows 0 .. Cin-1 = G (tiles below the diagonal stay zero), row Cin = 1^T a0.
// Built for bf16, Cin = 64 (the blocks that train without y1 by default); everything else keeps the gemm_tn route.
// ------------------------------------------------------------------------------------------------
#include "dwn_gemm_nn.h"                                   // MFMA vector types
#include "dwn_kernels.h"

#ifndef GRAM_SETS
#define GRAM_SETS 4                                        // register sets of one 32-row step each (4 x 16 B per lane) in flight
#endif
namespace {
constexpr int GRAM_C = 64;                                 // channels
constexpr int GRAM_WAVES = 8, GRAM_THREADS = 64 * GRAM_WAVES;
constexpr int GRAM_STEP = 32;                              // rows per step = k of one MFMA
constexpr int GRAM_RS = GRAM_C * 2 + 32;                   // LDS row stride (bytes): 16-byte aligned rows, 8-dword shift per row
constexpr int GRAM_FOLD_GROUPS = 8 / GRAM_SETS;            // fp32 -> fp64 fold every GRAM_FOLD_GROUPS * GRAM_SETS steps ...
constexpr int GRAM_FOLD_ROWS = GRAM_FOLD_GROUPS * GRAM_SETS * GRAM_STEP;      // ... = at most 256 rows summed in fp32
constexpr int GRAM_TILES = 10;                             // 16 x 16 tiles of G with tile row <= tile column
constexpr int GRAM_SLOTS = 4 * GRAM_TILES + 4;             // per-lane fp64 values of a wave: 10 tiles x 4 + 4 column-sum blocks
constexpr int GRAM_MIN_STEPS = 8;                          // a workgroup is worth launching for >= 8 steps per wave
static_assert(GRAM_FOLD_GROUPS >= 1 && GRAM_FOLD_ROWS <= 256, "fp32 partial sums cover at most 256 rows");
static_assert(GRAM_SLOTS * 64 * (int)sizeof(double) <= GRAM_WAVES * GRAM_STEP * GRAM_RS, "the reduction image reuses the staging tiles");

// tile t = 0 .. 9 in the order (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3)
__device__ __forceinline__ void gram_tile_of(int t, int& bi, int& bj) {
    bi = t < 4 ? 0 : t < 7 ? 1 : t < 9 ? 2 : 3;
    bj = t - (bi == 0 ? 0 : bi == 1 ? 3 : bi == 2 ? 5 : 6);
}

__global__ __launch_bounds__(GRAM_THREADS) void gram64_kernel(const bf16_t* __restrict__ a0, i64 ld, i64 M, i64 steps_per_wave,
                                                              double* __restrict__ gram, int nrep) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[GRAM_WAVES * GRAM_STEP * GRAM_RS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: the row range and the loop below stay scalar
    const int lr = lane & 15, lg = lane >> 4;
    unsigned char* sw = smem + wave * GRAM_STEP * GRAM_RS;          // this wave's 32-row tile

    const i64 nsteps = (M + GRAM_STEP - 1) / GRAM_STEP;
    i64 sbeg = ((i64)blockIdx.x * GRAM_WAVES + wave) * steps_per_wave;
    i64 send = sbeg + steps_per_wave;
    if (send > nsteps) send = nsteps;
    if (sbeg > send) sbeg = send;
    i64 row_end = send * GRAM_STEP;                                  // rows of this wave: [sbeg * 32, row_end)
    if (row_end > M) row_end = M;

    f32x4_t acc[GRAM_TILES], sacc[4];
    double acc64[GRAM_TILES][4], s64[4];
#pragma unroll
    for (int t = 0; t < GRAM_TILES; ++t) {
        acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc64[t][r] = 0.0;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) { sacc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f}; s64[b] = 0.0; }

    auto fold = [&]() {
#pragma unroll
        for (int t = 0; t < GRAM_TILES; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc64[t][r] += (double)acc[t][r];
            acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) { s64[b] += (double)sacc[b][0]; sacc[b] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }      // (every row of a ones product is the column sum)
    };

    if (sbeg < send) {
        // a lane's four 16-byte chunks of a step: rows (lane >> 3) + 8 i, channels 8 (lane & 7) ..
        const int lrow = lane >> 3, lcol = (lane & 7) * 8;
        const i64 last = send - 1;
        uint4 regs[GRAM_SETS][4];
        auto issue = [&](uint4 (&r)[4], i64 s) {                     // loads only: nothing here looks at what arrives
            if (s > last) s = last;                                  // (past the range: a line this wave has already fetched)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                i64 row = s * GRAM_STEP + lrow + 8 * i;
                if (row > M - 1) row = M - 1;
                r[i] = *reinterpret_cast<const uint4*>(a0 + row * ld + lcol);
            }
        };
        auto stage = [&](const uint4 (&r)[4], i64 s) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const i64 row = s * GRAM_STEP + lrow + 8 * i;
                const uint4 v = row < row_end ? r[i] : make_uint4(0, 0, 0, 0);
                *reinterpret_cast<uint4*>(sw + (lrow + 8 * i) * GRAM_RS + lcol * 2) = v;
            }
        };
        const bf16x8_t ones = bf16x8_t{0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80, 0x3F80};
        auto compute = [&]() {
            // transposed fragments: lane 4q + p of each 16-lane group addresses row 8 lg + 4 h + q, channels 4 p .. 4 p + 3
            const int q = lr >> 2, p = lr & 3;
            const int rb = 8 * lg + q;
            bf16x8_t f[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int colb = (b * 16 + 4 * p) * 2;
                auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sw + rb * GRAM_RS + colb));
                auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)(sw + (rb + 4) * GRAM_RS + colb));
                f[b] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            int t = 0;
#pragma unroll
            for (int bi = 0; bi < 4; ++bi)
#pragma unroll
                for (int bj = bi; bj < 4; ++bj, ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f[bi], f[bj], acc[t], 0, 0, 0);
#pragma unroll
            for (int b = 0; b < 4; ++b) sacc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, f[b], sacc[b], 0, 0, 0);
        };
        // The tile belongs to this wave alone and a wave's LDS instructions execute in order, so the stores of a step, its
        // transposed reads and the next step's stores need no barrier between waves — only the compiler must keep their order
        // (other lanes' stores feed this lane's reads)
#define GRAM_LDS_ORDER() do { asm volatile("" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)
#pragma unroll
        for (int u = 0; u < GRAM_SETS; ++u) {                       // (in the order they are consumed: the waits below count loads)
            issue(regs[u], sbeg + u);
            asm volatile("" ::: "memory");
        }
        // (a step past `send` inside the last group adds zeros: the trip count is the only thing that depends on the range)
        int groups = 0;
        for (i64 s = sbeg; s < send; s += GRAM_SETS) {
#pragma unroll
            for (int u = 0; u < GRAM_SETS; ++u) {
                stage(regs[u], s + u);
                GRAM_LDS_ORDER();
                issue(regs[u], s + u + GRAM_SETS);
                compute();
                GRAM_LDS_ORDER();
            }
            if (++groups == GRAM_FOLD_GROUPS) { fold(); groups = 0; }
        }
        fold();
#undef GRAM_LDS_ORDER
    }

    // the workgroup's partial: the waves add their fp64 values in wave order (a fixed order) into one image [slot][lane]
    __syncthreads();                                                 // every wave is done with its staging tile
    double* red = reinterpret_cast<double*>(smem);
    for (int w = 0; w < GRAM_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int t = 0; t < GRAM_TILES; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = (t * 4 + r) * 64 + lane;
                    red[k] = w == 0 ? acc64[t][r] : red[k] + acc64[t][r];
                }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int k = (4 * GRAM_TILES + b) * 64 + lane;
                red[k] = w == 0 ? s64[b] : red[k] + s64[b];
            }
        }
        __syncthreads();
    }
    // flush: accumulator register r of lane (c, g) of tile (bi, bj) is G[16 bi + 4 g + r][16 bj + c]
    DET_ENTER();
    double* out = gram + (i64)(blockIdx.x % (unsigned)nrep) * ((GRAM_C + 8) * GRAM_C);
    for (int k = tid; k < GRAM_SLOTS * 64; k += GRAM_THREADS) {
        const int slot = k >> 6, l = k & 63, c = l & 15, g = l >> 4;
        if (slot < 4 * GRAM_TILES) {
            int bi, bj;
            gram_tile_of(slot >> 2, bi, bj);
            atomicAdd(out + (bi * 16 + g * 4 + (slot & 3)) * GRAM_C + bj * 16 + c, red[k]);
        } else if (g == 0) {
            atomicAdd(out + GRAM_C * GRAM_C + (slot - 4 * GRAM_TILES) * 16 + c, red[k]);
        }
    }
    DET_EXIT();
}
}  // namespace

// how many replicas of [(Cin + 8)][Cin] doubles the Gram pass of (dtype, Cin) accumulates into (the caller zeroes them all);
// 1 = the gemm_tn route, full matrix in one replica
int gram_nrep(int dtype, int Cin) { return (dtype == DWN_BF16 && Cin == GRAM_C) ? DWN_GRAM_NREP : 1; }

// raw products [a0 | 1]^T a0 -> gram (gram_nrep(dtype, Cin) zeroed replicas); false in *done when this shape is not built here
int k_gram(const void* a0, i64 ld, i64 M, int Cin, double* gram, int dtype, bool* done, hipStream_t s) {
    *done = false;
    if (gram_nrep(dtype, Cin) == 1 || M <= 0) return 0;
    if (ld < Cin || ld % 8 || ((size_t)a0 & 15)) return dwn_set_error(-2, "gram: a0 must be 16-byte aligned with ld >= Cin a multiple of 8");
    const i64 nsteps = (M + GRAM_STEP - 1) / GRAM_STEP;
    const int bpc = resident_bpc(gram64_kernel, GRAM_THREADS, 0, 1);
    // one resident round; one workgroup per CU is the form the flush is sized for (a second one would double the adders)
    const i64 grid = resident_grid_x(bpc > 1 ? 1 : bpc, 1, (nsteps + GRAM_WAVES * GRAM_MIN_STEPS - 1) / (GRAM_WAVES * GRAM_MIN_STEPS));
    const i64 waves = grid * GRAM_WAVES;
    const i64 steps_per_wave = (nsteps + waves - 1) / waves;
    hipLaunchKernelGGL(gram64_kernel, dim3((unsigned)grid), dim3(GRAM_THREADS), 0, s, reinterpret_cast<const bf16_t*>(a0), ld, M,
                       steps_per_wave, gram, DWN_GRAM_NREP);
    DWN_CHECK_LAUNCH();
    *done = true;
    return 0;
}

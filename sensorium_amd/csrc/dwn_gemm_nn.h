// MFMA GEMM kernels for the point-wise (1x1x1) convolutions, cortex / readout grouped Conv1d and
// their weight gradients (reference call sites: src/models/dwiseneuro.py:91,118,207,276).
//
//  * gemm_nn : C[M][N] = load(A)[M][K] . B[N][K]^T.  M is the huge (b,t,h,w) dimension, K and N are
//    channel counts (64..4096).  The A operand goes global -> registers -> LDS so that the
//    producer's BN/SiLU/SE-gate/positional-encoding/BN-backward affine is applied in flight
//    (dwn_common.h loaders); the epilogue stages the tile through LDS so every global store is a full
//    contiguous row segment, and folds in the batch-norm Σ/Σ² of the *next* BN.
//    Two instantiations: resident-B (K <= one k-tile; weights stay in LDS, the next tile's rows are prefetched
//    under the MFMAs and the epilogue, branch-free fast epilogue so the compiler's vmcnt counts are exact) and
//    k-loop (next k-tile, or the next tile's first k-tile under the epilogue).  Staging is split into an issue
//    phase (raw registers) and a write phase (prologue math + ds_write) after the MFMAs.
//  * gemm_tn : dW[R][Cc] += load(P)^T . load(Q), contraction over M, split over exactly one resident round of
//    workgroups with fp32 atomics, XCD-aware tile order.  bf16 fragments come from row-major LDS tiles through
//    ds_read_b64_tr_b16.
//
// MFMA shapes: v_mfma_f32_16x16x32_bf16 (bf16 storage) and v_mfma_f32_16x16x4_f32 (fp32 parity
// mode, bit-exact fp32 FMA chain).  Operand maps (cdna_hip_programming.md §3): lane l holds
// A[row l&15][k = 8*(l>>4)+j], B[k = 8*(l>>4)+j][col l&15]; C/D: col = l&15, row = 4*(l>>4)+reg.
//
// Files: this header holds gemm_nn (kernel and launchers); the dwn_gemm_nn_*.hip files compile its instantiations (NN_COMBOS at the
// end), dwn_gemm.hip chooses among them on the host; gemm_tn lives in dwn_gemm_tn.hip.
#pragma once
#include "dwn_internal.h"
#include "dwn_launch.h"
#include <type_traits>

#ifndef NN_DMA_NST
#define NN_DMA_NST 3                 // stages of the LDS-DMA ring of gemm_nn_kernel<..., 3>
#endif
// fp32 products of gemm_nn on the bf16 matrix cores: every operand element is split into hi = bf16(x) and lo = bf16(x - hi) when
// it is staged into LDS, and a product is hi*hi + hi*lo + lo*hi accumulated in fp32 (three v_mfma_f32_16x16x32_bf16 per 32-deep
// k-tile and 16x16 block instead of eight v_mfma_f32_16x16x4_f32: a sixth of the matrix-core time; the dropped lo*lo term and the
// 16-17 significant bits of hi + lo leave a relative error of ~1e-5 per product, far inside the 1e-3 bar of the fp32 path).
// 0 = the native fp32 MFMA.
#ifndef NN_F32_X3
#define NN_F32_X3 1
#endif

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                      __builtin_bit_cast(bf16x8_t, b), acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    // one 16-byte chunk = 4 k-values per lane group; MFMA e consumes element e of every lane group
    static __device__ __forceinline__ void run(const uint4& a, const uint4& b, f32x4_t& acc) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    }
};

template <int KIND, typename T>
__device__ __forceinline__ uint4 load_op_packed(const LoadDesc& d, i64 row, int col) {
    if constexpr (KIND == LD_PLAIN) {
        return *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(d.p) + row * d.ld + col);
    } else {
        float v[TT<T>::KC];
        load_op<KIND, T>(d, row, col, v);
        return pack16<T>(v);
    }
}

// LDS-DMA: 64 lanes x 16 bytes land at lds_dst + 16 * lane (lds_dst wave-uniform); the source address is per lane.
// Invisible to the compiler's s_waitcnt bookkeeping: the consumer waits with an explicit s_waitcnt vmcnt.
static __device__ __forceinline__ void nn_glds16(const void* gsrc, unsigned lds_dst) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
// workgroup barrier for LDS hand-offs only (no vector-memory drain: DMA loads and stores stay in flight across it)
static __device__ __forceinline__ void nn_lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// bf16x3 staging of four fp32 k-values (16-byte chunk kc of a 32-deep tile row): hi halves to logical chunk kc/2 (bytes 8*(kc&1)..),
// lo halves to logical chunk 4 + kc/2; logical chunks are XOR-swizzled with the row like the plain layout
__device__ __forceinline__ void x3_store(unsigned char* rowp, int row, int kc, const uint4& v) {
    const float f0 = __uint_as_float(v.x), f1 = __uint_as_float(v.y), f2 = __uint_as_float(v.z), f3 = __uint_as_float(v.w);
    const unsigned h01 = pk_bf16(f0, f1), h23 = pk_bf16(f2, f3);
    const float r0 = f0 - __uint_as_float(h01 << 16), r1 = f1 - __uint_as_float(h01 & 0xffff0000u);
    const float r2 = f2 - __uint_as_float(h23 << 16), r3 = f3 - __uint_as_float(h23 & 0xffff0000u);
    const int ch = kc >> 1, off = (kc & 1) * 8;
    *reinterpret_cast<uint2*>(rowp + ((ch ^ (row & 7)) << 4) + off) = make_uint2(h01, h23);
    *reinterpret_cast<uint2*>(rowp + (((4 + ch) ^ (row & 7)) << 4) + off) = make_uint2(pk_bf16(r0, r1), pk_bf16(r2, r3));
}

// ------------------------------------------------------------------------------------------------
// NN — persistent: a workgroup owns one N-tile and a contiguous range of M-tiles.
//   * K <= one k-tile (the point-wise expand convs, K = 64 bf16): the weight tile is loaded once and stays
//     in LDS; the next M-tile's A rows are fetched (with their prologue) while the current tile is multiplied
//     and stored.
//   * MFMA operand roles are swapped (weights = A operand, activations = B operand) so that a lane's 4
//     accumulator registers are 4 *consecutive output channels* of one row: the tile is staged to LDS with
//     8/16-byte writes and leaves as whole 16-byte row segments.
//   * BN Σ/Σ² (and the SE gate gradient) are accumulated in registers across all tiles of the range and
//     flushed once per workgroup — per-tile global atomics on the same few hundred addresses serialise at
//     the memory side (MI355X_MICROARCH.md § Global float atomics, "contention").
// ------------------------------------------------------------------------------------------------
template <typename T, int ALD, int EPI, int BN, int SINGLE, bool SPLIT = false>
__global__ __launch_bounds__(256, 2) void gemm_nn_kernel(const GemmNN g) {
    constexpr int KC = TT<T>::KC;
    constexpr bool RO = EPI == EPI_READOUT || EPI == EPI_READOUT_LB;     // the readout epilogue, beta as an argument or in device memory
    constexpr int BM = 128;
    constexpr int ROWB = 128;                          // bytes per tile row per k-step
    constexpr int BK = ROWB / (int)sizeof(T);          // 64 bf16 / 32 f32
    constexpr bool X3 = !TT<T>::IS_BF16 && SPLIT;
    constexpr int NJ = BN / 32;                        // 16-column sub-tiles per wave (2x2 waves)
    constexpr int A_CH = BM * 8 / 256;
    constexpr int B_CH = BN * 8 / 256;
    constexpr int CROW = BN * (int)sizeof(T) + ((SINGLE == 3 && NN_DMA_NST >= 4) ? 0 : 16);     // epilogue staging row stride (bytes)
    // rows staged per epilogue pass (bf16: the whole tile in one pass — except the dh3 epilogue at 128 columns, whose per-pass
    // y3 prefetch (CROWS * CPR / 256 16-byte registers) on top of 64 accumulators spills at 128 rows: 64, or 32 in the k-loop form)
    constexpr int CROWS = TT<T>::IS_BF16 ? ((EPI == EPI_DH3 && BN == 128) ? (SINGLE == 0 ? 32 : 64) : 128) : 32;
    constexpr int NPASS = BM / CROWS;
    constexpr int CPR = BN / KC;                       // 16-byte chunks per output row
    // resident variants hold NKT k-tiles of both operands (SINGLE == 2: K <= two k-tiles); with 128 columns the
    // epilogue staging then aliases the A tiles (two workgroups per CU need <= 80 KB each) — the next tile's A rows
    // wait in registers until the epilogue is over, so nothing else touches that memory meanwhile
    constexpr int NKT = SINGLE == 2 ? 2 : 1;
    // SINGLE == 3: k-loop whose operand tiles arrive by LDS-DMA (global_load_lds_dwordx4, plain loaders, bf16, K % 64 == 0)
    // into a ring of NST stages: the loads of k-tile s+2 are issued before the MFMAs of k-tile s, across tile boundaries
    // and under the epilogue, with no staging registers.  One workgroup per CU (131 KB).  For the shapes whose k-loop is a
    // serial chain of HBM round trips: few M-tiles per workgroup and a long K (blocks 7-8, cortex, readouts).
    constexpr bool DMA = SINGLE == 3;
    // NN_DMA_NST = 4: three k-tiles in flight instead of two (96 KB per CU).  The epilogue staging then ALIASES the ring stage
    // the tile's last MFMAs have just released (the next load into it is issued at the next tile's first k-step, after the
    // epilogue's closing barrier); it is exactly one stage when its rows carry no padding, so the bank stagger of the
    // column-strided accumulator writes comes from an XOR swizzle of the 16-byte chunk index with the row instead.
    constexpr int NST = DMA ? NN_DMA_NST : 3;
    constexpr bool SC_ALIAS = DMA && NST >= 4;
    constexpr int SA_BYTES = NKT * BM * ROWB, SB_BYTES = NKT * BN * ROWB, SC_BYTES = CROWS * CROW;
    constexpr int STG_BYTES = SA_BYTES + SB_BYTES;
    constexpr bool ALIAS_C = (NKT == 2 && BN == 128);
    constexpr int R0_BYTES = ALIAS_C ? (SA_BYTES > SC_BYTES ? SA_BYTES : SC_BYTES) : SA_BYTES;
    static_assert(!SC_ALIAS || SC_BYTES <= STG_BYTES, "the aliased epilogue staging must fit one ring stage");
    constexpr int SMEM_BYTES = DMA ? NST * STG_BYTES + (SC_ALIAS ? 0 : SC_BYTES) : R0_BYTES + SB_BYTES + (ALIAS_C ? 0 : SC_BYTES);
    __shared__ __attribute__((aligned(16))) unsigned char smem_nn[SMEM_BYTES];
    unsigned char* const sA = smem_nn;
    unsigned char* const sB = smem_nn + (DMA ? SA_BYTES : R0_BYTES);
    unsigned char* sC = DMA ? smem_nn + (SC_ALIAS ? 0 : NST * STG_BYTES) : (ALIAS_C ? smem_nn : smem_nn + R0_BYTES + SB_BYTES);
    // byte offset of (row r, byte b of the row) in the staging tile
    auto sc_off = [&](int r, int b) -> int {
        if constexpr (SC_ALIAS) return r * CROW + ((((b >> 4) ^ (r & (CPR < 16 ? CPR - 1 : 15))) << 4) | (b & 15));
        else return r * CROW + b;
    };
    __shared__ float lred[2 * BN];

    const int tid = threadIdx.x;
    const int ntn = (g.N + BN - 1) / BN;
    const int ntm = (g.M + BM - 1) / BM;
    // XCD-aware order (gridDim.x is a multiple of 8; blocks b and b+8 share an XCD's L2): the N-tiles of one
    // M-range re-read the same A rows, so they get consecutive slots of one XCD.  M-ranges interleave over the XCDs
    // when their count allows it, and the M-tiles are split evenly (range sizes differ by at most one tile).
    // Per-sample weight matrices (the gated project conv): an XCD takes a CONTIGUOUS run of M-ranges instead, so that its
    // L2 only ever holds the weights of the few samples it is working on (32 samples x N x K do not fit one L2;
    // measured -5 % on blocks 4-8).
    const int bid = blockIdx.x;
    const int nranges = (int)(gridDim.x / ntn);
    int nt, mr;
    if (ntm < ntn) {
        // few M-tiles, many N-tiles (cortex, readouts: M = batch x frames): the weights are the big operand, so an XCD
        // takes a contiguous run of N-tiles with ALL their M-ranges -- each weight tile crosses the fabric once
        const int lid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);
        mr = lid % nranges;
        nt = lid / nranges;
    } else if ((nranges & 7) == 0 && !g.b_sample_stride) {
        const int jj = bid >> 3;
        nt = jj % ntn;
        mr = (jj / ntn) * 8 + (bid & 7);
    } else {
        const int lid = (bid & 7) * (int)(gridDim.x >> 3) + (bid >> 3);
        nt = lid % ntn;
        mr = lid / ntn;
    }
    const int mt_beg = (int)((i64)mr * ntm / nranges);
    const int mt_end = (int)((i64)(mr + 1) * ntm / nranges);
    if (mt_beg >= mt_end) { DET_EXIT(); return; }
    // (deterministic build) the dg epilogue adds to global words from inside the tile loop: the workgroup holds the ticket throughout
    if constexpr (EPI == EPI_DG) DET_ENTER();
    const int grp = blockIdx.y;
    const int n0 = nt * BN;
    const int acol0 = grp * g.K;
    const T* Bp = reinterpret_cast<const T*>(g.b) + (i64)grp * g.N * g.ldb;
    const int ccol0 = grp * g.N;
    // SINGLE (K <= one k-tile) is a separate instantiation: sharing one loop nest between the resident-B and the
    // k-loop variants made the compiler merge their s_waitcnt scoreboards and drain every prefetch early
    constexpr bool single = SINGLE == 1 || SINGLE == 2;

    // Staging is split in two (cdna_hip_programming.md "Async-STAGE split"): load_* only ISSUES the global loads into
    // raw registers; the prologue math, the bounds select and the ds_write happen in store_*, after the MFMAs of the
    // current tile.  (Selecting / converting inside load_* makes the compiler wait for the data before the MFMAs.)
    uint4 rp[NKT * A_CH], rq[NKT * A_CH], rb[NKT * B_CH];
    int ld_m0 = 0, ld_k0 = 0, ldb_k0 = 0;
    // A staging: this thread's 16-byte column chunk (kc = tid & 7) is the same for its A_CH rows, so the
    // per-channel prologue coefficients are loaded once per k-tile, not once per chunk
    ColCoef<ALD == LD_PE ? LD_PLAIN : ALD, T> cf;
    int cf_k = -1;
    const T* Ap = reinterpret_cast<const T*>(g.a.p);
    const T* Aq = reinterpret_cast<const T*>(g.a.q);
    auto load_a = [&](int m0, int k0) {
        ld_m0 = m0; ld_k0 = k0;
        const int kc = tid & 7;
        const int k = k0 + kc * KC;
        const bool kok = k < g.K;
        if constexpr (ALD == LD_PE) {
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                int m = m0 + (tid >> 3) + 32 * i;
                rp[i] = (m < g.M && kok) ? load_op_packed<LD_PE, T>(g.a, (i64)m, acol0 + k) : make_uint4(0, 0, 0, 0);
            }
        } else if (EPI == EPI_STORE_CAT && k >= g.K1) {
            // K-concatenated second operand (plain): A[m][k] = a2[m][k - K1]
            const T* A2p = reinterpret_cast<const T*>(g.a2);
#pragma unroll
            for (int i = 0; i < A_CH; ++i) {
                int m = m0 + (tid >> 3) + 32 * i;
                const bool ok = m < g.M && kok;
                rp[i] = *reinterpret_cast<const uint4*>(A2p + (ok ? (i64)m * g.a2_ld + (k - g.K1) : 0));
            }
        } else {
            if (kok && k != cf_k) { cf.load(g.a, acol0 + k); cf_k = k; }
#pragma unroll
            for (int kt = 0; kt < NKT; ++kt) {
                const int kq = k + kt * BK;                  // NKT == 2: plain loaders only (no per-k coefficients)
                const bool kqok = kq < g.K;
#pragma unroll
                for (int i = 0; i < A_CH; ++i) {
                    int m = m0 + (tid >> 3) + 32 * i;
                    const bool ok = m < g.M && kqok;
                    const i64 off = ok ? (i64)m * g.a.ld + acol0 + kq : 0;
                    rp[kt * A_CH + i] = *reinterpret_cast<const uint4*>(Ap + off);
                    if constexpr (decltype(cf)::two_tensors) rq[kt * A_CH + i] = *reinterpret_cast<const uint4*>(Aq + off);
                }
            }
        }
    };
    // m0b: first row of the tile the weights are for (selects the sample with per-sample weight matrices)
    auto load_b = [&](int k0, int m0b = 0) {
        ldb_k0 = k0;
        const T* Bt = Bp;
        if (g.b_sample_stride) Bt += (i64)(m0b / g.b_rows_per_sample) * g.b_sample_stride;
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int i = 0; i < B_CH; ++i) {
                int c = tid + 256 * i;
                int row = c >> 3, kc = c & 7;
                int n = n0 + row, k = k0 + kt * BK + kc * KC;
                const bool ok = n < g.N && k < g.K;
                rb[kt * B_CH + i] = *reinterpret_cast<const uint4*>(Bt + (ok ? (i64)n * g.ldb + k : 0));
            }
    };
    auto store_a = [&]() {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
        const int kk = ld_k0 + kt * BK + (tid & 7) * KC;
        const bool kok = kk < g.K;
#pragma unroll
        for (int i = 0; i < A_CH; ++i) {
            int c = tid + 256 * i;
            int row = c >> 3, kc = c & 7;
            const int m = ld_m0 + row;
            const bool ok = m < g.M && kok;
            uint4 v;
            if constexpr (ALD == LD_PE) v = rp[kt * A_CH + i];
            else if (EPI == EPI_STORE_CAT && kk >= g.K1) v = ok ? rp[kt * A_CH + i] : make_uint4(0, 0, 0, 0);
            else {
                if constexpr (decltype(cf)::two_tensors) v = ok ? cf.apply(g.a, (unsigned)m, rp[kt * A_CH + i], rq[kt * A_CH + i]) : make_uint4(0, 0, 0, 0);
                else v = ok ? cf.apply(g.a, (unsigned)m, rp[kt * A_CH + i], make_uint4(0, 0, 0, 0)) : make_uint4(0, 0, 0, 0);
            }
            if constexpr (X3) x3_store(sA + kt * (BM * ROWB) + row * ROWB, row, kc, v);
            else *reinterpret_cast<uint4*>(sA + kt * (BM * ROWB) + row * ROWB + ((kc ^ (row & 7)) << 4)) = v;
        }
        }
    };
    auto store_b = [&]() {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int i = 0; i < B_CH; ++i) {
                int c = tid + 256 * i;
                int row = c >> 3, kc = c & 7;
                const bool ok = (n0 + row) < g.N && (ldb_k0 + kt * BK + kc * KC) < g.K;
                if constexpr (X3) x3_store(sB + kt * (BN * ROWB) + row * ROWB, row, kc, ok ? rb[kt * B_CH + i] : make_uint4(0, 0, 0, 0));
                else *reinterpret_cast<uint4*>(sB + kt * (BN * ROWB) + row * ROWB + ((kc ^ (row & 7)) << 4)) =
                    ok ? rb[kt * B_CH + i] : make_uint4(0, 0, 0, 0);
            }
    };

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 15, lg = lane >> 4;
    f32x4_t acc[4][NJ];

    auto mma_tile = [&](const int stage_off = 0) {
        if constexpr (X3) {
            // one 32-deep k-tile per NKT: hi fragments in 16-byte chunks 0-3 of a row (8 consecutive k each), lo in chunks 4-7
#pragma unroll
            for (int kb = 0; kb < NKT; ++kb) {
                uint4 ah[4], al[4], bh[NJ], bl[NJ];
                const unsigned char* tA = sA + stage_off + kb * (BM * ROWB);
                const unsigned char* tB = sB + stage_off + kb * (BN * ROWB);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = wm * 64 + i * 16 + lr;
                    ah[i] = *reinterpret_cast<const uint4*>(tA + row * ROWB + ((lg ^ (row & 7)) << 4));
                    al[i] = *reinterpret_cast<const uint4*>(tA + row * ROWB + (((4 + lg) ^ (row & 7)) << 4));
                }
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const int row = wn * (BN / 2) + j * 16 + lr;
                    bh[j] = *reinterpret_cast<const uint4*>(tB + row * ROWB + ((lg ^ (row & 7)) << 4));
                    bl[j] = *reinterpret_cast<const uint4*>(tB + row * ROWB + (((4 + lg) ^ (row & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        // small terms first
                        Mma<bf16_t>::run(bl[j], ah[i], acc[i][j]);
                        Mma<bf16_t>::run(bh[j], al[i], acc[i][j]);
                        Mma<bf16_t>::run(bh[j], ah[i], acc[i][j]);
                    }
            }
            return;
        }
#pragma unroll
        for (int kb = 0; kb < 2 * NKT; ++kb) {
            uint4 af[4], bfr[NJ];
            const int chunk = (kb & 1) * 4 + lg;
            const unsigned char* tA = sA + stage_off + (kb >> 1) * (BM * ROWB);
            const unsigned char* tB = sB + stage_off + (kb >> 1) * (BN * ROWB);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                int row = wm * 64 + i * 16 + lr;
                af[i] = *reinterpret_cast<const uint4*>(tA + row * ROWB + ((chunk ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                int row = wn * (BN / 2) + j * 16 + lr;
                bfr[j] = *reinterpret_cast<const uint4*>(tB + row * ROWB + ((chunk ^ (row & 7)) << 4));
            }
            // swapped roles: D[n = 4*lg + r][m = lr] — acc[i][j][r] = C[m = i*16 + lr][n = j*16 + 4*lg + r]
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j) Mma<T>::run(bfr[j], af[i], acc[i][j]);
        }
    };

    // read-back role of this thread: one 16-byte column chunk, rows tid/CPR + k*(256/CPR)
    const int ch = tid % CPR;
    const int ncol = n0 + ch * KC;
    // a valid chunk of the same row for lanes past N (fast epilogue path): N % KC == 0, n0 < N
    const int nvalid_ch = (g.N - n0) / KC < CPR ? (g.N - n0) / KC : CPR;
    const int ch_e = ch < nvalid_ch ? ch : ch % nvalid_ch;
    const int ncol_e = n0 + ch_e * KC;
    float st0[KC], st1[KC], dgp[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) { st0[i] = 0.f; st1[i] = 0.f; dgp[i] = 0.f; }
    [[maybe_unused]] int dg_b = -1;                    // sample whose partial sums dgp currently holds
    T* Cp = reinterpret_cast<T*>(g.c);
    // EPI_DH3: this thread's column chunk never changes — BatchNorm-3 scale / shift / mean / invstd stay in registers
    // (scale / shift only; the second BatchNorm-backward sum is accumulated as sum(dh3 * y3) and centred once, when
    // the workgroup flushes — keeping mean / invstd live through the tile loop spills)
    [[maybe_unused]] float sc3[KC], sh3[KC];
    if constexpr (EPI == EPI_DH3) {
        ld_coef<KC>(g.coef3 + ncol_e, sc3);
        ld_coef<KC>(g.coef3 + (i64)g.coef3_ld + ncol_e, sh3);
    }
    [[maybe_unused]] float gt3[KC], gp3[KC];           // SE gate / pooled-gradient rows of sample gb3
    [[maybe_unused]] int gb3 = -1;
    constexpr bool NEEDY = (EPI == EPI_DG || EPI == EPI_DH3);     // the epilogue reads a second [M][N] tensor (g.y3)

    // epilogue barriers hand over LDS only; the DMA variant must not drain the k-tiles in flight for the next tile
    auto bar = [&]() {
        if constexpr (DMA) nn_lds_barrier();
        else __syncthreads();
    };
    // flush dgp (sample dg_b) through LDS: one global atomic per column per workgroup
    auto flush_dg = [&]() {
        if (tid < BN) lred[tid] = 0.f;
        bar();
        DET_WAVES_BEGIN
        if (ncol < g.N) {
#pragma unroll
            for (int i = 0; i < KC; ++i) atomicAdd(&lred[ch * KC + i], dgp[i]);
        }
        DET_WAVES_END
        bar();
        if (tid < BN && n0 + tid < g.N && dg_b >= 0) atomicAdd(g.dg + (i64)dg_b * g.dg_ld + n0 + tid, lred[tid]);
        bar();
#pragma unroll
        for (int i = 0; i < KC; ++i) dgp[i] = 0.f;
    };

    // ---- LDS-DMA ring (SINGLE == 3).  A wave's load instruction fills 8 tile rows (64 lanes x 16 B, contiguous in LDS from
    // a wave-uniform base); the XOR swizzle of the tile layout is applied on the SOURCE side (lane -> column chunk).
    // Rows past M / N are clamped to the last valid row: their products land in accumulator rows / columns the epilogue
    // never stores.
    [[maybe_unused]] int is_mt = mt_beg, is_k = 0, is_st = 0, n_issued = 0, n_done = 0;
    [[maybe_unused]] const int nk = g.K / BK;
    [[maybe_unused]] auto dma_issue = [&]() {
        if constexpr (DMA) {
            if (is_mt >= mt_end) return;
            const unsigned lds0 = (unsigned)(size_t)smem_nn + (unsigned)(is_st * STG_BYTES);
            const int r8 = lane >> 3, kc = (lane & 7) ^ r8;
            const int m0i = is_mt * BM, k0 = is_k * BK;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int grp8 = wave * 4 + j;
                int m = m0i + grp8 * 8 + r8;
                m = m < g.M ? m : g.M - 1;
                const T* src;
                if (EPI == EPI_STORE_CAT && k0 >= g.K1) src = reinterpret_cast<const T*>(g.a2) + (i64)m * g.a2_ld + (k0 - g.K1) + kc * KC;
                else src = Ap + (i64)m * g.a.ld + acol0 + k0 + kc * KC;
                nn_glds16(src, (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + (unsigned)grp8 * 1024u)));
            }
            const T* Bt = Bp;
            if (g.b_sample_stride) Bt += (i64)(m0i / g.b_rows_per_sample) * g.b_sample_stride;
#pragma unroll
            for (int j = 0; j < BN / 32; ++j) {
                const int grp8 = wave * (BN / 32) + j;
                int n = n0 + grp8 * 8 + r8;
                n = n < g.N ? n : g.N - 1;
                nn_glds16(Bt + (i64)n * g.ldb + k0 + kc * KC,
                          (unsigned)__builtin_amdgcn_readfirstlane((int)(lds0 + (unsigned)SA_BYTES + (unsigned)grp8 * 1024u)));
            }
            ++n_issued;
            is_st = is_st == NST - 1 ? 0 : is_st + 1;
            if (++is_k == nk) { is_k = 0; ++is_mt; }
        }
    };
    [[maybe_unused]] int cs_st = 0;                    // ring stage of the k-tile consumed next

    if constexpr (single) {
        load_b(0);
        store_b();
        load_a(mt_beg * BM, 0);
        store_a();
        __syncthreads();
    }
    // One tile, specialised at compile time on HN (a next tile exists: prefetch its A rows / stage them afterwards;
    // resident-B variant only) and on `fast` (see the epilogue).  The copies keep every path between the prefetch loads
    // and their use free of data-dependent branches, so the compiler's s_waitcnt vmcnt(N) counts are exact.
    auto tile = [&](const int mt, auto hn_c, auto fast_c) {
        [[maybe_unused]] constexpr bool HN = decltype(hn_c)::value;
        const int m0 = mt * BM;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        // EPI_DH3 fast path: the whole tile lies in one sample — its SE gate and pooled-gradient rows are fetched here,
        // under the MFMAs, not at the head of the epilogue
        if constexpr (EPI == EPI_DH3 && decltype(fast_c)::value) {
            const int b = m0 / g.rows_per_sample;
            if (b != gb3) {
                ld_coef<KC>(g.gate3 + (i64)b * g.dg_ld + ncol_e, gt3);
                ld_coef<KC>(g.dps3 + (i64)b * g.dg_ld + ncol_e, gp3);
                gb3 = b;
            }
        }
        if constexpr (DMA) {
            for (int kt = 0; kt < nk; ++kt) {
                // this wave's loads of the consumed k-tile have landed once at most the next k-tile's are outstanding
                // (loads retire in order; the epilogue's younger stores only make the wait stricter)
                if constexpr (NST >= 4) {
                    if (n_issued - n_done > 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (4 + BN / 32)) : "memory");
                    else if (n_issued - n_done > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + BN / 32) : "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else {
                    if (n_issued - n_done > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + BN / 32) : "memory");
                    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                nn_lds_barrier();                               // every wave's part landed; everyone is past the previous MFMAs
                dma_issue();                                    // k-tile +2 into the stage the previous MFMAs just released
                mma_tile(cs_st * STG_BYTES);
                ++n_done;
                cs_st = cs_st == NST - 1 ? 0 : cs_st + 1;
            }
            if constexpr (SC_ALIAS) {
                // the stage just consumed is free until the next tile's first k-step issues into it
                sC = smem_nn + (cs_st == 0 ? NST - 1 : cs_st - 1) * STG_BYTES;
                nn_lds_barrier();                               // every wave is done reading that stage
            }
        } else if constexpr (single) {
            if constexpr (HN) load_a((mt + 1) * BM, 0);         // in flight under the MFMAs and the epilogue
            mma_tile();
        } else {
            // this tile's first k-tile was issued before the previous tile's epilogue (or before the loop)
            store_a();
            store_b();
            __syncthreads();
            for (int k0 = 0; k0 < g.K; k0 += BK) {
                const bool has_next = (k0 + BK) < g.K;
                if (has_next) { load_a(m0, k0 + BK); load_b(k0 + BK, m0); }
                else if (mt + 1 < mt_end) { load_a(m0 + BM, 0); load_b(0, m0 + BM); }   // next tile: in flight under the epilogue
                mma_tile();
                __syncthreads();
                if (has_next) {
                    store_a();
                    store_b();
                    __syncthreads();
                }
            }
        }

        if constexpr (RO) {
            // out[b][n][t] = softplus_beta(acc + bias[n]); lanes lr = 16 consecutive rows m = b*Tn + t
            // (EPI_READOUT_LB: beta from device memory — a kernel-argument pointer, so one scalar load for the workgroup)
            const float beta = EPI == EPI_READOUT_LB ? *g.sp_beta_dev : g.sp_beta;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    int nl = n0 + wn * (BN / 2) + j * 16 + lg * 4 + r;
                    int n = ccol0 + nl;
                    if (nl >= g.N || n >= g.n_valid) continue;
                    float bias = g.bias ? g.bias[n] : 0.f;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        int m = m0 + wm * 64 + i * 16 + lr;
                        if (m >= g.M) continue;
                        float z = acc[i][j][r] + bias;
                        float bz = z * beta;
                        float o = bz > 20.f ? z : log1pf(__expf(bz)) / beta;
                        int b = m / g.Tn, t = m % g.Tn;
                        g.out_nct[((i64)b * g.n_valid + n) * g.Tn + t] = o;
                    }
                }
        } else {
            // ---- stage through LDS in passes of CROWS rows; leave as whole 16-byte row segments
            for (int pass = 0; pass < NPASS; ++pass) {
                const int prow0 = pass * CROWS;            // first tile row of this pass
                const int mp = m0 + prow0;
                // Fast path (every row of the tile valid, and for EPI_DG the pass inside one sample): every global
                // access below is UNCONDITIONAL — lanes past N redo a valid chunk of the same row (idempotent store,
                // their sums are never flushed) — so the compiler counts the stores exactly and the s_waitcnt of the
                // next tile's prefetched A rows (issued before these stores) does not drain them.
                constexpr bool fast = decltype(fast_c)::value;
                [[maybe_unused]] int pb3 = 0, pbound3 = 0;
                if constexpr (EPI == EPI_DH3 && !fast) {
                    pb3 = mp / g.rows_per_sample;
                    pbound3 = (pb3 + 1) * g.rows_per_sample;
                }
                // EPI_DG: fetch this pass's z3 chunks now so they are in flight across the LDS round trip
                [[maybe_unused]] uint4 zraw[CROWS * CPR / 256];
                if constexpr (NEEDY) {
                    if constexpr (fast) {
#pragma unroll
                        for (int it = 0; it < CROWS * CPR / 256; ++it) {
                            const int m = mp + tid / CPR + it * (256 / CPR);
                            zraw[it] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(g.y3) + (i64)m * g.ldy3 + ncol_e);
                        }
                    } else {
#pragma unroll
                        for (int it = 0; it < CROWS * CPR / 256; ++it) {
                            const int m = mp + tid / CPR + it * (256 / CPR);
                            const bool ok = m < g.M && ncol < g.N;
                            zraw[it] = *reinterpret_cast<const uint4*>(reinterpret_cast<const T*>(g.y3) + (ok ? (i64)m * g.ldy3 + ncol : 0));
                        }
                    }
                }
                if constexpr (ALIAS_C) { if (pass == 0) __syncthreads(); }    // every wave is done reading the A tiles
                if (CROWS >= 64 ? (wm == prow0 / 64 || CROWS == 128) : (wm == prow0 / 64)) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int trow = wm * 64 + i * 16 + lr;
                        if (trow >= prow0 && trow < prow0 + CROWS) {
#pragma unroll
                            for (int j = 0; j < NJ; ++j) {
                                const int col = wn * (BN / 2) + j * 16 + lg * 4;
                                unsigned char* dst = sC + sc_off(trow - prow0, col * (int)sizeof(T));
                                if (EPI == EPI_STORE_CAT && n0 + col < g.N) {
                                    const float4 bv = *reinterpret_cast<const float4*>(g.bias + ccol0 + n0 + col);
                                    acc[i][j][0] += bv.x; acc[i][j][1] += bv.y; acc[i][j][2] += bv.z; acc[i][j][3] += bv.w;
                                }
                                if constexpr (TT<T>::IS_BF16) {
                                    uint2 v;
                                    v.x = pk_bf16(acc[i][j][0], acc[i][j][1]);
                                    v.y = pk_bf16(acc[i][j][2], acc[i][j][3]);
                                    *reinterpret_cast<uint2*>(dst) = v;
                                } else {
                                    *reinterpret_cast<float4*>(dst) =
                                        make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
                                }
                            }
                        }
                    }
                }
                bar();
                if constexpr (fast) {
#pragma unroll
                    for (int it = 0; it < CROWS * CPR / 256; ++it) {
                        const int row = tid / CPR + it * (256 / CPR);
                        const int m = mp + row;
                        const uint4 raw = *reinterpret_cast<const uint4*>(sC + sc_off(row, ch_e * 16));
                        float v[KC];
                        unpack16<T>(raw, v);
                        if constexpr (EPI == EPI_DH3) {
                            float y[KC], dh[KC];
                            unpack16<T>(zraw[it], y);
#pragma unroll
                            for (int i = 0; i < KC; ++i) dh[i] = fmaf(y[i], sc3[i], sh3[i]);
                            silu_grad_n<KC>(dh, dh);
#pragma unroll
                            for (int i = 0; i < KC; ++i) dh[i] = fmaf(v[i], gt3[i], gp3[i]) * dh[i];
                            const uint4 packed = pack16<T>(dh);
                            *reinterpret_cast<uint4*>(Cp + (i64)m * g.ldc + ccol0 + ncol_e) = packed;
                            if (g.stats) {
                                float r[KC];
                                unpack16<T>(packed, r);            // the sums use the stored (rounded) values
#pragma unroll
                                for (int i = 0; i < KC; ++i) { st0[i] += r[i]; st1[i] = fmaf(r[i], y[i], st1[i]); }
                            }
                            continue;
                        }
                        *reinterpret_cast<uint4*>(Cp + (i64)m * g.ldc + ccol0 + ncol_e) = raw;
                        if (g.stats) {
#pragma unroll
                            for (int i = 0; i < KC; ++i) { st0[i] += v[i]; st1[i] += v[i] * v[i]; }
                        }
                        if constexpr (EPI == EPI_DG) {
                            float y[KC];
                            unpack16<T>(zraw[it], y);
#pragma unroll
                            for (int i = 0; i < KC; ++i) dgp[i] += v[i] * y[i];
                        }
                    }
                } else {
#pragma unroll
                for (int it = 0; it < CROWS * CPR / 256; ++it) {
                    const int row = tid / CPR + it * (256 / CPR);
                    const int m = mp + row;
                    if (m >= g.M || ncol >= g.N) continue;
                    const uint4 raw = *reinterpret_cast<const uint4*>(sC + sc_off(row, ch * 16));
                    float v[KC];
                    unpack16<T>(raw, v);
                    if constexpr (EPI == EPI_DH3) {
                        // sample of this row without a division per row: a pass crosses at most one boundary
                        // when rows_per_sample >= CROWS (pb3 / pbound3 are per-pass scalars)
                        const int b = g.rows_per_sample >= CROWS ? pb3 + (m >= pbound3 ? 1 : 0) : m / g.rows_per_sample;
                        float y[KC], dh[KC];
                        unpack16<T>(zraw[it], y);
                        if (b != gb3) {                      // rows of one tile almost always share the sample
                            gb3 = b;
                            ld_coef<KC>(g.gate3 + (i64)b * g.dg_ld + ncol, gt3);
                            ld_coef<KC>(g.dps3 + (i64)b * g.dg_ld + ncol, gp3);
                        }
#pragma unroll
                        for (int i = 0; i < KC; ++i) dh[i] = fmaf(y[i], sc3[i], sh3[i]);
                        silu_grad_n<KC>(dh, dh);
#pragma unroll
                        for (int i = 0; i < KC; ++i) dh[i] = fmaf(v[i], gt3[i], gp3[i]) * dh[i];
                        const uint4 packed = pack16<T>(dh);
                        *reinterpret_cast<uint4*>(Cp + (i64)m * g.ldc + ccol0 + ncol) = packed;
                        if (g.stats) {
                            float r[KC];
                            unpack16<T>(packed, r);
#pragma unroll
                            for (int i = 0; i < KC; ++i) { st0[i] += r[i]; st1[i] = fmaf(r[i], y[i], st1[i]); }
                        }
                        continue;
                    }
                    *reinterpret_cast<uint4*>(Cp + (i64)m * g.ldc + ccol0 + ncol) = raw;
                    if (g.stats) {
#pragma unroll
                        for (int i = 0; i < KC; ++i) { st0[i] += v[i]; st1[i] += v[i] * v[i]; }
                    }
                    if constexpr (EPI == EPI_DG) {
                        // a pass straddles a sample boundary only if rows_per_sample % CROWS != 0: the rows of
                        // the minority sample then use direct atomics
                        const int b = m / g.rows_per_sample;
                        float y[KC];
                        unpack16<T>(zraw[it], y);
                        const int b_pass = mp / g.rows_per_sample;
                        if (b == b_pass) {
#pragma unroll
                            for (int i = 0; i < KC; ++i) dgp[i] += v[i] * y[i];
                        } else {
                            // (the deterministic build never takes the dg epilogue: dwn_api.hip routes conv_pwl's backward through
                            // the per-sample products there — several waves add to one word here)
#pragma unroll
                            for (int i = 0; i < KC; ++i) atomicAdd(g.dg + (i64)b * g.dg_ld + ncol + i, v[i] * y[i]);
                        }
                    }
                }
                }
                if constexpr (EPI == EPI_DG) {
                    // dgp belongs to sample b_pass; flush when the next pass starts a different sample (uniform)
                    const int b_pass = mp / g.rows_per_sample;
                    dg_b = b_pass;
                    const int m_next = mp + CROWS;
                    const bool last = (pass == NPASS - 1) && (mt + 1 == mt_end);
                    const int b_next = (m_next < g.M ? m_next : g.M - 1) / g.rows_per_sample;
                    if (last || b_next != b_pass || m_next >= g.M) flush_dg();
                    else bar();
                } else {
                    bar();
                }
            }
        }
        if constexpr (single && HN) {
            if constexpr (RO) __syncthreads();   // no barrier in that epilogue: all waves must be done with sA
            store_a();
            __syncthreads();
        }
    };
    if constexpr (DMA) {
#pragma unroll
        for (int q = 0; q < NST - 1; ++q) dma_issue();
    }
    else if constexpr (!single) { load_a(mt_beg * BM, 0); load_b(0, mt_beg * BM); }
    for (int mt = mt_beg; mt < mt_end; ++mt) {
        const int m0_ = mt * BM;
        bool fast = m0_ + BM <= g.M;
        if constexpr (EPI == EPI_DG || EPI == EPI_DH3) fast = fast && (m0_ / g.rows_per_sample == (m0_ + BM - 1) / g.rows_per_sample);
        if constexpr (RO) fast = false;
        using T_ = std::true_type;
        using F_ = std::false_type;
        if constexpr (single) {
            if (mt + 1 < mt_end) { if (fast) tile(mt, T_{}, T_{}); else tile(mt, T_{}, F_{}); }
            else { if (fast) tile(mt, F_{}, T_{}); else tile(mt, F_{}, F_{}); }
        } else if constexpr (DMA) {
            if (fast) tile(mt, F_{}, T_{}); else tile(mt, F_{}, F_{});
        } else {
            tile(mt, F_{}, F_{});       // k-loop variant: its prefetches live inside the k loop; one generic copy
        }
    }
    if constexpr (!RO) {
        if (g.stats) {
            if constexpr (EPI == EPI_DH3) {            // sum(dh*(y - mean)*invstd) = invstd * (sum(dh*y) - mean*sum(dh))
                float mu3[KC], is3[KC];
                ld_coef<KC>(g.coef3 + 2 * (i64)g.coef3_ld + ncol_e, mu3);
                ld_coef<KC>(g.coef3 + 3 * (i64)g.coef3_ld + ncol_e, is3);
#pragma unroll
                for (int i = 0; i < KC; ++i) st1[i] = is3[i] * fmaf(-mu3[i], st0[i], st1[i]);
            }
            if (tid < 2 * BN) lred[tid] = 0.f;
            __syncthreads();
            DET_WAVES_BEGIN
            if (ncol < g.N) {
#pragma unroll
                for (int i = 0; i < KC; ++i) {
                    atomicAdd(&lred[ch * KC + i], st0[i]);
                    atomicAdd(&lred[BN + ch * KC + i], st1[i]);
                }
            }
            DET_WAVES_END
            __syncthreads();
            DET_ENTER();
            if (tid < 2 * BN) {
                int col = tid % BN, which = tid / BN;
                if (n0 + col < g.N)
                    stat_add(g.stats, (int)(blockIdx.x % DWN_NREP), g.stat_nchan, which, ccol0 + n0 + col, lred[tid]);
            }
        }
    }
    DET_EXIT();
}

template <typename T, int ALD, int EPI, int BNv, int SINGLE>
static int launch_nn_k(const GemmNN& g, hipStream_t s) {
    const int BM = 128;
    const int ntm = (g.M + BM - 1) / BM;
    const int ntn = (g.N + BNv - 1) / BNv;
    // persistent grid = exactly the resident workgroups (256 CUs x blocks/CU from the occupancy query: the unified
    // VGPR+AGPR budget decides, not the arch-VGPR count); every workgroup gets a contiguous range of M-tiles
    // (fallback 1, here and in launch_tn_t: the safe minimum — such a grid never exceeds the resident slots)
    const int bpc = resident_bpc(gemm_nn_kernel<T, ALD, EPI, BNv, SINGLE>, 256, 0, 1);
    // never more workgroups than resident slots (a second partial wave of persistent workgroups doubles the
    // kernel time); nranges * ntn must be a multiple of 8 for the XCD-major logical id
    int nranges = (256 * bpc) / (ntn * g.groups);
    if (nranges > ntm) nranges = ntm;
    if (nranges < 1) nranges = 1;
    while (nranges > 1 && (nranges * ntn) % 8 != 0) --nranges;
    if ((nranges * ntn) % 8 != 0) nranges = 8;
    dim3 grid(nranges * ntn, g.groups);
    if constexpr (!TT<T>::IS_BF16 && NN_F32_X3 != 0) {
        // fp32 products on the bf16 matrix cores (see NN_F32_X3): asked for per call (dwn_gemm_nn_args.f32_split; the eval-mode
        // forward does unless the caller wants the native fp32 MFMA)
        if (g.f32_split != 0) {
            hipLaunchKernelGGL((gemm_nn_kernel<T, ALD, EPI, BNv, SINGLE, true>), grid, dim3(256), 0, s, g);
            DWN_CHECK_LAUNCH();
            return 0;
        }
    }
    hipLaunchKernelGGL((gemm_nn_kernel<T, ALD, EPI, BNv, SINGLE>), grid, dim3(256), 0, s, g);
    DWN_CHECK_LAUNCH();
    return 0;
}

// resident-B single-k-tile instantiations exist for the loaders/epilogues whose hot shapes have K <= one k-tile (the
// point-wise expand conv and the project conv's data gradient); every other combination runs K <= BK through the
// k-loop variant (one step, no prefetch)
template <int ALD, int EPI> struct HasSingle {
    static constexpr bool value = (ALD == LD_PLAIN && (EPI == EPI_STORE || EPI == EPI_DG || EPI == EPI_DH3)) || (ALD == LD_PE && EPI == EPI_STORE);
};
// ... and resident two-k-tile instantiations (K <= 2 k-tiles: the 128-channel blocks) for the plain-loader hot shapes
template <int ALD, int EPI> struct HasSingle2 {
    static constexpr bool value = ALD == LD_PLAIN && (EPI == EPI_STORE || EPI == EPI_DG || EPI == EPI_DH3);
};

// LDS-DMA ring variant (SINGLE == 3): one workgroup per CU with a two-k-tile lead instead of two per CU with a one-k-tile lead.
// Used when a workgroup has few M-tiles to amortise its k chains over.
static bool nn_use_dma(const GemmNN& g, int bn) {
    if (g.K % 64 != 0 || g.K < 128 || (g.epi == EPI_STORE_CAT && g.K1 % 64 != 0)) return false;
    if (g.epi == EPI_READOUT) return false;   // softplus + transposed fp32 stores: that epilogue wants a second workgroup on the CU
    // measured (profiles/r2_gemm_dma.txt): wins 5-16 % on the gated project conv (per-sample weights, K = 448..1792) and on
    // K >= 512 products with at most ~5 tiles per CU; loses where K is four k-tiles (the epilogue dominates) and on the
    // big-M K-concat products
    if (g.b_sample_stride) return true;
    const long long tiles = (long long)((g.M + 127) / 128) * ((g.N + bn - 1) / bn) * g.groups;
    return tiles <= 5 * 256 && g.K >= 512;
}

template <typename T, int ALD, int EPI>
int launch_nn_t(const GemmNN& g, hipStream_t s) {
    constexpr int BK = 128 / (int)sizeof(T);
    // the dh3 epilogue keeps four per-column coefficient vectors live: with a whole 128 x 128 tile per epilogue pass it spills
    // (88-140 B/lane of scratch, measured 2.7 TB/s) and ran on 64-column tiles until round 5; staged in passes of 64 (32) rows it
    // fits, and where the channel count is a multiple of 128 the wider tile halves the A re-reads from L2 (stand-alone
    // 162 -> 148 us at 147456 x 896 x 128, 270 -> 238 us at K = 256; 448 columns = 3.5 tiles: no gain, stays at 64)
    const bool n64 = g.N <= 64 || (EPI == EPI_DH3 && !(TT<T>::IS_BF16 && g.N % 128 == 0));
    if constexpr (HasSingle<ALD, EPI>::value) {
        if (g.K <= BK) return n64 ? launch_nn_k<T, ALD, EPI, 64, 1>(g, s) : launch_nn_k<T, ALD, EPI, 128, 1>(g, s);
    }
    if constexpr (HasSingle2<ALD, EPI>::value) {
        if (g.K <= 2 * BK && !g.b_sample_stride)
            return n64 ? launch_nn_k<T, ALD, EPI, 64, 2>(g, s) : launch_nn_k<T, ALD, EPI, 128, 2>(g, s);
    }
    if constexpr (ALD == LD_PLAIN && TT<T>::IS_BF16 && EPI != EPI_READOUT && EPI != EPI_READOUT_LB) {   // (nn_use_dma: never for a readout epilogue)
        if (nn_use_dma(g, n64 ? 64 : 128))
            return n64 ? launch_nn_k<T, ALD, EPI, 64, 3>(g, s) : launch_nn_k<T, ALD, EPI, 128, 3>(g, s);
    }
    return n64 ? launch_nn_k<T, ALD, EPI, 64, 0>(g, s) : launch_nn_k<T, ALD, EPI, 128, 0>(g, s);
}

// Every (loader, epilogue) combination launch_nn_d (dwn_gemm.hip) can reach, each for bf16_t and float.  A combination's kernels
// are compiled in exactly one dwn_gemm_nn_*.hip, the one that holds its NN_INSTANTIATE line; every other file sees only the
// declaration below and instantiates nothing (a combination missing from the files fails the link, one named twice fails
// tools/kernel_digest.py and the test built on it).
#define NN_COMBOS(X) \
    X(LD_PLAIN, EPI_STORE) X(LD_PLAIN, EPI_DG) X(LD_PLAIN, EPI_DH3) X(LD_PLAIN, EPI_STORE_CAT) \
    X(LD_PLAIN, EPI_READOUT) X(LD_PLAIN, EPI_READOUT_LB) X(LD_BNACT, EPI_READOUT) \
    X(LD_PE, EPI_STORE) X(LD_BNACT, EPI_STORE) X(LD_AFFINE2, EPI_STORE) X(LD_GATE, EPI_STORE)
#define NN_DECLARE(ALD, EPI) \
    extern template int launch_nn_t<bf16_t, ALD, EPI>(const GemmNN&, hipStream_t); \
    extern template int launch_nn_t<float, ALD, EPI>(const GemmNN&, hipStream_t);
NN_COMBOS(NN_DECLARE)
#undef NN_DECLARE
#define NN_INSTANTIATE(T, ALD, EPI) template int launch_nn_t<T, ALD, EPI>(const GemmNN&, hipStream_t);

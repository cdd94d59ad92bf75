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
#include "dwn_internal.h"
#include "dwn_launch.h"
#include <type_traits>
int k_zero(void* p, size_t nbytes, hipStream_t s);        // dwn_elementwise.hip

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
static int launch_nn_t(const GemmNN& g, hipStream_t s) {
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
    if constexpr (ALD == LD_PLAIN && TT<T>::IS_BF16 && EPI != EPI_READOUT_LB) {   // (nn_use_dma: never for a readout epilogue)
        if (nn_use_dma(g, n64 ? 64 : 128))
            return n64 ? launch_nn_k<T, ALD, EPI, 64, 3>(g, s) : launch_nn_k<T, ALD, EPI, 128, 3>(g, s);
    }
    return n64 ? launch_nn_k<T, ALD, EPI, 64, 0>(g, s) : launch_nn_k<T, ALD, EPI, 128, 0>(g, s);
}

template <typename T>
static int launch_nn_d(const GemmNN& g, hipStream_t s) {
    if (g.K % TT<T>::KC != 0) return dwn_set_error(-2, "gemm_nn: K must be a multiple of the 16-byte vector");
    if (g.epi == EPI_READOUT && g.sp_beta_dev) {       // learnable beta: instantiations of their own, the fixed ones untouched
        if (g.a_kind == LD_PLAIN) return launch_nn_t<T, LD_PLAIN, EPI_READOUT_LB>(g, s);
        return dwn_set_error(-3, "gemm_nn: the readout epilogue with sp_beta_dev needs a plain loader");
    }
    if (g.epi == EPI_READOUT) {
        if (g.a_kind == LD_BNACT) return launch_nn_t<T, LD_BNACT, EPI_READOUT>(g, s);
        if (g.a_kind == LD_PLAIN) return launch_nn_t<T, LD_PLAIN, EPI_READOUT>(g, s);
        return dwn_set_error(-3, "gemm_nn: unsupported loader for readout epilogue");
    }
    if (g.N % TT<T>::KC != 0) return dwn_set_error(-2, "gemm_nn: N must be a multiple of the 16-byte vector");
    if (g.epi == EPI_DG) {
        if (g.s3 || g.t3) return dwn_set_error(-3, "gemm_nn: the dg epilogue reads the activated z3; s3/t3 must be NULL");
        if (g.a_kind == LD_PLAIN && g.groups == 1) return launch_nn_t<T, LD_PLAIN, EPI_DG>(g, s);
        return dwn_set_error(-3, "gemm_nn: unsupported loader for dg epilogue");
    }
    if (g.epi == EPI_DH3) {
        if (g.a_kind != LD_PLAIN || g.groups != 1 || !g.y3 || !g.gate3 || !g.dps3 || !g.coef3 || g.rows_per_sample <= 0)
            return dwn_set_error(-3, "gemm_nn: the dh3 epilogue needs a plain loader, groups == 1, y3, gate3, dps3, coef3, rows_per_sample");
        return launch_nn_t<T, LD_PLAIN, EPI_DH3>(g, s);
    }
    if (g.epi == EPI_STORE_CAT) {
        if (g.a_kind != LD_PLAIN || g.groups != 1 || g.K1 <= 0 || g.K1 % TT<T>::KC || !g.a2 || !g.bias)
            return dwn_set_error(-3, "gemm_nn: K-concat epilogue needs a plain loader, groups == 1, a2, bias and K1 % vector == 0");
        return launch_nn_t<T, LD_PLAIN, EPI_STORE_CAT>(g, s);
    }
    switch (g.a_kind) {
        case LD_PLAIN: return launch_nn_t<T, LD_PLAIN, EPI_STORE>(g, s);
        case LD_PE: return launch_nn_t<T, LD_PE, EPI_STORE>(g, s);
        case LD_BNACT: return launch_nn_t<T, LD_BNACT, EPI_STORE>(g, s);
        case LD_AFFINE2: return launch_nn_t<T, LD_AFFINE2, EPI_STORE>(g, s);
        case LD_GATE: return launch_nn_t<T, LD_GATE, EPI_STORE>(g, s);
    }
    return dwn_set_error(-3, "gemm_nn: unsupported loader kind");
}

int launch_gemm_nn(const GemmNN& g, int dtype, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0 || g.K <= 0) return 0;
    if (g.b_sample_stride) {
        const int bk = dtype == DWN_BF16 ? 64 : 32;
        if (g.b_rows_per_sample <= 0 || g.b_rows_per_sample % 128 || g.groups != 1 || g.K <= bk)
            return dwn_set_error(-2, "gemm_nn: per-sample weights need b_rows_per_sample % 128 == 0, groups == 1, K > one k-tile");
    }
    if (gemm_nn_kd_eligible(g, dtype)) return launch_gemm_nn_kd(g, s);
    if (gemm_nn_xl_eligible(g, dtype)) return launch_gemm_nn_xl(g, s);
    return dtype == DWN_BF16 ? launch_nn_d<bf16_t>(g, s) : launch_nn_d<float>(g, s);
}

// ------------------------------------------------------------------------------------------------
// TN (weight gradient): dW[R][Cc] += sum_m P[m][r] Q[m][c]
// ------------------------------------------------------------------------------------------------
#ifndef TN_MINW_PLAIN
#define TN_MINW_PLAIN 3
#endif
template <typename T> static __device__ __forceinline__ uint4 ones_vec();      // one 16-byte vector of 1.0
template <> __device__ __forceinline__ uint4 ones_vec<bf16_t>() { return make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u); }
template <> __device__ __forceinline__ uint4 ones_vec<float>() { return make_uint4(0x3F800000u, 0x3F800000u, 0x3F800000u, 0x3F800000u); }
template <typename T> struct TnCfg;
template <> struct TnCfg<bf16_t> { static constexpr int PAD = 32; };   // 8 rows x 32 B shift -> conflict-free tr reads
template <> struct TnCfg<float>  { static constexpr int PAD = 64; };   // 16-bank shift between the two rows of a half-wave

// single-tensor loaders fit three waves per SIMD (the kernel's pace is one global-load latency per 64-row step, so a
// third resident workgroup per CU is +50 % steps in flight); the two-tensor BatchNorm-backward loader needs the registers
template <int PLD, int QLD> struct TnOcc {
    static constexpr int value = (PLD == LD_AFFINE2 || PLD == LD_DY3 || QLD == LD_AFFINE2 || QLD == LD_DY3) ? 2 : TN_MINW_PLAIN;
};
template <typename T, int PLD, int QLD>
__global__ __launch_bounds__(256, (TnOcc<PLD, QLD>::value)) void gemm_tn_kernel(const GemmTN g) {
    constexpr int KC = TT<T>::KC;
    constexpr int BR = 128, BC = 128, BMK = TT<T>::IS_BF16 ? 64 : 32;   // M rows per step
    constexpr int RS = BR * (int)sizeof(T) + TnCfg<T>::PAD;      // LDS row stride (bytes), both tiles
    constexpr int CPR = BR / KC;                                  // 16-byte chunks per tile row
    constexpr int NCH = BMK * CPR / 256;                          // chunks per thread per tile (2 bf16 / 4 f32)
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BMK * RS];
    unsigned char* sP = smem;
    unsigned char* sQ = smem + BMK * RS;

    const int tid = threadIdx.x;
    const int ntc = (g.Cc + BC - 1) / BC;
    // XCD-aware order: the output tiles of one M-split re-read the same P / Q rows, so they get consecutive slots of
    // one XCD (workgroups are dealt to the 8 XCDs round-robin in linear id order) instead of 8 different L2s
    int tile_id = blockIdx.x, split_id = blockIdx.y;
    {
        const unsigned total = gridDim.x * gridDim.y, bid = blockIdx.x + gridDim.x * blockIdx.y;
        if ((total & 7u) == 0u) {
            const unsigned lid = (bid & 7u) * (total >> 3) + (bid >> 3);
            tile_id = (int)(lid % gridDim.x);
            split_id = (int)(lid / gridDim.x);
        }
    }
    const int rt = tile_id / ntc, ct = tile_id % ntc;
    const int r0 = rt * BR, c0 = ct * BC;
    const int grp = blockIdx.z;
    const int Rl = g.R_load > 0 ? g.R_load : g.R;
    const int pcol0 = grp * Rl, qcol0 = grp * g.Cc;
    i64 mbeg = (i64)split_id * g.rows_per_split;
    i64 mend = mbeg + g.rows_per_split;
    if (mend > g.M) mend = g.M;
    i64 dw_off = 0;
    if (g.rows_per_sample > 0) {           // per-sample products: split = (sample, part of the sample)
        const int b = split_id / g.splits_per_sample, j = split_id % g.splits_per_sample;
        mbeg = (i64)b * g.rows_per_sample + (i64)j * g.rows_per_split;
        mend = mbeg + g.rows_per_split;
        const i64 send = (i64)(b + 1) * g.rows_per_sample;
        if (mend > send) mend = send;
        dw_off = (i64)b * g.dw_sample_stride;
    }

    const int wave = tid >> 6, lane = tid & 63;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 15, lg = lane >> 4;

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // raw staged vectors: load_tiles only issues the global loads; the prologue math and the bounds select run in
    // store_tiles, after the MFMAs of the current step (otherwise the loads are waited for before the MFMAs)
    uint4 p1[NCH], p2[NCH], q1[NCH], q2[NCH];
    i64 ld_mb = 0;
    // this thread's column chunk (tid % CPR) never changes: hoist the prologue coefficients out of the M loop
    const int chq = tid % CPR;
    const int rcol = r0 + chq * KC, ccol = c0 + chq * KC;
    const bool rok = rcol < Rl, cok = ccol < g.Cc;
    ColCoef<(PLD == LD_PE || PLD == LD_CAT1) ? LD_PLAIN : PLD, T> cfp;
    ColCoef<QLD == LD_PE ? LD_PLAIN : QLD, T> cfq;
    if (rok) cfp.load(g.p, pcol0 + rcol);
    if (cok) cfq.load(g.q, qcol0 + ccol);
    const T* Pp = reinterpret_cast<const T*>(g.p.p);
    const T* Pq = reinterpret_cast<const T*>(g.p.q);
    const T* Qp = reinterpret_cast<const T*>(g.q.p);
    const T* Qq = reinterpret_cast<const T*>(g.q.q);
    // LD_CAT1: P = [p | q | 1] side by side; this thread's column chunk lies in one segment for the whole kernel
    // (cat_c1, cat_c2 are multiples of the 16-byte vector), so the segment only selects its base pointer and row stride
    i64 pld = g.p.ld;
    int pcol = pcol0 + rcol;
    [[maybe_unused]] bool p_ones = false;
    if constexpr (PLD == LD_CAT1) {
        if (rcol >= g.p.cat_c1 + g.p.cat_c2) p_ones = true;
        else if (rcol >= g.p.cat_c1) { Pp = Pq; pld = g.p.ld2; pcol = rcol - g.p.cat_c1; }
    }
    auto load_tiles = [&](i64 mb) {
        ld_mb = mb;
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            i64 m = mb + tid / CPR + (256 / CPR) * i;
            const bool mok = m < mend;
            i64 offp = (mok && rok) ? m * pld + pcol : 0;
            if constexpr (PLD == LD_CAT1) { if (p_ones) offp = 0; }
            const i64 offq = (mok && cok) ? m * g.q.ld + qcol0 + ccol : 0;
            if constexpr (PLD != LD_PE) {
                p1[i] = *reinterpret_cast<const uint4*>(Pp + offp);
                if constexpr (decltype(cfp)::two_tensors) p2[i] = *reinterpret_cast<const uint4*>(Pq + offp);
            } else {
                p1[i] = (mok && rok) ? load_op_packed<LD_PE, T>(g.p, m, pcol0 + rcol) : make_uint4(0, 0, 0, 0);
            }
            if constexpr (QLD != LD_PE) {
                q1[i] = *reinterpret_cast<const uint4*>(Qp + offq);
                if constexpr (decltype(cfq)::two_tensors) q2[i] = *reinterpret_cast<const uint4*>(Qq + offq);
            } else {
                q1[i] = (mok && cok) ? load_op_packed<LD_PE, T>(g.q, m, qcol0 + ccol) : make_uint4(0, 0, 0, 0);
            }
        }
    };
    auto store_tiles = [&]() {
        const uint4 z4 = make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            int mrow = tid / CPR + (256 / CPR) * i;
            const i64 m = ld_mb + mrow;
            const bool mok = m < mend;
            uint4 vp, vq;
            if constexpr (PLD == LD_PE) vp = p1[i];
            else if constexpr (PLD == LD_CAT1) vp = !(mok && rok) ? z4 : p_ones ? ones_vec<T>() : p1[i];
            else if constexpr (decltype(cfp)::two_tensors) vp = (mok && rok) ? cfp.apply(g.p, (unsigned)m, p1[i], p2[i]) : z4;
            else vp = (mok && rok) ? cfp.apply(g.p, (unsigned)m, p1[i], z4) : z4;
            if constexpr (QLD == LD_PE) vq = q1[i];
            else if constexpr (decltype(cfq)::two_tensors) vq = (mok && cok) ? cfq.apply(g.q, (unsigned)m, q1[i], q2[i]) : z4;
            else vq = (mok && cok) ? cfq.apply(g.q, (unsigned)m, q1[i], z4) : z4;
            *reinterpret_cast<uint4*>(sP + mrow * RS + chq * 16) = vp;
            *reinterpret_cast<uint4*>(sQ + mrow * RS + chq * 16) = vq;
        }
    };

    if (mbeg < mend) {
        load_tiles(mbeg);
        store_tiles();
    }
    __syncthreads();
    for (i64 mb = mbeg; mb < mend; mb += BMK) {
        const bool has_next = (mb + BMK) < mend;
        if (has_next) load_tiles(mb + BMK);
        if constexpr (TT<T>::IS_BF16) {
            // transposed fragments: lane 4q+p of each 16-lane group addresses row (8*lg + 4h + q), cols 4p..4p+3
            const int q = lr >> 2, p = lr & 3;
#pragma unroll
            for (int kb = 0; kb < BMK / 32; ++kb) {
                bf16x8_t af[4], bfr[4];
                const int rb = kb * 32 + 8 * lg + q;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    int colb = (wm * 64 + i * 16 + 4 * p) * 2;
                    auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4_t*)(sP + rb * RS + colb));
                    auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4_t*)(sP + (rb + 4) * RS + colb));
                    af[i] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int colb = (wn * 64 + j * 16 + 4 * p) * 2;
                    auto lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4_t*)(sQ + rb * RS + colb));
                    auto hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4_t*)(sQ + (rb + 4) * RS + colb));
                    bfr[j] = bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < BMK / 4; ++ks) {
                float af[4], bfr[4];
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    af[i] = *reinterpret_cast<const float*>(sP + (ks * 4 + lg) * RS + (wm * 64 + i * 16 + lr) * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    bfr[j] = *reinterpret_cast<const float*>(sQ + (ks * 4 + lg) * RS + (wn * 64 + j * 16 + lr) * 4);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();
        if (has_next) {
            store_tiles();
            __syncthreads();
        }
    }
    if (mbeg >= mend) { DET_EXIT(); return; }
    DET_ENTER();
    float* dw = g.dw + (i64)grp * g.R * g.lddw + dw_off;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int rr = r0 + wm * 64 + i * 16 + lg * 4 + r;
                int cc = c0 + wn * 64 + j * 16 + lr;
                if (rr < g.R && cc < g.Cc) {
                    if (g.overwrite == 2) dw[(i64)rr * g.lddw + cc] = acc[i][j][r];      // single M-split: this tile has one writer
                    else if (g.dw_f64) atomicAdd(reinterpret_cast<double*>(g.dw) + (i64)grp * g.R * g.lddw + dw_off + (i64)rr * g.lddw + cc, (double)acc[i][j][r]);
                    else atomicAdd(dw + (i64)rr * g.lddw + cc, acc[i][j][r]);
                }
            }
    DET_EXIT();
}

#define TRY_(x) do { int rc__ = (x); if (rc__ != 0) return rc__; } while (0)
// M-splits are sized for at most TN_SLOTS workgroups per CU: every split adds a 64 KB fp32 atomic flush per output tile, and the
// third resident workgroup's extra steps in flight buy less than its flushes cost (training step, A/B on one box: weight-gradient
// families 1.953 -> 1.912 ms with 2; 2.80 ms with 1)
#ifndef TN_SLOTS
#define TN_SLOTS 2
#endif
#ifndef TN_F64_SLOTS
#define TN_F64_SLOTS 2
#endif
template <typename T, int PLD, int QLD>
static int launch_tn_t(const GemmTN& g_in, hipStream_t s) {
    GemmTN g = g_in;
    if (g.rows_per_sample > 0) {
        if (g.groups != 1 || g.M % g.rows_per_sample) return dwn_set_error(-2, "gemm_tn: per-sample mode needs groups == 1 and M % rows_per_sample == 0");
        int bpc = resident_bpc(gemm_tn_kernel<T, PLD, QLD>, 256, 0, 1);
        const int nb = g.M / g.rows_per_sample;
        const int tiles = ((g.R + 127) / 128) * ((g.Cc + 127) / 128);
        if (bpc > TN_SLOTS) bpc = TN_SLOTS;
        int J = (256 * bpc) / (tiles * nb);
        const int maxj = (g.rows_per_sample + 511) / 512;
        if (J > maxj) J = maxj;
        if (J < 1) J = 1;
        int rows = (g.rows_per_sample + J - 1) / J;
        rows = (rows + 63) / 64 * 64;
        g.rows_per_split = rows;
        g.splits_per_sample = (g.rows_per_sample + rows - 1) / rows;
        g.nsplit = nb * g.splits_per_sample;
    } else if (g.nsplit <= 0) {
        // one resident round: tiles x splits = the workgroups the chip holds at once (a partial second round costs a
        // whole workgroup duration, and every split adds 64 KB of fp32 atomics per tile)
        int bpc = resident_bpc(gemm_tn_kernel<T, PLD, QLD>, 256, 0, 1);
        if (bpc > TN_SLOTS) bpc = TN_SLOTS;
        if (g.dw_f64 && bpc > TN_F64_SLOTS) bpc = TN_F64_SLOTS;      // every split adds one fp64 atomic per output element, all to the same addresses
        const int tiles = ((g.R + 127) / 128) * ((g.Cc + 127) / 128) * g.groups;
        int want = (256 * bpc) / tiles;
        const int maxsplit = (int)((g.M + 511) / 512);
        if (want > maxsplit) want = maxsplit;
        if (want < 1) want = 1;
        // prefer a split count that makes tiles x splits a multiple of 8 (XCD-aware tile order in the kernel)
        const int tiles_g = ((g.R + 127) / 128) * ((g.Cc + 127) / 128);
        for (int w = want; w >= 1 && w > want - 8; --w) {
            i64 rows = (g.M + w - 1) / w;
            rows = (rows + 63) / 64 * 64;
            g.rows_per_split = (int)rows;
            g.nsplit = (int)((g.M + rows - 1) / rows);
            if (((tiles_g * g.nsplit) & 7) == 0) break;
        }
        if (((tiles_g * g.nsplit) & 7) != 0) {       // none found: keep the fullest grid
            i64 rows = (g.M + want - 1) / want;
            rows = (rows + 63) / 64 * 64;
            g.rows_per_split = (int)rows;
            g.nsplit = (int)((g.M + rows - 1) / rows);
        }
    } else {
        // splits chosen by the caller: they must cover every row (a split past M is an idle workgroup, a row past the last
        // split would silently be left out of dW)
        if (g.rows_per_split <= 0 || (i64)g.nsplit * g.rows_per_split < (i64)g.M)
            return dwn_set_error(-2, "gemm_tn: nsplit > 0 needs rows_per_split > 0 and nsplit * rows_per_split >= M");
    }
    if (g.dw_f64 && (g.overwrite || g.rows_per_sample > 0)) return dwn_set_error(-2, "gemm_tn: dw_f64 excludes overwrite and per-sample mode");
    if (g.overwrite) {
        // dW = product: plain stores with one M-split (overwrite = 2 tells the kernel), else zero first and accumulate
        if (g.rows_per_sample > 0 || g.lddw != g.Cc) return dwn_set_error(-2, "gemm_tn: overwrite needs lddw == Cc and no per-sample mode");
        if (g.nsplit == 1) g.overwrite = 2;
        else TRY_(k_zero(g.dw, (size_t)g.groups * g.R * g.lddw * sizeof(float), s));
    }
    dim3 grid(((g.R + 127) / 128) * ((g.Cc + 127) / 128), g.nsplit, g.groups);
    hipLaunchKernelGGL((gemm_tn_kernel<T, PLD, QLD>), grid, dim3(256), 0, s, g);
    DWN_CHECK_LAUNCH();
    return 0;
}

template <typename T>
static int launch_tn_d(const GemmTN& g, hipStream_t s) {
    const int Rl = g.R_load > 0 ? g.R_load : g.R;
    if (Rl % TT<T>::KC != 0 || g.Cc % TT<T>::KC != 0)
        return dwn_set_error(-2, "gemm_tn: R and Cc must be multiples of the 16-byte vector");
    const int pk = g.p_kind, qk = g.q_kind;
    if (pk == LD_AFFINE2 && qk == LD_PE) return launch_tn_t<T, LD_AFFINE2, LD_PE>(g, s);
    if (pk == LD_PLAIN && qk == LD_BNACT) return launch_tn_t<T, LD_PLAIN, LD_BNACT>(g, s);
    if (pk == LD_PLAIN && qk == LD_GATE) return launch_tn_t<T, LD_PLAIN, LD_GATE>(g, s);
    if (pk == LD_PLAIN && qk == LD_PLAIN) return launch_tn_t<T, LD_PLAIN, LD_PLAIN>(g, s);
    if (pk == LD_AFFINE2 && qk == LD_PLAIN) return launch_tn_t<T, LD_AFFINE2, LD_PLAIN>(g, s);
    if (pk == LD_CAT1 && qk == LD_PLAIN) {
        if (g.p.cat_c1 <= 0 || g.p.cat_c2 < 0 || g.p.cat_c1 % TT<T>::KC || g.p.cat_c2 % TT<T>::KC || g.groups != 1 ||
            g.R < g.p.cat_c1 + g.p.cat_c2 || (g.p.cat_c2 > 0 && !g.p.q))
            return dwn_set_error(-2, "gemm_tn: LD_CAT1 needs groups == 1, segment widths in 16-byte vectors and R >= cat_c1 + cat_c2");
        return launch_tn_t<T, LD_CAT1, LD_PLAIN>(g, s);
    }
    return dwn_set_error(-3, "gemm_tn: unsupported loader combination");
}

int launch_gemm_tn(const GemmTN& g_in, int dtype, hipStream_t s) {
    if (g_in.M <= 0 || g_in.R <= 0 || g_in.Cc <= 0) return 0;
    const GemmTN& g = g_in;
    return dtype == DWN_BF16 ? launch_tn_d<bf16_t>(g, s) : launch_tn_d<float>(g, s);
}

// ------------------------------------------------------------------------------------------------
// conv_pw backward of the 64-channel blocks (Cin = 64, E = 448): ONE pass over dh1, and y1 is not read at all.
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


bool pw_bwd_fused_supported(int dtype, long long M, int E, int Cin) {
    return dtype == DWN_BF16 && (E == 448 || E == 384) && Cin == pwb::CIN && M > 0 && M % pwb::BM == 0 && M <= 0x7fffffffLL;
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
// res / res_coef / res_n (+ hinv, winv, Hin, Win, Hout, Wout for the gathered form): the shortcut branch's gradient in the epilogue
// (see PwbGather above); res rows are res_n * Cin wide
int launch_pw_bwd_fused(const void* dh1, const void* a0, const void* bp, const float* r3, void* da0, float* tacc,
                        long long M, int E, int Cin, int dtype, const void* res, const float* res_coef, int res_n,
                        const int* hinv, const int* winv, int Hin, int Win, int Hout, int Wout, hipStream_t s) {
    PwbGather gq; gq.hinv = hinv; gq.winv = winv; gq.Hin = Hin; gq.Win = Win; gq.Hout = Hout; gq.Wout = Wout;
    if (res && hinv && (!winv || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || M % ((long long)Hin * Win) || Hin + Win > 512))
        return dwn_set_error(-2, "pw_bwd_fused: the gathered shortcut form needs both inverse maps, M = frames * Hin * Win and Hin + Win <= 512");
    if (!pw_bwd_fused_supported(dtype, M, E, Cin))
        return dwn_set_error(-3, "pw_bwd_fused: built for bf16, Cin = 64, E = 448 or 384, M % 128 == 0 only");
    if (res && (!res_coef || res_n < 1 || res_n > 2)) return dwn_set_error(-3, "pw_bwd_fused: the residual term needs res_coef and res_n in {1, 2}");
    return E == 448 ? launch_pw_bwd_fused_t<7>(dh1, a0, bp, r3, da0, tacc, M, res, res_coef, res_n, gq, s)
                    : launch_pw_bwd_fused_t<6>(dh1, a0, bp, r3, da0, tacc, M, res, res_coef, res_n, gq, s);
}

// ------------------------------------------------------------------------------------------------
// TN (weight gradient): dW[R][Cc] += sum_m P[m][r] Q[m][c]
// ------------------------------------------------------------------------------------------------
#include "dwn_gemm_nn.h"                                   // operand maps (file head), MFMA vector types, load_op_packed
int k_zero(void* p, size_t nbytes, hipStream_t s);        // dwn_elementwise.hip

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

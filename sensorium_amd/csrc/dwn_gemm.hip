// dwn_gemm_nn's host side: argument checks and the choice among the A-direct kernel (dwn_gemm_kd.hip), the 256-row kernel
// (dwn_gemm_xl.hip) and the 128-row family gemm_nn_kernel (dwn_gemm_nn.h).  This file instantiates no kernel: every launch_nn_t
// it names is declared extern in dwn_gemm_nn.h and compiled in one of the dwn_gemm_nn_*.hip files.
#include "dwn_gemm_nn.h"

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

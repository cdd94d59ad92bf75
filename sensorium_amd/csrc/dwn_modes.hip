// Population modes (include/dwn.h dwn_modes_args): the leading eigenpairs of a symmetric N x N float64 matrix by
// block subspace iteration with Rayleigh-Ritz extraction, and the principal angles between two such subspaces.
//
//   symm      Y = scale * A Q on v_mfma_f64_16x16x4_f64.  One workgroup per strip of 32 rows of Y, all columns of the block; its
//             four waves take the four quarters of the sum over j (the quarter is N / 4 rounded up to the k-step: a function of N
//             alone) and wave 0 adds the other three in wave order through LDS.  A is read through its symmetry: the A operand
//             A[i][j] is loaded as A[j][i], so that the 16 lanes of a k-slice read 16 consecutive doubles of one row of A (and every
//             element of A is read exactly once per launch); Q is read the same way.  C/D lane map as in dwn_pairwise.hip:
//             col = lane & 15, row = (lane >> 4) + 4 * reg.
//   moments   one workgroup per row for the sum of squares, one workgroup folds the rows and the diagonal in a fixed order.
//   gram      G = X^T Z of two N x p blocks: one workgroup per 256 rows writes its p x p partial, the consumer adds the partials
//             in ascending order (the split is a function of N alone).
//   small     one workgroup: folds a Gram product, runs the cyclic Jacobi eigen-solver in round-robin order (p / 2 disjoint
//             rotations per step, a bounded number of sweeps), sorts descending and fixes the signs.
//   rotate    V = Q W and the per-column sums of squares of Y W - V diag(theta), per 256 rows; stop folds them, takes the
//             decision and raises the device flag every later kernel of the solve returns on.
//   orth      classical Gram-Schmidt, twice, column by column in one workgroup; a column whose norm after the projections is at
//             most ORTH_C N u ||Y||_F becomes an exact zero column (and stays one: A 0 = 0).
// No atomics, no scratch, no grid that depends on anything but the sizes: the same inputs give the same bits on every launch and in
// both builds (the file does not read DWN_DETERMINISTIC).
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include "dwn_philox.h"
#include "dwn_reduce.h"

namespace {

constexpr int MD_NT = 256;
constexpr int MD_WAVE = 64;
constexpr int MD_P = DWN_MODES_MAXP;       // widest block, and the row stride of every small matrix
constexpr int MD_STRIP = 32;               // rows of Y per symm workgroup
constexpr int MD_CH = 256;                 // rows per gram / rotate workgroup
constexpr int MD_ONT = 1024;               // threads of the orth workgroup
constexpr int MD_SWEEPS = 30;              // Jacobi: at most this many sweeps
constexpr double MD_U = 1.1102230246251565e-16;     // 2^-53
constexpr double MD_ORTH_C = DWN_MODES_ORTH_C;

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bool finished(const int* status) { return status && status[0] != 0; }

// ---- the start block: entry (i, c) is word c & 3 of philox(counter = (i, c >> 2, 0, 0), key = seed), mapped to (-1, 1)
__global__ __launch_bounds__(MD_NT) void modes_start_kernel(double* __restrict__ Q, i64 ldq, int N, int p, int pp, unsigned k0, unsigned k1,
                                                            int* __restrict__ status) {
    const i64 e = (i64)blockIdx.x * MD_NT + threadIdx.x;
    if (e == 0 && status) { status[0] = 0; status[1] = 0; status[2] = 0; status[3] = 0; }
    if (e >= (i64)N * pp) return;
    const i64 i = e / pp;
    const int c = (int)(e - i * pp);
    double v = 0.0;
    if (c < p) v = ((double)philox_word((unsigned)i, (unsigned)(c >> 2), 0u, 0u, k0, k1, c & 3) + 0.5) * (1.0 / 2147483648.0) - 1.0;
    Q[i * ldq + c] = v;
}

__global__ void modes_status_kernel(int* __restrict__ status) {
    if (threadIdx.x < 4) status[threadIdx.x] = 0;
}

// ---- Y = scale * A Q
template <int PT>
__global__ __launch_bounds__(MD_NT) void modes_symm_kernel(const double* __restrict__ A, i64 lda, int N, const double* __restrict__ Q,
                                                           i64 ldq, int p, double scale, double* __restrict__ Y, i64 ldy,
                                                           const int* __restrict__ status) {
    __shared__ double red[3][MD_STRIP][PT * 16];
    if (finished(status)) return;
    const int tid = threadIdx.x, lane = tid & (MD_WAVE - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / MD_WAVE);
    const int l15 = lane & 15, l4 = lane >> 4;
    const i64 i0 = (i64)blockIdx.x * MD_STRIP;
    const int quarter = ((N + 3) / 4 + 3) / 4 * 4;
    const int jb = wave * quarter, je = min(N, jb + quarter);
    const i64 r0 = i0 + l15, r1 = i0 + 16 + l15;
    const bool ok0 = r0 < N, ok1 = r1 < N;
    d4 acc[2][PT];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < PT; ++c) acc[a][c] = (d4){0.0, 0.0, 0.0, 0.0};
    for (int j = jb; j < je; j += 4) {
        const i64 jj = j + l4;
        const bool okj = jj < N;
        const double a0 = okj && ok0 ? A[jj * lda + r0] : 0.0;         // A[r0][jj] by symmetry
        const double a1 = okj && ok1 ? A[jj * lda + r1] : 0.0;
#pragma unroll
        for (int c = 0; c < PT; ++c) {
            const double b = okj ? Q[jj * ldq + c * 16 + l15] : 0.0;
            acc[0][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b, acc[0][c], 0, 0, 0);
            acc[1][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b, acc[1][c], 0, 0, 0);
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < PT; ++c)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wave - 1][a * 16 + l4 + 4 * r][c * 16 + l15] = acc[a][c][r];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < PT; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rl = a * 16 + l4 + 4 * r, cl = c * 16 + l15;
                double v = acc[a][c][r];
                v += red[0][rl][cl]; v += red[1][rl][cl]; v += red[2][rl][cl];
                const i64 row = i0 + rl;
                if (row < N) Y[row * ldy + cl] = cl < p ? scale * v : 0.0;
            }
}

// ---- trace and squared Frobenius norm
__global__ __launch_bounds__(MD_NT) void modes_rowsq_kernel(const double* __restrict__ A, i64 lda, int N, double* __restrict__ rowsq) {
    __shared__ double red[MD_NT];
    const double* row = A + (i64)blockIdx.x * lda;
    double s = 0.0;
    for (int j = threadIdx.x; j < N; j += MD_NT) s = fma(row[j], row[j], s);
    s = wg_tree_sum<MD_NT>(s, red);
    if (threadIdx.x == 0) rowsq[blockIdx.x] = s;
}

__global__ __launch_bounds__(MD_NT) void modes_moments_fold_kernel(const double* __restrict__ A, i64 lda, int N, double scale,
                                                                   const double* __restrict__ rowsq, double* __restrict__ out) {
    __shared__ double red[2][MD_NT];
    double v[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < N; i += MD_NT) { v[0] += A[(i64)i * lda + i]; v[1] += rowsq[i]; }
    wg_tree_sum<MD_NT, 2>(v, red);
    if (threadIdx.x == 0) { out[0] = scale * v[0]; out[1] = (scale * scale) * v[1]; }
}

// ---- part[ch][a][b] = sum over the rows i of chunk ch of X[i][a] Z[i][b]
__global__ __launch_bounds__(MD_NT) void modes_gram_kernel(const double* __restrict__ X, i64 ldx, int pa, const double* __restrict__ Z, i64 ldz,
                                                           int pb, int N, double* __restrict__ part, const int* __restrict__ status) {
    __shared__ double xs[32][MD_P];
    __shared__ double zs[32][MD_P];
    if (finished(status)) return;
    const int tid = threadIdx.x, ta = (tid >> 4) * 4, tb = (tid & 15) * 4;
    const i64 base = (i64)blockIdx.x * MD_CH;
    double acc[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int rb = 0; rb < MD_CH; rb += 32) {
        if (base + rb >= N) break;                                   // uniform
        for (int e = tid; e < 32 * MD_P; e += MD_NT) {
            const int r = e >> 6, c = e & (MD_P - 1);
            const i64 row = base + rb + r;
            xs[r][c] = (row < N && c < pa) ? X[row * ldx + c] : 0.0;
            zs[r][c] = (row < N && c < pb) ? Z[row * ldz + c] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < 32; ++r) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v) acc[u][v] = fma(xs[r][ta + u], zs[r][tb + v], acc[u][v]);
        }
        __syncthreads();
    }
    double* dst = part + (i64)blockIdx.x * MD_P * MD_P;
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) dst[(ta + u) * MD_P + tb + v] = acc[u][v];
}

// ---- the small symmetric eigenproblem, in LDS, by all MD_NT threads of one workgroup.
// H: in the matrix (both triangles), out its diagonal form; W: out the rotation, columns = eigenvectors of the input.
// Round-robin order: step s of a sweep pairs (s + i, s - i) mod (n - 1) for i >= 1 and (s, n - 1) for i = 0, n = p rounded up to
// even; the pairs of a step are disjoint, so their rotations commute and are applied together.  Returns false on a non-finite input.
__device__ bool jacobi_eigh(double (*H)[MD_P], double (*W)[MD_P], int p, double* cs, int* flag) {
    const int tid = threadIdx.x;
    if (tid == 0) *flag = 0;
    __syncthreads();
    int bad = 0;
    for (int e = tid; e < p * p; e += MD_NT) {
        const int a = e / p, b = e - a * p;
        if (!is_finite(H[a][b])) bad = 1;
        W[a][b] = a == b ? 1.0 : 0.0;
    }
    if (bad) *flag = 1;                       // every writer writes the same value
    __syncthreads();
    if (*flag) return false;
    __syncthreads();
    const int n = (p + 1) & ~1, half = n / 2;
    for (int sweep = 0; sweep < MD_SWEEPS; ++sweep) {
        if (tid == 0) *flag = 0;
        __syncthreads();
        for (int s = 0; s < n - 1; ++s) {
            // the rotations of this step
            if (tid < half) {
                int a = tid == 0 ? s : (s + tid) % (n - 1), b = tid == 0 ? n - 1 : (s - tid + (n - 1)) % (n - 1);
                const int pi = min(a, b), qi = max(a, b);
                double c = 1.0, sn = 0.0;
                if (qi < p) {
                    const double hpq = H[pi][qi], hpp = H[pi][pi], hqq = H[qi][qi];
                    const double g = 100.0 * fabs(hpq);
                    if (hpq != 0.0 && !(fabs(hpp) + g == fabs(hpp) && fabs(hqq) + g == fabs(hqq))) {
                        const double th = (hqq - hpp) / (2.0 * hpq);
                        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        sn = t * c;
                        *flag = 1;
                    }
                }
                cs[3 * tid] = c; cs[3 * tid + 1] = sn;
                reinterpret_cast<int*>(cs + 3 * tid + 2)[0] = pi; reinterpret_cast<int*>(cs + 3 * tid + 2)[1] = qi;
            }
            __syncthreads();
            // columns: H <- H J, W <- W J
            for (int e = tid; e < half * p; e += MD_NT) {
                const int i = e / p, r = e - i * p;
                const double c = cs[3 * i], sn = cs[3 * i + 1];
                const int pi = reinterpret_cast<int*>(cs + 3 * i + 2)[0], qi = reinterpret_cast<int*>(cs + 3 * i + 2)[1];
                if (qi >= p || sn == 0.0) continue;
                const double hp = H[r][pi], hq = H[r][qi];
                H[r][pi] = c * hp - sn * hq; H[r][qi] = sn * hp + c * hq;
                const double wp = W[r][pi], wq = W[r][qi];
                W[r][pi] = c * wp - sn * wq; W[r][qi] = sn * wp + c * wq;
            }
            __syncthreads();
            // rows: H <- J^T H, and the eliminated pair set to an exact zero
            for (int e = tid; e < half * p; e += MD_NT) {
                const int i = e / p, r = e - i * p;
                const double c = cs[3 * i], sn = cs[3 * i + 1];
                const int pi = reinterpret_cast<int*>(cs + 3 * i + 2)[0], qi = reinterpret_cast<int*>(cs + 3 * i + 2)[1];
                if (qi >= p || sn == 0.0) continue;
                const double hp = H[pi][r], hq = H[qi][r];
                double np_ = c * hp - sn * hq, nq = sn * hp + c * hq;
                if (r == qi) np_ = 0.0;
                if (r == pi) nq = 0.0;
                H[pi][r] = np_; H[qi][r] = nq;
            }
            __syncthreads();
        }
        if (!*flag) break;                    // read after the step's last barrier: the same value in every thread
        __syncthreads();
    }
    __syncthreads();
    return true;
}

// mode 0: H given (row stride MD_P); 1: H = the symmetrised fold of nch Gram partials; 2: H = M^T M of the folded M, values = sqrt.
// Out: values[MD_P] descending (zero beyond p), W[p][MD_P] with column c the eigenvector of values[c], its entry of largest magnitude
// (lowest index on ties) positive.  A non-finite input gives NaN values and NaN W.
__global__ __launch_bounds__(MD_NT) void modes_small_kernel(int mode, const double* __restrict__ src, int nch, int p, double* __restrict__ values,
                                                            double* __restrict__ Wout, const int* __restrict__ status) {
    __shared__ double H[MD_P][MD_P];
    __shared__ double W[MD_P][MD_P];
    __shared__ double cs[3 * MD_P / 2];
    __shared__ double d[MD_P];
    __shared__ int rank[MD_P];
    __shared__ int flag;
    if (finished(status)) return;
    const int tid = threadIdx.x;
    for (int e = tid; e < p * p; e += MD_NT) {
        const int a = e / p, b = e - a * p;
        double v;
        if (mode == 0) v = src[a * MD_P + b];
        else {
            v = 0.0;
            for (int ch = 0; ch < nch; ++ch) v += src[((i64)ch * MD_P + a) * MD_P + b];
        }
        (mode == 2 ? W : H)[a][b] = v;
    }
    __syncthreads();
    if (mode == 1) {
        for (int e = tid; e < p * p; e += MD_NT) {                   // the owner of a pair (a > b) writes both of its entries
            const int a = e / p, b = e - a * p;
            if (a <= b) continue;
            const double v = 0.5 * (H[a][b] + H[b][a]);
            H[a][b] = v; H[b][a] = v;
        }
        __syncthreads();
    } else if (mode == 2) {
        for (int e = tid; e < p * p; e += MD_NT) {
            const int a = e / p, b = e - a * p, lo = min(a, b), hi = max(a, b);
            double v = 0.0;
            for (int r = 0; r < p; ++r) v = fma(W[r][lo], W[r][hi], v);
            H[a][b] = v;
        }
        __syncthreads();
    }
    const bool ok = jacobi_eigh(H, W, p, cs, &flag);
    if (!ok) {
        const double nan = qnan_d();
        for (int c = tid; c < MD_P; c += MD_NT) values[c] = c < p ? nan : 0.0;
        for (int e = tid; e < p * MD_P; e += MD_NT) Wout[e] = (e & (MD_P - 1)) < p ? nan : 0.0;
        return;
    }
    if (tid < p) d[tid] = H[tid][tid];
    __syncthreads();
    if (tid < p) {
        int r = 0;
        for (int j = 0; j < p; ++j) r += (d[j] > d[tid] || (d[j] == d[tid] && j < tid)) ? 1 : 0;
        rank[tid] = r;
    }
    __syncthreads();
    if (tid < p) {
        // column tid of W goes to column rank[tid]; its sign from its entry of largest magnitude
        int best = 0;
        double bm = fabs(W[0][tid]);
        for (int r = 1; r < p; ++r) if (fabs(W[r][tid]) > bm) { bm = fabs(W[r][tid]); best = r; }
        const double sg = W[best][tid] < 0.0 ? -1.0 : 1.0;
        const int c = rank[tid];
        for (int r = 0; r < p; ++r) Wout[r * MD_P + c] = sg * W[r][tid];
        const double v = d[tid];
        values[c] = mode == 2 ? sqrt(fmax(v, 0.0)) : v;
    }
    for (int c = p + tid; c < MD_P; c += MD_NT) values[c] = 0.0;
    for (int e = tid; e < p * MD_P; e += MD_NT) if ((e & (MD_P - 1)) >= p) Wout[e] = 0.0;
}

// ---- V = Q W; rpart[ch][c] = sum over the chunk's rows of ((Y W)[i][c] - V[i][c] theta[c])^2
__global__ __launch_bounds__(MD_NT) void modes_rotate_kernel(const double* __restrict__ Q, i64 ldq, const double* __restrict__ Y, i64 ldy, int N,
                                                             int p, const double* __restrict__ theta, const double* __restrict__ W,
                                                             double* __restrict__ V, i64 ldv, int pp, double* __restrict__ rpart,
                                                             const int* __restrict__ status) {
    __shared__ double Ws[MD_P][MD_P];
    __shared__ double rs[MD_NT / MD_WAVE][MD_P];
    if (finished(status)) return;
    const int tid = threadIdx.x, c = tid & (MD_P - 1), g = tid / MD_P;
    for (int e = tid; e < MD_P * MD_P; e += MD_NT) Ws[e >> 6][e & (MD_P - 1)] = (e >> 6) < p ? W[e] : 0.0;
    __syncthreads();
    const double th = c < p ? theta[c] : 0.0;
    const i64 base = (i64)blockIdx.x * MD_CH;
    double s = 0.0;
    for (int r = g; r < MD_CH; r += MD_NT / MD_P) {
        const i64 row = base + r;
        if (row >= N) break;
        const double* q = Q + row * ldq;
        const double* y = Y + row * ldy;
        double v = 0.0, yw = 0.0;
        for (int a = 0; a < p; ++a) { v = fma(q[a], Ws[a][c], v); yw = fma(y[a], Ws[a][c], yw); }
        if (c < p) {
            const double res = yw - v * th;
            s = fma(res, res, s);
        }
        if (c < pp) V[row * ldv + c] = c < p ? v : 0.0;
    }
    rs[g][c] = s;
    __syncthreads();
    if (g == 0) rpart[(i64)blockIdx.x * MD_P + c] = ((rs[0][c] + rs[1][c]) + rs[2][c]) + rs[3][c];
}

// ---- the residual norms and the decision.  status: 0 done, 1 converged, 2 rounds
__global__ __launch_bounds__(MD_WAVE) void modes_stop_kernel(const double* __restrict__ rpart, int nch, int p, int k, double tol,
                                                             const double* theta, double* values, double* __restrict__ residuals,
                                                             int* __restrict__ status) {
    __shared__ double r[MD_P];
    if (finished(status)) return;
    const int c = threadIdx.x;
    double s = 0.0;
    if (c < p) for (int ch = 0; ch < nch; ++ch) s += rpart[(i64)ch * MD_P + c];
    r[c] = sqrt(s);
    residuals[c] = c < p ? r[c] : 0.0;
    values[c] = c < p ? theta[c] : 0.0;
    __syncthreads();
    if (c != 0) return;
    bool conv = true;
    const double lim = tol * fabs(theta[0]);
    for (int i = 0; i < k; ++i) conv = conv && r[i] <= lim;          // false on NaN
    status[2] += 1;
    if (conv) { status[1] = 1; status[0] = 1; }
    else if (theta[0] != theta[0]) status[0] = 1;                    // nothing a further round could mend
}

// ---- Q = orth(Y): classical Gram-Schmidt, twice, in one workgroup.  Q may be Y.
// A thread owns the rows tid, tid + MD_ONT, ...: the projections and the updates of a row never leave its thread, only the sums over
// the rows do.  A sum: the thread's rows in ascending order, the fixed butterfly inside the wave, the MD_ONT / 64 waves in ascending
// order; the split is a function of N alone.
__device__ __forceinline__ double orth_fold(const double (*part)[MD_ONT / MD_WAVE], int a) {
    double s = part[a][0];
#pragma unroll
    for (int w = 1; w < MD_ONT / MD_WAVE; ++w) s += part[a][w];
    return s;
}

__global__ __launch_bounds__(MD_ONT) void modes_orth_kernel(const double* Y, i64 ldy, double* Q, i64 ldq, int N, int p, int pp,
                                                            const int* __restrict__ status) {
    __shared__ double part[MD_P][MD_ONT / MD_WAVE];
    __shared__ double hs[MD_P];
    if (finished(status)) return;
    const int tid = threadIdx.x, lane = tid & (MD_WAVE - 1), wave = tid / MD_WAVE;
    double f = 0.0;
    for (int i = tid; i < N; i += MD_ONT) {
        for (int c = 0; c < pp; ++c) {
            const double v = c < p ? Y[(i64)i * ldy + c] : 0.0;
            Q[(i64)i * ldq + c] = v;
            f = fma(v, v, f);
        }
    }
    f = wave_sum(f);
    if (lane == 0) part[0][wave] = f;
    __syncthreads();
    const double tau = MD_ORTH_C * (double)N * MD_U * sqrt(orth_fold(part, 0));
    __syncthreads();
    for (int c = 0; c < p; ++c) {
        for (int pass = 0; pass < 2; ++pass) {
            for (int a0 = 0; a0 < c; a0 += 8) {
                double h[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int i = tid; i < N; i += 2 * MD_ONT) {                // two rows at a time: their loads are in flight together
                    const int i2 = i + MD_ONT;
                    const bool two = i2 < N;
                    const double* q = Q + (i64)i * ldq;
                    const double* q2 = Q + (i64)(two ? i2 : i) * ldq;
                    double t[8], t2[8];
                    const double w = q[c], w2 = two ? q2[c] : 0.0;
#pragma unroll
                    for (int u = 0; u < 8; ++u) { t[u] = a0 + u < c ? q[a0 + u] : 0.0; t2[u] = (two && a0 + u < c) ? q2[a0 + u] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) { h[u] = fma(t[u], w, h[u]); h[u] = fma(t2[u], w2, h[u]); }
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const double t = wave_sum(h[u]);
                    if (lane == 0 && a0 + u < c) part[a0 + u][wave] = t;
                }
            }
            __syncthreads();
            if (tid < c) hs[tid] = orth_fold(part, tid);
            __syncthreads();
            for (int i = tid; i < N; i += 2 * MD_ONT) {
                const int i2 = i + MD_ONT;
                const bool two = i2 < N;
                double* q = Q + (i64)i * ldq;
                double* q2 = Q + (i64)(two ? i2 : i) * ldq;
                double w = q[c], w2 = q2[c];
                for (int a0 = 0; a0 < c; a0 += 8) {
                    double t[8], t2[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) { t[u] = a0 + u < c ? q[a0 + u] : 0.0; t2[u] = a0 + u < c ? q2[a0 + u] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 8; ++u) if (a0 + u < c) { w = fma(-t[u], hs[a0 + u], w); w2 = fma(-t2[u], hs[a0 + u], w2); }
                }
                q[c] = w;
                if (two) q2[c] = w2;
            }
        }
        double s = 0.0;
        for (int i = tid; i < N; i += MD_ONT) { const double w = Q[(i64)i * ldq + c]; s = fma(w, w, s); }
        s = wave_sum(s);
        __syncthreads();                                              // hs and part of the last pass have been read
        if (lane == 0) part[0][wave] = s;
        __syncthreads();
        const double nrm = sqrt(orth_fold(part, 0));
        const bool drop = nrm <= tau;                                 // false on NaN: a NaN column stays NaN
        const double inv = 1.0 / nrm;
        for (int i = tid; i < N; i += MD_ONT) {
            double* q = Q + (i64)i * ldq + c;
            *q = drop ? 0.0 : *q * inv;
        }
        __syncthreads();                                              // part[0] is written again by the next column
    }
}

// ---- the sign rule on the columns of V: one workgroup per column, lowest index on ties
__global__ __launch_bounds__(MD_NT) void modes_sign_kernel(double* __restrict__ V, i64 ldv, int N) {
    __shared__ double bm[MD_NT];
    __shared__ int bi[MD_NT];
    const int c = blockIdx.x, tid = threadIdx.x;
    double m = -1.0;
    int at = 0x7fffffff;
    for (int i = tid; i < N; i += MD_NT) {
        const double v = fabs(V[(i64)i * ldv + c]);
        if (v > m) { m = v; at = i; }
    }
    bm[tid] = m; bi[tid] = at;
    __syncthreads();
    for (int s = MD_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const double m2 = bm[tid + s];
            const int a2 = bi[tid + s];
            if (m2 > bm[tid] || (m2 == bm[tid] && a2 < bi[tid])) { bm[tid] = m2; bi[tid] = a2; }
        }
        __syncthreads();
    }
    const int best = bi[0];
    if (best >= N) return;                                           // a NaN column: nothing to compare
    const bool flip = V[(i64)best * ldv + c] < 0.0;
    __syncthreads();
    if (!flip) return;
    for (int i = tid; i < N; i += MD_NT) V[(i64)i * ldv + c] = -V[(i64)i * ldv + c];
}

// ---- overlap: captured numerator tr(Va^T T) from the folded Gram partials
__global__ __launch_bounds__(MD_WAVE) void modes_trace_fold_kernel(const double* __restrict__ part, int nch, int k, double* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int c = 0; c < k; ++c) {
        double v = 0.0;
        for (int ch = 0; ch < nch; ++ch) v += part[((i64)ch * MD_P + c) * MD_P + c];
        t += v;
    }
    out[0] = t;
}

inline int pad16(int p) { return (p + 15) / 16 * 16; }
inline int nchunks(int N) { return (N + MD_CH - 1) / MD_CH; }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

int launch_symm(const double* A, i64 lda, int N, const double* Q, i64 ldq, int p, double scale, double* Y, i64 ldy, const int* status,
                hipStream_t s) {
    const dim3 grid((unsigned)((N + MD_STRIP - 1) / MD_STRIP)), block(MD_NT);
    switch (pad16(p) / 16) {
    case 1: hipLaunchKernelGGL(modes_symm_kernel<1>, grid, block, 0, s, A, lda, N, Q, ldq, p, scale, Y, ldy, status); break;
    case 2: hipLaunchKernelGGL(modes_symm_kernel<2>, grid, block, 0, s, A, lda, N, Q, ldq, p, scale, Y, ldy, status); break;
    case 3: hipLaunchKernelGGL(modes_symm_kernel<3>, grid, block, 0, s, A, lda, N, Q, ldq, p, scale, Y, ldy, status); break;
    default: hipLaunchKernelGGL(modes_symm_kernel<4>, grid, block, 0, s, A, lda, N, Q, ldq, p, scale, Y, ldy, status); break;
    }
    DWN_CHECK_LAUNCH();
    return 0;
}

int launch_moments(const double* A, i64 lda, int N, double scale, double* rowsq, double* out, hipStream_t s) {
    hipLaunchKernelGGL(modes_rowsq_kernel, dim3((unsigned)N), dim3(MD_NT), 0, s, A, lda, N, rowsq);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(modes_moments_fold_kernel, dim3(1), dim3(MD_NT), 0, s, A, lda, N, scale, rowsq, out);
    DWN_CHECK_LAUNCH();
    return 0;
}

int launch_gram(const double* X, i64 ldx, int pa, const double* Z, i64 ldz, int pb, int N, double* part, const int* status, hipStream_t s) {
    hipLaunchKernelGGL(modes_gram_kernel, dim3((unsigned)nchunks(N)), dim3(MD_NT), 0, s, X, ldx, pa, Z, ldz, pb, N, part, status);
    DWN_CHECK_LAUNCH();
    return 0;
}

int launch_orth(const double* Y, i64 ldy, double* Q, i64 ldq, int N, int p, const int* status, hipStream_t s) {
    hipLaunchKernelGGL(modes_orth_kernel, dim3(1), dim3(MD_ONT), 0, s, Y, ldy, Q, ldq, N, p, pad16(p), status);
    DWN_CHECK_LAUNCH();
    return 0;
}

int launch_ritz(const double* Q, i64 ldq, const double* Y, i64 ldy, int N, int p, int k, double tol, const double* theta, const double* W,
                double* V, i64 ldv, double* rpart, double* values, double* residuals, int* status, hipStream_t s) {
    hipLaunchKernelGGL(modes_rotate_kernel, dim3((unsigned)nchunks(N)), dim3(MD_NT), 0, s, Q, ldq, Y, ldy, N, p, theta, W, V, ldv, pad16(p), rpart,
                       (const int*)status);
    DWN_CHECK_LAUNCH();
    hipLaunchKernelGGL(modes_stop_kernel, dim3(1), dim3(MD_WAVE), 0, s, (const double*)rpart, nchunks(N), p, k, tol, theta, values, residuals,
                       status);
    DWN_CHECK_LAUNCH();
    return 0;
}

}  // namespace

// the workspaces, in doubles, carved in this order at 256-byte boundaries
size_t k_modes_ritz_ws_bytes(int N) { return up256((size_t)nchunks(N) * MD_P * sizeof(double)); }
size_t k_modes_moments_ws_bytes(int N) { return up256((size_t)N * sizeof(double)); }
size_t k_modes_solve_ws_bytes(int N, int p) {
    const size_t blk = up256((size_t)N * pad16(p) * sizeof(double));
    return 2 * blk + up256((size_t)nchunks(N) * MD_P * MD_P * sizeof(double)) + up256(MD_P * sizeof(double)) +
           up256((size_t)MD_P * MD_P * sizeof(double)) + k_modes_ritz_ws_bytes(N) + k_modes_moments_ws_bytes(N);
}
size_t k_modes_overlap_ws_bytes(int N, int k, int with_matrix) {
    size_t b = up256((size_t)nchunks(N) * MD_P * MD_P * sizeof(double)) + up256((size_t)MD_P * MD_P * sizeof(double));
    if (with_matrix) b += up256((size_t)N * pad16(k) * sizeof(double)) + k_modes_moments_ws_bytes(N);
    return b;
}

int k_modes_symm(const dwn_modes_args& a, hipStream_t s) {
    return launch_symm(a.A, a.lda, a.N, a.Q, a.ldq, a.p, a.scale, a.Y, a.ldy, nullptr, s);
}

int k_modes_moments(const dwn_modes_args& a, hipStream_t s) {
    return launch_moments(a.A, a.lda, a.N, a.scale, (double*)a.ws, a.moments, s);
}

int k_modes_orth(const dwn_modes_args& a, hipStream_t s) { return launch_orth(a.Y, a.ldy, a.Q, a.ldq, a.N, a.p, nullptr, s); }

int k_modes_small_eigh(const dwn_modes_args& a, hipStream_t s) {
    hipLaunchKernelGGL(modes_small_kernel, dim3(1), dim3(MD_NT), 0, s, 0, (const double*)a.H, 0, a.p, a.values, a.W, (const int*)nullptr);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_modes_ritz(const dwn_modes_args& a, hipStream_t s) {
    hipLaunchKernelGGL(modes_status_kernel, dim3(1), dim3(MD_WAVE), 0, s, a.status);
    DWN_CHECK_LAUNCH();
    return launch_ritz(a.Q, a.ldq, a.Y, a.ldy, a.N, a.p, a.k, a.tol, a.values, a.W, a.V, a.ldv, (double*)a.ws, a.values, a.residuals,
                       a.status, s);
}

int k_modes_solve(const dwn_modes_args& a, hipStream_t s) {
    const int pp = pad16(a.p);
    char* w = (char*)a.ws;
    const size_t blk = up256((size_t)a.N * pp * sizeof(double));
    double* Q = (double*)w; w += blk;
    double* Y = (double*)w; w += blk;
    double* gpart = (double*)w; w += up256((size_t)nchunks(a.N) * MD_P * MD_P * sizeof(double));
    double* theta = (double*)w; w += up256(MD_P * sizeof(double));
    double* W = (double*)w; w += up256((size_t)MD_P * MD_P * sizeof(double));
    double* rpart = (double*)w; w += k_modes_ritz_ws_bytes(a.N);
    double* rowsq = (double*)w;
    const i64 total = (i64)a.N * pp;
    hipLaunchKernelGGL(modes_start_kernel, dim3((unsigned)((total + MD_NT - 1) / MD_NT)), dim3(MD_NT), 0, s, Q, (i64)pp, a.N, a.p, pp,
                       (unsigned)(a.seed & 0xffffffffull), (unsigned)(a.seed >> 32), a.status);
    DWN_CHECK_LAUNCH();
    int rc = launch_moments(a.A, a.lda, a.N, a.scale, rowsq, a.moments, s);
    if (rc) return rc;
    if ((rc = launch_orth(Q, pp, Q, pp, a.N, a.p, nullptr, s))) return rc;
    // one product before the first round: the basis lies in range(A), so the modes of a rank A does not have are exact zeros
    if ((rc = launch_symm(a.A, a.lda, a.N, Q, pp, a.p, a.scale, Y, pp, nullptr, s))) return rc;
    if ((rc = launch_orth(Y, pp, Q, pp, a.N, a.p, nullptr, s))) return rc;
    for (int it = 0; it < a.max_iters; ++it) {
        if ((rc = launch_symm(a.A, a.lda, a.N, Q, pp, a.p, a.scale, Y, pp, a.status, s))) return rc;
        if ((rc = launch_gram(Q, pp, a.p, Y, pp, a.p, a.N, gpart, a.status, s))) return rc;
        hipLaunchKernelGGL(modes_small_kernel, dim3(1), dim3(MD_NT), 0, s, 1, (const double*)gpart, nchunks(a.N), a.p, theta, W,
                           (const int*)a.status);
        DWN_CHECK_LAUNCH();
        if ((rc = launch_ritz(Q, pp, Y, pp, a.N, a.p, a.k, a.tol, theta, W, a.V, a.ldv, rpart, a.values, a.residuals, a.status, s))) return rc;
        if ((rc = launch_orth(Y, pp, Q, pp, a.N, a.p, a.status, s))) return rc;
    }
    hipLaunchKernelGGL(modes_sign_kernel, dim3((unsigned)a.p), dim3(MD_NT), 0, s, a.V, a.ldv, a.N);
    DWN_CHECK_LAUNCH();
    return 0;
}

int k_modes_overlap(const dwn_modes_args& a, hipStream_t s) {
    char* w = (char*)a.ws;
    double* gpart = (double*)w; w += up256((size_t)nchunks(a.N) * MD_P * MD_P * sizeof(double));
    double* W = (double*)w; w += up256((size_t)MD_P * MD_P * sizeof(double));
    int rc = launch_gram(a.Q, a.ldq, a.k, a.Y, a.ldy, a.k, a.N, gpart, nullptr, s);
    if (rc) return rc;
    hipLaunchKernelGGL(modes_small_kernel, dim3(1), dim3(MD_NT), 0, s, 2, (const double*)gpart, nchunks(a.N), a.k, a.values, W,
                       (const int*)nullptr);
    DWN_CHECK_LAUNCH();
    if (!a.A) return 0;
    const int pp = pad16(a.k);
    double* T = (double*)w; w += up256((size_t)a.N * pp * sizeof(double));
    double* rowsq = (double*)w;
    if ((rc = launch_moments(a.A, a.lda, a.N, a.scale, rowsq, a.moments, s))) return rc;
    if ((rc = launch_symm(a.A, a.lda, a.N, a.Q, a.ldq, a.k, a.scale, T, pp, nullptr, s))) return rc;
    if ((rc = launch_gram(a.Q, a.ldq, a.k, T, pp, a.k, a.N, gpart, nullptr, s))) return rc;
    hipLaunchKernelGGL(modes_trace_fold_kernel, dim3(1), dim3(MD_WAVE), 0, s, (const double*)gpart, nchunks(a.N), a.k, a.moments + 2);
    DWN_CHECK_LAUNCH();
    return 0;
}

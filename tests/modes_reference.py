"""Float64 checker of the population modes: the start block bit for bit (the Philox of
tests/rf_reference.py), the block subspace iteration restated in numpy, the case lists of the GPU tests and the a-priori bounds
they assert at.  The truth is numpy.linalg.eigh; residuals of returned pairs are recomputed in longdouble.  numpy only; written for
this project and held to eigh by tests/test_modes_reference_cpu.py.

Definitions (include/dwn.h): start block entry (i, c) = ((double) w + 0.5) 2^-31 - 1 with w = word c & 3 of philox4x32-10(counter =
(i, c >> 2, 0, 0), key = (seed & 0xffffffff, seed >> 32)); Q = orth(scale A orth(start)); one round: Y = scale A Q, H = sym(Q^T Y), H = W diag(theta) W^T with
theta descending, V = Q W, r_c = ||Y W e_c - theta_c V e_c||_2, stop when max_{i < k} r_i <= tol |theta_0|, else Q = orth(Y);
orth: classical Gram-Schmidt twice, a column whose norm after the projections is <= ORTH_C N u ||Y||_F becomes a zero column.

Bounds (u = 2^-53; every GPU assertion is at TWICE the bound given here):
  symm        |Y - scale A Q|_il <= (N + 4) u |scale| sum_j |A_ij| |Q_jl|: a quarter of the sum is a chain of at most N / 4 + 1 fused
              multiply-adds (one rounding each), the quarters are joined by three additions, the scale is one multiplication.
  moments     trace: (N / 256 + 9 + 1) u sum |A_ii| |scale| <= (N + 10) u ...; frobenius2: (N + 20) u sum A_ij^2 scale^2 (a row: N /
              256 fused terms and an 8-level tree, the rows: the same again, two multiplications by the scale).
  small_eigh  a rotation changes two rows and two columns with at most 4 roundings per element; a row is touched by 2 (p - 1)
              rotations per sweep; quadratic convergence ends the sweeps of a p <= 64 matrix within 8: the computed diagonal is
              that of a matrix within 64 p u ||H||_F of H, so every eigenvalue is within JACOBI_C p u ||H||_F (Weyl), JACOBI_C = 64.
              |W^T W - I| and |H W - W diag| / ||H||_F are of the same form.
  orth        entry (a, c), a < c, of Q^T Q: after the second pass the projection coefficient is a dot product of N terms of two
              unit-norm columns, error <= (N + 2) u, its removal adds p roundings per earlier column, <= p^2 u in all; the
              diagonal carries the normalisation, <= (N + 4) u: max |Q^T Q - I| <= (2 N + p^2 + 8) u.  (Twice is enough: the
              first pass leaves at most (N + p) u kappa(Y), which the second reduces to the level above unless the column
              was dropped as dependent.)
  vectors     V = Q W: the two above and the p-term rotation: (2 N + p^2 + 8) u + (JACOBI_C p + 2 p) u.
  residuals   reported against recomputed from the returned pair: the issue's form (N + c) u ||A||_F with c = 2 p + 8 (the
              product, the two rotations, the norm).  A worst-case derivation carries a further sqrt(p) (the column of W spreads
              over p columns of Y); the test asserts the tighter form.
  values      for a symmetric A every theta is within ||A v - theta v|| / ||v|| of an eigenvalue; on a gapped case |theta_i -
              lambda_i| <= r_i^2 / gap_i (Kato-Temple), gap_i the distance from theta_i to the nearest OTHER eigenvalue; the
              floor EIG_C N u ||A||_2, EIG_C = 4, stands for eigh's own error and the rounding of the Rayleigh quotient.
  subspace    sin of the largest principal angle between V_k and eigh's top k <= ||R_k||_F / (theta_k - lambda_{k+1})
              (Davis-Kahan), plus the floor over the same gap and the orthonormality bound of V.
  cosines     M = Va^T Vb carries (N + 2) u per entry (columns of norm <= 1), so its singular values move by at most k (N + 2) u
              (Weyl); they are returned as the square roots of the eigenvalues of M^T M, which carry e2 = (JACOBI_C k + k + 2) u
              ||M||_F^2: |sigma - sigma_ref| <= k (N + 2) u + min(sqrt(e2), e2 / sigma_ref).  A cosine near 0 next to one near 1
              is therefore known to about 1e-7 only; cosines that are all small, or all near 1, to a few hundred u."""
import numpy as np

from tests import rf_reference as rf

U = 2.0 ** -53
ORTH_C = 8.0
JACOBI_C = 64.0
EIG_C = 4.0
MAXP = 64
LANE_NS = (1, 15, 16, 17, 63, 64, 65, 129, 130)
LANE_PS = (1, 16, 17, 32, 64)
EIGH_PS = (1, 2, 3, 16, 17, 64)


def start_block(N, p, seed=0):
    """float64 [N, p]: every entry a function of (seed, row, column) alone."""
    nblk = (p + 3) // 4
    key = (seed & rf.MASK, (seed >> 32) & rf.MASK)
    w = rf.philox(np.arange(N, dtype=np.uint64)[:, None], np.arange(nblk, dtype=np.uint64)[None, :], np.uint64(0), np.uint64(0), key)
    w = w.reshape(N, nblk * 4)[:, :p].astype(np.float64)
    return (w + 0.5) * 2.0 ** -31 - 1.0


def orth(Y):
    """Classical Gram-Schmidt, twice, with the drop rule of the kernel."""
    N, p = Y.shape
    Q = np.array(Y, dtype=np.float64)
    tau = ORTH_C * N * U * np.sqrt((Q * Q).sum())
    for c in range(p):
        for _ in range(2):
            Q[:, c] -= Q[:, :c] @ (Q[:, :c].T @ Q[:, c])
        nrm = np.sqrt((Q[:, c] ** 2).sum())
        Q[:, c] = 0.0 if nrm <= tau else Q[:, c] / nrm
    return Q


def sign_rule(V):
    """Every column's entry of largest magnitude (lowest index on ties) made positive."""
    V = np.array(V)
    for c in range(V.shape[1]):
        if V[np.argmax(np.abs(V[:, c])), c] < 0:
            V[:, c] = -V[:, c]
    return V


def small_eigh(H):
    """eigh, descending, with the sign rule."""
    w, W = np.linalg.eigh(H)
    return w[::-1].copy(), sign_rule(W[:, ::-1])


def iterate(A, k, oversample=8, max_iters=64, tol=1e-10, seed=0, scale=1.0, mutate=None):
    """The iteration of dwn_modes_solve restated: dict(values, vectors, residuals, converged, rounds).  ``mutate``: one of the
    mistakes the bounds must catch ('raw_residual': residuals against the un-rotated Y; 'unsorted': eigenvalues left as eigh
    orders them; 'no_scale': the scale dropped)."""
    N = A.shape[0]
    p = min(k + oversample, N)
    s = 1.0 if mutate == "no_scale" else scale
    Q = orth(s * (A @ orth(start_block(N, p, seed))))          # one product before the first round: the basis lies in range(A)
    theta, V, r, conv, rounds = np.zeros(p), np.zeros((N, p)), np.zeros(p), False, 0
    for _ in range(max_iters):
        Y = s * (A @ Q)
        H = Q.T @ Y
        H = 0.5 * (H + H.T)
        if not np.isfinite(H).all():
            theta, r, rounds = np.full(p, np.nan), np.full(p, np.nan), rounds + 1
            break
        theta, W = small_eigh(H)
        if mutate == "unsorted":
            theta, W = theta[::-1].copy(), W[:, ::-1]
        V = Q @ W
        R = (Y if mutate == "raw_residual" else Y @ W) - V * theta
        r = np.sqrt((R * R).sum(axis=0))
        rounds += 1
        if (r[:k] <= tol * abs(theta[0])).all():
            conv = True
            break
        Q = orth(Y)
    return dict(values=theta[:k], vectors=sign_rule(V[:, :k]), residuals=r[:k], converged=conv, rounds=rounds)


def planted(N, spectrum, seed, tail=1.0):
    """A symmetric [N, N] matrix with the given leading eigenvalues and a tail uniform in [0, tail], bit-symmetric."""
    rng = np.random.default_rng(seed)
    lam = np.zeros(N)
    m = min(N, len(spectrum))
    lam[:m] = spectrum[:m]
    if tail > 0 and N > m:
        lam[m:] = np.sort(rng.uniform(0, tail, N - m))[::-1]
    E, _ = np.linalg.qr(rng.normal(size=(N, N)))
    A = (E * lam) @ E.T
    return 0.5 * (A + A.T)


GAPPED = (50.0, 30.0, 20.0, 12.0, 8.0, 5.0)
# name, N, matrix builder, k, oversample, gapped, converges (the GPU test asserts `converged` and the CPU test half of max_iters)
SOLVE_CASES = (
    [(f"gapped-{N}", N, (lambda N=N: planted(N, GAPPED, 100 + N)), min(6, N), 10, True, True) for N in (15, 16, 17, 63, 64, 65, 129, 130)] +
    [("slow-130", 130, lambda: planted(130, tuple(1.0 / (1 + i) for i in range(130)), 7, tail=0.0), 4, 12, False, True),
     ("rank3-40", 40, lambda: planted(40, (9.0, 4.0, 1.0), 11, tail=0.0), 5, 8, False, True),
     ("k1-63", 63, lambda: planted(63, GAPPED, 12), 1, 8, True, True),
     ("kN-15", 15, lambda: planted(15, GAPPED, 13), 15, 8, False, True),
     ("one", 1, lambda: np.array([[3.0]]), 1, 8, False, True)])
MAX_ITERS, TOL = 64, 1e-10


def lane_pin_operands(N, p, lda_pad, scale_exp, seed):
    """Small-integer A = A^T (no further symmetry) in a [N, N + lda_pad] array and Q [N, p] with distinct rows and columns: every
    product and sum is exact in float64."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-7, 8, size=(N, N)).astype(np.float64)
    A = np.tril(A) + np.tril(A, -1).T
    A += np.diag(np.arange(N) % 5)
    Q = rng.integers(-5, 6, size=(N, p)).astype(np.float64) + 16.0 * np.arange(p)[None, :] + 1024.0 * np.arange(N)[:, None]
    store = np.full((N, N + lda_pad), 777.0)
    store[:, :N] = A
    return store, Q, 2.0 ** scale_exp


def symm_bound(A, Q, scale):
    return (A.shape[0] + 4) * U * abs(scale) * (np.abs(A) @ np.abs(Q))


def symm_mutants(A, Q, scale):
    """What a wrong kernel would return: the f32 C/D row map (row 4 (lane >> 4) + reg where the f64 form has (lane >> 4) + 4 reg),
    Q read transposed inside its 16 x 16 tiles, the scale dropped."""
    N, p = Q.shape
    Y = scale * (A @ Q)
    out = {}
    rows = np.arange(N)
    blk, r = rows // 16 * 16, rows % 16
    src = blk + (r % 4) * 4 + r // 4
    out["f32_row_map"] = Y[np.minimum(src, N - 1)]
    Np, pp = -(-N // 16) * 16, -(-p // 16) * 16
    Qp = np.zeros((Np, max(pp, 16)))
    Qp[:N, :p] = Q
    Qt = Qp.copy()
    for i in range(0, Np, 16):
        for j in range(0, Qp.shape[1], 16):
            Qt[i:i + 16, j:j + 16] = Qp[i:i + 16, j:j + 16].T
    out["transposed_q"] = scale * (A @ Qt[:N, :p])
    out["no_scale"] = A @ Q
    return out


def moments_bounds(A, scale):
    N = A.shape[0]
    return (N + 10) * U * abs(scale) * np.abs(np.diag(A)).sum(), (N + 20) * U * scale * scale * (A * A).sum()


def eigh_bound(H):
    return JACOBI_C * H.shape[0] * U * np.sqrt((H * H).sum())


def orth_bound(N, p):
    return (2 * N + p * p + 8) * U


def vectors_bound(N, p):
    return orth_bound(N, p) + (JACOBI_C * p + 2 * p) * U


def residual_bound(A, p):
    return (A.shape[0] + 2 * p + 8) * U * np.sqrt((A * A).sum())


def true_residuals(A, values, vectors):
    """||A v - theta v||_2 of each returned pair, in longdouble."""
    Al, Vl = A.astype(np.longdouble), vectors.astype(np.longdouble)
    R = Al @ Vl - Vl * values.astype(np.longdouble)
    return np.sqrt((R * R).sum(axis=0)).astype(np.float64), R.astype(np.float64)


def check_pairs(A, values, vectors, residuals, k, p, gapped, label=""):
    """Every path-independent claim about returned pairs of the symmetric matrix A, at TWICE the bounds of the header; returns the
    worst ratio to the single bound of each claim (for DESIGN.md 12u)."""
    N = A.shape[0]
    lam, E = np.linalg.eigh(A)
    lam, E = lam[::-1], E[:, ::-1]
    norm2 = max(abs(lam[0]), abs(lam[-1]))
    floor = EIG_C * N * U * norm2
    rc, R = true_residuals(A, values, vectors)
    live = np.abs(vectors).sum(axis=0) > 0                      # a zero column: the mode of a rank the matrix does not have
    ratios = {}
    assert (np.diff(values) <= 0).all(), f"{label}: values not descending: {values}"
    assert np.array_equal(sign_rule(vectors), vectors), f"{label}: the sign rule does not hold"
    G = vectors[:, live].T @ vectors[:, live]
    ratios["orthonormal"] = np.abs(G - np.eye(G.shape[0])).max() / vectors_bound(N, p) if live.any() else 0.0
    assert ratios["orthonormal"] <= 2, f"{label}: |V^T V - I| is {ratios['orthonormal']:.3g} bounds"
    assert (values[~live] == 0).all() and (residuals[~live] == 0).all(), f"{label}: a zero mode with a value"
    rb = residual_bound(A, p)
    ratios["residual"] = np.abs(residuals - rc).max() / rb if rb > 0 else 0.0
    assert ratios["residual"] <= 2, f"{label}: reported and recomputed residuals differ by {ratios['residual']:.3g} bounds"
    near = np.abs(values[:, None] - lam[None, :]).min(axis=1)
    ratios["eigenvalue"] = (near / (rc + floor)).max() if floor > 0 else float(near.max() > 0)
    assert ratios["eigenvalue"] <= 2, f"{label}: a value is {ratios['eigenvalue']:.3g} bounds from every eigenvalue"
    if gapped:
        kt, dk_gap = [], values[k - 1] - (lam[k] if k < N else -np.inf)
        for i in range(k):
            gap = np.abs(np.delete(lam, i) - values[i]).min()
            kt.append(abs(values[i] - lam[i]) / (rc[i] ** 2 / gap + floor))
        ratios["kato_temple"] = max(kt)
        assert ratios["kato_temple"] <= 2, f"{label}: Kato-Temple missed by {ratios['kato_temple']:.3g}"
        if k < N:
            Ek = E[:, :k]
            sin = np.linalg.norm(vectors - Ek @ (Ek.T @ vectors), 2)
            bound = np.sqrt((R * R).sum()) / dk_gap + floor / dk_gap + vectors_bound(N, p)
            ratios["davis_kahan"] = sin / bound
            assert ratios["davis_kahan"] <= 2, f"{label}: Davis-Kahan missed by {ratios['davis_kahan']:.3g}"
    return ratios


def cosines(Va, Vb):
    return np.linalg.svd(Va.T @ Vb, compute_uv=False)


def cosine_bound(sigma_ref, N, k):
    dM = k * (N + 2) * U
    e2 = (JACOBI_C * k + k + 2) * U * float((sigma_ref ** 2).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        return dM + np.where(sigma_ref > 0, np.minimum(np.sqrt(e2), e2 / np.maximum(sigma_ref, 1e-300)), np.sqrt(e2))


def captured(Va, B, scale=1.0):
    """(tr(Va^T scale B Va) / tr(scale B), its bound): the products carry (N + 4) u and (N / 256 + 34) u relative to the sums of
    magnitudes, the traces (N + 10) u."""
    num, den = np.trace(Va.T @ (scale * B) @ Va), scale * np.trace(B)
    mag = np.trace(np.abs(Va).T @ (abs(scale) * np.abs(B)) @ np.abs(Va))
    return num / den, ((2 * B.shape[0] + 48) * U * mag + (B.shape[0] + 10) * U * abs(num)) / abs(den)

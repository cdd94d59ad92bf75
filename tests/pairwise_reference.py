"""Float64 / longdouble checker of the population structure (sensorium_amd/population.py, csrc/dwn_pairwise.hip).

Plain numpy, every definition in its obvious concatenate-and-centre form, sums in ``numpy.longdouble`` where the platform has one
(U_REF of tests/trial_score_reference.py says what it is).  A trial is ``(Y, group)``: responses ``[N, K]`` over its KEPT frames
(the cut is the caller's) and a group id or None; a group id carried by one trial counts as no group.  Nothing in this file was
fitted to a measurement.

Sample sets (``sample_sets``), with ybar[g] the average over the R >= 2 repeats of group g:
    total   every (trial, frame): y                          signal  (group, frame): ybar
    noise   (group, repeat, frame): y - ybar, and NO degrees-of-freedom correction: its co-moment is divided by R K.
``comoments`` is the two-pass form  C_ij = sum (x_i - mean_i)(x_j - mean_j),  ``corr_matrix`` the project's ``corr`` convention
(C_ij / n) / ((sqrt(C_ii / n) + eps)(sqrt(C_jj / n) + eps)), ``compare`` the per-neuron and the all-pairs Pearson correlation of
two matrices over the off-diagonal entries.

The chunking restated (``chunks``, ``stage``, ``emulate``): a chunk is one trial (total) or one repeat group (signal, noise), in
the order the tables hold them (repeat groups and single trials in order of first appearance, the trials of a group together).
The kernels centre a chunk about its own mean m_b, append the column sqrt(na nb / (na + nb)) (m_b - m_a) — m_a, na the running
mean and count — pad with zero columns to the k-step 4, advance the mean by (m_b - m_a) nb / (na + nb), and add Z Z^T.

Error bounds (u = 2^-53; first order, constants rounded up so that second-order terms are covered for n u < 2^-20)
-------------------------------------------------------------------------------------------------------------------------------
Let A_i >= |value| of neuron i (2 max|y| for the noise set), n the samples, G the chunks, Rmax the most repeats of a group.
 (a) every mean the kernels hold (chunk or running) errs by at most (n_src + 6 G + 8) u A_i, n_src the raw values behind the set
     (tests/trial_score_reference.py (a), (e)); a repeat average, and so every value derived from one, errs by (Rmax + 2) u A_i.
     Both are folded into  e_i = (n_src + 6 G + 8 + 2 (Rmax + 2)) u A_i.
 (b) inside a chunk the staged value is z = a + d + rho: a the exactly centred value, d the (constant) error of the centre, rho
     the rounding / repeat-average error of the value.  sum_k a_k = 0 exactly, so  sum z_i z_j - sum a_i a_j = n_b d_i d_j +
     sum (a_i rho_j + a_j rho_i) + ...: the centre enters in SECOND order, the value errors give at most
     e_j sqrt(n_b W_i) + e_i sqrt(n_b W_j) (Cauchy-Schwarz; W the chunk's own moment) plus 2 u sqrt(W_i W_j).
 (c) the merge column c D, c = sqrt(na nb / n) <= sqrt(nb), D = m_b - m_a known to 2 e: its product errs by at most
     2 sqrt(nb) (sqrt(X_i) e_j + sqrt(X_j) e_i) + 8 u sqrt(X_i X_j) + 4 nb e_i e_j, X = c^2 D^2 the merge's share of C_ii.  This is
     the price of merging — FIRST order in the error of a mean — and over all chunks sum sqrt(nb X_b) and sum sqrt(nb W_b) are each at
     most sqrt(n C_ii) (Cauchy-Schwarz).
 (d) the product is one float64 accumulator per element over n + G non-zero columns in a fixed order: any order errs by at most
     (n + G) u sum_k |z_ki z_kj| <= (n + G) u sqrt(C_ii C_jj).
 Together, per element — the form of c_bound of 12o with (Ma, Mb) = (C_ii, C_jj), which is what is used:
     E_C(i, j) = (n + 8 G + 16) u sqrt(C_ii C_jj) + 4 (e_i sqrt(n C_jj) + e_j sqrt(n C_ii)) + 10 n e_i e_j + (n + 16) U_REF sqrt(C_ii C_jj)
 (the last term is the checker's own sums).  No condition number of C_ij itself appears.
 Correlation matrix: pearson_bound of 12o element by element (``corr_bound``); an element of a constant neuron's row has no
 bound (inf): there the kernels' sums are exact and 0 is asserted exactly.
 Comparison of two GIVEN matrices: a two-sweep Pearson over n = M - 1 entries is inside pearson_bound(n, 1, ...) and the
 all-pairs one, merged from M rows, inside pearson_bound(pairs, M, ...).  When the matrices themselves carry errors EA, EB
 (``compare_propagated_bound``):  dr = sum_j EA_j (|db_j| / (n sa sb) + |r| |da_j| / (n sa^2)) + the same with a and b exchanged.
The tests assert at TWICE these bounds.
"""
import numpy as np

from tests.trial_score_reference import LD, U, U_REF, c_bound, m2_bound, mean_err, pearson_bound, split_groups  # noqa: F401

KINDS = ("total", "signal", "noise")
KSTEP = 4


def units_of(trials):
    """(repeat groups, all units) of ``[(Y, group), ...]``: lists of ``[N, K]`` arrays, in table order."""
    groups, units = split_groups([(y, y, g) for y, g in trials])
    return [[y for _, y in u] for u in groups], [[y for _, y in u] for u in units]


def sample_sets(trials):
    """kind -> longdouble [N, n]: the concatenation every definition is written over."""
    groups, units = units_of(trials)
    N = units[0][0].shape[0]
    cat = lambda parts: np.concatenate(parts, axis=1) if parts else np.zeros((N, 0), dtype=LD)      # noqa: E731
    total = cat([y.astype(LD) for u in units for y in u])
    signal, noise = [], []
    for g in groups:
        Y = np.stack([y.astype(LD) for y in g])                 # [R, N, K]
        ybar = Y.mean(axis=0)
        signal.append(ybar)
        noise.extend(list(Y - ybar[None]))
    return {"total": total, "signal": cat(signal), "noise": cat(noise)}


def comoments(X):
    """Two-pass longdouble: (mean [N], C [N, N]); zeros for an empty set."""
    N, n = X.shape
    if n == 0:
        return np.zeros(N, dtype=LD), np.zeros((N, N), dtype=LD)
    m = X.mean(axis=1)
    D = X - m[:, None]
    return m, D @ D.T


def comoments_loop(X):
    """The same once more as a brute-force triple loop in float64 python scalars (small cases only)."""
    N, n = X.shape
    m = [sum(float(v) for v in X[i]) / n for i in range(N)]
    C = np.zeros((N, N))
    for i in range(N):
        for j in range(N):
            C[i, j] = sum((float(X[i, k]) - m[i]) * (float(X[j, k]) - m[j]) for k in range(n))
    return np.array(m), C


def corr_matrix(C, n, eps=1e-8):
    """The project's ``corr`` convention on a co-moment matrix; NaN everywhere for n = 0."""
    N = C.shape[0]
    if n == 0:
        return np.full((N, N), np.nan)
    C = np.asarray(C, dtype=LD)
    s = np.sqrt(np.diag(C) / n) + LD(eps)
    return np.asarray((C / n) / (s[:, None] * s[None, :]), dtype=np.float64)


def compare(A, B, sel=None, eps=1e-8):
    """(per_neuron [M], summary [8]) of two [N, N] matrices over the selected off-diagonal entries: per selected row the Pearson
    correlation (``corr`` convention) of A[i, j] with B[i, j]; summary = ordered pairs, Pearson over all, mean A, mean B, std A,
    std B, mean |A - B|, RMS of A - B.  A NaN entry makes its row and the summary NaN."""
    A, B = np.asarray(A, dtype=LD), np.asarray(B, dtype=LD)
    sel = np.arange(A.shape[0]) if sel is None else np.asarray(sel)
    M = len(sel)
    a, b = A[np.ix_(sel, sel)], B[np.ix_(sel, sel)]
    off = ~np.eye(M, dtype=bool)
    per = np.full(M, np.nan)
    for m in range(M):
        x, y = a[m][off[m]], b[m][off[m]]
        if len(x):
            dx, dy = x - x.mean(), y - y.mean()
            sx, sy = np.sqrt((dx * dx).mean()), np.sqrt((dy * dy).mean())
            per[m] = float((dx * dy).mean() / ((sx + LD(eps)) * (sy + LD(eps))))
    x, y = a[off], b[off]
    summary = np.full(8, np.nan)
    summary[0] = len(x)
    if len(x) and not (np.isnan(x).any() or np.isnan(y).any()):       # a NaN entry on either side: all of it is NaN
        dx, dy = x - x.mean(), y - y.mean()
        sx, sy = np.sqrt((dx * dx).mean()), np.sqrt((dy * dy).mean())
        summary[1:] = [float(v) for v in ((dx * dy).mean() / ((sx + LD(eps)) * (sy + LD(eps))), x.mean(), y.mean(), sx, sy,
                                          np.abs(x - y).mean(), np.sqrt(((x - y) ** 2).mean()))]
    return per, summary


# ---- the chunking restated, in float64 as the kernels compute ----
def chunks(trials, kind, noise_about_grand_mean=False):
    """The chunks of ``kind`` in table order: float64 [N, n_b] value arrays (NOT yet centred about the chunk mean)."""
    groups, units = units_of(trials)
    out = []
    for u in units:
        if kind == "total":
            out.extend(y.astype(np.float64) for y in u)
        elif len(u) >= 2:
            Y = np.stack([y.astype(np.float64) for y in u])
            ybar = Y.sum(axis=0) / len(u)
            if kind == "signal":
                out.append(ybar)
            else:
                centre = Y.mean(axis=(0, 2))[None, :, None] if noise_about_grand_mean else ybar[None]
                out.append(np.concatenate(list(Y - centre), axis=1))
    return out


def stage(chs, mean, count, drop_merge=False):
    """Z [cols, N] float64 of a list of chunks against the running (mean [N], count); returns (Z, mean, count)."""
    N = chs[0].shape[0]
    cols_out = []
    mean = np.array(mean, dtype=np.float64)
    for v in chs:
        nb = v.shape[1]
        mb = v.sum(axis=1) / nb
        cols_out.append((v - mb[:, None]).T)
        merge = np.zeros(N)
        if count > 0:
            n = count + nb
            if not drop_merge:
                merge = np.sqrt(count * nb / n) * (mb - mean)
            mean = mean + (mb - mean) * (nb / n)
        else:
            mean = mb.copy()
        cols_out.append(merge[None])
        pad = -(nb + 1) % KSTEP
        if pad:
            cols_out.append(np.zeros((pad, N)))
        count += nb
    return np.concatenate(cols_out, axis=0), mean, count


def emulate(trials, kind, flush_after=(), **mutation):
    """The kernels' path in float64: (C, mean, count) after flushing the chunk list in the pieces ``flush_after`` cuts (indices
    into the chunk list).  ``mutation``: ``drop_merge`` / ``noise_about_grand_mean``."""
    chs = chunks(trials, kind, noise_about_grand_mean=mutation.get("noise_about_grand_mean", False))
    N = trials[0][0].shape[0]
    C, mean, count = np.zeros((N, N)), np.zeros(N), 0
    cuts = [0] + sorted(set(flush_after)) + [len(chs)]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        if hi > lo:
            Z, mean, count = stage(chs[lo:hi], mean, count, drop_merge=mutation.get("drop_merge", False))
            for k0 in range(0, Z.shape[0], KSTEP):          # one accumulator, ascending k, a k-step at a time
                C = C + Z[k0:k0 + KSTEP].T @ Z[k0:k0 + KSTEP]
    return C, mean, count


def raw_sum_comoments(X):
    """What the checker guards against: sum x_i x_j - n mean_i mean_j in float64."""
    X = np.asarray(X, dtype=np.float64)
    n = X.shape[1]
    m = X.sum(axis=1) / n
    return X @ X.T - n * np.outer(m, m)


# ---- the MFMA f64 16x16x4 C/D lane map (cdna: col = lane & 15, row = (lane >> 4) + 4 reg) and what a wrong one does ----
def mfma_f64_store(D, rowmap="f64"):
    """A 16 x 16 result tile as a kernel writes it when it believes ``rowmap``: the hardware holds D[(lane >> 4) + 4 reg][lane & 15]
    in (lane, reg); the kernel stores it at the row its formula gives."""
    out = np.zeros_like(D)
    for lane in range(64):
        for reg in range(4):
            row = (lane >> 4) + 4 * reg if rowmap == "f64" else 4 * (lane >> 4) + reg
            out[row, lane & 15] = D[(lane >> 4) + 4 * reg, lane & 15]
    return out


# ---- bounds ----
def set_stats(trials, kind):
    """(n, G, n_src, Rmax, A [N]) of a sample set."""
    groups, units = units_of(trials)
    N = units[0][0].shape[0]
    src = [y for u in units for y in u] if kind == "total" else [y for g in groups for y in g]
    n_src = sum(y.shape[1] for y in src)
    A = np.max([np.abs(y.astype(np.float64)).max(axis=1) for y in src], axis=0) if src else np.zeros(N)
    Rmax = max([len(g) for g in groups], default=1)
    if kind == "total":
        return n_src, len(src), n_src, 1, A
    if kind == "signal":
        return sum(g[0].shape[1] for g in groups), len(groups), n_src, Rmax, A
    return n_src, len(groups), n_src, Rmax, 2.0 * A


def value_err(n_src, G, Rmax, A):
    return (n_src + 6 * G + 8 + 2 * (Rmax + 2)) * U * np.asarray(A, dtype=np.float64)


def comoment_bound(trials, kind, C):
    """[N, N]: E_C of the docstring for the co-moments ``C`` (the checker's) of ``kind``."""
    n, G, n_src, Rmax, A = set_stats(trials, kind)
    d = np.diag(np.asarray(C, dtype=np.float64))
    e = value_err(n_src, G, Rmax, A)
    S = np.sqrt(np.outer(d, d))
    return ((n + 8 * G + 16) * U * S + 4 * (np.outer(e, np.sqrt(n * d)) + np.outer(np.sqrt(n * d), e)) + 10 * n * np.outer(e, e)
            + (n + 16) * U_REF * S)


def corr_bound(trials, kind, C, eps=1e-8):
    """[N, N]: the bound of the correlation matrix; inf in the rows and columns of a neuron with C_ii = 0."""
    n, G, n_src, Rmax, A = set_stats(trials, kind)
    C = np.asarray(C, dtype=np.float64)
    d = np.diag(C)
    EC = comoment_bound(trials, kind, C)
    s = np.sqrt(d / max(n, 1)) + eps
    den = max(n, 1) * np.outer(s, s)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.diag(EC) / (2 * d) + 4 * U
        b = EC / den + np.abs(C / den) * (rel[:, None] + rel[None, :] + 8 * U)
    ok = d > 0
    return np.where(np.outer(ok, ok), b, np.inf)


def compare_bound(A, B, sel=None, eps=1e-8):
    """(per_neuron bound [M], summary bound [8]) for two GIVEN matrices (no input error)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    sel = np.arange(A.shape[0]) if sel is None else np.asarray(sel)
    M = len(sel)
    a, b = A[np.ix_(sel, sel)], B[np.ix_(sel, sel)]
    off = ~np.eye(M, dtype=bool)
    per = np.full(M, np.inf)
    n = M - 1
    for m in range(M):
        x, y = a[m][off[m]], b[m][off[m]]
        if n > 0 and np.isfinite(x).all() and np.isfinite(y).all():
            dx, dy = x - x.mean(), y - y.mean()
            per[m] = pearson_bound(n, 1, (dx * dx).sum(), (dy * dy).sum(), (dx * dy).sum(), np.abs(x).max(), np.abs(y).max(), eps)
    x, y = a[off], b[off]
    sb = np.full(8, np.inf)
    sb[0] = 0.0
    if len(x) and np.isfinite(x).all() and np.isfinite(y).all():
        p = len(x)
        dx, dy = x - x.mean(), y - y.mean()
        Mx, My, Ax, Ay = (dx * dx).sum(), (dy * dy).sum(), np.abs(x).max(), np.abs(y).max()
        sb[1] = pearson_bound(p, M, Mx, My, (dx * dy).sum(), Ax, Ay, eps)
        sb[2], sb[3] = mean_err(p, M, Ax), mean_err(p, M, Ay)
        with np.errstate(divide="ignore", invalid="ignore"):
            sb[4] = np.sqrt(Mx / p) * (m2_bound(p, M, Mx, Ax) / (2 * Mx) + 4 * U) if Mx > 0 else np.inf
            sb[5] = np.sqrt(My / p) * (m2_bound(p, M, My, Ay) / (2 * My) + 4 * U) if My > 0 else np.inf
        sb[6] = (p + M + 8) * (U + U_REF) * np.abs(x - y).mean()
        sb[7] = (p + M + 8) * (U + U_REF) * np.sqrt(((x - y) ** 2).mean())
    return per, sb


def compare_propagated_bound(A, B, EA, EB, sel=None, eps=1e-8):
    """[M]: how far per_neuron may move when A and B are only known to EA, EB entry by entry (first order, times 9/8), on top
    of ``compare_bound``."""
    A, B, EA, EB = (np.asarray(x, dtype=np.float64) for x in (A, B, EA, EB))
    sel = np.arange(A.shape[0]) if sel is None else np.asarray(sel)
    M = len(sel)
    off = ~np.eye(M, dtype=bool)
    ix = np.ix_(sel, sel)
    out = np.full(M, np.inf)
    base, _ = compare_bound(A, B, sel, eps)
    for m in range(M):
        x, y, ex, ey = (t[ix][m][off[m]] for t in (A, B, EA, EB))
        n = len(x)
        if n == 0 or not (np.isfinite(x).all() and np.isfinite(y).all() and np.isfinite(ex).all() and np.isfinite(ey).all()):
            continue
        dx, dy = x - x.mean(), y - y.mean()
        sx, sy = np.sqrt((dx * dx).mean()), np.sqrt((dy * dy).mean())
        if sx == 0 or sy == 0:
            continue
        r = (dx * dy).mean() / (sx * sy)
        # centring a perturbation cannot enlarge its 1-norm by more than a factor 2
        dr = (2 * ex * (np.abs(dy) / (n * sx * sy) + abs(r) * np.abs(dx) / (n * sx * sx))).sum()
        dr += (2 * ey * (np.abs(dx) / (n * sx * sy) + abs(r) * np.abs(dy) / (n * sy * sy))).sum()
        out[m] = base[m] + 1.125 * dr
    return out

"""Float64 checker of the trial-level scores (sensorium_amd/evaluation.py, csrc/dwn_trial_score.hip).

Plain numpy, every definition in its obvious concatenate-and-``np.var`` form, sums in ``numpy.longdouble`` where the platform
has one (x86: 64-bit significand; elsewhere it is float64 and U_REF below says so).  A trial is ``(P, Y, group)``: prediction and
target ``[N, K]`` over its KEPT frames (the cut is applied by the caller) and a group id or None.  A group id carried by one trial
only counts as no group.  The GPU tests assert the bounds derived here; nothing in this file was fitted to a measurement.

Error bounds (u = 2^-53; first-order terms, every constant rounded up so that the second-order terms are covered for n u < 2^-20)
---------------------------------------------------------------------------------------------------------------------------------
The kernel handles one group g (R repeats x K frames, n_g = R K values x of one neuron, |x| <= A) at a time:
 (a) group mean  m^ = fl(sum x) / n_g.  A float64 sum of n_g terms in ANY order errs by at most (n_g - 1) u sum|x|, so
     |m^ - m| <= (n_g + 1) u A.  A frame mean over the R repeats errs by at most (R + 1) u A.
 (b) within-frame sum  W = sum_t sum_r (x_rt - c_t)^2 with c_t the computed frame mean, off by d_t.  Exactly,
     sum_r (x_r - c)^2 = sum_r (x_r - xbar)^2 + R (xbar - c)^2: the error of the centre enters in SECOND order, + R d_t^2.  The
     terms are not negative, so rounding and summation cost at most (n_g + 3) u W.
 (c) between-frame sum  B = sum_t (c_t - m^)^2 against sum_t a_t^2, a_t = xbar_t - m.  The centres are off by e_t = d_t - d_m,
     |e_t| <= 2 e: sum (a_t + e_t)^2 - sum a_t^2 = 2 sum a_t e_t + sum e_t^2, at most 4 e sqrt(K B) + 4 K e^2 (Cauchy-Schwarz).
     This is FIRST order in the error of a mean.  Group moment M_g = W + R B (exact identity), so
         |M_g^ - M_g| <= (n_g + 6) u M_g + 4 e sqrt(n_g M_g) + 5 n_g e^2.
     (R = 1: one sweep about m^, sum (x - m^)^2 = M_g + n_g d_m^2: inside the same bound.)
 (d) Chan merge k of the running (na, ma, Ma) with the group (nb, mb, Mb): M = Ma + Mb + X_k, X_k = D^2 na nb / n, D = mb - ma
     (exact identity).  The computed D is off by at most 2 e, so X_k is off by (na nb / n)(4 |D| e + 4 e^2)
     <= 4 e sqrt(nb X_k) + 4 nb e^2 (na nb / n <= nb), again FIRST order in e, plus 8 u relative for the roundings of one merge.
     Over all merges sum_k sqrt(nb X_k) <= sqrt(n M) (Cauchy-Schwarz, sum nb = n, sum X_k <= M), and likewise
     sum_g sqrt(n_g M_g) <= sqrt(n M).
 (e) every mean the kernel holds, group or running, after k merges:  |error| <= e = (n + 6 G + 8) u A  (a merge is the convex
     combination ma + D f, f = nb / n: the incoming errors combine convexly, its three roundings add at most 6 u A).
 Together, for a set of n values merged from G groups:
     E_M2(n, G, M, A)          = (n + 8 G + 16) u M + 8 e sqrt(n M) + 10 n e^2
     E_C (n, G, Ma, Mb, Aa, Ab) = (n + 8 G + 16) u sqrt(Ma Mb) + 4 (e_a sqrt(n Mb) + e_b sqrt(n Ma)) + 10 n e_a e_b
 where for the co-moment the sum of the |terms| is at most sqrt(Ma Mb) by Cauchy-Schwarz at every level (within, between, merge),
 so no condition number of C itself appears.  Sets C and D follow from the same W and B (M2ybar = B, M2loo = W / (R - 1)^2 + R B,
 C_y_loo = -W / (R - 1) + R B, |terms| <= sqrt(M2y M2loo) by Cauchy-Schwarz on (sqrt W, sqrt(R B))), so the same formulas hold.
 SSres = sum (y - p)^2 has no centre:  E_res = (n + G + 4) u SSres.   SSwithin = sum_g W_g / (R_g - 1) has only second-order
 centre terms:  E_ssw = (n + G + 8) u SSwithin + n e^2.
 The checker's own sums (longdouble, or pairwise float64) err by at most (n + 16) U_REF of the same magnitudes; this is added.

 Pearson  r = (C/n) / ((sa + eps)(sb + eps)), sa = sqrt(Ma / n):  the relative error of sa + eps is at most that of sa,
 E_Ma / (2 Ma) + 2 u, so
     |dr| <= E_C / (n (sa + eps)(sb + eps)) + |r| (E_Ma / (2 Ma) + E_Mb / (2 Mb) + 8 u)            (pearson_bound)
 In the form |dr| <= c n u:  c = 2 + 8 (A_a / s_a + A_b / s_b) + O(G / n).  The 2 is the part that needs nothing but
 Cauchy-Schwarz; the second term is the price of STREAMING: a mean is only known to e ~ n u A when the next group is merged,
 and (c), (d) see that error in first order.  A kernel that swept all trials twice would have c = 2 and could not be flushed.
 A neuron with Ma = 0 or Mb = 0 has no such bound (inf); there the kernel's sums are exact and r = 0 is asserted exactly.

 fev, feve:  TV = M2y / (n - 1), NV = SSwithin / n_gf, MSE = SSres / n with E_TV = E_M2 / (n - 1) + 2 u TV, E_NV = E_ssw / n_gf +
 2 u NV, E_MSE = E_res / n + 2 u MSE.  With the condition number kappa = TV / (TV - NV) and E_D = E_TV + E_NV + u (TV - NV):
     fev  = 1 / kappa:          |d fev|  <= fev  [kappa E_D / TV + E_TV / TV] + 4 u
     feve = 1 - (MSE - NV) / (TV - NV):
                                |d feve| <= kappa [(E_MSE + E_NV + u |MSE - NV|) / TV + |1 - feve| E_D / TV] + 4 u (1 + |1 - feve|)
 both times 9/8 for the second-order terms, valid while kappa E_D / TV <= 1/16 (otherwise inf: no bound is claimed).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
U_REF = float(np.finfo(LD).eps) / 2.0
STATE_ROWS = 17
SCORE_NAMES = ("single_trial_corr", "corr_to_average", "fev", "feve", "oracle_corr")


def frame_cut(x, skip_first=0, limit_length=None, skip_last=0):
    """The reference's slicing (src/submission.py:12-17), on the last axis."""
    if limit_length is not None:
        x = x[..., :limit_length]
    x = x[..., skip_first:]
    if skip_last:
        x = x[..., :-skip_last]
    return x


def split_groups(trials):
    """(repeat groups, in order of first appearance: lists of (P, Y)), ordered list of ALL units [(P, Y), ...] as the tables hold
    them: a unit is a repeat group or one trial."""
    members, order = {}, []
    for i, (P, Y, group) in enumerate(trials):
        key = ("g", group) if group is not None else ("t", i)
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append((np.asarray(P), np.asarray(Y)))
    units = [members[k] for k in order]
    for unit in units:
        if len({p.shape[1] for p, _ in unit}) != 1:
            raise ValueError("unequal lengths inside a group")
    return [u for u in units if len(u) >= 2], units


def _pearson(a, b, eps):
    """a, b [N, n] longdouble: the Pearson form of the definitions; NaN for n = 0."""
    n = a.shape[1]
    if n == 0:
        return np.full(a.shape[0], np.nan)
    da, db = a - a.mean(axis=1, keepdims=True), b - b.mean(axis=1, keepdims=True)
    sa, sb = np.sqrt((da * da).sum(axis=1) / n), np.sqrt((db * db).sum(axis=1) / n)
    return ((da * db).sum(axis=1) / n) / ((sa + LD(eps)) * (sb + LD(eps)))


def _concat(parts, N):
    return np.concatenate(parts, axis=1) if parts else np.zeros((N, 0), dtype=LD)


def views(trials):
    """The concatenations every definition is written over, longdouble [N, .]: P, Y of all trials; of the repeat trials; the
    averages over repeats; the leave-one-out means; the within-frame variances (ddof = 1) per (group, frame)."""
    groups, units = split_groups(trials)
    N = units[0][0][0].shape[0]
    Pa = _concat([p.astype(LD) for u in units for p, _ in u], N)
    Ya = _concat([y.astype(LD) for u in units for _, y in u], N)
    Pr, Yr, Pbar, Ybar, Loo, Within = [], [], [], [], [], []
    for g in groups:
        P = np.stack([p.astype(LD) for p, _ in g])                # [R, N, K]
        Y = np.stack([y.astype(LD) for _, y in g])
        R = P.shape[0]
        Pr.append(np.concatenate(list(P), axis=1)); Yr.append(np.concatenate(list(Y), axis=1))
        Pbar.append(P.mean(axis=0)); Ybar.append(Y.mean(axis=0))
        Loo.append(np.concatenate(list((R * Y.mean(axis=0)[None] - Y) / (R - 1)), axis=1))
        Within.append(np.var(Y, axis=0, ddof=1))
    return dict(N=N, Pa=Pa, Ya=Ya, Pr=_concat(Pr, N), Yr=_concat(Yr, N), Pbar=_concat(Pbar, N), Ybar=_concat(Ybar, N),
                Loo=_concat(Loo, N), Within=_concat(Within, N), n_groups=len(groups), n_units=len(units))


def scores(trials, eps=1e-8):
    """dict: the five scores [N] float64, the counts, and TV / NV / MSE (longdouble) for the bounds."""
    v = views(trials)
    N = v["N"]
    n_all, n_rep, n_gf = v["Pa"].shape[1], v["Yr"].shape[1], v["Ybar"].shape[1]
    out = {"single_trial_corr": _pearson(v["Pa"], v["Ya"], eps), "corr_to_average": _pearson(v["Pbar"], v["Ybar"], eps),
           "oracle_corr": _pearson(v["Yr"], v["Loo"], eps)}
    nan = np.full(N, np.nan, dtype=LD)
    if n_rep:
        TV = np.var(v["Yr"], axis=1, ddof=1)
        NV = v["Within"].mean(axis=1)
        MSE = ((v["Yr"] - v["Pr"]) ** 2).mean(axis=1)
        ok = (TV > 0) & (TV - NV > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["fev"] = np.where(ok, (TV - NV) / TV, nan)
            out["feve"] = np.where(ok, 1 - (MSE - NV) / (TV - NV), nan)
    else:
        TV = NV = MSE = nan
        out["fev"], out["feve"] = nan, nan
    out = {k: np.asarray(x, dtype=np.float64) for k, x in out.items()}
    out.update(n_all=n_all, n_repeat=n_rep, n_group_frames=n_gf, TV=TV, NV=NV, MSE=MSE)
    return out


def scores_loop(trials, eps=1e-8):
    """Scores 2 to 4 once more, element by element from the definitions (python loops over group, frame and repeat, float64
    accumulation about explicitly computed means): a second statement that shares no array expression with ``scores``."""
    groups, _ = split_groups(trials)
    N = trials[0][0].shape[0]
    out = {k: np.full(N, np.nan) for k in ("corr_to_average", "fev", "feve", "oracle_corr")}
    if not groups:
        return out
    for j in range(N):
        pb, yb, ys, los, res, within, kept = [], [], [], [], 0.0, 0.0, 0
        for g in groups:
            R, K = len(g), g[0][0].shape[1]
            for t in range(K):
                ps = [float(p[j, t]) for p, _ in g]
                yy = [float(y[j, t]) for _, y in g]
                pm, ym = sum(ps) / R, sum(yy) / R
                pb.append(pm); yb.append(ym)
                within += sum((y - ym) ** 2 for y in yy) / (R - 1)
                kept += 1
                for p, y in zip(ps, yy):
                    ys.append(y); los.append((R * ym - y) / (R - 1)); res += (y - p) ** 2
        def pear(a, b):
            n = len(a)
            ma, mb = sum(a) / n, sum(b) / n
            va = sum((x - ma) ** 2 for x in a) / n
            vb = sum((x - mb) ** 2 for x in b) / n
            c = sum((x - ma) * (y - mb) for x, y in zip(a, b)) / n
            return c / ((va ** 0.5 + eps) * (vb ** 0.5 + eps))
        out["corr_to_average"][j] = pear(pb, yb)
        out["oracle_corr"][j] = pear(ys, los)
        n = len(ys)
        my = sum(ys) / n
        TV = sum((y - my) ** 2 for y in ys) / (n - 1)
        NV, MSE = within / kept, res / n
        if TV > 0 and TV - NV > 0:
            out["fev"][j] = (TV - NV) / TV
            out["feve"][j] = 1 - (MSE - NV) / (TV - NV)
    return out


def moments(trials):
    """The kernel's state [17, N] (include/dwn.h) from the concatenations, float64; rows of an empty set are 0."""
    v = views(trials)
    st = np.zeros((STATE_ROWS, v["N"]), dtype=LD)

    def five(a, b, rows):
        if a.shape[1] == 0:
            return
        ma, mb = a.mean(axis=1), b.mean(axis=1)
        da, db = a - ma[:, None], b - mb[:, None]
        for r, x in zip(rows, (ma, mb, (da * da).sum(axis=1), (db * db).sum(axis=1), (da * db).sum(axis=1))):
            if r is not None:
                st[r] = x
    five(v["Pa"], v["Ya"], (0, 1, 2, 3, 4))
    five(v["Pbar"], v["Ybar"], (9, 10, 11, 12, 13))
    five(v["Yr"], v["Loo"], (5, 14, 6, 15, 16))
    if v["Yr"].shape[1]:
        st[7] = ((v["Yr"] - v["Pr"]) ** 2).sum(axis=1)
        st[8] = v["Within"].sum(axis=1)
    return st.astype(np.float64)


def summary(sc, fev_threshold=0.15):
    """[mean r1, mean r2, mean r4, mean of feve over fev >= threshold, their number, n_all, n_repeat, n_group_frames]"""
    with np.errstate(invalid="ignore"):
        mask = sc["fev"] >= fev_threshold
    feve = float(np.mean(sc["feve"][mask].astype(LD))) if mask.any() else float("nan")
    return np.array([float(np.mean(sc[k].astype(LD))) for k in ("single_trial_corr", "corr_to_average", "oracle_corr")]
                    + [feve, float(mask.sum()), sc["n_all"], sc["n_repeat"], sc["n_group_frames"]], dtype=np.float64)


# ---- the bounds of the docstring (numpy float64 arrays per neuron; n, G scalars) ----
def mean_err(n, G, A):
    return (n + 6 * G + 8) * U * np.asarray(A, dtype=np.float64)


def m2_bound(n, G, M, A):
    M = np.asarray(M, dtype=np.float64)
    e = mean_err(n, G, A)
    return (n + 8 * G + 16) * U * M + 8 * e * np.sqrt(n * M) + 10 * n * e * e + (n + 16) * U_REF * M


def c_bound(n, G, Ma, Mb, Aa, Ab):
    Ma, Mb = np.asarray(Ma, dtype=np.float64), np.asarray(Mb, dtype=np.float64)
    ea, eb = mean_err(n, G, Aa), mean_err(n, G, Ab)
    return ((n + 8 * G + 16) * U * np.sqrt(Ma * Mb) + 4 * (ea * np.sqrt(n * Mb) + eb * np.sqrt(n * Ma)) + 10 * n * ea * eb
            + (n + 16) * U_REF * np.sqrt(Ma * Mb))


def res_bound(n, G, ssres):
    return (n + G + 4) * U * np.asarray(ssres, dtype=np.float64) + (n + 16) * U_REF * np.asarray(ssres, dtype=np.float64)


def ssw_bound(n, G, ssw, A):
    e = mean_err(n, G, A)
    return (n + G + 8) * U * np.asarray(ssw, dtype=np.float64) + n * e * e + (n + 16) * U_REF * np.asarray(ssw, dtype=np.float64)


def pearson_bound(n, G, Ma, Mb, Cab, Aa, Ab, eps=1e-8):
    Ma, Mb, Cab = (np.asarray(x, dtype=np.float64) for x in (Ma, Mb, Cab))
    sa, sb = np.sqrt(Ma / n), np.sqrt(Mb / n)
    den = n * (sa + eps) * (sb + eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = m2_bound(n, G, Ma, Aa) / (2 * Ma) + m2_bound(n, G, Mb, Ab) / (2 * Mb) + 8 * U
        b = c_bound(n, G, Ma, Mb, Aa, Ab) / den + np.abs(Cab / den) * rel
    return np.where((Ma > 0) & (Mb > 0), b, np.inf)


def state_bounds(trials, st=None):
    """[17, N]: the bound of every state row for these trials (means: mean_err; moments: m2_bound / c_bound / res / ssw)."""
    v = views(trials)
    st = moments(trials) if st is None else st
    absmax = lambda a: np.abs(a).max(axis=1).astype(np.float64) if a.shape[1] else np.zeros(v["N"])
    Ap, Ay = absmax(v["Pa"]), absmax(v["Ya"])
    n_all, n_rep, n_gf = v["Pa"].shape[1], v["Yr"].shape[1], v["Ybar"].shape[1]
    Gu, Gg = v["n_units"], v["n_groups"]
    b = np.zeros_like(st)
    b[0], b[1] = mean_err(n_all, Gu, Ap), mean_err(n_all, Gu, Ay)
    b[2], b[3], b[4] = m2_bound(n_all, Gu, st[2], Ap), m2_bound(n_all, Gu, st[3], Ay), c_bound(n_all, Gu, st[2], st[3], Ap, Ay)
    if n_rep:
        b[5] = b[14] = mean_err(n_rep, Gg, Ay)
        b[6] = m2_bound(n_rep, Gg, st[6], Ay)
        b[7] = res_bound(n_rep, Gg, st[7])
        b[8] = ssw_bound(n_rep, Gg, st[8], Ay)
        # sets C and D inherit the errors of the n_rep element sums they are formed from (docstring): counts n_rep, not n_gf
        b[9], b[10] = mean_err(n_rep, Gg, Ap), mean_err(n_rep, Gg, Ay)
        b[11], b[12] = m2_bound(n_rep, Gg, st[11], Ap), m2_bound(n_rep, Gg, st[12], Ay)
        b[13] = c_bound(n_rep, Gg, st[11], st[12], Ap, Ay)
        b[15] = m2_bound(n_rep, Gg, st[15], Ay)
        b[16] = c_bound(n_rep, Gg, st[6], st[15], Ay, Ay)
    return b


def score_bounds(trials, eps=1e-8):
    """dict of [N] bounds for the five scores, plus kappa = TV / (TV - NV)."""
    v = views(trials)
    st = moments(trials)
    sc = scores(trials, eps)
    absmax = lambda a: np.abs(a).max(axis=1).astype(np.float64) if a.shape[1] else np.zeros(v["N"])
    Ap, Ay = absmax(v["Pa"]), absmax(v["Ya"])
    n_all, n_rep, n_gf = sc["n_all"], sc["n_repeat"], sc["n_group_frames"]
    Gu, Gg = v["n_units"], v["n_groups"]
    out = {"single_trial_corr": pearson_bound(n_all, Gu, st[2], st[3], st[4], Ap, Ay, eps)}
    inf = np.full(v["N"], np.inf)
    if not n_rep:
        out.update(corr_to_average=inf, fev=inf, feve=inf, oracle_corr=inf, kappa=inf)
        return out
    # set C: n_gf terms, but its sums carry the errors of the n_rep-element sweeps: bound with the larger count in the error terms
    with np.errstate(divide="ignore", invalid="ignore"):
        sa, sb = np.sqrt(st[11] / n_gf), np.sqrt(st[12] / n_gf)
        den = n_gf * (sa + eps) * (sb + eps)
        rel = m2_bound(n_rep, Gg, st[11], Ap) / (2 * st[11]) + m2_bound(n_rep, Gg, st[12], Ay) / (2 * st[12]) + 8 * U
        cta = c_bound(n_rep, Gg, st[11], st[12], Ap, Ay) / den + np.abs(st[13] / den) * rel
    out["corr_to_average"] = np.where((st[11] > 0) & (st[12] > 0), cta, np.inf)
    out["oracle_corr"] = pearson_bound(n_rep, Gg, st[6], st[15], st[16], Ay, Ay, eps)
    TV, NV, MSE = (np.asarray(sc[k], dtype=np.float64) for k in ("TV", "NV", "MSE"))
    E_TV = m2_bound(n_rep, Gg, st[6], Ay) / (n_rep - 1) + 2 * U * TV
    E_NV = ssw_bound(n_rep, Gg, st[8], Ay) / n_gf + 2 * U * NV
    E_MSE = res_bound(n_rep, Gg, st[7]) / n_rep + 2 * U * MSE
    with np.errstate(divide="ignore", invalid="ignore"):
        kappa = TV / (TV - NV)
        E_D = E_TV + E_NV + U * np.abs(TV - NV)
        fev, feve = sc["fev"], sc["feve"]
        b_fev = 1.125 * (fev * (kappa * E_D / TV + E_TV / TV) + 4 * U)
        b_feve = 1.125 * (kappa * ((E_MSE + E_NV + U * np.abs(MSE - NV)) / TV + np.abs(1 - feve) * E_D / TV)
                          + 4 * U * (1 + np.abs(1 - feve)))
        ok = np.isfinite(fev) & (kappa * E_D / TV <= 1.0 / 16)
    out["fev"], out["feve"], out["kappa"] = np.where(ok, b_fev, np.inf), np.where(ok, b_feve, np.inf), kappa
    return out

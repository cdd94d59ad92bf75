"""Float64 checker of the parametric receptive-field fits (include/dwn.h dwn_gauss2d_args): the
elliptical-Gaussian Levenberg-Marquardt fit and the temporal profile, statement by statement as the kernels take them — the same
expressions in the same association, the same Cholesky recurrences, the same clamps and decisions — differing only in the order of
the sums over the cells (numpy's pairwise sums against lane-strided partials and a butterfly) and in the last bits of exp / log.
numpy only; written for this project and held to brute force by tests/test_rf_fit_reference_cpu.py.

Model: f = b + a exp(-q / 2), q = (l11 dx)^2 + (l21 dx + l22 dy)^2, dx = x - cx, dy = y - cy,
p = (b, a, cy, cx, log l11, l21, log l22)."""
import numpy as np

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
NP = 7
COLUMNS = ("status", "iterations", "baseline", "amplitude", "cy", "cx", "sigma_major", "sigma_minor", "theta", "sse", "r2", "se_cy",
           "se_cx", "se_amplitude", "lambda", "row")
TRIES = 16


def grid(gh, gw):
    y, x = np.divmod(np.arange(gh * gw), gw)
    return y.astype(np.float64), x.astype(np.float64)


def shape(p, gh, gw):
    """e = exp(-q / 2) [G] and the intermediates (u, v, dx, dy, l11, l21, l22)."""
    y, x = grid(gh, gw)
    l11, l21, l22 = np.exp(p[4]), p[5], np.exp(p[6])
    dx, dy = x - p[3], y - p[2]
    u, v = l11 * dx, l21 * dx + l22 * dy
    q = u * u + v * v
    return np.exp(-0.5 * q), (u, v, dx, dy, l11, l21, l22)


def model(p, gh, gw):
    e, _ = shape(p, gh, gw)
    return p[0] + p[1] * e


def residual(p, m, gh, gw):
    e, _ = shape(p, gh, gw)
    return m - (p[0] + p[1] * e)


def sse(p, m, gh, gw):
    r = residual(p, m, gh, gw)
    return float((r * r).sum())


def jacobian(p, gh, gw, fit_baseline=True):
    """J [G, 7] = d f / d p."""
    e, (u, v, dx, dy, l11, l21, l22) = shape(p, gh, gw)
    ae = p[1] * e
    J = np.empty((gh * gw, NP))
    J[:, 0] = 1.0 if fit_baseline else 0.0
    J[:, 1] = e
    J[:, 2] = ae * (v * l22)
    J[:, 3] = ae * (u * l11 + v * l21)
    J[:, 4] = -(ae * (u * u))
    J[:, 5] = -(ae * (v * dx))
    J[:, 6] = -(ae * (v * (l22 * dy)))
    return J


def normal(p, m, gh, gw, fit_baseline=True):
    """(JtJ [7, 7], Jt r [7], S) at p."""
    J = jacobian(p, gh, gw, fit_baseline)
    r = residual(p, m, gh, gw)
    A = np.empty((NP, NP))
    for i in range(NP):
        for j in range(i, NP):
            A[i, j] = A[j, i] = (J[:, i] * J[:, j]).sum()
    g = np.array([(J[:, i] * r).sum() for i in range(NP)])
    if not fit_baseline:
        A[0, 0] = 1.0
    return A, g, float((r * r).sum())


def cholesky(A, lam):
    """Lower factor of A + lam diag(A) by the kernel's recurrence, or None when a pivot is not positive and finite."""
    M = A.copy()
    for i in range(NP):
        M[i, i] = M[i, i] + lam * M[i, i]
    L = np.zeros((NP, NP))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(NP):
            d = M[j, j]
            for q in range(j):
                d = d - L[j, q] * L[j, q]
            ok = ok and bool(d > 0.0) and bool(np.isfinite(d))
            piv = np.sqrt(d)
            L[j, j] = piv
            for i in range(j + 1, NP):
                s = M[i, j]
                for q in range(j):
                    s = s - L[i, q] * L[j, q]
                L[i, j] = s / piv
    return L if ok else None


def solve(L, rhs):
    z = np.zeros(NP)
    x = np.zeros(NP)
    for i in range(NP):
        s = rhs[i]
        for q in range(i):
            s = s - L[i, q] * z[q]
        z[i] = s / L[i, i]
    for i in range(NP - 1, -1, -1):
        s = z[i]
        for q in range(i + 1, NP):
            s = s - L[q, i] * x[q]
        x[i] = s / L[i, i]
    return x


def covariance(A):
    """C = A^-1 through the same factor, or None."""
    L = cholesky(A, 0.0)
    if L is None:
        return None
    return np.stack([solve(L, np.eye(NP)[i]) for i in range(NP)], axis=1)


def start(m, gh, gw, fit_baseline=True, rel_threshold=0.5):
    """(p0, info) or (None, info) when the map has no fit; info: b0, sd2 = sum (m - b0)^2, sstot."""
    y, x = grid(gh, gw)
    G = gh * gw
    with np.errstate(all="ignore"):
        per = (y == 0) | (y == gh - 1) | (x == 0) | (x == gw - 1)
        b0 = float(m[per].sum() / float(2 * gh + 2 * gw - 4)) if fit_baseline else 0.0
        mean = m.sum() / float(G)
        d = m - b0
        sd2 = float((d * d).sum())
        sstot = float(((m - mean) * (m - mean)).sum())
        info = dict(b0=b0, sd2=sd2, sstot=sstot)
        if not np.all(np.isfinite(m)) or m.min() == m.max():
            return None, info
        i = int(np.argmax(np.abs(d)))                            # the first maximum: the lowest index
        a0 = float(d[i])
        if a0 == 0.0:
            return None, info
        keep = np.abs(d) >= rel_threshold * abs(a0)
        w = np.where(keep, d * d, 0.0)
        sw = w.sum()
        cy, cx = (w * y).sum() / sw, (w * x).sum() / sw
        ey, ex = y - cy, x - cx
        sy, sx = np.sqrt((w * (ey * ey)).sum() / sw), np.sqrt((w * (ex * ex)).sum() / sw)
        sy, sx = max(float(sy), 0.5), max(float(sx), 0.5)
    return np.array([b0, a0, cy, cx, -np.log(sx), 0.0, -np.log(sy)]), info


def derived(p):
    """(sigma_major, sigma_minor, theta) in closed form."""
    l11, l21, l22 = np.exp(p[4]), p[5], np.exp(p[6])
    pxx, pxy, pyy = l11 * l11 + l21 * l21, l21 * l22, l22 * l22
    det = (l11 * l22) * (l11 * l22)
    cxx, cyy, cxy = pyy / det, pxx / det, (0.0 - pxy) / det
    hd = 0.5 * (cxx - cyy)
    lmaj = 0.5 * (cxx + cyy) + np.sqrt(hd * hd + cxy * cxy)
    lmin = (1.0 / det) / lmaj
    theta = 0.5 * np.arctan2(2.0 * cxy, cxx - cyy)
    if theta <= -0.5 * np.pi:
        theta += np.pi
    return float(np.sqrt(lmaj)), float(np.sqrt(lmin)), float(theta)


def spatial_covariance(p):
    """The 2 x 2 covariance of the Gaussian in (x, y), for the eigh test."""
    l11, l21, l22 = np.exp(p[4]), p[5], np.exp(p[6])
    Lm = np.array([[l11, 0.0], [l21, l22]])
    return np.linalg.inv(Lm.T @ Lm)


def fit_one(m, gh, gw, *, fit_baseline=True, rel_threshold=0.5, max_iter=100, xtol=1e-8, ftol=1e-12, row=0):
    """(params [7], table [16], p0 or None, C or None) of one map m [G] (any float dtype; taken as float64)."""
    m = np.asarray(m, dtype=np.float64).ravel()
    G = gh * gw
    nan = np.nan
    p0, info = start(m, gh, gw, fit_baseline, rel_threshold)
    if p0 is None:
        base = info["b0"] if np.isfinite(info["b0"]) else nan
        s = info["sd2"] if np.isfinite(info["sd2"]) else nan
        params = np.array([base, 0.0, nan, nan, nan, nan, nan])
        table = np.array([2.0, 0.0, base, 0.0, nan, nan, nan, nan, nan, s, 0.0, nan, nan, nan, 0.0, float(row)])
        return params, table, None, None
    p = p0.copy()
    gmax = max(gh, gw)
    ulo, uhi = -np.log(2.0 * float(gmax)), -np.log(0.3)
    A, g, S = normal(p, m, gh, gw, fit_baseline)
    lam, status, iters = 1e-3, 1, 0
    for it in range(1, max_iter + 1):
        iters = it
        accepted = conv_x = False
        dec = 0.0
        for _ in range(TRIES):
            L = cholesky(A, lam)
            if L is None:
                lam *= 10.0
                continue
            dp = solve(L, g)
            pn = p + dp
            if not fit_baseline:
                pn[0] = p[0]
            pn[2] = min(max(pn[2], -1.0), float(gh)); pn[3] = min(max(pn[3], -1.0), float(gw))
            pn[4] = min(max(pn[4], ulo), uhi); pn[6] = min(max(pn[6], ulo), uhi)
            sa = xtol * abs(p[1])
            if all(abs(pn[k] - p[k]) < (sa if k < 2 else xtol) for k in range(NP)):
                conv_x = True
                break
            with np.errstate(all="ignore"):
                Sn = sse(pn, m, gh, gw)
            if np.isfinite(Sn) and Sn < S:
                dec = S - Sn
                p, S = pn, Sn
                lam = max(lam / 10.0, 1e-12)
                accepted = True
                break
            lam *= 10.0
        if conv_x:
            status = 0
            break
        if not accepted:
            break
        A, g, _ = normal(p, m, gh, gw, fit_baseline)
        if dec <= ftol * S:
            status = 0
            break
    smaj, smin, theta = derived(p)
    C = covariance(A)
    se = [nan, nan, nan]
    if C is not None:
        s2 = S / float(G - (NP if fit_baseline else NP - 1))
        with np.errstate(all="ignore"):
            se = [float(np.sqrt(C[k, k] * s2)) for k in (2, 3, 1)]
    r2 = 1.0 - S / info["sstot"] if info["sstot"] > 0.0 else 0.0
    table = np.array([float(status), float(iters), p[0], p[1], p[2], p[3], smaj, smin, theta, S, r2, se[0], se[1], se[2], lam, float(row)])
    return p, table, p0, C


def fit(maps, sel=None, **kw):
    """(params [M, 7], table [M, 16], starts, covariances) over maps [R, gh, gw]."""
    maps = np.asarray(maps)
    _, gh, gw = maps.shape
    rows = np.arange(maps.shape[0]) if sel is None else np.asarray(sel)
    out = [fit_one(maps[r], gh, gw, row=int(r), **kw) for r in rows]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [o[2] for o in out], [o[3] for o in out])


def param_scale(p):
    a = abs(p[1])
    return np.array([a, a, 1.0, 1.0, 1.0, 1.0, 1.0])


def param_bound(p, S, C, xtol=1e-8, ftol=1e-12):
    """|p_kernel - p_checker|_i <= 4 (xtol scale_i + sqrt(2 ftol S C_ii)): two answers near one stationary point, each within a
    step-criterion or an ftol stop of it, times 2 for the neglected second order."""
    return 4.0 * (xtol * param_scale(p) + np.sqrt(2.0 * ftol * S * np.abs(np.diag(C))))


def derived_jacobian(p, h=1e-6):
    """d (sigma_major, sigma_minor, theta) / d (log l11, l21, log l22) by central differences [3, 3] (propagates param_bound)."""
    out = np.zeros((3, 3))
    for k, idx in enumerate((4, 5, 6)):
        a, b = p.copy(), p.copy()
        a[idx] += h; b[idx] -= h
        da, db = np.array(derived(a)), np.array(derived(b))
        d = da - db
        d[2] = (d[2] + 0.5 * np.pi) % np.pi - 0.5 * np.pi        # theta modulo pi
        out[:, k] = d / (2 * h)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
def profile(params, maps, fit_baseline=True):
    """(profile [N, L], separability [N], bound [N, L]) of maps [N, L, gh, gw] on the spatial shape of params [N, 7]; the bound is
    G 2^-53 sum |terms| of every sum, carried through the 2 x 2 solve to first order."""
    maps = np.asarray(maps, dtype=np.float64)
    N, Lg, gh, gw = maps.shape
    G = gh * gw
    Gd = float(G)
    prof, sep, bound = np.full((N, Lg), np.nan), np.full(N, np.nan), np.zeros((N, Lg))
    for n in range(N):
        p = np.asarray(params[n], dtype=np.float64)
        if not np.all(np.isfinite(p)):
            continue
        e, _ = shape(p, gh, gw)
        se1, se2 = e.sum(), (e * e).sum()
        det = Gd * se2 - se1 * se1
        sse_all = sst_all = 0.0
        gam = G * EPS64
        for l in range(Lg):
            v = maps[n, l].ravel()
            sm, sme = v.sum(), (v * e).sum()
            if fit_baseline:
                al = (Gd * sme - se1 * sm) / det if det > 0.0 else 0.0
                bl = (sm - al * se1) / Gd
                mu = sm / Gd
                # first order: every sum s carries gam sum |terms|; a = num / det
                asm, asme = np.abs(v).sum(), (np.abs(v) * e).sum()
                dnum = gam * (Gd * asme + se1 * asm + se1 * asm) + 3 * EPS64 * (Gd * abs(sme) + abs(se1 * sm))
                ddet = gam * (Gd * se2 + 2 * se1 * se1) + 3 * EPS64 * (Gd * se2 + se1 * se1)
                bound[n, l] = (dnum + abs(al) * ddet) / det + EPS64 * abs(al) if det > 0.0 else 0.0
            else:
                al = sme / se2 if se2 > 0.0 else 0.0
                bl = mu = 0.0
                asme = (np.abs(v) * e).sum()
                bound[n, l] = (gam * asme + abs(al) * gam * se2) / se2 + EPS64 * abs(al) if se2 > 0.0 else 0.0
            r, t = v - (bl + al * e), v - mu
            sse_all += (r * r).sum(); sst_all += (t * t).sum()
            prof[n, l] = al
        sep[n] = 1.0 - sse_all / sst_all if sst_all > 0.0 else 0.0
    return prof, sep, bound


# ------------------------------------------------------------------------------------------------------------------------------
GRIDS = ((5, 7), (8, 8), (8, 12), (16, 16), (18, 32), (36, 64), (64, 64))
NOISE_LEVELS = (0.0, 0.02, 0.1)


def maps_per_case(gh, gw):
    return 24 if gh * gw >= 2304 else 48


def planted_maps(gh, gw, count, noise, seed):
    """(maps fp32 [count, gh, gw], truth [count, 7] as p) of the issue's generator: centre at least one cell inside, sigma_major in
    [0.8, min(gh, gw) / 3], sigma_minor in [0.6, sigma_major], any angle, amplitude +-[0.5, 2], baseline in [-0.2, 0.2], white
    noise of `noise` |a|, rounded to fp32."""
    rng = np.random.default_rng(seed)
    y, x = grid(gh, gw)
    maps, truth = np.zeros((count, gh * gw), dtype=np.float32), np.zeros((count, NP))
    for k in range(count):
        cy, cx = rng.uniform(1.0, gh - 2.0), rng.uniform(1.0, gw - 2.0)
        smaj = rng.uniform(0.8, max(min(gh, gw) / 3.0, 0.8))
        smin = rng.uniform(0.6, smaj)
        th = rng.uniform(-0.5 * np.pi, 0.5 * np.pi)
        a = rng.uniform(0.5, 2.0) * rng.choice([-1.0, 1.0])
        b = rng.uniform(-0.2, 0.2)
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        cov = R @ np.diag([smaj ** 2, smin ** 2]) @ R.T             # in (x, y)
        P = np.linalg.inv(cov)
        l22 = np.sqrt(P[1, 1]); l21 = P[0, 1] / l22; l11 = np.sqrt(P[0, 0] - l21 * l21)
        p = np.array([b, a, cy, cx, np.log(l11), l21, np.log(l22)])
        f = model(p, gh, gw) + noise * abs(a) * rng.normal(size=gh * gw)
        maps[k] = f.astype(np.float32)
        truth[k] = p
    return maps.reshape(count, gh, gw), truth


def case_seed(gh, gw, level):
    return 1000 * gh + 10 * gw + level

"""CPU tests of the float64 checker of the parametric receptive-field fits (tests/rf_fit_reference.py)
against independent statements: its Jacobian against central differences and float64 torch autograd, its solutions against
scipy.optimize.least_squares from the same start, the closed-form sigmas and angle against numpy.linalg.eigh, the profile against
numpy.linalg.lstsq, the planted-filter case of tests/test_rf_reference_cpu.py fitted, and the share of generated maps the checker
leaves unconverged, with the seeds the GPU tests use.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

from tests import rf_fit_reference as gf
from tests import rf_reference as rf
from tests.test_rf_reference_cpu import PLANTED, planted_case

POINTS = [(5, 7, np.array([0.1, 1.3, 2.2, 3.4, np.log(0.8), 0.3, np.log(1.1)])),
          (8, 12, np.array([-0.2, -0.7, 3.0, 7.0, np.log(0.5), -0.4, np.log(0.9)])),
          (18, 32, np.array([0.0, 2.0, 9.5, 20.25, np.log(0.25), 0.05, np.log(0.4)]))]


@pytest.mark.parametrize("gh, gw, p", POINTS)
def test_jacobian_equals_central_differences_and_autograd(gh, gw, p):
    J = gf.jacobian(p, gh, gw)
    num = np.zeros_like(J)
    for k in range(gf.NP):
        h = 1e-6
        a, b = p.copy(), p.copy()
        a[k] += h; b[k] -= h
        num[:, k] = (gf.model(a, gh, gw) - gf.model(b, gh, gw)) / (2 * h)
    err_fd = float(np.abs(J - num).max())
    y, x = (torch.from_numpy(v) for v in gf.grid(gh, gw))
    pt = torch.from_numpy(p.copy()).requires_grad_(True)

    def f(q):
        dx, dy = x - q[3], y - q[2]
        u, v = torch.exp(q[4]) * dx, q[5] * dx + torch.exp(q[6]) * dy
        return q[0] + q[1] * torch.exp(-0.5 * (u * u + v * v))
    auto = torch.autograd.functional.jacobian(f, pt).numpy()
    err_ad = float(np.abs(J - auto).max())
    print(f"jacobian {gh} x {gw}: max |J| {np.abs(J).max():.3f}, vs central differences {err_fd:.2e}, vs autograd {err_ad:.2e}")
    assert err_fd < 1e-8 and err_ad < 1e-14
    assert np.all(gf.jacobian(p, gh, gw, fit_baseline=False)[:, 0] == 0.0)
    # the normal equations are the Jacobian's
    m = gf.model(p, gh, gw) + 0.01 * np.cos(np.arange(gh * gw))
    A, g, S = gf.normal(p, m, gh, gw)
    r = gf.residual(p, m, gh, gw)
    # (sums of G products of mixed sign in two orders: G 2^-53 of the largest entry)
    assert np.allclose(A, J.T @ J, rtol=0, atol=gh * gw * gf.EPS64 * np.abs(A).max())
    assert np.allclose(g, J.T @ r, rtol=0, atol=gh * gw * gf.EPS64 * np.abs(J).max() * np.abs(r).sum()) and np.isclose(S, r @ r, rtol=1e-13)


def test_cholesky_and_solve_equal_numpy():
    rng = np.random.default_rng(3)
    B = rng.normal(size=(12, gf.NP))
    A = B.T @ B
    L = gf.cholesky(A, 0.0)
    rhs = rng.normal(size=gf.NP)
    print("cholesky: max |L - numpy|", float(np.abs(L - np.linalg.cholesky(A)).max()))
    assert np.allclose(L, np.linalg.cholesky(A), rtol=1e-12, atol=1e-13)
    assert np.allclose(gf.solve(L, rhs), np.linalg.solve(A, rhs), rtol=1e-10)
    assert np.allclose(gf.covariance(A), np.linalg.inv(A), rtol=1e-9)
    D = A + 0.5 * np.diag(np.diag(A))
    assert np.allclose(gf.cholesky(A, 0.5), np.linalg.cholesky(D), rtol=1e-12, atol=1e-13)
    bad = A.copy(); bad[3, 3] = -1.0
    assert gf.cholesky(bad, 0.0) is None and gf.cholesky(np.full((gf.NP, gf.NP), np.nan), 0.0) is None


@pytest.mark.parametrize("gh, gw, noise", [(5, 7, 0.02), (8, 12, 0.1), (18, 32, 0.1), (16, 16, 0.0)])
def test_solutions_equal_scipy_least_squares_from_the_same_start(gh, gw, noise):
    opt = pytest.importorskip("scipy.optimize")
    maps, _ = gf.planted_maps(gh, gw, 12, noise, 77)
    P, T, starts, Cs = gf.fit(maps)
    worst = worst_s = 0.0
    for k in range(len(maps)):
        m = maps[k].astype(np.float64).ravel()
        res = opt.least_squares(lambda q: -gf.residual(q, m, gh, gw), starts[k], jac=lambda q: gf.jacobian(q, gh, gw), method="lm",
                                xtol=1e-14, ftol=1e-14, gtol=1e-14)
        S_scipy = float(res.fun @ res.fun)
        bound = gf.param_bound(P[k], T[k, 9], Cs[k])
        worst = max(worst, float((np.abs(res.x - P[k]) / bound).max()))
        # a stop on the step criterion leaves |dp_i| <= xtol scale_i, that is at most (sum_i sqrt(A_ii) xtol scale_i)^2 / 2 of S:
        # on noiseless data, where S ~ 1e-16 is the fp32 rounding of the map, that is of the order of S itself
        A, _, _ = gf.normal(P[k], m, gh, gw)
        slack = 0.5 * float((np.sqrt(np.diag(A)) * 1e-8 * gf.param_scale(P[k])).sum()) ** 2
        worst_s = max(worst_s, (T[k, 9] - S_scipy - slack) / max(S_scipy, 1e-300))
    print(f"scipy {gh} x {gw} noise {noise}: worst |p - p_scipy| / bound {worst:.3g}, worst relative S excess {worst_s:.2e}, "
          f"statuses {np.bincount(T[:, 0].astype(int), minlength=3).tolist()}")
    assert np.all(T[:, 0] == 0) and worst <= 1.0
    assert worst_s <= 1e-9                                        # 1e3 ftol: the same minimum


def test_closed_form_sigmas_and_angle_equal_eigh():
    rng = np.random.default_rng(5)
    worst = 0.0
    for _ in range(200):
        p = np.array([0.0, 1.0, 0.0, 0.0, rng.uniform(-2, 1), rng.normal() * 0.7, rng.uniform(-2, 1)])
        smaj, smin, theta = gf.derived(p)
        w, v = np.linalg.eigh(gf.spatial_covariance(p))                  # ascending, in (x, y)
        ang = np.arctan2(v[1, 1], v[0, 1])
        d = (theta - ang + 0.5 * np.pi) % np.pi - 0.5 * np.pi
        worst = max(worst, abs(smaj - np.sqrt(w[1])) / smaj, abs(smin - np.sqrt(w[0])) / smin, abs(d))
        assert -0.5 * np.pi < theta <= 0.5 * np.pi and smaj >= smin
    print("closed form vs eigh: worst deviation", worst)
    assert worst < 1e-9
    round_ = np.array([0.0, 1.0, 0.0, 0.0, np.log(0.5), 0.0, np.log(0.5)])
    assert gf.derived(round_) == (2.0, 2.0, 0.0)
    tall = np.array([0.0, 1.0, 0.0, 0.0, np.log(1.0), 0.0, np.log(0.5)])   # sigma_y = 2 > sigma_x = 1: the major axis is the y axis
    assert gf.derived(tall)[2] == pytest.approx(0.5 * np.pi) and gf.derived(tall)[:2] == pytest.approx((2.0, 1.0))


@pytest.mark.parametrize("fit_baseline", [True, False])
def test_profile_equals_lstsq(fit_baseline):
    rng = np.random.default_rng(11)
    gh, gw, L = 8, 12, 5
    p = np.array([[0.0, 1.0, 3.0, 7.0, np.log(0.8), 0.2, np.log(0.9)], [0.1, -1.0, 4.5, 2.0, np.log(0.5), 0.0, np.log(0.5)]])
    maps = rng.normal(size=(2, L, gh, gw)).astype(np.float32)
    prof, sep, bound = gf.profile(p, maps, fit_baseline)
    worst = 0.0
    for n in range(2):
        e, _ = gf.shape(p[n], gh, gw)
        X = np.stack([np.ones_like(e), e], axis=1) if fit_baseline else e[:, None]
        sse = sst = 0.0
        for l in range(L):
            v = maps[n, l].astype(np.float64).ravel()
            coef, res, _, _ = np.linalg.lstsq(X, v, rcond=None)
            worst = max(worst, abs(coef[-1] - prof[n, l]))
            sse += float(res[0]); sst += float(((v - (v.mean() if fit_baseline else 0.0)) ** 2).sum())
        assert sep[n] == pytest.approx(1 - sse / sst, abs=1e-12)
    print(f"profile vs lstsq (baseline {fit_baseline}): worst |a_l - lstsq| {worst:.2e}; largest bound {bound.max():.2e}")
    assert worst < 1e-12 and 0 < bound.max() < 1e-12
    nanp = p.copy(); nanp[1, 2:] = np.nan
    prof2, sep2, _ = gf.profile(nanp, maps, fit_baseline)
    assert np.all(np.isnan(prof2[1])) and np.isnan(sep2[1]) and np.array_equal(prof2[0], prof[0])


def test_no_fit_rows():
    gh, gw = 5, 7
    for m, base, s in ((np.full(35, 0.75), 0.75, 0.0), (np.zeros(35), 0.0, 0.0)):
        p, t, p0, C = gf.fit_one(m, gh, gw, row=4)
        assert p0 is None and C is None
        assert p[0] == base and p[1] == 0.0 and np.all(np.isnan(p[2:]))
        assert t[:4].tolist() == [2.0, 0.0, base, 0.0] and np.all(np.isnan(t[4:9])) and t[9] == s and t[10] == 0.0
        assert np.all(np.isnan(t[11:14])) and t[14] == 0.0 and t[15] == 4.0
    m = np.arange(35.0) / 8.0
    m[17], m[18] = np.nan, np.inf                                # interior cells: the perimeter mean stays finite
    p, t, _, _ = gf.fit_one(m, gh, gw)
    assert t[0] == 2.0 and np.isfinite(t[2]) and np.isnan(t[9]) and p[0] == t[2]
    m[0] = np.nan
    assert np.isnan(gf.fit_one(m, gh, gw)[1][2])
    # a constant map is refused with the baseline held, too; a zero-baseline fit returns b = 0 exactly
    assert gf.fit_one(np.full(35, 0.75), gh, gw, fit_baseline=False)[1][0] == 2.0
    maps, _ = gf.planted_maps(8, 8, 3, 0.02, 1)
    P, T, _, _ = gf.fit(maps, fit_baseline=False)
    assert np.all(P[:, 0] == 0.0) and np.all(T[:, 2] == 0.0)
    assert gf.COLUMNS[10] == "r2" and len(gf.COLUMNS) == 16


@pytest.mark.parametrize("kind", ["binary", "sparse"])
def test_planted_filter_fitted(kind):
    """The planted filter of tests/test_rf_reference_cpu.py: centre (3, 7), sigma 1.2, temporal profile (0.2, 0.6, 1, 0.5, 0.1)."""
    x, r, f = planted_case(kind)
    st = rf.State(1, PLANTED["L"], PLANTED["gh"], PLANTED["gw"])
    for k0 in range(0, PLANTED["clips"], 128):
        rf.accumulate(st, x[k0:k0 + 128], r[k0:k0 + 128], skip=0, s0=127.5, r0=np.array([r[:32].mean()], dtype=np.float32))
    cov, _, summary = rf.finalize(st)
    cov32 = cov.astype(np.float32)
    res = planted_fit_figures(cov32, int(summary[0, 0]))
    print(f"planted filter fitted ({kind}): {res}")
    check_planted_fit(res)


def planted_fit_figures(cov32, lag):
    """The figures the issue asserts, from a map fp32 [1, L, gh, gw] and its peak lag (shared with the GPU model test)."""
    gh, gw = cov32.shape[2:]
    p, t, _, _ = gf.fit_one(cov32[0, lag], gh, gw)
    prof, sep, _ = gf.profile(p[None], cov32)
    return dict(status=int(t[0]), iterations=int(t[1]), cy=float(t[4]), cx=float(t[5]), sigma_major=float(t[6]), sigma_minor=float(t[7]),
                r2=float(t[10]), profile=(prof[0] / prof[0, 2]).round(4).tolist(), separability=float(sep[0]))


def check_planted_fit(res):
    assert res["status"] == 0
    assert abs(res["cy"] - 3.0) <= 0.1 and abs(res["cx"] - 7.0) <= 0.1
    assert abs(res["sigma_major"] - 1.2) <= 0.1 and abs(res["sigma_minor"] - 1.2) <= 0.1
    assert np.abs(np.array(res["profile"]) - np.array([0.2, 0.6, 1.0, 0.5, 0.1])).max() <= 0.05
    assert res["r2"] >= 0.9 and res["separability"] >= 0.85


@pytest.mark.parametrize("gh, gw", gf.GRIDS)
def test_checker_leaves_out_at_most_one_percent(gh, gw):
    """The cap of the GPU parameter comparison, the checker's half: per grid and noise level at most 1 % of the generated maps (the
    seeds of tests/test_gpu_rf_fit.py) may be left unconverged by the checker itself."""
    for lv, noise in enumerate(gf.NOISE_LEVELS):
        maps, truth = gf.planted_maps(gh, gw, gf.maps_per_case(gh, gw), noise, gf.case_seed(gh, gw, lv))
        _, T, _, _ = gf.fit(maps)
        out = int((T[:, 0] != 0).sum())
        print(f"{gh} x {gw} noise {noise}: {out} of {len(maps)} not converged; iterations max {int(T[:, 1].max())}, worst centre error "
              f"{float(np.abs(T[:, 4:6] - truth[:, 2:4]).max()):.2e}")
        assert out <= 0.01 * len(maps)

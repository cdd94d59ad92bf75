"""The parametric receptive-field fit kernels against the float64 checker tests/rf_fit_reference.py, on
planted elliptical Gaussians over the grids 5 x 7, 8 x 8, 8 x 12, 16 x 16, 18 x 32, 36 x 64 and 64 x 64 (fewer cells than lanes, a
multiple of 64, ragged tails, the production grid and the largest one) at noise 0, 0.02 and 0.1 of the amplitude:

(a) path-free quality: S evaluated by the checker at the kernel's parameters exceeds S at the checker's parameters by at most
    TAU S.  Measured on the device (profiles/rf_fit_time.txt): the worst relative excess is 2.4e-15 on the noisy maps and 1.2e-8
    on the noiseless ones, where S ~ 1e-16 is itself formed from residuals of 1e-8 that carry the 1e-16 rounding of the model
    value (its evaluation floor; the parameters there agree to 1e-7 of their bound).  Asserted at ten times those figures.
(b) parameters: |p_kernel - p_checker|_i <= 4 (xtol scale_i + sqrt(2 ftol S C_ii)) on the maps both fits converged on (the cap:
    at most 2 % of a case may be left out, at most 1 % by the checker: tests/test_rf_fit_reference_cpu.py), the derived columns
    at that bound propagated, iteration counts in the printout only.
(c) noiseless maps: the truth within 2 (sqrt(C_ii) 2^-24 ||m||_2 + xtol scale_i), the first-order effect of rounding the map to fp32.
(d) bits: a row is the same through any row table and any M; maps with no fit give exactly the stated row and leave their
    neighbours' bits alone; a held baseline stays 0 exactly.
(e) the profile entry against the checker at the kernel's own params, at the checker's carried bound; bit for bit on integers.
(f) refusals launch nothing.
Every test prints what it measured before it asserts."""
import ctypes as C
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rf_fit_reference as gf  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

XTOL, FTOL = 1e-8, 1e-12
TAU = {True: 10 * 2.4e-15, False: 10 * 1.2e-8}         # by "the map has noise": ten times the measured worst relative excess
_CASES = {}


def device_fit(maps, sel=None, **kw):
    from sensorium_amd import ops
    t = torch.from_numpy(np.ascontiguousarray(maps)).to(dev())
    s = None if sel is None else torch.tensor(list(sel), dtype=torch.int32, device=dev())
    params, table, start = ops.gauss2d_fit(t, s, **kw)
    torch.cuda.synchronize()
    return params.cpu().numpy(), table.cpu().numpy(), start.cpu().numpy()


def case(gh, gw, lv):
    """Maps, truth, the checker's fit and the device's, computed once per (grid, noise level)."""
    key = (gh, gw, lv)
    if key not in _CASES:
        maps, truth = gf.planted_maps(gh, gw, gf.maps_per_case(gh, gw), gf.NOISE_LEVELS[lv], gf.case_seed(gh, gw, lv))
        P, T, starts, Cs = gf.fit(maps)
        pk, tk, sk = device_fit(maps)
        _CASES[key] = dict(maps=maps, truth=truth, P=P, T=T, starts=starts, C=Cs, pk=pk, tk=tk, sk=sk)
    return _CASES[key]


def kept(c):
    """The maps inside the cap: both converged."""
    return np.nonzero((c["tk"][:, 0] == 0) & (c["T"][:, 0] == 0))[0]


CASE_IDS = [(gh, gw, lv) for gh, gw in gf.GRIDS for lv in range(len(gf.NOISE_LEVELS))]


@pytest.mark.parametrize("gh, gw, lv", CASE_IDS)
def test_sse_at_the_kernel_s_parameters_is_the_checker_s_minimum(gh, gw, lv):
    c = case(gh, gw, lv)
    worst, n = -np.inf, 0
    for k in range(len(c["maps"])):
        if c["tk"][k, 0] == 2 or c["T"][k, 0] == 2:
            continue
        m = c["maps"][k].astype(np.float64).ravel()
        Sk, Sc = gf.sse(c["pk"][k], m, gh, gw), gf.sse(c["P"][k], m, gh, gw)
        worst = max(worst, (Sk - Sc) / Sc)
        n += 1
    tau = TAU[lv > 0]
    print(f"{gh} x {gw} noise {gf.NOISE_LEVELS[lv]}: worst relative excess of S {worst:.3e} over {n} maps (asserted at {tau:.1e}); "
          f"S from {c['T'][:, 9].min():.2e} to {c['T'][:, 9].max():.2e}")
    assert n == len(c["maps"]) and worst <= tau


def se_columns(p, S, m, gh, gw):
    A, _, _ = gf.normal(p, m, gh, gw)
    Cv = gf.covariance(A)
    return np.sqrt(np.diag(Cv)[[2, 3, 1]] * S / float(gh * gw - gf.NP)), A


@pytest.mark.parametrize("gh, gw, lv", CASE_IDS)
def test_parameters_and_derived_columns_inside_the_cap(gh, gw, lv):
    c = case(gh, gw, lv)
    keep = kept(c)
    left = len(c["maps"]) - len(keep)
    disagree = int((c["tk"][:, 0] != c["T"][:, 0]).sum())
    worst = dict(p=0.0, sigma=0.0, theta=0.0, r2=0.0, se=0.0)
    G = gh * gw
    tau = TAU[lv > 0]
    for k in keep:
        m = c["maps"][k].astype(np.float64).ravel()
        p, S, Cv = c["P"][k], c["T"][k, 9], c["C"][k]
        bp = gf.param_bound(p, S, Cv, XTOL, FTOL)
        dpar = np.abs(c["pk"][k] - p)
        worst["p"] = max(worst["p"], float((dpar / bp).max()))
        assert np.array_equal(c["tk"][k, 2:6], c["pk"][k, :4]) and c["tk"][k, 15] == k
        # sigmas and theta: the closed form's Jacobian times the bound of the three shape parameters, and its own rounding
        Jd = np.abs(gf.derived_jacobian(p))
        bd = Jd @ bp[4:7] + 16 * gf.EPS64 * np.array([c["T"][k, 6], c["T"][k, 7], np.pi]) * (1.0 + Jd.sum(axis=1))
        dd = c["tk"][k, 6:9] - c["T"][k, 6:9]
        dd[2] = (dd[2] + 0.5 * np.pi) % np.pi - 0.5 * np.pi
        worst["sigma"] = max(worst["sigma"], float((np.abs(dd[:2]) / bd[:2]).max()))
        worst["theta"] = max(worst["theta"], float(abs(dd[2]) / bd[2]))
        # r2 = 1 - S / SStot: S within (a), both sums in another order
        sstot = float(((m - m.mean()) ** 2).sum())
        br2 = (tau + 4 * G * gf.EPS64) * S / sstot + 4 * gf.EPS64
        worst["r2"] = max(worst["r2"], abs(c["tk"][k, 10] - c["T"][k, 10]) / br2)
        # standard errors: sqrt(C_ii S / (G - 7)); their gradient in p by central differences times the parameter bound, S within
        # (a), and the inverse's own rounding G 2^-53 cond(A)
        se0, A = se_columns(p, S, m, gh, gw)
        grad = np.zeros((3, gf.NP))
        for i in range(gf.NP):
            h = 1e-6 * gf.param_scale(p)[i]
            a, b = p.copy(), p.copy()
            a[i] += h; b[i] -= h
            grad[:, i] = (se_columns(a, S, m, gh, gw)[0] - se_columns(b, S, m, gh, gw)[0]) / (2 * h)
        bse = np.abs(grad) @ bp + se0 * (0.5 * tau + 8 * G * gf.EPS64 * np.linalg.cond(A))
        worst["se"] = max(worst["se"], float((np.abs(c["tk"][k, 11:14] - c["T"][k, 11:14]) / bse).max()))
    its = int((c["tk"][keep, 1] != c["T"][keep, 1]).sum())
    print(f"{gh} x {gw} noise {gf.NOISE_LEVELS[lv]}: left out {left} of {len(c['maps'])} (statuses disagree on {disagree}); worst "
          f"|difference| / bound: params {worst['p']:.3g}, sigmas {worst['sigma']:.3g}, theta {worst['theta']:.3g}, r2 {worst['r2']:.3g}, "
          f"standard errors {worst['se']:.3g}; iteration counts differ on {its}, kernel max {int(c['tk'][:, 1].max())}, "
          f"checker max {int(c['T'][:, 1].max())}")
    assert left <= 0.02 * len(c["maps"])
    assert all(v <= 1.0 for v in worst.values()), worst
    # the start vector the kernel leaves in its workspace is the checker's, to the order of the sums
    s0 = np.stack(c["starts"])
    assert np.allclose(c["sk"][:, :7], s0, rtol=0, atol=64 * G * gf.EPS64 * max(gh, gw))


@pytest.mark.parametrize("gh, gw", gf.GRIDS)
def test_noiseless_maps_recover_the_truth(gh, gw):
    c = case(gh, gw, 0)
    worst = centre = 0.0
    for k in range(len(c["maps"])):
        m = c["maps"][k].astype(np.float64).ravel()
        t = c["truth"][k]
        bound = 2.0 * (np.sqrt(np.abs(np.diag(c["C"][k]))) * gf.EPS32 * np.linalg.norm(m) + XTOL * gf.param_scale(t))
        err = np.abs(c["pk"][k] - t)
        worst, centre = max(worst, float((err / bound).max())), max(centre, float(err[2:4].max()))
    print(f"{gh} x {gw} noiseless: worst |p - truth| / bound {worst:.3f}, worst centre error {centre:.2e} cell")
    assert np.all(c["tk"][:, 0] == 0) and worst <= 1.0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("gh, gw", [(5, 7), (8, 8), (18, 32), (64, 64)])
def test_row_table_order_and_count_do_not_change_a_row(gh, gw):
    c = case(gh, gw, 2)
    rows = [7, 2, 2, 11, 0, len(c["maps"]) - 1, 5]               # another order, a repeated row, M = 7: two workgroups, one ragged
    pk, tk, sk = device_fit(c["maps"], sel=rows)
    one_p, one_t, _ = device_fit(c["maps"][3:4])
    print(f"{gh} x {gw}: rows {rows} through the table; bits equal: params {np.array_equal(bits(pk), bits(c['pk'][rows]))}, "
          f"table {np.array_equal(bits(tk[:, :15]), bits(c['tk'][rows][:, :15]))}")
    assert np.array_equal(bits(pk), bits(c["pk"][rows])) and np.array_equal(bits(sk), bits(c["sk"][rows]))
    assert np.array_equal(bits(tk[:, :15]), bits(c["tk"][rows][:, :15])) and tk[:, 15].tolist() == [float(r) for r in rows]
    assert np.array_equal(bits(one_p[0]), bits(c["pk"][3])) and np.array_equal(bits(one_t[0, :15]), bits(c["tk"][3, :15]))


def test_maps_with_no_fit_give_the_stated_row_and_leave_their_neighbours_alone():
    gh, gw = 8, 12
    c = case(gh, gw, 1)
    maps = c["maps"][:9].copy()
    nan = np.nan
    maps[1] = 0.75                                               # constant
    maps[4] = 0.0                                                # all zero
    maps[6] = (np.arange(gh * gw).reshape(gh, gw) % 17 / 8.0).astype(np.float32)      # eighths: the perimeter mean is exact
    maps[6, 3, 4], maps[6, 5, 6] = np.nan, np.inf                # interior cells
    pk, tk, sk = device_fit(maps, sel=[0, 1, 2, 3, 4, 5, 6, 7, 8, 40])          # and a row outside the maps
    base6 = float(np.concatenate([maps[6, 0], maps[6, -1], maps[6, 1:-1, 0], maps[6, 1:-1, -1]]).astype(np.float64).sum() / 36.0)
    want = {1: (0.75, 0.0), 4: (0.0, 0.0), 6: (base6, nan), 9: (nan, nan)}
    for k, (base, s) in want.items():
        row = [2.0, 0.0, base, 0.0, nan, nan, nan, nan, nan, s, 0.0, nan, nan, nan, 0.0, float(k if k < 9 else 40)]
        print(f"row {k}: table {tk[k].tolist()}")
        assert np.array_equal(tk[k], np.array(row), equal_nan=True)
        assert np.array_equal(pk[k], np.array([base, 0.0, nan, nan, nan, nan, nan]), equal_nan=True) and np.all(np.isnan(sk[k]))
        if k < 9:
            P, T, _, _ = gf.fit(maps[k:k + 1])
            assert np.array_equal(T[0, :15], tk[k, :15], equal_nan=True) and np.array_equal(P[0], pk[k], equal_nan=True)
    clean = [0, 2, 3, 5, 7, 8]
    assert np.array_equal(bits(pk[clean]), bits(c["pk"][clean])) and np.array_equal(bits(tk[clean]), bits(c["tk"][clean]))
    # a constant map with the baseline held is refused too
    assert device_fit(maps[1:2], fit_baseline=False)[1][0, 0] == 2.0


def test_held_baseline_stays_zero_exactly():
    gh, gw = 8, 12
    maps, truth = gf.planted_maps(gh, gw, 12, 0.02, 5)
    y, x = gf.grid(gh, gw)
    for k in range(len(maps)):                                   # the same fields on a zero baseline
        p = truth[k].copy(); p[0] = 0.0
        maps[k] = (gf.model(p, gh, gw).reshape(gh, gw) + (maps[k].astype(np.float64) - gf.model(truth[k], gh, gw).reshape(gh, gw))).astype(np.float32)
    pk, tk, sk = device_fit(maps, fit_baseline=False)
    P, T, _, Cs = gf.fit(maps, fit_baseline=False)
    ratio = max(float((np.abs(pk[k] - P[k])[1:] / gf.param_bound(P[k], T[k, 9], Cs[k])[1:]).max()) for k in range(len(maps)))
    print(f"held baseline: baselines {sorted(set(pk[:, 0].tolist()))}, statuses {tk[:, 0].tolist()}, worst |difference| / bound {ratio:.3g}")
    assert np.all(bits(pk[:, 0]) == 0) and np.all(bits(tk[:, 2]) == 0) and np.all(bits(sk[:, 0]) == 0)
    assert np.all(tk[:, 0] == 0) and np.all(T[:, 0] == 0) and ratio <= 1.0
    assert np.allclose(tk[:, 11:14], T[:, 11:14], rtol=1e-6)     # six parameters in the degrees of freedom


# ---------------------------------------------------------------------------------------------------------------------- profile
def device_profile(params, maps, fit_baseline=True):
    from sensorium_amd import ops
    prof, sep = ops.gauss2d_profile(torch.from_numpy(np.ascontiguousarray(params)).to(dev()), torch.from_numpy(np.ascontiguousarray(maps)).to(dev()),
                                    fit_baseline=fit_baseline)
    torch.cuda.synchronize()
    return prof.cpu().numpy(), sep.cpu().numpy()


@pytest.mark.parametrize("fit_baseline", [True, False])
@pytest.mark.parametrize("gh, gw, L", [(5, 7, 3), (8, 12, 5), (18, 32, 2), (36, 64, 70)])
def test_profile_equals_the_checker_at_the_kernel_s_own_params(gh, gw, L, fit_baseline):
    c = case(gh, gw, 1)
    N = 6
    rng = np.random.default_rng(gh * gw + L)
    prof_true = rng.normal(size=(N, L))
    maps = np.zeros((N, L, gh, gw), dtype=np.float32)
    for n in range(N):
        e, _ = gf.shape(c["pk"][n], gh, gw)
        maps[n] = (prof_true[n][:, None] * e[None] + 0.05 * rng.normal(size=(L, gh * gw)) + (0.1 if fit_baseline else 0.0)).reshape(L, gh, gw)
    params = c["pk"][:N].copy()
    params[4, 2:] = np.nan                                       # a row with no fit
    got, sep = device_profile(params, maps, fit_baseline)
    want, wsep, bound = gf.profile(params, maps, fit_baseline)
    ok = [n for n in range(N) if n != 4]
    ratio = float((np.abs(got[ok] - want[ok]) / bound[ok]).max())
    dsep = float(np.abs(sep[ok] - wsep[ok]).max())
    print(f"profile {gh} x {gw} L {L} baseline {fit_baseline}: worst |difference| / bound {ratio:.3f} (largest bound {bound.max():.2e}), "
          f"separability {wsep[ok].round(4).tolist()}, worst difference {dsep:.2e}")
    assert ratio <= 1.0 and np.all(np.isnan(got[4])) and np.isnan(sep[4])
    # separability: a quotient of two sums of G L squares, each in another order (the sums of squared residuals are stationary
    # in the fitted coefficients, so the coefficients' own error enters in second order only)
    assert dsep <= 8 * gh * gw * L * gf.EPS64


def test_profile_is_exact_on_integer_data_with_a_dyadic_profile():
    """A shape so narrow that exp(-q / 2) is 1 on its centre cell and underflows to 0 elsewhere: every sum is a sum of integers."""
    gh, gw, L, N = 8, 12, 5, 5
    rng = np.random.default_rng(4)
    params = np.zeros((N, 7))
    maps = np.zeros((N, L, gh, gw), dtype=np.float32)
    dy = np.array([0.25, -1.5, 3.0, 0.0, 8.0])
    for n in range(N):
        cy, cx = int(rng.integers(0, gh)), int(rng.integers(0, gw))
        params[n] = (0.0, 1.0, cy, cx, 5.0, 0.0, 5.0)
        back = rng.integers(-4, 5, size=(L, gh, gw)).astype(np.float64)
        back[:, cy, cx] = 0
        back -= np.round(back.sum(axis=(1, 2), keepdims=True) / (gh * gw - 1))       # any integers: the background need not be centred
        maps[n] = back
        maps[n, :, cy, cx] = dy * (n + 1) * 16
    for fit_baseline in (True, False):
        got, sep = device_profile(params, maps, fit_baseline)
        want, wsep, _ = gf.profile(params, maps, fit_baseline)
        print(f"integer data (baseline {fit_baseline}): profile of neuron 1 {got[1].tolist()}, separability {sep.tolist()}")
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(sep), bits(wsep))
    assert np.array_equal(device_profile(params, maps, False)[0], dy[None] * 16 * np.arange(1, N + 1)[:, None])


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing():
    import sensorium_amd._lib as L
    d = dev()
    maps = torch.zeros(4, 8, 12, device=d)
    sentinel = -123.25
    params = torch.full((4, 7), sentinel, dtype=torch.float64, device=d)
    table = torch.full((4, 16), sentinel, dtype=torch.float64, device=d)
    ws = torch.full((4, 8), sentinel, dtype=torch.float64, device=d)

    def args(**kw):
        a = L.Gauss2dArgs()
        a.R, a.gh, a.gw, a.M, a.fit_baseline, a.max_iter = 4, 8, 12, 4, 1, 100
        a.rel_threshold, a.xtol, a.ftol = 0.5, XTOL, FTOL
        a.maps, a.sel, a.params, a.table, a.ws, a.ws_bytes = maps.data_ptr(), None, params.data_ptr(), table.data_ptr(), ws.data_ptr(), 4 * 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    stream = torch.cuda.current_stream().cuda_stream
    codes = {}
    for name, kw in (("gh = 2", dict(gh=2, gw=48)), ("G = 4097", dict(gh=17, gw=241)), ("M = 0", dict(M=0)), ("small workspace", dict(ws_bytes=4 * 64 - 8))):
        codes[name] = L.lib.dwn_gauss2d_fit(C.byref(args(**kw)), d.index, stream)
        assert L.lib.dwn_gauss2d_ws_bytes(C.byref(args(**kw))) == (4 * 64 if name == "small workspace" else 0)
    torch.cuda.synchronize()
    print("refusals:", codes)
    assert codes == {"gh = 2": -2, "G = 4097": -2, "M = 0": -2, "small workspace": -3}
    for t in (params, table, ws):
        assert bool((t == sentinel).all())
    from sensorium_amd import ops
    with pytest.raises(ValueError):
        ops.gauss2d_fit(torch.zeros(3, 2, 12, device=d))
    assert L.lib.dwn_gauss2d_fit(C.byref(args()), d.index, stream) == 0          # the same arguments, complete: runs
    torch.cuda.synchronize()
    assert bool((table[:, 0] == 2.0).all()) and bool((table[:, 15] == torch.arange(4, device=d)).all())


# ----------------------------------------------------------------------------------------------------------------------- digest
def rf_fit_digest():
    """(number of tensors, sha256) over params, table and start of two grids through a row table, and the profile of one."""
    h, n = hashlib.sha256(), 0
    for gh, gw, lv in ((8, 12, 2), (18, 32, 1), (36, 64, 2)):
        maps, _ = gf.planted_maps(gh, gw, 10, gf.NOISE_LEVELS[lv], 99)
        maps[3] = 0.5
        outs = device_fit(maps, sel=[9, 0, 1, 2, 3, 4, 5, 6, 7, 8, 4])
        for t in outs:
            h.update(t.tobytes()); n += 1
        held = device_fit(maps, fit_baseline=False, rel_threshold=0.25, max_iter=3)
        for t in held:
            h.update(t.tobytes()); n += 1
        lagged = np.stack([maps * s for s in (0.5, 1.0, -0.25)], axis=1).astype(np.float32)
        for t in device_profile(outs[0][1:], lagged):
            h.update(t.tobytes()); n += 1
    return n, h.hexdigest()

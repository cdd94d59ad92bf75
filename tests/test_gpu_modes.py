"""Population modes at kernel level, every stage through sensorium_amd.ops against tests/modes_reference.py: the
lane map of the float64 MFMA pinned bit for bit on exact operands first, then every stage at TWICE the bound the checker derives."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests import modes_reference as ref  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

pytestmark = pytest.mark.gpu


def block(X):
    """A numpy [N, p] array as a device block (padded row stride)."""
    from sensorium_amd import ops
    b = ops.modes_block(X.shape[0], X.shape[1], dev())
    b.copy_(torch.from_numpy(np.ascontiguousarray(X)))
    return b


def matrix(store, N):
    """The [N, N] view of a device copy of ``store`` [N, lda]."""
    return torch.from_numpy(np.ascontiguousarray(store)).to(dev())[:, :N]


@pytest.mark.parametrize("N", ref.LANE_NS)
def test_lane_map_pin_symm_is_exact_on_small_integers(N):
    from sensorium_amd import ops
    for p in ref.LANE_PS:
        if p > N:
            continue
        for pad, e in ((0, 0), (3, -3)):
            store, Q, scale = ref.lane_pin_operands(N, p, pad, e, seed=1000 * N + p)
            want = scale * (store[:, :N] @ Q)
            Y = ops.modes_symm(matrix(store, N), block(Q), scale)
            assert Y.stride(0) == ops.modes_pad(p) and int(torch.count_nonzero(Y._base[:, p:])) == 0
            assert np.array_equal(Y.cpu().numpy(), want), f"N = {N}, p = {p}, lda = N + {pad}: not bit for bit"


def test_symm_on_real_data():
    from sensorium_amd import ops
    rng = np.random.default_rng(3)
    worst = 0.0
    for N, p, scale in ((130, 24, 1.0 / 37), (65, 64, 1.0), (17, 5, -2.5)):
        A = ref.planted(N, ref.GAPPED, N) * rng.uniform(0.5, 2.0)
        Q = rng.normal(size=(N, p))
        Y = ops.modes_symm(matrix(A, N), block(Q), scale).cpu().numpy()
        want = (scale * (A.astype(np.longdouble) @ Q.astype(np.longdouble))).astype(np.float64)
        ratio = float((np.abs(Y - want) / ref.symm_bound(A, Q, scale)).max())
        worst = max(worst, ratio)
        assert ratio <= 2, f"N = {N}, p = {p}: {ratio:.3g} bounds"
    print(f"symm: worst ratio to the single bound {worst:.3g}")


@pytest.mark.parametrize("p", ref.EIGH_PS)
def test_small_eigh(p):
    from sensorium_amd import ops
    rng = np.random.default_rng(p)
    H = rng.normal(size=(p, p))
    H = 0.5 * (H + H.T)
    rep = np.diag(np.repeat([3.0, -1.0, 0.0], p)[:p])                     # repeated eigenvalues, rotated
    E, _ = np.linalg.qr(rng.normal(size=(p, p)))
    rep = E @ rep @ E.T
    rep = 0.5 * (rep + rep.T)
    for name, M in (("random", H), ("repeated", rep)):
        values, W = (t.cpu().numpy() for t in ops.modes_small_eigh(torch.from_numpy(M).to(dev())))
        b = ref.eigh_bound(M)
        want = np.linalg.eigvalsh(M)[::-1]
        r1 = np.abs(values - want).max() / b
        r2 = np.abs(W.T @ W - np.eye(p)).max() / (ref.JACOBI_C * p * ref.U)
        r3 = np.abs(M @ W - W * values).max() / b
        print(f"small_eigh p = {p} {name}: ratios {r1:.3g} {r2:.3g} {r3:.3g}")
        assert max(r1, r2, r3) <= 2 and (np.diff(values) <= 0).all()
        assert np.array_equal(ref.sign_rule(W), W)
    d = rng.permutation(np.arange(p, dtype=np.float64) - 2.5)
    values, W = (t.cpu().numpy() for t in ops.modes_small_eigh(torch.from_numpy(np.diag(d)).to(dev())))
    order = np.argsort(-d, kind="stable")
    assert np.array_equal(values, d[order]) and np.array_equal(W, np.eye(p)[:, order])         # a diagonal input: bit for bit
    bad = H.copy()
    bad[0, p - 1] = bad[p - 1, 0] = np.nan
    values, W = ops.modes_small_eigh(torch.from_numpy(bad).to(dev()))
    assert bool(torch.isnan(values).all())


def test_orth():
    from sensorium_amd import ops
    rng = np.random.default_rng(8)
    worst = 0.0
    for N, p in ((17, 16), (130, 24), (65, 64), (600, 17), (1, 1)):
        Y = rng.normal(size=(N, p)) * np.logspace(0, -5, p)
        Q = ops.modes_orth(block(Y)).cpu().numpy()
        r = np.abs(Q.T @ Q - np.eye(p)).max() / ref.orth_bound(N, p)
        span = np.linalg.norm(Y - Q @ (Q.T @ Y)) / (p * ref.orth_bound(N, p) * np.linalg.norm(Y))
        worst = max(worst, r, span)
        assert r <= 2 and span <= 2, f"N = {N}, p = {p}: {r:.3g}, {span:.3g} bounds"
    print(f"orth: worst ratio to the single bound {worst:.3g}")
    Y = rng.normal(size=(40, 6))
    Y[:, 3] = Y[:, 0] - 2 * Y[:, 1]
    Q = ops.modes_orth(block(Y)).cpu().numpy()
    keep = [0, 1, 2, 4, 5]
    assert (Q[:, 3] == 0).all() and np.abs(Q[:, keep].T @ Q[:, keep] - np.eye(5)).max() <= 2 * ref.orth_bound(40, 6)
    assert (ops.modes_orth(block(np.zeros((9, 4)))).cpu().numpy() == 0).all()


def test_ritz_stage_alone():
    from sensorium_amd import ops
    A = ref.planted(65, ref.GAPPED, 4)
    Q = ref.orth(ref.start_block(65, 16))
    Y = A @ Q
    H = Q.T @ Y
    theta, W = ref.small_eigh(0.5 * (H + H.T))
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev())      # noqa: E731
    V, r, status = ops.modes_ritz(block(Q), block(Y), to(theta), to(W), 6, 1e-10)
    R = Y @ W - (Q @ W) * theta
    assert np.abs(V.cpu().numpy() - Q @ W).max() <= 2 * (16 + 2) * ref.U
    assert np.abs(r.cpu().numpy() - np.sqrt((R * R).sum(axis=0))).max() <= 2 * ref.residual_bound(A, 16)
    assert status.cpu().tolist() == [0, 0, 1, 0]
    assert ops.modes_ritz(block(Q), block(Y), to(theta), to(W), 6, 1e3)[2].cpu().tolist() == [1, 1, 1, 0]


_SOLVED = {}


def solved(case):
    """One solve per case, shared by the tests (left unchanged)."""
    from sensorium_amd.population import modes
    name, N, build, k, oversample, gapped, converges = case
    if name not in _SOLVED:
        A = build()
        _SOLVED[name] = (A, modes(torch.from_numpy(A).to(dev()), k, oversample=oversample, max_iters=ref.MAX_ITERS, tol=ref.TOL))
    return _SOLVED[name]


@pytest.mark.parametrize("case", ref.SOLVE_CASES, ids=[c[0] for c in ref.SOLVE_CASES])
def test_solve_on_planted_spectra(case):
    name, N, build, k, oversample, gapped, converges = case
    A, m = solved(case)
    assert all(t.is_cuda for t in (m.values, m.vectors, m.residuals, m.trace, m.frobenius2, m.converged, m.rounds))
    assert m.values.shape == (k,) and m.vectors.shape == (N, k) and m.converged.dtype == torch.bool and m.rounds.dtype == torch.int32
    values, vectors, residuals = (t.cpu().numpy() for t in (m.values, m.vectors, m.residuals))
    ratios = ref.check_pairs(A, values, vectors, residuals, k, min(k + oversample, N), gapped, name)
    s = m.summary()
    print(f"{name}: rounds {s['rounds']}, ratios to the single bounds {({a: float(f'{b:.3g}') for a, b in ratios.items()})}")
    if converges:
        assert s["converged"] and 1 <= s["rounds"] <= ref.MAX_ITERS
        assert (residuals <= ref.TOL * abs(values[0])).all()
    tb, fb = ref.moments_bounds(A, 1.0)
    assert abs(s["trace"] - np.trace(A)) <= 2 * tb and abs(float(m.frobenius2) - (A * A).sum()) <= 2 * fb
    assert s["k"] == k and np.isclose(s["participation_ratio"], np.trace(A) ** 2 / (A * A).sum())
    assert np.isclose(s["leading_explained"], values[0] / np.trace(A)) and torch.equal(m.explained(), m.values / m.trace)


def test_rank_deficient_modes_are_exact_zeros():
    case = ref.SOLVE_CASES[[c[0] for c in ref.SOLVE_CASES].index("rank3-40")]
    A, m = solved(case)
    assert int(torch.count_nonzero(m.values[3:])) == 0 and int(torch.count_nonzero(m.vectors[:, 3:])) == 0 and bool(m.converged)
    from sensorium_amd.population import modes
    z = modes(torch.zeros(12, 12, dtype=torch.float64, device=dev()), 3)
    assert bool(z.converged) and int(torch.count_nonzero(z.values)) == 0 and int(torch.count_nonzero(z.vectors)) == 0
    assert not bool(torch.isnan(z.residuals).any())


def test_moments_exact_on_integers_and_bounded_on_real_data():
    from sensorium_amd import ops
    store, _, _ = ref.lane_pin_operands(130, 1, 3, 0, seed=5)
    got = ops.modes_moments(matrix(store, 130), 0.25).cpu().numpy()
    A = store[:, :130]
    assert got[0] == 0.25 * np.trace(A) and got[1] == 0.0625 * (A * A).sum()
    B = ref.planted(600, ref.GAPPED, 6)
    got = ops.modes_moments(matrix(B, 600), 1.0 / 3).cpu().numpy()
    tb, fb = ref.moments_bounds(B, 1.0 / 3)
    Bl = B.astype(np.longdouble)
    assert abs(got[0] - float(np.trace(Bl) / 3)) <= 2 * tb and abs(got[1] - float((Bl * Bl).sum() / 9)) <= 2 * fb


def digest_cases():
    from sensorium_amd.population import compare_modes, modes
    out = []
    for name in ("gapped-65", "slow-130", "rank3-40"):
        case = ref.SOLVE_CASES[[c[0] for c in ref.SOLVE_CASES].index(name)]
        A = torch.from_numpy(case[2]()).to(dev())
        m = modes(A, case[3], oversample=case[4], scale=0.25)
        c = compare_modes(m, modes(A, case[3], oversample=case[4], seed=3), A, 0.25)
        out += [m.values, m.vectors.contiguous(), m.residuals, m.trace, m.frobenius2, m.rounds, m.converged, c.cosines, c.captured]
    return out


def modes_digest():
    """sha256 over the results of fixed cases (tests/test_gpu_modes_det.py)."""
    h, n = hashlib.sha256(), 0
    for t in digest_cases():
        h.update(t.cpu().numpy().tobytes())
        n += 1
    return n, h.hexdigest()


def test_two_launches_agree_bit_for_bit_and_a_power_of_two_scale_is_exact():
    from sensorium_amd.population import modes
    a, b = modes_digest(), modes_digest()
    print(f"modes digest of {a[0]} tensors: {a[1]}")
    assert a == b
    A = ref.planted(65, ref.GAPPED, 165)
    m1 = modes(torch.from_numpy(A * 8.0).to(dev()), 6, scale=0.125)                   # co-moments with 1 / n a power of two
    m2 = modes(torch.from_numpy(A).to(dev()), 6)
    for name in ("values", "vectors", "residuals", "trace", "frobenius2", "rounds"):
        assert torch.equal(getattr(m1, name), getattr(m2, name)), name


@pytest.mark.parametrize("poison", [float("nan"), float("inf")])
def test_nan_and_inf_return_normally(poison):
    from sensorium_amd.population import modes
    A = ref.planted(65, ref.GAPPED, 165)
    A[7, 40] = A[40, 7] = poison
    m = modes(torch.from_numpy(A).to(dev()), 4, max_iters=64)
    s = m.summary()
    assert not s["converged"] and bool(torch.isnan(m.values).all()) and 1 <= s["rounds"] <= 64


def test_solve_is_capturable():
    from sensorium_amd.population import modes
    A = torch.from_numpy(ref.planted(65, ref.GAPPED, 165)).to(dev())
    eager = modes(A, 6)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        modes(A, 6)                                                                    # warm the allocator on the side stream
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        m = modes(A, 6)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(m.values, eager.values) and torch.equal(m.vectors, eager.vectors) and bool(m.converged)


def test_overlap():
    from sensorium_amd import ops
    rng = np.random.default_rng(9)
    N, k = 130, 5
    E, _ = np.linalg.qr(rng.normal(size=(N, N)))
    Va = E[:, :k]
    phi = np.array([0.05, 0.4, 0.9, 1.2, 1.5])
    cases = (("identical", Va, np.ones(k)), ("orthogonal", E[:, k:2 * k], None),
             ("rotated", Va * np.cos(phi) + E[:, k:2 * k] * np.sin(phi), np.cos(phi)))
    for name, Vb, known in cases:
        got = ops.modes_overlap(block(Va), block(Vb))[0].cpu().numpy()
        want = ref.cosines(Va, Vb)
        b = ref.cosine_bound(np.maximum(want, 0), N, k)
        assert (np.abs(got - want) <= 2 * b).all() and (np.diff(got) <= 0).all(), f"{name}: {got} against {want}"
        if known is not None:
            assert (np.abs(got - np.sort(known)[::-1]) <= 2 * b + 4 * N * ref.U).all()      # (the planted blocks are orthonormal to N u)
        else:
            assert got.max() <= 2 * b.max() + 4 * N * ref.U
    B = ref.planted(N, ref.GAPPED, 2)
    cos, mom = ops.modes_overlap(block(Va), block(Va), matrix(B, N), 0.25)
    want, bound = ref.captured(Va, B, 0.25)
    mom = mom.cpu().numpy()
    assert abs(mom[2] / mom[0] - want) <= 2 * bound

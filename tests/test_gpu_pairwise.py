"""The population-structure kernels against the longdouble checker tests/pairwise_reference.py, at TWICE the
bounds derived in its docstring (none was fitted to a measurement), and bit for bit where every operation is exact.  Every trial
lies in a buffer of its own with an odd offset of the kept frames, an odd row stride (rows are 4-byte aligned only) and NaN
everywhere outside the kept frames: a load outside them would show in every matrix.  The first test pins the C/D lane map of
v_mfma_f64_16x16x4_f64.  Every test prints what it measured before it asserts (worst ratio to the bound)."""
import hashlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import pairwise_cases as pc  # noqa: E402
from tests import pairwise_reference as ref  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

EPS = 1e-8
TILE = 64


def device_trials(trials, poison=float("nan")):
    """[(view [N, K + 2] of a poisoned buffer, group)]: the kept frames are [1, K + 1) of the view (FrameCut(1, None, 1)), the view
    starts at an odd offset of a buffer with an odd row stride."""
    out = []
    for i, (Y, g) in enumerate(trials):
        N, K = Y.shape
        first = 2 + 2 * (i % 3)                                       # view offset first - 1: odd
        ld = (first + K + 3 + (i % 2) * 4) | 1
        b = torch.full((N, ld), poison, dtype=torch.float32)
        b[:, first:first + K] = torch.from_numpy(np.ascontiguousarray(Y))
        out.append((b.to(dev())[:, first - 1:first + K + 1], g))
    return out


def gpu_run(trials, kinds=ref.KINDS, flush_after=(), flush_frames=1 << 30, dtype=torch.float64):
    """PairwiseCorrelation over the trials, flushed after the trials whose index is in ``flush_after``; returns (accumulator,
    CorrelationMatrices)."""
    from sensorium_amd.evaluation import FrameCut
    from sensorium_amd.population import PairwiseCorrelation
    acc = PairwiseCorrelation(trials[0][0].shape[0], dev(), kinds, FrameCut(1, None, 1), EPS, flush_frames)
    for i, (x, g) in enumerate(device_trials(trials)):
        acc.add(x, g)
        if i in flush_after:
            acc.flush()
    return acc, acc.compute(dtype)


def check(trials, res, label, kinds=ref.KINDS):
    """Counts exact; C, mean and the correlation matrix within twice the derived bounds; C bit-symmetric.  Returns the worst
    ratios to the (single) bound."""
    sets = ref.sample_sets(trials)
    worst = {}
    for kind in kinds:
        X = sets[kind]
        n = X.shape[1]
        assert res.counts[kind] == n, (kind, res.counts[kind], n)
        m, C = ref.comoments(X)
        C64 = np.asarray(C, dtype=np.float64)
        got = res.comoments(kind).cpu().numpy()
        R = getattr(res, kind).cpu().numpy()
        if n == 0:
            assert np.all(got == 0) and np.isnan(R).all()
            continue
        assert np.array_equal(got, got.T), f"{label} {kind}: C is not bit-symmetric"
        _, G, n_src, Rmax, A = ref.set_stats(trials, kind)
        finite = np.isfinite(C64)
        rc = np.abs(got - C64)[finite] / ref.comoment_bound(trials, kind, C64)[finite]
        rm = np.abs(res.mean(kind).cpu().numpy() - np.asarray(m, dtype=np.float64)) / ref.value_err(n_src, G, Rmax, A)
        cb = ref.corr_bound(trials, kind, C64, EPS)
        claim = np.isfinite(cb)
        rr = np.abs(R - ref.corr_matrix(C, n, EPS))[claim] / cb[claim]
        flat = ~claim & finite
        assert np.all(R[flat] == 0.0), f"{label} {kind}: a constant neuron's row is not exactly zero"
        worst[kind] = (float(np.nanmax(rc, initial=0.0)), float(np.nanmax(rm[np.isfinite(rm)], initial=0.0)), float(np.nanmax(rr, initial=0.0)))
    print(f"pairwise {label}: worst ratio to the derived bound (C, mean, corr): "
          + "; ".join(f"{k} {v[0]:.3g} {v[1]:.3g} {v[2]:.3g}" for k, v in worst.items()))
    assert all(max(v) <= 2.0 for v in worst.values()), worst
    return worst


def exact(trials, kinds, label):
    acc, res = gpu_run(trials, kinds)
    sets = ref.sample_sets(trials)
    for kind in kinds:
        m, C = ref.comoments(sets[kind])
        got = res.comoments(kind).cpu().numpy()
        C64 = np.asarray(C, dtype=np.float64)
        bad = np.argwhere(got != C64)
        assert bad.size == 0, f"{label} {kind}: {len(bad)} of {C64.size} elements differ, first at {bad[0]}: {got[tuple(bad[0])]} != {C64[tuple(bad[0])]}"
        assert np.array_equal(res.mean(kind).cpu().numpy(), np.asarray(m, dtype=np.float64)), (label, kind)
        assert res.counts[kind] == sets[kind].shape[1]
    print(f"pairwise {label}: {', '.join(kinds)} bit for bit on {trials[0][0].shape[0]} neurons")


def test_lane_map_pin_exact_integer_rows_on_two_tile_rows():
    """Exact-integer rows that all differ, N = 2 tiles + 1: the f32 row map, a transposed mirror or a wrong operand slice each
    move integers to other elements (tests/test_pairwise_reference_cpu.py shows they fall far outside)."""
    N = 2 * TILE + 1
    exact(pc.integer_case(N), ref.KINDS, "lane-map pin, equal chunk means")
    exact(pc.integer_case(N, groups=2, equal_means=False), ("signal", "noise"), "lane-map pin, merge coefficient 2")
    exact(pc.integer_pair_case(N), ("total",), "lane-map pin, two single trials")


@pytest.mark.parametrize("N", [1, 5, 16, 17, 63, 64, 65, 130])
def test_exact_integers_around_the_tile_edges(N):
    exact(pc.integer_case(N, repeats=3), ref.KINDS, f"N = {N}, equal chunk means, 3 repeats")
    exact(pc.integer_case(N, groups=2, repeats=5, equal_means=False), ("signal", "noise"), f"N = {N}, merge coefficient 2, 5 repeats")
    exact(pc.integer_pair_case(N), ("total",), f"N = {N}, two single trials")


@pytest.mark.parametrize("N", [1, 5, 16, 17, 63, 64, 65, 129, 130])
def test_neuron_counts_around_the_tile_edges(N):
    trials = pc.shape_case(N, 5, 3)
    check(trials, gpu_run(trials)[1], f"N = {N}, K = 5, 3 groups")


@pytest.mark.parametrize("K", [1, 3, 4, 5, 250])
def test_kept_frames_around_the_k_step(K):
    trials = pc.shape_case(17, K, 2, repeats=3)
    check(trials, gpu_run(trials)[1], f"N = 17, K = {K}, 2 groups of 3")


@pytest.mark.parametrize("chunks", [1, 2, 3, 7])
def test_chunk_counts(chunks):
    trials = pc.shape_case(33, 6, chunks)
    check(trials, gpu_run(trials)[1], f"N = 33, K = 6, {chunks} groups")


def test_mixed_groups_constant_and_offset_neuron_and_both_output_types():
    trials = pc.mixed_case()
    acc, res = gpu_run(trials)
    check(trials, res, "mixed case (groups of 2, 3, 5; single trials; a constant neuron; one at mean = 1e4 sigma)")
    for kind in ref.KINDS:
        R = getattr(res, kind).cpu().numpy()
        assert np.all(R[pc.CONSTANT] == 0) and np.all(R[:, pc.CONSTANT] == 0)
        assert abs(R[pc.OFFSET, pc.OFFSET] - 1.0) < 1e-6
        R32 = acc.compute(torch.float32)
        got32 = getattr(R32, kind)
        assert got32.dtype == torch.float32
        assert np.array_equal(got32.cpu().numpy(), R.astype(np.float32)), f"{kind}: fp32 output is not the double rounded once"
        assert np.array_equal(R32.comoments(kind).cpu().numpy(), res.comoments(kind).cpu().numpy())      # finalize leaves the state
    # only single trials: signal and noise have no sample, NaN everywhere; the state stays zero
    singles = [(y, None) for y, _ in trials[:3]]
    _, res = gpu_run(singles)
    check(singles, res, "single trials only")
    assert res.counts["signal"] == res.counts["noise"] == 0 and torch.isnan(res.signal).all() and torch.isnan(res.noise).all()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_non_finite_value_reaches_only_its_own_row_and_column(bad):
    trials = pc.mixed_case(N=70)
    who = 66
    clean = gpu_run(trials)[1]
    dirty_trials = [(y.copy(), g) for y, g in trials]
    dirty_trials[4][0][who, 2] = bad                                   # inside the 5-group: every kind sees it
    dirty = gpu_run(dirty_trials)[1]
    keep = np.ones(70, dtype=bool)
    keep[who] = False
    for kind in ref.KINDS:
        for a, b in ((clean.comoments(kind), dirty.comoments(kind)), (getattr(clean, kind), getattr(dirty, kind))):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            assert np.array_equal(a[np.ix_(keep, keep)], b[np.ix_(keep, keep)]), kind
            assert not np.isfinite(b[who]).any() and not np.isfinite(b[:, who]).any(), kind
        assert np.array_equal(clean.mean(kind).cpu().numpy()[keep], dirty.mean(kind).cpu().numpy()[keep])
    print(f"pairwise non-finite ({bad}): rows and columns other than {who} are bit for bit those of the clean run")


def state_bits(res, kinds=ref.KINDS):
    return [res._states[k].cpu().numpy().tobytes() for k in kinds]


def test_several_flushes_equal_one_bit_for_bit():
    """The trials of every group adjacent, so that flushing between units keeps the table order; launches of 1, 2 and all units,
    and an accumulator that cuts its own launches (flush_frames below one group)."""
    trials = sorted(pc.mixed_case(N=70), key=lambda t: {"a": 0, None: 1, "b": 2, "lonely": 3, "c": 4}[t[1]])
    groups = [g for _, g in trials]
    ends = [i for i in range(len(trials)) if i + 1 == len(trials) or groups[i + 1] != groups[i] or groups[i] is None]
    one = gpu_run(trials)[1]
    check(trials, one, "flush test, one flush")
    for cuts in (ends[:1], ends[::2], ends):
        many = gpu_run(trials, flush_after=set(cuts))[1]
        assert state_bits(one) == state_bits(many), f"flushing after trials {cuts} changed the state"
        assert one.counts == many.counts
    auto = gpu_run(trials, flush_frames=16)[1]
    assert state_bits(one) == state_bits(auto) and one.counts == auto.counts
    print(f"pairwise flushes: one launch, {len(ends)} launches and launches of at most 16 columns give the same bits")


def pairwise_digest():
    """sha256 over the states, the matrices and the comparison of fixed cases (tests/test_gpu_pairwise_det.py)."""
    from sensorium_amd.population import compare
    h, n = hashlib.sha256(), 0
    for trials in (pc.mixed_case(N=70), pc.shape_case(130, 37, 3, repeats=3)):
        res = gpu_run(trials)[1]
        cmp_ = compare(res.total, res.noise)
        for t in [res._states[k] for k in ref.KINDS] + [getattr(res, k) for k in ref.KINDS] + [cmp_.per_neuron, cmp_._summary]:
            h.update(t.cpu().numpy().tobytes())
            n += 1
    return n, h.hexdigest()


def test_two_launches_agree_bit_for_bit():
    a, b = pairwise_digest(), pairwise_digest()
    print(f"pairwise digest of {a[0]} tensors: {a[1]}")
    assert a == b


def test_staged_operand_layout():
    """Z as dwn_pair_stage leaves it: k-major, ldz = N rounded up to the tile, zero beyond N, the merge column and the zero
    columns of every chunk where the header says, equal to the float64 restatement within the mean's bound."""
    from sensorium_amd import ops
    trials = pc.shape_case(21, 6, 2, repeats=3)
    dts = device_trials(trials)
    for kind in ref.KINDS:
        state = torch.zeros(22, 21, dtype=torch.float64, device=dev())
        tables = ops.pair_tables([(x, 1, 6) for x, _ in dts], [(0, 3, 6), (3, 3, 6)], 21, dev())
        n, Z = ops.pair_accumulate(state, kind, tables, 0, return_staged=True)
        want, mean, count = ref.stage(ref.chunks(trials, kind), np.zeros(21), 0)
        Z = Z.cpu().numpy()
        assert n == count and Z.shape == (want.shape[0], TILE) and want.shape[0] % 4 == 0
        assert np.all(Z[:, 21:] == 0)
        zero_rows = np.all(want == 0, axis=1)
        assert np.all(Z[zero_rows] == 0)
        _, G, n_src, Rmax, A = ref.set_stats(trials, kind)
        e = ref.value_err(n_src, G, Rmax, A)
        # a centred value errs by e + u |z|, the merge column by c 2 e + 4 u |z| with c <= sqrt(n_b) <= 4.3
        assert np.all(np.abs(Z[:, :21] - want) <= 2 * (9 * e[None] + 4 * ref.U * np.abs(want)))
        assert np.all(np.abs(state[-1].cpu().numpy() - mean) <= 2 * e)


def test_compare_with_and_without_selection_and_a_nan_row():
    from sensorium_amd.population import compare
    rng = np.random.default_rng(11)
    N = 131
    A = rng.normal(size=(N, N)); A = (A + A.T) / 2
    B = 0.7 * A + 0.3 * rng.normal(size=(N, N)); B = (B + B.T) / 2 + 1e3          # a large common offset: centring must not cancel
    Abuf = torch.full((N, N + 3), float("nan"), dtype=torch.float64)               # a leading dimension of its own
    Abuf[:, :N] = torch.from_numpy(A)
    sel = np.array([130, 0, 64, 63, 65, 7, 100, 1, 129])
    for name, a, b, s in (("all", A, B, None), ("selection", A, B, sel), ("one neuron", A, B, np.array([5]))):
        res = compare(Abuf.to(dev())[:, :N], torch.from_numpy(b).to(dev()), None if s is None else torch.from_numpy(s).to(dev()), EPS)
        per, summ = ref.compare(a, b, s, EPS)
        pb, sb = ref.compare_bound(a, b, s, EPS)
        got, gs = res.per_neuron.cpu().numpy(), res._summary.cpu().numpy()
        if name == "one neuron":
            assert np.isnan(got).all() and gs[0] == 0 and np.isnan(gs[1:]).all() and res.summary()["pairs"] == 0
            continue
        rp, rs = np.abs(got - per) / pb, np.abs(gs - summ)[1:] / sb[1:]
        print(f"pairwise compare {name}: worst ratio to the derived bound per neuron {rp.max():.3g}, summary {rs.max():.3g}")
        assert gs[0] == summ[0] == len(per) * (len(per) - 1) and rp.max() <= 2.0 and rs.max() <= 2.0
        order = np.argsort(per, kind="stable")[:3]
        worst = res.worst(3).cpu().numpy()
        assert worst.dtype == np.int64 and set(worst) == set((np.arange(N) if s is None else s)[order])
    An = A.copy()
    An[64, 3] = np.nan
    res = compare(torch.from_numpy(An).to(dev()), torch.from_numpy(B).to(dev()))
    got, gs = res.per_neuron.cpu().numpy(), res._summary.cpu().numpy()
    per, _ = ref.compare(A, B, None, EPS)
    assert np.isnan(got[64]) and np.array_equal(np.delete(got, 64), np.delete(compare(torch.from_numpy(A).to(dev()), torch.from_numpy(B).to(dev())).per_neuron.cpu().numpy(), 64))
    assert gs[0] == N * (N - 1) and np.isnan(gs[1:]).all()
    assert 64 not in res.worst(N).cpu().numpy() and len(res.worst(N)) == N - 1
    # a selection that leaves the NaN column out is clean again; an index outside [0, N) is NaN, not a fault
    res = compare(torch.from_numpy(An).to(dev()), torch.from_numpy(B).to(dev()), [0, 1, 2, 64, 70])
    assert torch.isfinite(res.per_neuron).all() and np.isfinite(res._summary.cpu().numpy()).all()
    res = compare(torch.from_numpy(A).to(dev()), torch.from_numpy(B).to(dev()), [0, 1, N, 5])
    assert torch.isnan(res.per_neuron).all() and np.isnan(res._summary.cpu().numpy()[1:]).all()

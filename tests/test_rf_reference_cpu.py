"""CPU tests of the float64 checker of the receptive-field mapping (tests/rf_reference.py) against brute
force: the Philox known answers, the vectorised generator against a scalar restatement, the stimulus' addressing, the accumulate
against an einsum over explicitly shifted arrays, the finaliser against numpy.cov / corrcoef, the invariance of the covariance
under the two centres at its a-priori bound, the summary against a plain restatement, and the planted-filter case that the GPU
tests run through the kernels.  Every test prints what it measured before it asserts."""
import numpy as np
import pytest

from tests import rf_reference as rf


def test_philox_known_answers():
    for counter, key, want in rf.KNOWN_ANSWERS:
        got = rf.philox_scalar(counter, key)
        vec = rf.philox(*[np.array([c]) for c in counter], key)[0]
        print("philox", [hex(w) for w in got])
        assert tuple(got) == want and tuple(int(w) for w in vec) == want


def _scalar_noise(batch, frames, gh, gw, hold, seed, first_clip):
    out = np.zeros((batch, frames, gh * gw), dtype=np.uint32)
    for b in range(batch):
        for t in range(frames):
            for q in range(gh * gw):
                out[b, t, q] = rf.philox_scalar((q >> 2, t // hold, first_clip + b, 0), (seed & rf.MASK, seed >> 32))[q & 3]
    return out


@pytest.mark.parametrize("gh, gw, hold, seed, first_clip", [(3, 7, 1, 0, 0), (5, 5, 2, 0xDEADBEEF12345678, 7), (1, 1, 3, 1, 2 ** 32 - 2)])
def test_vectorised_generator_equals_scalar_on_a_ragged_grid(gh, gw, hold, seed, first_clip):
    assert (gh * gw) % 4 != 0                                   # the last counter is partly used
    got = rf.noise_words(2, 5, gh, gw, hold=hold, seed=seed, first_clip=first_clip)
    want = _scalar_noise(2, 5, gh, gw, hold, seed, first_clip)
    print("words differing:", int((got != want).sum()), "of", want.size)
    assert np.array_equal(got, want)


def test_noise_addressing_hold_chunks_window_and_template():
    kw = dict(kind="binary", cell=2, hold=3, window=(1, 2, 6, 8), pad=5.0, behavior=(1.0, 2.0), pupil_center=(3.0, 4.0), seed=11)
    x = rf.noise(6, 7, (9, 11), **kw)
    assert x.shape == (6, 5, 7, 9, 11) and x.dtype == np.float32
    # hold: frames 0-2, 3-5 and 6 are three different draws, constant inside a group
    v = x[:, 0]
    assert np.array_equal(v[:, 0], v[:, 1]) and np.array_equal(v[:, 1], v[:, 2]) and np.array_equal(v[:, 3], v[:, 5])
    assert not np.array_equal(v[:, 2], v[:, 3]) and not np.array_equal(v[:, 5], v[:, 6])
    # chunk invariance: clip k of a batch starting at 2 is clip 2 + k of the whole
    part = rf.noise(3, 7, (9, 11), first_clip=2, **kw)
    assert np.array_equal(part, x[2:5])
    # window and pad; cells are 2 x 2 blocks; values are the two levels only
    win = v[:, :, 1:7, 2:10]
    outside = np.ones((9, 11), dtype=bool)
    outside[1:7, 2:10] = False
    assert np.all(v[:, :, outside] == 5.0)
    assert np.array_equal(win[:, :, 0::2, 0::2], win[:, :, 1::2, 1::2]) and np.array_equal(win[:, :, 0::2, 0::2], win[:, :, 0::2, 1::2])
    assert set(np.unique(win)) == {np.float32(63.5), np.float32(191.5)}
    share = float((win == np.float32(191.5)).mean())
    print("bright share", share)
    assert 0.4 < share < 0.6
    # template channels
    for c, want in zip(range(1, 5), (1.0, 2.0, 3.0, 4.0)):
        assert np.all(x[:, c] == want)
    y = rf.noise(1, 2, (4, 4), in_channels=6, video_channel=2, behavior=(1.0, 2.0), pupil_center=(3.0, 4.0))
    assert [float(y[0, c, 0, 0, 0]) for c in (0, 1, 3, 4, 5)] == [1.0, 2.0, 3.0, 4.0, 0.0]
    # a different seed and a different clip give a different draw
    assert not np.array_equal(rf.noise(1, 2, (8, 8), seed=1), rf.noise(1, 2, (8, 8), seed=2))
    assert not np.array_equal(rf.noise(1, 2, (8, 8), seed=1 << 32), rf.noise(1, 2, (8, 8), seed=0))


def test_sparse_densities():
    zero = rf.noise(2, 3, (8, 8), kind="sparse", density=0.0)[:, 0]
    one = rf.noise(2, 3, (8, 8), kind="sparse", density=1.0)[:, 0]
    tenth = rf.noise(8, 16, (16, 16), kind="sparse", density=0.1)[:, 0]
    shares = [float((tenth == v).mean()) for v in (63.5, 127.5, 191.5)]
    print("sparse shares at density 0.1 (dark, background, bright):", shares)
    assert np.all(zero == 127.5) and not np.any(one == 127.5) and set(np.unique(one)) == {np.float32(63.5), np.float32(191.5)}
    assert abs(shares[0] - 0.05) < 0.01 and abs(shares[2] - 0.05) < 0.01 and abs(shares[1] - 0.9) < 0.02


def _case(seed=0, B=3, N=4, T=9, H=7, W=10, window=(1, 1, 6, 8), cell=2, quantised=False):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, size=(B, 2, T, H, W)).astype(np.float32)
    r = rng.normal(size=(B, N, T)).astype(np.float32) * 3 + 2
    if quantised:
        r = np.round(r * 16) / 16
    return x, r.astype(np.float32), window, cell


@pytest.mark.parametrize("L, skip", [(1, 0), (3, 0), (3, 5), (4, 3)])
def test_accumulate_equals_einsum_over_shifted_arrays(L, skip):
    x, r, window, cell = _case()
    s0, r0 = 100.0, np.array([0.5, -1.0, 2.0, 0.0], dtype=np.float32)
    st = rf.State(4, L, 3, 4)
    rf.accumulate(st, x[:2], r[:2], channel=1, window=window, cell=cell, skip=skip, s0=s0, r0=r0)
    rf.accumulate(st, x[2:], r[2:], channel=1, window=window, cell=cell, skip=skip, s0=s0, r0=r0)
    # brute force: block means by reshape, explicit shifted copies
    y0, x0, wh, ww = window
    T = x.shape[2]
    v = x[:, 1, :, y0:y0 + wh, x0:x0 + ww].astype(np.float64).reshape(3, T, 3, 2, 4, 2).mean(axis=(3, 5)).reshape(3, T, 12) - s0
    u = (r - r0[None, :, None]).astype(np.float64)              # the definition forms u in fp32 (the block means are exact there)
    assert (r - r0[None, :, None]).dtype == np.float32
    t0 = max(skip, L - 1)
    shifted = np.stack([v[:, t0 - l:T - l] for l in range(L)], axis=1)          # [B, L, T - t0, G]
    want = np.einsum("bnt,bltg->nlg", u[:, :, t0:], shifted)
    err = float(np.abs(st.Cuv - want).max())
    print("accumulate vs einsum: max abs err", err, "K", st.K)
    assert st.K == 3 * (T - t0)
    assert np.allclose(st.Cuv, want, rtol=0, atol=1e-9 * np.abs(want).max())
    assert np.allclose(st.U1, u[:, :, t0:].sum(axis=(0, 2))) and np.allclose(st.U2, (u[:, :, t0:] ** 2).sum(axis=(0, 2)))
    assert np.allclose(st.V1, shifted.sum(axis=(0, 2))) and np.allclose(st.V2, (shifted ** 2).sum(axis=(0, 2)))
    flat = st.flat()
    back = rf.State.from_flat(flat, 4, L, 3, 4, st.K)
    assert np.array_equal(back.Cuv, st.Cuv) and np.array_equal(back.V2, st.V2) and np.array_equal(back.U2, st.U2)


def test_finalize_equals_numpy_cov_and_corrcoef():
    x, r, window, cell = _case(seed=3, B=6, T=12)
    L, skip = 3, 2
    st = rf.State(4, L, 3, 4)
    r0 = r.mean(axis=(0, 2)).astype(np.float32)
    rf.accumulate(st, x, r, channel=1, window=window, cell=cell, skip=skip, s0=127.5, r0=r0)
    cov, z, _ = rf.finalize(st)
    u = (r - r0[None, :, None]).astype(np.float32)             # the data the definition correlates: u is formed in fp32
    v = rf.cell_values(x, 1, window, cell, 0.0).astype(np.float64)
    worst_c = worst_z = 0.0
    for n in range(4):
        for l in range(L):
            for g in range(12):
                a = u[:, n, skip:].astype(np.float64).ravel()
                b = v[:, skip - l:12 - l, g].ravel()
                c = np.cov(a, b, bias=True)[0, 1]
                rho = np.corrcoef(a, b)[0, 1]
                worst_c = max(worst_c, abs(cov[n, l].ravel()[g] - c))
                worst_z = max(worst_z, abs(z[n, l].ravel()[g] - rho * np.sqrt(st.K)))
    print("finalize vs numpy.cov / corrcoef: worst", worst_c, worst_z)
    assert worst_c < 1e-10 and worst_z < 1e-10


def test_cov_is_invariant_under_the_centres_at_the_float64_bound():
    x, r, window, cell = _case(seed=5, B=8, T=12, quantised=True)      # integers and sixteenths: u and v form exactly in fp32
    sd_s, sd_r = 74.0, 3.0
    results = []
    for s0, r0 in ((127.5, 2.0), (127.5 + 100 * sd_s, 2.0 + 100 * sd_r), (127.5 - 100 * sd_s, 2.0 - 100 * sd_r)):
        st = rf.State(4, 3, 3, 4)
        rf.accumulate(st, x, r, channel=1, window=window, cell=cell, skip=0, s0=s0, r0=np.full(4, r0, dtype=np.float32))
        results.append((rf.covariance(st), rf.cov_f64_bound(st)))
    for cov, bound in results[1:]:
        ratio = float((np.abs(cov - results[0][0]) / (bound + results[0][1])).max())
        print("cov shift invariance: worst |difference| / bound", ratio, "bound", float(bound.max()))
        assert ratio <= 1.0
    assert float(results[1][1].max()) < 1e-6 * float(np.abs(results[0][0]).max())      # the bound itself says something


def _plain_summary(cov, z, gh, gw, rel):
    out = []
    for n in range(cov.shape[0]):
        energy = [float(sum(c * c for c in cov[n, l].ravel())) for l in range(cov.shape[1])]
        if not sum(energy) > 0:
            out.append([0, 0, np.nan, np.nan, np.nan, np.nan, 0, 0])
            continue
        l = min(i for i, e in enumerate(energy) if e == max(energy))
        flat = cov[n, l].ravel()
        peak = max(abs(c) for c in flat)
        i = min(k for k, c in enumerate(flat) if abs(c) == peak)
        cells = [(k // gw, k % gw, c * c) for k, c in enumerate(flat) if abs(c) >= rel * peak]
        sw = sum(w for _, _, w in cells)
        cy, cx = sum(w * y for y, _, w in cells) / sw, sum(w * x for _, x, w in cells) / sw
        sy = np.sqrt(sum(w * (y - cy) ** 2 for y, _, w in cells) / sw)
        sx = np.sqrt(sum(w * (x - cx) ** 2 for _, x, w in cells) / sw)
        out.append([l, z[n, l].ravel()[i], cy, cx, sy, sx, energy[l] / sum(energy), len(cells)])
    return np.array(out, dtype=np.float64)


def test_summary_equals_a_plain_restatement_with_ties_and_the_zero_neuron():
    gh, gw, L, N = 3, 4, 3, 5
    rng = np.random.default_rng(9)
    st = rf.State(N, L, gh, gw)
    st.K = 64
    st.U1[:] = 0.0; st.U2[:] = 64.0; st.V1[:] = 0.0; st.V2[:] = 64.0 * 4.0
    C = rng.integers(-9, 10, size=(N, L, gh * gw)).astype(np.float64)
    C[1] = 0.0                                                   # the all-zero neuron
    C[2] = 0.0; C[2, 1, 5] = 8.0; C[2, 2, 7] = -8.0              # two lags of equal energy: the lower lag wins
    C[3] = 0.0; C[3, 0, 2] = -6.0; C[3, 0, 9] = 6.0; C[3, 0, 4] = 3.0      # two peak cells of equal size: the lower index wins
    st.Cuv = C * 64.0
    cov, z, summary = rf.finalize(st, rel_threshold=0.5)
    want = _plain_summary(cov.reshape(N, L, -1), z.reshape(N, L, -1), gh, gw, 0.5)
    print("summary\n", summary)
    assert np.allclose(summary, want, rtol=0, atol=1e-12, equal_nan=True)
    assert summary[1].tolist()[:2] == [0.0, 0.0] and np.all(np.isnan(summary[1, 2:6])) and summary[1, 6] == 0 and summary[1, 7] == 0
    assert summary[2, 0] == 1 and summary[2, 7] == 1 and (summary[2, 2], summary[2, 3]) == (1.0, 1.0) and summary[2, 6] == 0.5
    assert summary[3, 0] == 0 and summary[3, 1] < 0 and summary[3, 7] == 3      # the peak cell is index 2 (negative); 3.0 >= 0.5 * 6.0 is kept
    assert z[2, 1].ravel()[5] == 32.0 == summary[2, 1]            # cov 8, var_u 1, var_v 4, K 64: z = 8 * 8 / 2


PLANTED = dict(gh=8, gw=12, L=5, T=16, clips=512, seed=2023, contrast=64.0)


def planted_case(kind):
    """(stimulus [B, 5, T, 8, 12], responses [B, 1, T], filter) of the planted-filter case."""
    p = PLANTED
    x = rf.noise(p["clips"], p["T"], (p["gh"], p["gw"]), kind=kind, seed=p["seed"], contrast=p["contrast"], density=0.1)
    f = rf.planted_filter(p["gh"], p["gw"])
    r = rf.planted_response(x[:, 0], f, 127.5, 0.3 / p["contrast"])
    return x, r, f


def planted_condition(cov, summary, f):
    """(cosine, peak lag, cy, cx) of neuron 0 against the planted filter."""
    c = np.asarray(cov, dtype=np.float64)[0].ravel()
    cos = float(c @ f.ravel() / (np.linalg.norm(c) * np.linalg.norm(f)))
    return cos, int(summary[0, 0]), float(summary[0, 2]), float(summary[0, 3])


@pytest.mark.parametrize("kind", ["binary", "sparse"])
def test_planted_filter_is_recovered(kind):
    x, r, f = planted_case(kind)
    st = rf.State(1, PLANTED["L"], PLANTED["gh"], PLANTED["gw"])
    for k0 in range(0, PLANTED["clips"], 128):
        rf.accumulate(st, x[k0:k0 + 128], r[k0:k0 + 128], skip=0, s0=127.5, r0=np.array([r[:32].mean()], dtype=np.float32))
    cov, _, summary = rf.finalize(st)
    cos, lag, cy, cx = planted_condition(cov, summary, f)
    print(f"planted filter ({kind}): K {st.K}, cosine {cos:.3f}, peak lag {lag}, centre ({cy:.2f}, {cx:.2f})")
    assert st.K == 6144
    assert lag == 2 and cos >= 0.9 and abs(cy - 3.0) <= 0.25 and abs(cx - 7.0) <= 0.25

"""The correlation kernels through the C-ABI (include/dwn.h dwn_corr_moments / dwn_corr_loss_finalize / dwn_corr_loss_backward,
DESIGN.md 12i) against the float64 checker tests/corr_reference.py (itself held to ``corr`` and to float64 autograd on the CPU:
tests/test_correlation_loss_cpu.py).  Every case prints what it measured before it asserts.

Bounds, derived, not measured (n = counted rows x T, u64 = 2^-53):
  moments   float64 sums of n terms in another order than the checker's: 64 n u64, relative to the moment's own scale — the mean of
            |p| (|t|) for the means, the moment itself for M2p / M2t (sums of non-negative terms), sqrt(M2p M2t) >= sum |dp dt| for C.
  r         three moments enter, each to the bound above, and a handful of correctly rounded float64 operations: 4 x 64 n u64 + 2^-50.
  loss      the checker's float64 value rounded to fp32, within 1 ulp (the float64 error above is far below half an ulp: the ulp
            covers a double rounding at a tie).
  dpred     1 fp32 ulp of the checker's element plus |g share rho| x 1e-9 x the neuron's largest |(t - mt) / (n a c)|: the slack of
            the cancellation between the two terms in float64 (|g share rho| <= 1 in every case here, so this is never wider than
            1e-9 x that magnitude).
Rows of weight 0 hold NaN in p and t: they must not be read.  Every output buffer sits between two guard bands that must come back
untouched, every case is launched twice and the two sets of outputs must agree bit for bit.
"""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import corr_reference as cr  # noqa: E402
from tests.gpu_helpers import dev, stream  # noqa: E402

U64 = 2.0 ** -53
GUARD, SENTINEL = 64, -7777.0
G = 0.75                                  # the incoming gradient of every case
WEIGHT_KINDS = ("all", "subset", "one", "none")


def guarded(n, dtype, misalign=0):
    flat = torch.full((n + 2 * GUARD + misalign,), SENTINEL, dtype=dtype, device=dev())
    return flat, flat[GUARD + misalign:GUARD + misalign + n]


def guards_ok(flat, n, misalign=0):
    return bool((flat[:GUARD + misalign] == SENTINEL).all()) and bool((flat[GUARD + misalign + n:] == SENTINEL).all())


def row_weights(B, kind, seed):
    """The weight column of one mouse: non-zero magnitudes differ from 1 (they must not enter), zeros are exact."""
    rng = np.random.default_rng(seed)
    w = np.zeros(B, np.float32)
    if kind == "all":
        rows = np.arange(B)
    elif kind == "subset":
        rows = np.sort(rng.choice(B, size=max(1, B // 2), replace=False)) if B > 1 else np.arange(1)
    elif kind == "one":
        rows = np.array([int(rng.integers(B))])
    else:
        rows = np.array([], dtype=np.int64)
    w[rows] = (0.25 + rng.integers(1, 8, size=len(rows)) / 4.0).astype(np.float32)
    return w


def make_case(B, N, T, kind, seed):
    """Softplus-like predictions, ReLU'd targets; degenerate neurons in the same tensors (a constant target, a constant prediction;
    n = 1 arises with one row and T = 1); NaN in the rows of weight 0."""
    rng = np.random.default_rng(seed)
    p = (np.abs(rng.normal(size=(B, N, T))) * 2 + 0.05).astype(np.float32)
    t = (np.maximum(rng.normal(size=(B, N, T)), 0) * 6).astype(np.float32)
    degenerate = {}
    if N >= 7:
        t[:, 1, :] = 2.5
        p[:, N - 2, :] = 1.375
        t[:, 3, :] = 0.0                  # an all-zero (silent) neuron: the common constant target
        degenerate = dict(const_t=[1, 3], const_p=[N - 2])
    w = row_weights(B, kind, seed + 1)
    p[w == 0] = np.nan
    t[w == 0] = np.nan
    return p, t, w, degenerate


def launch(p, t, w, share, reduction, g=G, misalign=0, w_stride=1, eps=cr.EPS):
    """moments -> finalize -> f64_to_f32 -> backward on the device; everything comes back as numpy."""
    import sensorium_amd._lib as L
    B, N = p.shape[:2]
    T = p.shape[2] if p.ndim == 3 else 1
    n_el = B * N * T
    pf, pd = guarded(n_el, torch.float32, misalign)
    tf, td = guarded(n_el, torch.float32, misalign)
    df, dd = guarded(n_el, torch.float32, misalign)
    pd.copy_(torch.from_numpy(p).reshape(-1))
    td.copy_(torch.from_numpy(t).reshape(-1))
    wmat = torch.full((B, w_stride), float("nan"), dtype=torch.float32)
    wmat[:, 0] = torch.from_numpy(w)
    wd = wmat.to(dev())
    sf, sd = guarded(8 * N + 1, torch.float64)
    share_d = torch.tensor([share], dtype=torch.float32, device=dev())
    g_d = torch.tensor([g], dtype=torch.float32, device=dev())
    acc = torch.zeros(1, dtype=torch.float64, device=dev())
    out32 = torch.empty(1, dtype=torch.float32, device=dev())
    a = L.CorrArgs()
    a.B, a.N, a.T, a.reduction, a.eps, a.w_stride = B, N, T, L.CORR_SUM if reduction == "sum" else L.CORR_MEAN, eps, w_stride
    a.pred, a.target, a.w, a.dpred = pd.data_ptr(), td.data_ptr(), wd.data_ptr(), dd.data_ptr()
    a.stat, a.count = sd.data_ptr(), sd.data_ptr() + 8 * 8 * N
    a.share, a.gscale, a.loss_acc = share_d.data_ptr(), g_d.data_ptr(), acc.data_ptr()
    nws = L.lib.dwn_corr_ws_bytes(C.byref(a))
    assert nws == 8 * math.ceil(N / 256)
    wf, wsd = guarded(nws // 8, torch.float64)
    a.ws, a.ws_bytes = wsd.data_ptr(), nws
    L.check(L.lib.dwn_corr_moments(C.byref(a), 0, stream()), "dwn_corr_moments")
    L.check(L.lib.dwn_corr_loss_finalize(C.byref(a), 0, stream()), "dwn_corr_loss_finalize")
    L.check(L.lib.dwn_f64_to_f32(acc.data_ptr(), out32.data_ptr(), 1, 0, stream()), "dwn_f64_to_f32")
    L.check(L.lib.dwn_corr_loss_backward(C.byref(a), 0, stream()), "dwn_corr_loss_backward")
    torch.cuda.synchronize()
    assert guards_ok(pf, n_el, misalign) and guards_ok(tf, n_el, misalign) and guards_ok(df, n_el, misalign), "guard band (p, t, dpred)"
    assert guards_ok(sf, 8 * N + 1) and guards_ok(wf, nws // 8), "guard band (stat, workspace)"
    stat = sd.cpu().numpy()
    return dict(stat=stat[:8 * N].reshape(8, N), count=float(stat[8 * N]), acc=float(acc.cpu()[0]), loss=out32.cpu().numpy()[0],
                dpred=dd.cpu().numpy().reshape(p.shape))


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else np.float64(a[k]).view(np.uint64),
                              np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else np.float64(b[k]).view(np.uint64))
               for k in a)


def check_case(p, t, w, degenerate, reduction, share, label, misalign=0, w_stride=1):
    got = launch(p, t, w, share, reduction, misalign=misalign, w_stride=w_stride)
    again = launch(p, t, w, share, reduction, misalign=misalign, w_stride=w_stride)
    assert same_bits(got, again), f"{label}: two launches differ"
    B, N = p.shape[:2]
    T = p.shape[2] if p.ndim == 3 else 1
    mom = cr.moments(p, t, w)
    n = mom["n"]
    assert got["count"] == n == int((w != 0).sum()) * T
    co = cr.coefficients(mom)
    st = got["stat"]
    assert np.isfinite(st).all() and np.isfinite(got["dpred"]).all() and np.isfinite(got["loss"])
    if n == 0:
        assert not st.any() and got["acc"] == 0.0 and got["loss"] == 0.0 and not got["dpred"].any()
        print(f"{label}: no counted row -> stat, loss, dpred exactly 0")
        return
    P, Tt = cr.select_rows(p, t, w)
    bound = 64 * n * U64
    scales = [np.abs(P).mean(0), np.abs(Tt).mean(0), mom["M2p"], mom["M2t"], np.sqrt(mom["M2p"] * mom["M2t"])]
    worst = 0.0
    for row, (key, scale) in enumerate(zip(("mean_p", "mean_t", "M2p", "M2t", "C"), scales)):
        err = np.abs(st[row] - mom[key])
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(scale > 0, err / scale, 0.0))))
        assert (err <= bound * scale).all(), f"{label}: {key} off by {np.max(err - bound * scale):.3e} beyond the bound"
    r_err = float(np.max(np.abs(st[5] - co["r"])))
    assert r_err <= 4 * bound + 2.0 ** -50, f"{label}: r off by {r_err:.3e}"
    for row, key in ((6, "c1"), (7, "c2")):
        assert (np.abs(st[row] - co[key]) <= (8 * bound + 2.0 ** -48) * np.abs(co[key])).all(), f"{label}: {key}"
    for j in degenerate.get("const_t", []):
        assert st[3][j] == 0.0 and st[4][j] == 0.0 and st[5][j] == 0.0 and not got["dpred"][:, j].any(), f"{label}: constant target {j}"
    for j in degenerate.get("const_p", []):
        assert st[2][j] == 0.0 and st[5][j] == 0.0 and st[7][j] == 0.0, f"{label}: constant prediction {j}"
    if n == 1:
        assert not st[2:6].any() and not got["dpred"].any(), f"{label}: n = 1"
    want_loss = cr.loss_term(p, t, w, share, cr.EPS, reduction)
    want32 = np.float32(want_loss)
    loss_ulps = abs(float(got["loss"]) - float(want32)) / float(cr.ulp32(want_loss))
    d_want, mag = cr.grad_term(p, t, w, share, G, cr.EPS, reduction)
    rho = 1.0 if reduction == "sum" else 1.0 / N
    factor = abs(G * share * rho)
    assert factor <= 1.0
    d_err = np.abs(got["dpred"].astype(np.float64) - d_want.astype(np.float32).astype(np.float64))
    d_bound = cr.ulp32(d_want) + factor * 1e-9 * (mag[None, :, None] if p.ndim == 3 else mag[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        d_ulps = float(np.nanmax(np.where(d_want != 0, d_err / cr.ulp32(d_want), 0.0)))
    print(f"{label}: n={n} moments {worst / U64:.1f} u64 (bound {64 * n}), r err {r_err:.2e}, loss {float(got['loss']):.7g} "
          f"({loss_ulps:.2f} ulp), dpred worst {d_ulps:.2f} ulp")
    assert loss_ulps <= 1.0, f"{label}: loss {got['loss']!r} vs {want32!r}"
    assert (d_err <= d_bound).all(), f"{label}: dpred off by up to {np.max(d_err - d_bound):.3e} beyond the bound"
    assert not got["dpred"][w == 0].any(), f"{label}: rows of weight 0 must get exactly 0"


@pytest.mark.parametrize("T", (1, 3, 16, 31, 32))
@pytest.mark.parametrize("N", (1, 7, 65, 257))
@pytest.mark.parametrize("B", (1, 2, 5))
def test_kernels_against_the_checker(B, N, T):
    """All four kinds of weights per shape; the reduction and the stride of the weight column alternate with the shape."""
    for k, kind in enumerate(WEIGHT_KINDS):
        seed = 1000 * B + 10 * N + T + 7 * k
        p, t, w, deg = make_case(B, N, T, kind, seed)
        reduction = "sum" if (B + N + T + k) % 2 else "mean"
        share = 0.625 if reduction == "mean" else float(np.float32(0.625 / N))   # an fp32 value; |g share rho| <= 1 with the sum too
        check_case(p, t, w, deg, reduction, share, f"B{B} N{N} T{T} {kind} {reduction}", w_stride=1 + (N + k) % 3)


@pytest.mark.parametrize("name,B,N,T,kind,misalign", [
    ("two_dim", 5, 65, None, "subset", 0),            # (B, N) tensors: T = 1
    ("misaligned", 2, 65, 16, "all", 1),              # T % 4 == 0 off the 16-byte grid: the scalar instantiation
    ("misaligned3", 5, 7, 32, "subset", 3),
    ("rounds_vec", 2, 33, 128, "all", 0),             # a row of the tile is longer than 256 units: two rounds per sweep
    ("rounds_scalar", 3, 40, 100, "subset", 0),       # seven rounds, a unit range of a neuron straddling two of them
    ("wide_vec", 3, 1000, 64, "subset", 0),           # many workgroups, lanes-per-row 256
    ("long_stream", 9, 4099, 31, "subset", 0),        # the backward's grid-stride loop wraps (more than 4096 chunks), ragged last tile
])
def test_other_paths(name, B, N, T, kind, misalign):
    p, t, w, deg = make_case(B, N, T or 1, kind, 4242 + N)
    if T is None:
        p, t = p[:, :, 0].copy(), t[:, :, 0].copy()
    check_case(p, t, w, deg, "mean", 0.5, name, misalign=misalign, w_stride=2)


@pytest.mark.parametrize("T", (16, 31))
def test_centred_moments_at_a_large_offset(T):
    """Predictions 1e6 + k/16: tests/test_correlation_loss_cpu.py shows that float64 raw sums (sum p^2 - n mp^2) miss this bound by
    orders of magnitude (1e-3 relative) while centred float64 sums in any order meet it."""
    p, t = cr.centred_case(T=T)
    w = np.array([1, 0, 1, 1, 1], np.float32)
    p[1], t[1] = np.nan, np.nan
    got = launch(p, t, w, 1.0, "mean")
    k = (p[w != 0].astype(np.float64) - 1.0e6).transpose(0, 2, 1).reshape(-1, p.shape[1])
    m2_true = ((k - k.mean(0)) ** 2).sum(0)
    m2_err = float(np.max(np.abs(got["stat"][2] - m2_true) / m2_true))
    r_want = cr.pearson(p, t, w)
    r_err = float(np.max(np.abs(got["stat"][5] - r_want)) / np.max(np.abs(r_want)))
    raw_err = float(np.max(np.abs(cr.moments(p, t, w, raw=True)["M2p"] - m2_true) / m2_true))
    print(f"centred T={T}: M2p rel err {m2_err:.2e}, r rel err {r_err:.2e} (bound {cr.CENTRED_BOUND:.0e}; float64 raw sums: {raw_err:.2e})")
    assert raw_err > 1e3 * cr.CENTRED_BOUND
    assert m2_err <= cr.CENTRED_BOUND and r_err <= cr.CENTRED_BOUND
    assert np.max(np.abs(got["stat"][0] - (1.0e6 + k.mean(0)))) <= 1e-9


def test_skipped_rows_are_never_read():
    """The same counted rows with NaN, with Inf and with ordinary numbers in the rows of weight 0: identical bits everywhere."""
    p, t, w, _ = make_case(5, 65, 16, "subset", 99)
    outs = []
    for fillv in (np.nan, np.inf, 3.0):
        q, s = p.copy(), t.copy()
        q[w == 0], s[w == 0] = fillv, fillv
        outs.append(launch(q, s, w, 0.5, "mean"))
    assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2])
    assert np.isfinite(outs[0]["loss"]) and np.isfinite(outs[0]["dpred"]).all() and not outs[0]["dpred"][w == 0].any()
    # a NaN weight counts its row (NaN != 0, as in CorrelationMetric); the magnitudes of the others do not enter
    w2 = w.copy()
    w2[w != 0] = 17.0
    assert same_bits(outs[0], launch(p, t, w2, 0.5, "mean"))


def test_loss_accumulates_over_mice():
    """Two finalize calls into one caller-zeroed double add up in call order, as dwn_poisson_loss_forward does."""
    import sensorium_amd._lib as L
    pa, ta, wa, _ = make_case(5, 65, 16, "subset", 5)
    pb, tb, wb, _ = make_case(5, 7, 3, "all", 6)
    one = launch(pa, ta, wa, 0.25, "mean")["acc"] + launch(pb, tb, wb, 0.75, "mean")["acc"]
    acc = torch.zeros(1, dtype=torch.float64, device=dev())
    keep = []
    for p, t, w, share in ((pa, ta, wa, 0.25), (pb, tb, wb, 0.75)):
        B, N, T = p.shape
        pd, td, wd = (torch.from_numpy(v).to(dev()) for v in (p, t, w))
        stat = torch.empty(8 * N + 1, dtype=torch.float64, device=dev())
        sh = torch.tensor([share], dtype=torch.float32, device=dev())
        ws = torch.empty(math.ceil(N / 256), dtype=torch.float64, device=dev())
        a = L.CorrArgs()
        a.B, a.N, a.T, a.reduction, a.eps, a.w_stride = B, N, T, L.CORR_MEAN, cr.EPS, 1
        a.pred, a.target, a.w, a.stat, a.count = pd.data_ptr(), td.data_ptr(), wd.data_ptr(), stat.data_ptr(), stat.data_ptr() + 64 * N
        a.share, a.loss_acc, a.ws, a.ws_bytes = sh.data_ptr(), acc.data_ptr(), ws.data_ptr(), ws.numel() * 8
        L.check(L.lib.dwn_corr_moments(C.byref(a), 0, stream()), "dwn_corr_moments")
        L.check(L.lib.dwn_corr_loss_finalize(C.byref(a), 0, stream()), "dwn_corr_loss_finalize")
        keep.append((pd, td, wd, stat, sh, ws))
    torch.cuda.synchronize()
    assert float(acc.cpu()[0]) == one


DIGEST_CASES = ((5, 257, 32, "subset"), (5, 65, 31, "all"), (2, 7, 3, "one"), (3, 1000, 64, "subset"), (5, 65, 16, "none"))


def corr_digest():
    """sha256 over every output of a fixed set of cases: the product and the -DDWN_DETERMINISTIC build must print the same."""
    h = hashlib.sha256()
    n = 0
    for B, N, T, kind in DIGEST_CASES:
        p, t, w, _ = make_case(B, N, T, kind, 31337 + N)
        got = launch(p, t, w, 0.5, "mean")
        for k in ("stat", "dpred"):
            h.update(np.ascontiguousarray(got[k]).tobytes())
            n += 1
        h.update(np.float64(got["count"]).tobytes() + np.float64(got["acc"]).tobytes() + np.float32(got["loss"]).tobytes())
        n += 3
    return n, h.hexdigest()


def test_two_runs_give_one_digest():
    assert corr_digest() == corr_digest()

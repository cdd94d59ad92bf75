"""The retinotopic-readout-gain kernels through the C-ABI (include/dwn.h dwn_spatial_gain_forward / _backward) against
the float64 checker tests/spatial_reference.py (itself held to float64 grid_sample and autograd on the CPU:
tests/test_spatial_reference_cpu.py).

Every general case prints, per output, the worst ratio of |kernel - float64| to the checker's rounding floor (derived from operation
counts in the checker's docstring) and asserts it at TWICE the floor: the factor 2 covers the ulp error of the device's exp, which
the floor does not model.  The observed worst ratios are in DESIGN.md 12p.

The element pass tiles 128 neurons x min(T, 32) frames, two samples per batch group; the bucketing walks the neurons 256 at a
time; the dG pass takes 32 frames per wave and stages 64 bucket entries at a time, with 16-byte loads where T % 4 == 0 / K % 4 == 0.
The 100 general cases cover (Hf, Wf) in {(1,1), (1,4), (2,2), (3,5), (8,8)} x K in {1, 8, 24, 32, 64} completely and walk
N in {1, 127, 129, 300}, T in {1, 7, 33, 65}, B in {1, 3} and the two map dtypes across them; T = 33 and 65 cross the frame tiles,
N = 127 / 129 / 300 the neuron tile and the bucketing's round, B = 3 the batch group, and N = 300 on a map of few cells the 64-entry
batches of the dG pass; the tile-edge cases add T = 16 / 32 / 64 (the 16-byte staging; once with Hf Wf N odd, where the
buckets end on an odd multiple of 8 bytes), 31, 17 and 129.
Every output buffer and the workspace sit between guard bands that must come back untouched."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import spatial_reference as sr  # noqa: E402
from tests.gpu_helpers import dev  # noqa: E402

GUARD, SENTINEL = 64, -7777.0
OUTPUTS = ("dy", "dg", "dpos", "dweight", "dbias")
BOUND = 2.0               # times the floor; above it a ratio is a finding to explain, never a tolerance
MAPS = ((1, 1), (1, 4), (2, 2), (3, 5), (8, 8))
KS = (1, 8, 24, 32, 64)
NS, TS, BS = (1, 127, 129, 300), (1, 7, 33, 65), (1, 3)


def guarded(shape, dtype=torch.float32, fill=SENTINEL):
    n = math.prod(shape)
    flat = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=dev())
    view = flat[GUARD:GUARD + n].view(shape)
    if fill != SENTINEL:
        view.fill_(fill)
    return flat, view


def guards_ok(flat, n):
    return bool((flat[:GUARD] == SENTINEL).all()) and bool((flat[GUARD + n:] == SENTINEL).all())


def make_inputs(B, N, T, Hf, Wf, K, seed, bf16=False, scale=0.7):
    gen = torch.Generator().manual_seed(seed)
    y = torch.empty(B, N, T).exponential_(1.0, generator=gen) + 0.01
    g = torch.randn(B, T, Hf, Wf, K, generator=gen)
    if bf16:
        g = g.bfloat16()
    pos = torch.from_numpy(sr.draw_positions(np.random.default_rng(seed), N, Hf, Wf))
    weight = torch.randn(N, K, generator=gen) * (scale / math.sqrt(K))
    bias = torch.randn(N, generator=gen) * 0.3
    dout = torch.randn(B, N, T, generator=gen)
    return y, g, pos, weight, bias, dout


def _args(L, y, g, pos, weight, bias, m):
    a = L.SpatialGainArgs()
    a.B, a.N, a.T = y.shape
    a.Hf, a.Wf, a.K = g.shape[2:]
    a.g_dtype = L.DWN_BF16 if g.dtype == torch.bfloat16 else L.DWN_F32
    a.max_log_gain = m
    a.y, a.g, a.pos, a.weight, a.bias = y.data_ptr(), g.data_ptr(), pos.data_ptr(), weight.data_ptr(), bias.data_ptr()
    return a


def gpu_forward(y, g, pos, weight, bias, m):
    import sensorium_amd._lib as L
    yd, gd, pd, wd, bd = (t.to(dev()).contiguous() for t in (y, g, pos, weight, bias))
    flat, out = guarded(tuple(y.shape))
    a = _args(L, yd, gd, pd, wd, bd, m)
    a.out = out.data_ptr()
    L.check(L.lib.dwn_spatial_gain_forward(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_spatial_gain_forward")
    torch.cuda.synchronize()
    assert guards_ok(flat, y.numel()), "dwn_spatial_gain_forward wrote outside out"
    return out.cpu()


def gpu_backward(y, g, pos, weight, bias, m, dout, want=OUTPUTS, dg_fill=SENTINEL):
    import sensorium_amd._lib as L
    yd, gd, pd, wd, bd, dd = (t.to(dev()).contiguous() for t in (y, g, pos, weight, bias, dout))
    shapes = dict(dy=y.shape, dg=g.shape, dpos=pos.shape, dweight=weight.shape, dbias=bias.shape)
    bufs = {k: guarded(tuple(shapes[k]), fill=dg_fill if k == "dg" else SENTINEL) for k in OUTPUTS if k in want}
    a = _args(L, yd, gd, pd, wd, bd, m)
    a.dout = dd.data_ptr()
    for k, (_, view) in bufs.items():
        setattr(a, k, view.data_ptr())
    need = L.lib.dwn_spatial_gain_ws_bytes(C.byref(a))
    assert need > 0 and need % 16 == 0
    wflat, ws = guarded((need // 8,), torch.float64)
    assert ws.data_ptr() % 16 == 0
    a.ws, a.ws_bytes = ws.data_ptr(), need
    L.check(L.lib.dwn_spatial_gain_backward(C.byref(a), 0, torch.cuda.current_stream().cuda_stream), "dwn_spatial_gain_backward")
    torch.cuda.synchronize()
    assert guards_ok(wflat, need // 8), "dwn_spatial_gain_backward wrote outside the workspace"
    for k, (flat, view) in bufs.items():
        assert guards_ok(flat, view.numel()), f"dwn_spatial_gain_backward wrote outside {k}"
    return {k: view.cpu() for k, (_, view) in bufs.items()}


def checker(y, g, pos, weight, bias, m, dout):
    return sr.reference(y.numpy(), g.float().numpy(), pos.numpy(), weight.numpy(), bias.numpy(), m, dout.numpy())


def ratios(ref, out, grads):
    """Worst |kernel - float64| / floor per output; a floor of 0 (an exactly zero value) demands an exact 0."""
    res = {}
    for name, got in [("out", out)] + list(grads.items()):
        err = np.abs(got.double().numpy() - ref[name])
        fl = ref["floor"][name]
        assert np.all(err[fl == 0] == 0), name
        res[name] = float(np.max(err[fl > 0] / fl[fl > 0])) if np.any(fl > 0) else 0.0
    return res


def check_case(B, N, T, Hf, Wf, K, bf16, m=1.0, seed=0):
    y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed + 7 * B + 13 * N + 17 * T + 19 * K + 23 * Hf + 29 * Wf, bf16)
    out = gpu_forward(y, g, pos, weight, bias, m)
    grads = gpu_backward(y, g, pos, weight, bias, m, dout)
    r = ratios(checker(y, g, pos, weight, bias, m, dout), out, grads)
    print(f"spatial_gain B={B} N={N} T={T} map={Hf}x{Wf} K={K} {'bf16' if bf16 else 'fp32'} m={m}: error / floor " +
          " ".join(f"{k}={v:.3f}" for k, v in r.items()))
    return r


def assert_ratios(worst):
    print("worst error / floor: " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        assert v <= BOUND, (k, v, BOUND)


def merge(worst, r):
    for k, v in r.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ------------------------------------------------------------------------------------------------------------ 1. general cases
def general_cases(i_map, i_k):
    """Four cases of one (map, K) pair: a Latin walk over N, T, B and the dtype, shifted by the pair's index."""
    i = i_map * len(KS) + i_k
    return [(BS[(i + j) % 2], NS[(i + j) % 4], TS[(i // 4 + i + 2 * j + j // 2) % 4], bool((i + j // 2 + j) % 2)) for j in range(4)]


def general_cases_cover_every_value():
    seen = [set(), set(), set(), set()]
    pairs = set()
    for i_map in range(len(MAPS)):
        for i_k in range(len(KS)):
            cases = general_cases(i_map, i_k)
            assert len(set(cases)) == 4
            for c in cases:
                for s, v in zip(seen, c):
                    s.add(v)
                pairs.add((c[1], c[2]))
    assert seen == [set(BS), set(NS), set(TS), {False, True}] and len(pairs) == 16


@pytest.mark.parametrize("i_k", range(len(KS)), ids=[f"K{k}" for k in KS])
@pytest.mark.parametrize("i_map", range(len(MAPS)), ids=[f"{h}x{w}" for h, w in MAPS])
def test_general(i_map, i_k):
    general_cases_cover_every_value()
    worst = {}
    for B, N, T, bf16 in general_cases(i_map, i_k):
        merge(worst, check_case(B, N, T, *MAPS[i_map], KS[i_k], bf16))
    assert_ratios(worst)


@pytest.mark.parametrize("B,N,T,Hf,Wf,K,bf16,m", [(2, 128, 32, 8, 8, 16, True, 1.0), (5, 130, 31, 3, 5, 8, False, 2.0),
                                                   (1, 257, 64, 2, 2, 32, True, 0.5), (4, 3, 17, 8, 8, 64, False, 1.0),
                                                   (1, 300, 16, 1, 1, 8, True, 1.0), (3, 200, 129, 1, 4, 3, False, 1.0),
                                                   (2, 129, 32, 3, 5, 8, True, 1.0)])      # Hf Wf N odd with T % 4 == 0: s stays 16-byte aligned
def test_tile_edges(B, N, T, Hf, Wf, K, bf16, m):
    assert_ratios(check_case(B, N, T, Hf, Wf, K, bf16, m=m, seed=1))


# ------------------------------------------------------------------------------------------------------------ 2. bit for bit
def test_zero_heads_are_the_identity():
    for B, N, T, Hf, Wf, K, bf16 in ((3, 200, 5, 3, 5, 8, False), (2, 129, 33, 8, 8, 32, True), (1, 1, 1, 1, 1, 1, False)):
        y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed=5, bf16=bf16)
        y[0, 0, 0] = -0.0
        weight.zero_(); bias.zero_()
        out = gpu_forward(y, g, pos, weight, bias, 1.0)
        got = gpu_backward(y, g, pos, weight, bias, 1.0, dout)
        assert torch.equal(out.view(torch.int32), y.view(torch.int32))
        assert torch.equal(got["dy"].view(torch.int32), dout.view(torch.int32))
        assert not bool(got["dpos"].any()) and not bool(got["dg"].any())


@pytest.mark.parametrize("B,N,T,bf16", [(3, 200, 33, False), (5, 130, 7, True)])
def test_integer_and_dyadic_sums_are_exact(B, N, T, bf16):
    """weight = bias = 0: a = 0, gain = sech^2 = 1 and s = m dout y = dout y, small integers.  On the 3 x 5 map the cell centres and
    the fractions 0, 1/4, 1/2 are exact in fp32 (x = (j + f) / 2 - 1, y = j + f - 1), so the bilinear weights are multiples of 1/16
    and samp, for small-integer G, a multiple of 1/16 below 2^4: every product and every sum is exact, in fp32 and in float64."""
    gen = torch.Generator().manual_seed(11)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    Hf, Wf, K = 3, 5, 8
    y, dout = ri(0, 7, B, N, T), ri(-3, 3, B, N, T)
    g = ri(-4, 4, B, T, Hf, Wf, K)
    if bf16:
        g = g.bfloat16()
    fx, fy = ri(0, 2, N) / 4, ri(0, 2, N) / 4
    jx, jy = ri(0, Wf - 2, N), ri(0, Hf - 2, N)
    pos = torch.stack([(jx + fx) / 2 - 1, (jy + fy) - 1], dim=1)
    weight, bias = torch.zeros(N, K), torch.zeros(N)
    out = gpu_forward(y, g, pos, weight, bias, 1.0)
    got = gpu_backward(y, g, pos, weight, bias, 1.0, dout)
    assert torch.equal(out, y) and torch.equal(got["dy"], dout)
    assert not bool(got["dpos"].any()) and not bool(got["dg"].any())
    ref = checker(y, g, pos, weight, bias, 1.0, dout)
    ce = ref["cells"]
    assert np.array_equal(ce["fx"], fx.numpy()) and np.array_equal(ce["fy"], fy.numpy())
    want_w, want_b = ref["dweight"], ref["dbias"]
    assert np.array_equal(want_w * 16, np.round(want_w * 16)) and np.abs(want_w).max() < 2 ** 20 and np.abs(want_w).max() > 0
    assert np.array_equal(got["dweight"].double().numpy(), want_w) and np.array_equal(got["dbias"].double().numpy(), want_b)


# ------------------------------------------------------------------------------------------------------------ 3. position extremes
def test_position_extremes():
    """3 x 5 map (cell centres exact in fp32).  Neurons at cell centres, on +-1, at +-1.5 and at +-1e30 on either axis: a clamped
    coordinate's gradient is exactly 0 (the checker's floor is 0 there, which demands it) and everything else is within the floor."""
    B, T, Hf, Wf, K = 2, 7, 3, 5, 8
    xs = [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, -1.5, 1e30, -1e30, 0.3]
    ys = [-1.0, 0.0, 1.0, 1.5, -1.5, 1e30, -1e30, -0.4]
    grid = [(x, yv) for x in xs for yv in ys]
    N = len(grid)
    y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed=3)
    pos = torch.tensor(grid, dtype=torch.float32)
    out = gpu_forward(y, g, pos, weight, bias, 1.0)
    got = gpu_backward(y, g, pos, weight, bias, 1.0, dout)
    ref = checker(y, g, pos, weight, bias, 1.0, dout)
    assert_ratios(ratios(ref, out, got))
    outside_x = pos[:, 0].abs() > 1
    outside_y = pos[:, 1].abs() > 1
    assert bool(outside_x.any()) and bool(outside_y.any())
    assert bool((got["dpos"][outside_x, 0] == 0).all()) and bool((got["dpos"][outside_y, 1] == 0).all())
    assert bool((got["dpos"][~outside_x, 0] != 0).all()) and bool((got["dpos"][~outside_y, 1] != 0).all())
    assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(v).all()) for v in got.values())


# ------------------------------------------------------------------------------------------------------------ 4. occupancy extremes
def test_all_neurons_in_one_cell():
    B, N, T, Hf, Wf, K = 2, 300, 7, 8, 8, 8
    y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed=8, bf16=True)
    rng = np.random.default_rng(8)
    frac = rng.uniform(0.05, 0.95, size=(N, 2))
    pos = torch.from_numpy((((np.array([3.0, 5.0]) + frac) / 7.0) * 2.0 - 1.0).astype(np.float32))
    out = gpu_forward(y, g, pos, weight, bias, 1.0)
    got = gpu_backward(y, g, pos, weight, bias, 1.0, dout, dg_fill=float("nan"))
    assert_ratios(ratios(checker(y, g, pos, weight, bias, 1.0, dout), out, got))
    touched = torch.zeros(Hf, Wf, dtype=torch.bool)
    touched[5:7, 3:5] = True
    assert bool((got["dg"][:, :, ~touched] == 0).all()) and bool((got["dg"][:, :, touched] != 0).all())


def test_empty_cells_come_back_as_exact_zeros():
    """Neurons spread over the left half of a 3 x 5 map only; dg is pre-filled with NaN: the kernel writes every cell."""
    B, N, T, Hf, Wf, K = 3, 40, 5, 3, 5, 24
    y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed=12)
    pos[:, 0] = pos[:, 0].abs() * -0.4 - 0.55                                # px in (0.1, 0.9): cells 0 and 1 of 5
    out = gpu_forward(y, g, pos, weight, bias, 1.0)
    got = gpu_backward(y, g, pos, weight, bias, 1.0, dout, dg_fill=float("nan"))
    assert_ratios(ratios(checker(y, g, pos, weight, bias, 1.0, dout), out, got))
    assert bool((got["dg"][:, :, :, 2:] == 0).all()) and bool(got["dg"][:, :, :, :2].any())


# ------------------------------------------------------------------------------------------------------------ 5. a non-finite position
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_nonfinite_position_poisons_exactly_its_neuron(bad):
    B, N, T, Hf, Wf, K = 3, 131, 5, 3, 5, 8
    y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed=6)
    j = 77
    keep = torch.arange(N) != j
    without = [t[:, keep] if t.dim() == 3 else t[keep] for t in (y, pos, weight, bias, dout)]
    clean_out = gpu_forward(without[0], g, *without[1:4], 1.0)
    clean = gpu_backward(without[0], g, *without[1:4], 1.0, without[4])
    pb = pos.clone()
    pb[j, 1] = bad
    out = gpu_forward(y, g, pb, weight, bias, 1.0)
    got = gpu_backward(y, g, pb, weight, bias, 1.0, dout)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert bool(torch.isnan(out[:, j]).all()) and bool(torch.isnan(got["dy"][:, j]).all())
    assert torch.equal(bits(out[:, keep]), bits(clean_out)) and torch.equal(bits(got["dy"][:, keep]), bits(clean["dy"]))
    for k in ("dpos", "dweight", "dbias"):
        assert bool(torch.isnan(got[k][j]).all()), k
        assert torch.equal(bits(got[k][keep]), bits(clean[k])), k
    assert bool(torch.isfinite(got["dg"]).all()) and torch.equal(bits(got["dg"]), bits(clean["dg"]))


# ------------------------------------------------------------------------------------------------------------ 6. null outputs
def test_null_outputs_leave_the_others_unchanged():
    y, g, pos, weight, bias, dout = make_inputs(5, 130, 33, 3, 5, 8, seed=4, bf16=True)
    full = gpu_backward(y, g, pos, weight, bias, 1.0, dout)
    for want in (("dy", "dpos", "dweight", "dbias"), ("dy", "dg"), ("dy",), ("dg",), ("dpos",), ("dweight", "dbias")):
        got = gpu_backward(y, g, pos, weight, bias, 1.0, dout, want=want)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k].view(torch.int32), full[k].view(torch.int32)), (want, k)


# ------------------------------------------------------------------------------------------------------------ 7. repeats
DIGEST_CASES = ((3, 300, 33, 8, 8, 32, True), (2, 129, 65, 3, 5, 24, False), (1, 127, 7, 1, 4, 1, False))


def spatial_digest():
    """sha256 over out, dy, dg, dpos, dweight, dbias of DIGEST_CASES, each launched twice: (digest, tensors, differing)."""
    sha, tensors, differing = hashlib.sha256(), 0, 0
    for B, N, T, Hf, Wf, K, bf16 in DIGEST_CASES:
        y, g, pos, weight, bias, dout = make_inputs(B, N, T, Hf, Wf, K, seed=9, bf16=bf16)
        runs = []
        for _ in range(2):
            got = gpu_backward(y, g, pos, weight, bias, 1.0, dout)
            runs.append([gpu_forward(y, g, pos, weight, bias, 1.0)] + [got[k] for k in OUTPUTS])
        for p, q in zip(*runs):
            tensors += 1
            differing += int(not torch.equal(p.view(torch.int32), q.view(torch.int32)))
            sha.update(p.numpy().tobytes())
    return sha.hexdigest(), tensors, differing


def test_two_launches_give_equal_bits():
    digest, tensors, differing = spatial_digest()
    print(f"spatial_gain digest {digest} tensors={tensors} differing={differing}")
    assert tensors == 6 * len(DIGEST_CASES) and differing == 0

"""The guarded optimizer step on the device: dwn_grad_sumsq_multi, dwn_step_guard_finalize and
dwn_adamw_ema_multi_guarded through the C-ABI on arenas with guard bands and odd float offsets (the sharded optimizer's layout,
as tests/test_gpu_tail.py), then FusedAdamWEma(max_grad_norm=..., skip_nonfinite=...) and MouseModel.train_step.

References are float64 torch on the CPU: oracle.adamw_step / ema_update for the state, sqrt(((grad_scale * g.double()) ** 2).sum())
for the norm.  Bounds: the state (p, exp_avg, exp_avg_sq, ema) is held to gpu_helpers.ADAMW_BOUND = 1e-6 (float32 storage alone
costs 3.4e-7); the norm to 1e-9 relative (squares are exact in double, so the error of the sum is at most n * 2^-53 = 1.1e-10
at the 1 000 003 elements used here; two summation orders on the CPU differ by 2e-14); counts, the skip flag and everything a
skipped step must leave alone are exact."""
import ctypes as C
import io
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import dwiseneuro_oracle as orc  # noqa: E402
from tests import gpu_helpers as H  # noqa: E402
from tests import guarded_helpers as G  # noqa: E402
from tests.gpu_helpers import dev, rel, stream  # noqa: E402

GUARD = 64
SENT = 12345.678            # guard-band sentinel
NORM_BOUND = 1e-9
_GENTRY = np.dtype([("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("ema", "<u8"),
                    ("numel", "<i8"), ("is_int64", "<i4"), ("pad", "<i4"), ("step", "<u8")])
SIZES = [1, 3, 255, 256, 257, 4097, 16 * 256 + 1, 1_000_003]
LR, DECAY, GSCALE = G.LR, G.DECAY, G.GSCALE


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    return lib


def _layout(sizes):
    """Slices of one arena: a 64-float guard band on either side of each, and every other slice starting at an odd float offset
    (never 16-byte aligned), as tests/test_gpu_tail.py lays its optimizer tensors out."""
    pos, spans = 0, []
    for i, n in enumerate(sizes):
        pos += GUARD
        if i % 2 == 0 and pos % 2 == 0:
            pos += 1
        spans.append((pos, n))
        pos += n
    return spans, pos + GUARD


def _arena_host(spans, total, tensors):
    a = torch.full((total,), SENT)
    for (s, n), t in zip(spans, tensors):
        a[s:s + n] = t
    return a


def _outside_untouched(arena, spans):
    m = torch.ones(arena.numel(), dtype=torch.bool)
    for s, n in spans:
        m[s:s + n] = False
    return bool((arena.cpu()[m] == torch.tensor(SENT)).all())


def _sizes(ntensors):
    if ntensors == 1:
        return [1_000_003]
    if ntensors == 2:
        return [257, 1_000_003]
    return [SIZES[i % 7] for i in range(ntensors - 1)] + [1_000_003]


_ref_norm = G.ref_norm


class Rig:
    """Arenas for p / exp_avg / exp_avg_sq / ema / grad, one int64 step counter per entry, the device table of dwn_guarded_entry,
    the guard, the two [sumsq, nonfinite] pairs and the partials workspace."""

    def __init__(self, L, sizes, state=None, has_ema=None, steps=None, max_blocks=16):
        self.L, self.sizes, self.max_blocks = L, list(sizes), max_blocks
        n = len(sizes)
        self.has_ema = [True] * n if has_ema is None else list(has_ema)
        self.spans, self.total = _layout(sizes)
        zeros = [torch.zeros(k) for k in sizes]
        state = state or {}
        self.host0 = {k: _arena_host(self.spans, self.total, state.get(k, zeros)) for k in ("p", "m", "v", "ema")}
        self.ar = {k: v.to(dev()) for k, v in self.host0.items()}
        self.grad = torch.full((self.total,), SENT, device=dev())
        self.steps = torch.tensor([0] * n if steps is None else list(steps), dtype=torch.int64, device=dev())
        ent = np.zeros(n, dtype=_GENTRY)
        for i, (s, k) in enumerate(self.spans):
            ent[i] = (self.ar["p"].data_ptr() + 4 * s, self.grad.data_ptr() + 4 * s, self.ar["m"].data_ptr() + 4 * s,
                      self.ar["v"].data_ptr() + 4 * s, self.ar["ema"].data_ptr() + 4 * s if self.has_ema[i] else 0, k, 0, 0,
                      self.steps.data_ptr() + 8 * i)
        self.table = torch.from_numpy(np.frombuffer(ent.tobytes(), dtype=np.uint8).copy()).to(dev())
        self.guard = torch.zeros(C.sizeof(L.StepGuard), dtype=torch.uint8, device=dev())
        self.pairs = torch.zeros(4, dtype=torch.float64, device=dev())
        self.ws_bytes = int(L.lib.dwn_grad_guard_workspace_bytes(n, max_blocks))
        assert self.ws_bytes == max_blocks * 16
        # the workspace sits in front of a guard band of its own: a partial written past the end shows
        self.ws = torch.full((self.ws_bytes // 8 + GUARD,), SENT, dtype=torch.float64, device=dev())

    def set_grads(self, grads):
        self.grad_host = _arena_host(self.spans, self.total, grads)
        self.grad.copy_(self.grad_host)

    def head_of(self, i):
        """floats of entry i in front of the first 16-byte boundary, and floats behind the last whole float4"""
        s, n = self.spans[i]
        addr = self.grad.data_ptr() + 4 * s
        head = min(((16 - addr % 16) % 16) // 4, n)
        return head, (n - head) % 4

    def sumsq(self, gscale=GSCALE, pair=0, ntensors=None, first=0):
        n = len(self.sizes) - first if ntensors is None else ntensors
        self.L.check(self.L.lib.dwn_grad_sumsq_multi(self.table.data_ptr() + 64 * first, n, self.max_blocks, gscale, self.ws.data_ptr(),
                                                     self.ws_bytes, self.pairs.data_ptr() + 16 * pair, 0, stream()),
                     "dwn_grad_sumsq_multi")

    def finalize(self, max_norm=0.0, skip_nonfinite=1, second_pair=False):
        self.L.check(self.L.lib.dwn_step_guard_finalize(self.pairs.data_ptr(), self.pairs.data_ptr() + 16 if second_pair else None,
                                                        max_norm, skip_nonfinite, self.table.data_ptr(), len(self.sizes),
                                                        self.guard.data_ptr(), 0, stream()), "dwn_step_guard_finalize")

    def adamw(self, wd=0.05, gscale=GSCALE, lr=LR):
        rc = self.L.lib.dwn_adamw_ema_multi_guarded(self.table.data_ptr(), len(self.sizes), self.max_blocks, lr, 0.9, 0.999, 1e-8, wd,
                                                    DECAY, gscale, self.guard.data_ptr(), 0, stream())
        self.L.check(rc, "dwn_adamw_ema_multi_guarded")
        return rc

    def step(self, grads, max_norm=0.0, skip_nonfinite=1, wd=0.05):
        self.set_grads(grads)
        self.sumsq()
        self.finalize(max_norm, skip_nonfinite)
        self.adamw(wd)
        return self.read_guard()

    def read_guard(self):
        return self.L.StepGuard.from_buffer_copy(self.guard.cpu().numpy().tobytes())

    def slices(self, k):
        host = (self.ar[k] if k != "grad" else self.grad).cpu()
        return [host[s:s + n] for s, n in self.spans]

    def bands_ok(self):
        return all(_outside_untouched(self.ar[k], self.spans) for k in self.ar) and _outside_untouched(self.grad, self.spans) \
            and bool((self.ws[self.ws_bytes // 8:].cpu() == SENT).all())


def _rand_grads(sizes, seed, scale=0.02):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in sizes]


# ------------------------------------------------------------------------------------------------ sum of squares
_BIG = {}


def _big_case(ntensors):
    """gradients and their float64 norm, computed once per table size and shared by the max_blocks cases"""
    if ntensors not in _BIG:
        sizes = _sizes(ntensors)
        grads = _rand_grads(sizes, 11 + ntensors)
        _BIG[ntensors] = (sizes, grads, _ref_norm(grads)[0])
    return _BIG[ntensors]


@pytest.mark.parametrize("max_blocks", [1, 16, 64])
@pytest.mark.parametrize("ntensors", [1, 2, 37])
def test_sumsq_norm_reproducible_and_reads_only(L, ntensors, max_blocks):
    sizes, grads, want = _big_case(ntensors)
    rig = Rig(L, sizes, max_blocks=max_blocks)
    rig.set_grads(grads)
    rig.sumsq()
    first_pair, first_ws = rig.pairs[:2].clone(), rig.ws.clone()
    rig.ws[:rig.ws_bytes // 8].fill_(-1.0)               # the second launch must not depend on what the workspace held
    rig.sumsq()
    rig.finalize(max_norm=0.0)
    torch.cuda.synchronize()
    pair = rig.pairs[:2].cpu()
    got = math.sqrt(float(pair[0]))
    err = abs(got - want) / want
    print(f"GUARDFIG sumsq n{ntensors} blocks{max_blocks} norm {got:.12e} rel {err:.3e}")
    assert err < NORM_BOUND and float(pair[1]) == 0.0
    assert torch.equal(rig.pairs[:2].view(torch.int64), first_pair.view(torch.int64)), "two launches gave different bits"
    assert torch.equal(rig.ws.view(torch.int64), first_ws.view(torch.int64)), "the partials differ between two launches"
    g = rig.read_guard()
    assert abs(g.norm - want) / want < NORM_BOUND and g.coef == 1.0 and g.skip == 0 and g.nonfinite == 0
    assert (g.good_steps, g.skipped_steps) == (1, 0)
    assert torch.equal(rig.grad.cpu(), rig.grad_host), "the gradients were written"
    assert rig.bands_ok()
    assert torch.equal(rig.steps.cpu(), torch.ones(ntensors, dtype=torch.int64)), "a taken step advances every counter by one"


def test_sumsq_subtable_and_second_pair(L):
    """The sharded layout: entries [0, k) into the first pair, entries [k, n) into the second, the finaliser adds them; an empty
    sub-table gives a zero pair."""
    sizes = [SIZES[i % 7] for i in range(9)]
    grads = _rand_grads(sizes, 5)
    rig = Rig(L, sizes)
    rig.set_grads(grads)
    rig.sumsq(pair=0, ntensors=4)
    rig.sumsq(pair=1, first=4)
    rig.finalize(second_pair=True)
    torch.cuda.synchronize()
    pairs = rig.pairs.cpu()
    wa, wb, wall = _ref_norm(grads[:4])[0], _ref_norm(grads[4:])[0], _ref_norm(grads)[0]
    assert abs(math.sqrt(float(pairs[0])) - wa) / wa < NORM_BOUND and abs(math.sqrt(float(pairs[2])) - wb) / wb < NORM_BOUND
    assert abs(rig.read_guard().norm - wall) / wall < NORM_BOUND
    rig.sumsq(pair=1, ntensors=0)
    torch.cuda.synchronize()
    assert rig.pairs[2:].cpu().tolist() == [0.0, 0.0] and rig.bands_ok()


# ------------------------------------------------------------------------------------------------ range
def test_all_zero_gradients(L):
    sizes = [1, 257, 4097]
    rig = Rig(L, sizes)
    g = rig.step([torch.zeros(n) for n in sizes], max_norm=1.0)
    assert g.norm == 0.0 and g.coef == 1.0 and g.skip == 0 and g.nonfinite == 0
    for k in ("p", "m", "v", "ema"):
        assert all(bool(torch.isfinite(t).all()) for t in rig.slices(k)), k


def test_huge_gradients_give_a_finite_norm_and_a_step_that_clips(L):
    """1000 elements of 3e25: the float32 square overflows, the float64 one does not; the clipped step is AdamW on coef * g."""
    sizes = [1000, 257]
    case = H.adamw_case(3, sizes, 1)
    grads = [torch.full((1000,), 3e25), torch.zeros(257)]
    want, _ = _ref_norm(grads)
    rig = Rig(L, sizes, state={k: [c[k] for c in case] for k in ("p", "m", "v", "ema")})
    g = rig.step(grads, max_norm=1.0)
    assert math.isfinite(g.norm) and abs(g.norm - want) / want < NORM_BOUND and g.nonfinite == 0 and g.skip == 0
    coef = min(1.0, 1.0 / (want + 1e-6))
    assert g.coef == pytest.approx(coef, rel=2e-7) and g.coef < 1e-20
    for i, c in enumerate(case):
        p, m, v = orc.adamw_step(c["p"].double(), grads[i].double() * GSCALE * coef, c["m"].double(), c["v"].double(), 1, LR,
                                 weight_decay=0.05)
        for k, ref in (("p", p), ("m", m), ("v", v), ("ema", orc.ema_update(c["ema"].double(), p, DECAY))):
            assert rel(rig.slices(k)[i], ref) < H.ADAMW_BOUND, (k, i)
    assert rig.bands_ok()


def test_denormal_only_gradients(L):
    sizes = [257, 3]
    grads = [torch.full((n,), 1e-40) for n in sizes]
    assert all(float(g[0]) != 0.0 for g in grads)
    want, _ = _ref_norm(grads)
    rig = Rig(L, sizes)
    rig.set_grads(grads)
    rig.sumsq()
    rig.finalize(max_norm=1.0)
    g = rig.read_guard()
    assert want > 0 and abs(g.norm - want) / want < NORM_BOUND and g.coef == 1.0 and g.skip == 0 and g.nonfinite == 0


# ------------------------------------------------------------------------------------------------ non-finite detection
NF_SIZES = [1, 4097, 257, 1002, 3]
_NF = {}


def _nf_grads():
    if not _NF:
        _NF["g"] = _rand_grads(NF_SIZES, 23)
    return _NF["g"]


@pytest.mark.parametrize("value", [float("inf"), float("-inf"), float("nan")], ids=["pinf", "ninf", "nan"])
@pytest.mark.parametrize("where", ["first", "last", "head", "tail", "single", "last_entry"])
def test_one_nonfinite_element_is_counted_and_skips(L, where, value):
    rig = Rig(L, NF_SIZES, max_blocks=16)
    head, tail = rig.head_of(1)
    assert head >= 1 and tail >= 1, "the layout must give entry 1 an unaligned head and a scalar tail"
    n1 = NF_SIZES[1]
    entry, idx = {"first": (1, 0), "last": (1, n1 - 1), "head": (1, head - 1), "tail": (1, n1 - tail), "single": (0, 0),
                  "last_entry": (len(NF_SIZES) - 1, 1)}[where]
    grads = [g.clone() for g in _nf_grads()]
    grads[entry][idx] = value
    want, bad = _ref_norm(grads)
    assert bad == 1
    rig.set_grads(grads)
    rig.sumsq()
    rig.finalize(max_norm=0.0, skip_nonfinite=1)
    g = rig.read_guard()
    assert g.nonfinite == 1 and g.skip == 1 and (g.good_steps, g.skipped_steps) == (0, 1)
    assert abs(g.norm - want) / want < NORM_BOUND, "the non-finite element is left out of the sum, nothing else is"
    assert int(rig.steps.sum()) == 0, "a skipped step advances no counter"


def test_nonfinite_without_skip_is_torchs_behaviour(L):
    """skip_nonfinite off: the NaN reaches the parameters as it does under torch.optim.AdamW — data, not a fault."""
    rig = Rig(L, NF_SIZES)
    grads = [g.clone() for g in _nf_grads()]
    grads[2][5] = float("nan")
    grads[3][7] = float("inf")
    rig.set_grads(grads)
    rig.sumsq()
    rig.finalize(max_norm=1.0, skip_nonfinite=0)
    assert rig.adamw() == 0
    torch.cuda.synchronize()
    g = rig.read_guard()
    assert g.nonfinite == 2 and g.skip == 0 and (g.good_steps, g.skipped_steps) == (1, 0)


# ------------------------------------------------------------------------------------------------ skipped step
def test_skipped_step_leaves_everything_but_the_ema(L):
    sizes = [1, 3, 257, 4097, 255, 1002]
    has_ema = [i % 3 != 2 for i in range(len(sizes))]
    case = H.adamw_case(31, sizes, 1000)
    steps0 = [999 + i for i in range(len(sizes))]
    rig = Rig(L, sizes, state={k: [c[k] for c in case] for k in ("p", "m", "v", "ema")}, has_ema=has_ema, steps=steps0)
    grads = [c["grads"][0].clone() for c in case]
    grads[3][100] = float("nan")
    g = rig.step(grads, max_norm=1.0, skip_nonfinite=1)
    assert g.skip == 1 and g.nonfinite == 1 and (g.good_steps, g.skipped_steps) == (0, 1)
    for k in ("p", "m", "v"):
        assert torch.equal(rig.ar[k].cpu(), rig.host0[k]), f"{k} was written by a skipped step"
    assert torch.equal(rig.steps.cpu(), torch.tensor(steps0)), "a step counter advanced"
    for i, c in enumerate(case):
        got = rig.slices("ema")[i]
        if not has_ema[i]:
            assert torch.equal(got, c["ema"]), "an entry without EMA had its slice of the EMA arena written"
        else:
            assert rel(got, orc.ema_update(c["ema"].double(), c["p"].double(), DECAY)) < H.ADAMW_BOUND
            assert sizes[i] < 3 or not torch.equal(got, c["ema"]), "the EMA leg must still run"
    assert rig.bands_ok()
    g = rig.step([c["grads"][1] for c in case], max_norm=0.0)
    assert g.skip == 0 and (g.good_steps, g.skipped_steps) == (1, 1)
    assert torch.equal(rig.steps.cpu(), torch.tensor(steps0) + 1)


# ------------------------------------------------------------------------------------------------ trajectory
@pytest.mark.parametrize("clip", [False, True], ids=["skip_only", "clip"])
@pytest.mark.parametrize("step0", G.TRAJ_STEP0)
def test_ten_step_trajectory_with_two_skipped_steps(L, step0, clip):
    """Ten calls, steps 3 and 7 carrying a NaN: float64 AdamW over the eight good gradients with counts step0 .. step0 + 7 and ten
    EMA lerps (tests/guarded_helpers.py; tensors of more than three elements norm-relative, the 1- and 3-element ones per element
    against the magnitude of the update's operands).  clip: max_norm per step puts norm / max_norm at 3 on even steps and at 0.5 on odd ones —
    both far from 1, so the rounding of the comparison cannot flip the branch — and on odd steps coef is exactly 1."""
    sizes = G.TRAJ_SIZES
    case = G.traj_case(step0)
    has_ema = [i != 2 for i in range(len(sizes))]
    rig = Rig(L, sizes, state={k: [c[k] for c in case] for k in ("p", "m", "v", "ema")}, has_ema=has_ema,
              steps=[step0 - 1] * len(sizes), max_blocks=16)
    ref, scale = G.traj_reference(case, step0, clip, has_ema, with_scale=True)
    for s in range(10):
        grads, norm, bad, max_norm, coef = G.traj_step(case, s, clip)
        g = rig.step(grads, max_norm=max_norm, skip_nonfinite=1, wd=G.WD)
        assert g.nonfinite == bad and g.skip == int(s in G.BAD_STEPS)
        assert abs(g.norm - norm) / norm < NORM_BOUND
        if not clip or s % 2 == 1:
            assert g.coef == 1.0
        else:
            assert g.coef == pytest.approx(coef, rel=2e-7)
    torch.cuda.synchronize()
    g = rig.read_guard()
    assert (g.good_steps, g.skipped_steps) == (8, 2)
    assert torch.equal(rig.steps.cpu(), torch.full((len(sizes),), step0 + 7, dtype=torch.int64))
    worst = {}
    for k in ("p", "m", "v", "ema"):
        for i, r in enumerate(ref):
            if k == "ema" and not has_ema[i]:
                assert torch.equal(rig.slices(k)[i], case[i]["ema"])
                continue
            e = G.traj_error(rig.slices(k)[i], r[k], scale[i][k])
            worst[k] = max(worst.get(k, 0.0), e)
            assert e < H.ADAMW_BOUND, f"{k} of tensor {i}: {e:.3e}"
    assert rig.bands_ok()
    print(f"GUARDFIG trajectory step{step0} clip{int(clip)} " + " ".join(f"{k} {v:.3e}" for k, v in worst.items()))


def test_mixed_step_counts_in_one_launch(L):
    sizes = [4097, 257]
    case = H.adamw_case(53, sizes, 1000)
    rig = Rig(L, sizes, state={k: [c[k] for c in case] for k in ("p", "m", "v", "ema")}, steps=[4, 4999])
    grads = [c["grads"][0] for c in case]
    g = rig.step(grads, max_norm=0.0, wd=0.05)
    assert g.skip == 0 and rig.steps.cpu().tolist() == [5, 5000]
    for i, (c, t) in enumerate(zip(case, (5, 5000))):
        p, m, v = orc.adamw_step(c["p"].double(), grads[i].double() * GSCALE, c["m"].double(), c["v"].double(), t, LR, weight_decay=0.05)
        for k, want in (("p", p), ("m", m), ("v", v), ("ema", orc.ema_update(c["ema"].double(), p, DECAY))):
            assert rel(rig.slices(k)[i], want) < H.ADAMW_BOUND, (k, t)
        # the other entry's count gives another parameter: the two references are told apart at this bound
        other = orc.adamw_step(c["p"].double(), grads[i].double() * GSCALE, c["m"].double(), c["v"].double(), 5005 - t, LR,
                               weight_decay=0.05)[0]
        assert rel(other, p) > 10 * H.ADAMW_BOUND


# ------------------------------------------------------------------------------------------------ Python level
NEW_ENTRIES = ("dwn_grad_sumsq_multi", "dwn_step_guard_finalize", "dwn_adamw_ema_multi_guarded", "dwn_grad_guard_workspace_bytes")
OPT_SIZES = [257, 4097, 3, 1]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(n, generator=g) * 0.1).to(dev())) for n in OPT_SIZES]


def _opt_grads(nsteps, seed=1, nan_at=()):
    out = []
    for s in range(nsteps):
        gs = _rand_grads(OPT_SIZES, seed * 100 + s)
        if s in nan_at:
            gs[1][17] = float("nan")
        out.append(gs)
    return out


def _run(opt, params, grads):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g.to(dev())
        opt.step()


def _state_equal(pa, oa, pb, ob):
    for a, b in zip(pa, pb):
        if not torch.equal(a.detach(), b.detach()):
            return False
        sa, sb = oa.state[a], ob.state[b]
        if int(sa["step"]) != int(sb["step"]) or not torch.equal(sa["exp_avg"], sb["exp_avg"]) \
                or not torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]):
            return False
    return True


def test_default_optimizer_takes_the_old_path(L, monkeypatch):
    from sensorium_amd.optim import FusedAdamWEma
    calls = {"old": 0}
    old = L.lib.dwn_adamw_ema_multi

    def counted(*a):
        calls["old"] += 1
        return old(*a)

    def forbidden(*a):
        raise AssertionError("a default-constructed FusedAdamWEma called an entry of the guarded step")

    monkeypatch.setattr(L.lib, "dwn_adamw_ema_multi", counted)
    for name in NEW_ENTRIES:
        monkeypatch.setattr(L.lib, name, forbidden)
    params = _params()
    opt = FusedAdamWEma(params, lr=LR)
    _run(opt, params, _opt_grads(2))
    torch.cuda.synchronize()
    assert calls["old"] == 2 and opt.guard_stats() is None
    assert all(type(opt.state[p]["step"]) is int and opt.state[p]["step"] == 2 for p in params)


def test_guarded_table_cache_is_keyed_by_the_live_parameters(L):
    """Alternating sets of parameters with a gradient (forward(x, index) with different mice) each keep their own device table:
    coming back to a set uploads nothing, and a parameter left out keeps its step count."""
    from sensorium_amd.optim import FusedAdamWEma
    params = _params(5)
    opt = FusedAdamWEma(params, lr=LR, skip_nonfinite=True)
    grads = [g.to(dev()) for g in _rand_grads(OPT_SIZES, 77)]

    def step(live):
        for i, p in enumerate(params):
            p.grad = grads[i] if i in live else None
        opt.step()

    step({0, 1, 2, 3})
    full = opt._tables[("guarded", None)]._dev
    step({0, 2})
    part = opt._tables[("guarded", (id(params[0]), id(params[2])))]._dev
    step({0, 1, 2, 3})
    step({0, 2})
    assert opt._tables[("guarded", None)]._dev is full and opt._tables[("guarded", (id(params[0]), id(params[2])))]._dev is part
    assert len(opt._tables) == 2
    assert [int(opt.state[p]["step"]) for p in params] == [4, 2, 4, 2] and opt.guard_stats()["good_steps"] == 4


@pytest.mark.parametrize("first,second", [(True, True), (True, False), (False, True)], ids=["guarded", "to_unguarded", "to_guarded"])
def test_state_dict_round_trip_continues_bit_for_bit(L, first, second):
    """Three steps (the second carries a NaN), state_dict -> a fresh optimizer of the second mode -> three more steps, against the
    same six steps without the round trip (the mode changed in place on the one optimizer): every parameter, moment and count equal
    bit for bit.  The elementwise kernels and the fixed-order norm are deterministic, so equality is the bound."""
    from sensorium_amd.optim import FusedAdamWEma
    kw = lambda on: dict(max_grad_norm=0.05, skip_nonfinite=True) if on else {}       # noqa: E731
    grads = _opt_grads(6, nan_at=(1,) if first else ())
    pa = _params()
    oa = FusedAdamWEma(pa, lr=LR, **kw(first))
    _run(oa, pa, grads[:3])
    if first:
        st = oa.guard_stats()
        assert st["skipped_steps"] == 1 and st["good_steps"] == 2 and st["coef"] < 1.0
        assert all(torch.is_tensor(oa.state[p]["step"]) and oa.state[p]["step"].dtype == torch.int64 and oa.state[p]["step"].is_cuda
                   and oa.state[p]["step"].dim() == 0 for p in pa)
    buf = io.BytesIO()
    torch.save(oa.state_dict(), buf)             # through a file image, as a checkpoint goes (load_state_dict keeps the tensors it is given)
    sd = torch.load(io.BytesIO(buf.getvalue()), weights_only=False)
    assert all(type(s["step"]) is int and s["step"] == (2 if first else 3) for s in sd["state"].values())
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    ob = FusedAdamWEma(pb, lr=LR, **kw(second))
    ob.load_state_dict(sd)
    assert all(torch.is_tensor(ob.state[p]["step"]) == second for p in pb)
    assert _state_equal(pa, oa, pb, ob)
    oa.max_grad_norm, oa.skip_nonfinite = (0.05, True) if second else (None, False)
    _run(oa, pa, grads[3:])
    _run(ob, pb, grads[3:])
    torch.cuda.synchronize()
    assert _state_equal(pa, oa, pb, ob)
    assert int(oa.state[pa[0]]["step"]) == (5 if first else 6)


def test_guarded_step_in_a_captured_graph(L):
    """What the device-side design exists for: one guarded step captured in a graph (one stream: a linear graph), replayed with a
    NaN gradient — skipped — and then with a clean one — taken, with the right step count."""
    from sensorium_amd.optim import FusedAdamWEma
    params = _params(3)
    p0 = [p.detach().cpu().double() for p in params]
    emas = [p.detach().clone() + 0.001 for p in params]
    e0 = [e.cpu().double() for e in emas]
    opt = FusedAdamWEma(params, lr=LR, weight_decay=0.05, ema_params=emas, ema_decay=DECAY, max_grad_norm=1e9, skip_nonfinite=True)
    g_warm, g_bad, g_good = _opt_grads(3, seed=9, nan_at=(1,))
    static = [torch.zeros_like(p) for p in params]
    for p, s in zip(params, static):
        p.grad = s

    def load(gs):
        for s, g in zip(static, gs):
            s.copy_(g.to(dev()))

    load(g_warm)
    opt.step()                                   # uploads the pointer table and allocates the guard's buffers before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    torch.cuda.synchronize()
    # (the capture records, it does not run)
    assert opt.guard_stats()["good_steps"] == 1
    after_warm = [p.detach().clone() for p in params]
    load(g_bad)
    graph.replay()
    st = opt.guard_stats()
    assert st["skipped"] and st["nonfinite"] == 1 and st["skipped_steps"] == 1 and st["good_steps"] == 1
    assert all(torch.equal(p.detach(), a) for p, a in zip(params, after_warm))
    assert all(int(opt.state[p]["step"]) == 1 for p in params)
    load(g_good)
    graph.replay()
    st = opt.guard_stats()
    assert not st["skipped"] and st["coef"] == 1.0 and st["good_steps"] == 2 and st["skipped_steps"] == 1
    for i, p in enumerate(params):
        rp, rm, rv = orc.adamw_step(p0[i], g_warm[i].double(), torch.zeros_like(p0[i]), torch.zeros_like(p0[i]), 1, LR, weight_decay=0.05)
        e = orc.ema_update(orc.ema_update(e0[i], rp, DECAY), rp, DECAY)              # the warm-up's lerp, then the skipped step's
        rp, rm, rv = orc.adamw_step(rp, g_good[i].double(), rm, rv, 2, LR, weight_decay=0.05)
        e = orc.ema_update(e, rp, DECAY)
        assert rel(p, rp) < H.ADAMW_BOUND and rel(opt.state[p]["exp_avg"], rm) < H.ADAMW_BOUND
        assert rel(opt.state[p]["exp_avg_sq"], rv) < H.ADAMW_BOUND and rel(emas[i], e) < H.ADAMW_BOUND
        assert int(opt.state[p]["step"]) == 2


TWIN_MAX_NORM = 1e-2        # far below the tiny model's gradient norm: every step of the test clips


def _tiny_model(golden_dir):
    from sensorium_amd.argus_models import MouseModel
    from tests.test_gpu_step import TINY_KW, golden_sd
    z, sd = golden_sd(golden_dir, "tiny_model_train.npz")
    okw = {"lr": LR, "weight_decay": 0.05, "max_grad_norm": TWIN_MAX_NORM, "skip_nonfinite": True}
    model = MouseModel({"nn_module": ("dwiseneuro", dict(TINY_KW)), "loss": ("mice_poisson", {}), "optimizer": ("AdamW", okw),
                        "device": "cuda:0", "amp": False, "iter_size": 1})
    model.nn_module.load_state_dict(sd, strict=True)
    model.set_ema(0.9)
    batch = [torch.from_numpy(z["x"]), [[torch.from_numpy(z[f"target_{m}"]) for m in range(2)], torch.from_numpy(z["mice_weights"])]]
    return model, batch


def test_train_step_with_an_inf_activation_is_skipped(golden_dir):
    """MouseModel.train_step with the guard from the optimizer spec: clean step, a step whose cortex output holds one Inf (forward
    hook), clean step.  The middle step leaves every parameter, moment and count bit-identical, moves the EMA and is reported.
    The untouched twin is an optimizer of its own over copies of the parameters and of the EMA that is handed the model's very
    gradients on the two clean steps and never sees the bad one — so no run-to-run noise of a second backward pass stands between
    the two, and after the third step EVERY parameter, first and second moment equals the twin's within gpu_helpers.ADAMW_BOUND, the
    step counts are equal, and the model's EMA is the twin's trajectory plus the one extra lerp of the skipped step (float64)."""
    from sensorium_amd.optim import FusedAdamWEma
    model, batch = _tiny_model(golden_dir)
    net, opt = model.nn_module, model.get_optimizer()
    assert opt.guarded and opt.max_grad_norm == TWIN_MAX_NORM and opt.skip_nonfinite
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    params = [p for p in net.parameters() if p.requires_grad]
    ema_by_name = dict(model.model_ema.ema.named_parameters())
    emas = [ema_by_name[n] for n in names]
    assert opt.folds_ema_of(model.model_ema)
    tparams = [torch.nn.Parameter(p.detach().clone()) for p in params]
    temas = [e.detach().clone() for e in emas]
    twin = FusedAdamWEma(tparams, lr=LR, weight_decay=0.05, ema_params=temas, ema_decay=0.9, max_grad_norm=TWIN_MAX_NORM,
                         skip_nonfinite=True)
    model_step, feed = opt.step, {"twin": True}

    def step_both():
        if feed["twin"]:
            for q, p in zip(tparams, params):
                q.grad = p.grad.detach().clone()
            twin.step()
        return model_step()

    opt.step = step_both                        # train_step calls self.optimizer.step()

    def same_as_twin(what):
        worst = 0.0
        for n, p, q in zip(names, params, tparams):
            assert int(opt.state[p]["step"]) == int(twin.state[q]["step"]), (what, n)
            for k, a, b in (("p", p, q), ("exp_avg", opt.state[p]["exp_avg"], twin.state[q]["exp_avg"]),
                            ("exp_avg_sq", opt.state[p]["exp_avg_sq"], twin.state[q]["exp_avg_sq"])):
                e = rel(a, b)
                worst = max(worst, e)
                assert e < H.ADAMW_BOUND, f"{what}: {k} of {n}: {e:.3e}"
        return worst

    model.train_step(batch)
    st1, tw1 = opt.guard_stats(), twin.guard_stats()
    assert not st1["skipped"] and st1["coef"] < 0.5 and abs(st1["norm"] - tw1["norm"]) <= NORM_BOUND * tw1["norm"]
    same_as_twin("first step")
    for e, t, n in zip(emas, temas, names):
        assert rel(e, t) < H.ADAMW_BOUND, n
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in params]
    ema_before = [e.detach().clone() for e in emas]

    def poison(module, args, out):
        out = out.clone()
        out.view(-1)[0] = float("inf")
        return out

    handle = net.cortex.register_forward_hook(poison)
    feed["twin"] = False
    model.train_step(batch)
    handle.remove()
    feed["twin"] = True
    st = opt.guard_stats()
    assert st["skipped"] and st["nonfinite"] > 0 and (st["good_steps"], st["skipped_steps"]) == (1, 1)
    moved = 0
    for n, p, e, (p0, m0, v0), e0 in zip(names, params, emas, before, ema_before):
        assert torch.equal(p.detach(), p0) and torch.equal(opt.state[p]["exp_avg"], m0) and torch.equal(opt.state[p]["exp_avg_sq"], v0), n
        assert int(opt.state[p]["step"]) == 1, n
        assert rel(e, orc.ema_update(e0.double().cpu(), p0.double().cpu(), 0.9)) < H.ADAMW_BOUND, n
        moved += int(not torch.equal(e.detach(), e0))
    assert moved > len(names) // 2, "the EMA leg must run on a skipped step"
    model.train_step(batch)
    torch.cuda.synchronize()
    st3, tw3 = opt.guard_stats(), twin.guard_stats()
    assert not st3["skipped"] and (st3["good_steps"], st3["skipped_steps"]) == (2, 1) and (tw3["good_steps"], tw3["skipped_steps"]) == (2, 0)
    assert st3["coef"] < 0.5 and abs(st3["norm"] - tw3["norm"]) <= NORM_BOUND * tw3["norm"]
    assert abs(st3["coef"] - tw3["coef"]) <= 2e-7 * tw3["coef"], "the clip coefficient of the step after a skip is the step's own"
    worst = same_as_twin("the step after the skipped one")
    assert all(int(opt.state[p]["step"]) == 2 for p in params)
    worst_e = 0.0
    for n, e, e0, (p1, _, _), q in zip(names, emas, ema_before, before, tparams):
        want = orc.ema_update(orc.ema_update(e0.double().cpu(), p1.double().cpu(), 0.9), q.detach().double().cpu(), 0.9)
        worst_e = max(worst_e, rel(e, want))
        assert rel(e, want) < H.ADAMW_BOUND, n
    print(f"GUARDFIG twin p/m/v {worst:.3e} ema {worst_e:.3e} norm {st3['norm']:.6e} coef {st3['coef']:.3e}")

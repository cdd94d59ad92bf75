"""The checker of the 3x3 spatial depth-wise kernels (tests/dws3_reference.py) checked itself, on the CPU:

  pinning   its float64 values equal tests/dw_reference.py's (and through test_dw_reference_cpu.py the oracle's) and the oracle's
            directly, on two cases;
  room      a float32 emulation of each path's arithmetic (tile and weights rounded where the path rounds them, taps summed in pairs
            for the dot2 paths and as a chain for the generic ones) puts ZERO elements over the bound on every random case;
  teeth     each mutation a wrong kernel could amount to exceeds the bound on the random case of the matching rule and changes the
            exact case by at least one unit;
  coverage  every built instantiation is reached by a random AND an exact case, per storage type;
  exact     every exact case meets the preconditions under which any summation order gives the same bits.
"""
import pytest
import torch

from oracle import dwiseneuro_oracle as orc
from tests import dw_reference as DR
from tests import dws3_reference as R

CPU = torch.device("cpu")
TOL = 1e-12


def _first(cases, **want):
    for c in cases:
        if all(getattr(c, k) == v for k, v in want.items()):
            return c
    raise AssertionError(want)


# ---- pinning --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [dict(direction="bwd", rule="s2", cin=0, Win=16, rows_band=2),
                                  dict(direction="bwd", rule="s1c", cin=64, Win=8, rows_band=2)], ids=["stored-s2", "rebuilt-s1"])
def test_values_equal_dw_reference_and_oracle(want):
    c = _first(R.RANDOM_CASES, **want)
    o = R.make_operands(c, CPU)
    y1 = DR.conv_pw_f64(o.a0, o.w1) if c.cin else o.y1.double()
    y2, _ = R.forward_reference(o)
    y2_dr = DR.dw_spatial_fwd_f64(y1, o.scale, o.shift, o.w, c.planes, c.Hin, c.Win, c.stride)
    assert DR.rel_l2(y2, y2_dr) < TOL
    g, _ = R.gradient(o)
    b = R.backward_reference(o)
    dh1, dw, s0, s1 = DR.dw_spatial_bwd_f64(y1, o.scale, o.shift, o.mean, o.invstd, g.reshape(-1, c.C), o.w, c.planes, c.Hin, c.Win,
                                            c.stride)
    assert DR.rel_l2(b["dh1"], dh1) < TOL and DR.rel_l2(b["dW"], dw) < TOL
    (r0, r1), _ = R.backward_stats(o, dh1, b["yhat"])
    assert DR.rel_l2(r0, s0) < TOL and DR.rel_l2(r1, s1) < TOL
    # the oracle directly: x [B = 1, T = planes, H, W, C]
    h = (y1.view(1, c.planes, c.Hin, c.Win, c.C) * o.scale.double() + o.shift.double()).requires_grad_(True)
    wo = o.w.double().t().reshape(c.C, 1, 1, 3, 3).clone().requires_grad_(True)
    y2o = orc.dw_spatial(orc.silu(h), wo, c.stride)
    y2o.backward(g.reshape(1, c.planes, o.Hout, o.Wout, c.C))
    assert DR.rel_l2(y2, y2o.detach().reshape(-1, c.C)) < TOL
    assert DR.rel_l2(b["dh1"], h.grad.reshape(-1, c.C)) < TOL and DR.rel_l2(b["dW"], wo.grad.reshape(c.C, 9)) < TOL


# ---- coverage and dispatch --------------------------------------------------------------------------------------------------------------
def test_every_built_instantiation_is_reached_by_a_random_and_an_exact_case():
    built = set(R.BUILT)
    assert len(built) == len(R.BUILT) == 109
    for name, cases in (("random", R.RANDOM_CASES), ("exact", R.EXACT_CASES)):
        reached = {R.case_dispatch(c) + (c.dtype,) for c in cases}
        assert not [r for r in reached if r[0] == "refuse"], name
        assert reached - built == set(), (name, sorted(reached - built, key=str))     # the restated dispatch invents no kernel
        assert built - reached == set(), (name, sorted(built - reached, key=str))
    ids = [R.case_id(c) for c in R.RANDOM_CASES] + ["x-" + R.case_id(c) for c in R.EXACT_CASES]
    assert len(set(ids)) == len(ids)
    for cases in (R.RANDOM_CASES, R.EXACT_CASES):                                     # no case runs twice under two rule names
        assert len({tuple(c[:12]) for c in cases}) == len(cases)


def test_wrap_cases_take_a_second_iteration_of_the_persistent_loop():
    """work > gridDim.x for every occupancy the hardware allows (32 waves and 160 KB of LDS per CU), on every kernel family."""
    wrap = [c for c in R.RANDOM_CASES if c.rule == "wrap"]
    for c in wrap:
        work, gx = R.grid_bound(c)
        print("DWS3-WRAP", R.case_id(c), f"work={work} grid_x<={gx}", flush=True)
        assert work > gx, (c, work, gx)
    fams = {(R.case_dispatch(c)[0], R.case_dispatch(c)[1][0] if R.case_dispatch(c)[0] == "fwd_chain" else None, c.dtype) for c in wrap}
    assert fams >= {("fwd_chain", 1, "bf16"), ("fwd_chain", 2, "bf16"), ("bwd_s1c", None, "bf16"), ("bwd_s2", None, "bf16"),
                    ("fwd_pair", None, "bf16"), ("bwd_pair", None, "bf16"), ("bwd_generic", None, "bf16"),
                    ("fwd_generic", None, "f32"), ("bwd_generic", None, "f32")}
    # resident_grid_x as dwn_launch.h has it
    assert R.resident_grid_x(3, 7, 65) == 65 and R.resident_grid_x(2, 7, 130) == 73 and R.resident_grid_x(2, 14, 37, True) == 32
    assert R.resident_grid_x(1, 512, 9) == 1 and R.resident_grid_x(2, 7, 3, True) == 8


def test_auto_band_cases_take_more_than_one_band_and_the_even_split_moves_it():
    """The auto_bands cases leave rows_band to the library on a plane that needs at least two bands, and the even split gives
    another height than the largest band that fits; the last band is then shorter than the others or equal to them."""
    want = {("fwd", "f32", 1): (10, 9, 3), ("fwd", "f32", 2): (9, 7, 2), ("fwd", "bf16", 1): (10, 9, 3), ("fwd", "bf16", 2): (9, 7, 2),
            ("bwd", "f32", 1): (8, 7, 4), ("bwd", "f32", 2): (16, 13, 2), ("bwd", "bf16", 1): (8, 7, 4), ("bwd", "bf16", 2): (16, 13, 2)}
    paths = set()
    for cases in (R.RANDOM_CASES, R.EXACT_CASES):
        auto = [c for c in cases if c.rule == "auto_bands"]
        assert len(auto) == 8 and {(c.direction, c.dtype, c.stride) for c in auto} == set(want)
        for c in auto:
            assert c.rows_band == 0
            greedy, rb, nb, _ = R.banded_plan(c.direction, c.dtype, c.Hin, c.Win, c.stride)
            rows = c.Hin if c.direction == "bwd" else (c.Hin - 1) // c.stride + 1
            print("DWS3-AUTO", R.case_id(c), f"rows={rows} greedy={greedy} band={rb} bands={nb} last={rows - (nb - 1) * rb}", flush=True)
            assert (greedy, rb, nb) == want[(c.direction, c.dtype, c.stride)]             # worked by hand from the launchers' rule
            assert nb >= 2 and rb != greedy and 0 < rows - (nb - 1) * rb <= rb
            paths.add(R.case_dispatch(c) + (c.dtype,))
    assert paths == {("fwd_generic", ("f32", 3, 1, 512), "f32"), ("fwd_generic", ("f32", 3, 2, 512), "f32"),
                     ("fwd_pair", (1, 512), "bf16"), ("fwd_pair", (2, 512), "bf16"), ("bwd_generic", ("f32", 3, 1), "f32"),
                     ("bwd_generic", ("f32", 3, 2), "f32"), ("bwd_pair", (), "bf16"), ("bwd_generic", ("bf16", 3, 2), "bf16")}


def test_dispatch_restates_the_launchers():
    d = R.dws3_dispatch
    # library chunk heights (launch_fc_rb, launch_s1c_rb) and the rounding of rows_band to a built height
    assert d("fwd", "bf16", 4, 18, 32, 448, 1) == ("fwd_chain", (1, 16, 4, 0))
    assert d("fwd", "bf16", 4, 9, 16, 448, 1) == ("fwd_chain", (1, 8, 6, 0))
    assert d("fwd", "bf16", 4, 36, 64, 448, 2) == ("fwd_chain", (2, 16, 2, 0))
    assert d("fwd", "bf16", 4, 9, 16, 448, 2) == ("fwd_chain", (2, 4, 1, 0))
    assert d("fwd", "bf16", 4, 18, 32, 448, 1, rows_band=7) == ("fwd_chain", (1, 16, 8, 0))
    assert d("fwd", "bf16", 4, 18, 32, 448, 1, rows_band=5, cin=64) == ("fwd_chain", (1, 16, 8, 64))
    assert d("fwd", "bf16", 4, 36, 64, 448, 2, cin=128) == ("fwd_chain", (2, 16, 2, 128))
    assert d("bwd", "bf16", 4, 18, 32, 448, 1) == ("bwd_s1c", (16, 4, 0))
    assert d("bwd", "bf16", 4, 9, 16, 448, 1, rows_band=3, cin=64) == ("bwd_s1c", (8, 4, 64))
    assert d("bwd", "bf16", 4, 36, 64, 448, 2) == ("bwd_s2", (16, 0))
    # the even rounding of the stride-2 backward band, and its clip to the plane
    assert R.s2_band(9, 4, 0, 3) == 4 and R.s2_band(9, 4, 0, 2) == 2 and R.s2_band(3, 4, 0, 8) == 4 and R.s2_band(36, 16, 0, 0) % 2 == 0
    # what the walk refuses goes to the pair / generic kernels; 512-thread workgroups from Hin * Win = 512
    assert d("fwd", "bf16", 3, 16, 32, 72, 1, impl=1) == ("fwd_pair", (1, 512))
    assert d("fwd", "bf16", 3, 9, 16, 72, 2, impl=1) == ("fwd_pair", (2, 256))
    assert d("fwd", "f32", 3, 16, 32, 72, 1) == ("fwd_generic", ("f32", 3, 1, 512))
    assert d("fwd", "bf16", 3, 16, 33, 72, 3) == ("fwd_generic", ("bf16", 3, 0, 256))
    assert d("bwd", "bf16", 3, 7, 11, 72, 1) == ("bwd_pair", ())
    assert d("bwd", "bf16", 3, 7, 22, 72, 2) == ("bwd_generic", ("bf16", 3, 2))
    assert d("bwd", "f32", 3, 10, 13, 72, 3) == ("bwd_generic", ("f32", 3, 0))
    # refusals
    assert d("fwd", "f32", 1, 4, 4, 12, 1) == ("refuse", -2) and d("bwd", "bf16", 1, 4, 4, 12, 1) == ("refuse", -2)
    assert d("fwd", "f32", 1, 1, 2048, 8, 1) == ("refuse", -5) and d("bwd", "bf16", 1, 1, 2048, 8, 1, impl=1) == ("refuse", -5)
    assert d("fwd", "bf16", 2, 9, 16, 72, 1, cin=64) == ("refuse", -3) and d("bwd", "bf16", 2, 9, 11, 64, 1, cin=64) == ("refuse", -3)
    assert d("bwd", "f32", 2, 9, 16, 64, 1, cin=64) == ("refuse", -3)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=R.case_id)
def test_exact_case_preconditions(case):
    o = R.make_operands(case, CPU, "exact")
    ref = R.exact_reference(o)                       # asserts the preconditions
    # the general float64 reference agrees with the integer one to float64 rounding (SiLU(h >= 17) is not h in float64)
    if case.direction == "fwd":
        assert float((R.forward_reference(o)[0] - ref["y2"]).abs().max()) < 1e-4
    else:
        b = R.backward_reference(o)
        assert float((b["dh1"] - ref["dh1"]).abs().max()) < 1e-4 and float((b["dW"] - ref["dW"]).abs().max()) < 1e-2
    # taps: every tap position is non-zero in some channel (a permutation of taps shows somewhere)
    assert bool((o.w != 0).any(1).all())


# ---- room -------------------------------------------------------------------------------------------------------------------------------
ROOM = {}


@pytest.mark.parametrize("case", R.RANDOM_CASES, ids=R.case_id)
def test_room_float32_emulation_stays_within_the_bound(case):
    o = R.make_operands(case, CPU)
    path = R.case_dispatch(case)[0]
    if case.direction == "fwd":
        ref, bound = R.forward_reference(o)
        got = R.emulate_forward(o)
        assert not torch.isnan(got.float()).any()
        figs = {"y2": R.max_ratio(got, ref, bound)}
        (s, q), (bs, bq) = R.forward_stats(o, got)
        figs["sum"] = R.max_ratio(got.float().sum(0), s, bs)
        figs["sumsq"] = R.max_ratio((got.float() ** 2).sum(0), q, bq)
    else:
        b = R.backward_reference(o)
        dh1, dW = R.emulate_backward(o)
        figs = {"dh1": R.max_ratio(dh1, b["dh1"], b["dh1_bound"]), "dW": R.max_ratio(dW, b["dW"], b["dW_bound"])}
        (s, q), (bs, bq) = R.backward_stats(o, dh1, b["yhat"])
        yhat32 = (R._y1_f32(o) * o.invstd + (-o.mean * o.invstd))
        figs["sum"] = R.max_ratio(dh1.float().sum(0), s, bs)
        figs["sum_yhat"] = R.max_ratio((dh1.float() * yhat32).sum(0), q, bq)
    for k, (ratio, over) in figs.items():
        key = (path, case.dtype, k)
        ROOM[key] = max(ROOM.get(key, 0.0), ratio)
    print("DWS3-ROOM", R.case_id(case), " ".join(f"{k}={r:.3f}" for k, (r, _) in figs.items()), flush=True)
    assert all(over == 0 for _, over in figs.values()), figs


def test_room_summary():
    """Largest ratio per path, storage type and output over the cases above (pytest -s shows the table of DESIGN.md 12s)."""
    for key in sorted(ROOM):
        print("DWS3-ROOM-MAX", *key, f"{ROOM[key]:.3f}", flush=True)
    assert all(v <= 1.0 for v in ROOM.values())


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------
# mutation -> the rule whose cases it belongs to (and the directions it is spelled out for)
TEETH = [
    ("drop_tap", dict(rule="chain", stride=1, Win=16, rows_band=4)),
    ("drop_tap", dict(rule="s1c", cin=0, Win=16, rows_band=4)),
    ("drop_tap", dict(rule="stride3", dtype="f32", direction="fwd")),
    ("drop_tap", dict(rule="stride3", dtype="f32", direction="bwd")),
    ("halo_neighbour", dict(rule="chain", stride=1, Win=32, rows_band=2)),
    ("halo_neighbour", dict(rule="chain", stride=2, Win=16, rows_band=1)),
    ("seam_row", dict(rule="chain", stride=1, Win=8, rows_band=6)),
    ("seam_row", dict(rule="chain", stride=2, Win=32, rows_band=3)),
    ("seam_row", dict(rule="chain_rc", stride=1, Win=16, rows_band=8, cin=128)),
    ("seam_row", dict(rule="s1c", cin=64, Win=32, rows_band=2)),
    ("phase", dict(rule="chain", stride=2, Win=64, rows_band=2)),
    ("phase", dict(rule="refused_width", stride=2, Win=13, dtype="f32", direction="fwd")),
    ("last_plane", dict(rule="chain", stride=1, Win=16, rows_band=2)),
    ("last_plane", dict(rule="s2", cin=0, Win=32, rows_band=0)),
    ("swap_planes", dict(rule="chain", stride=2, Win=16, rows_band=4)),
    ("swap_planes", dict(rule="s1c", cin=128, Win=8, rows_band=8)),
    ("chan_tail", dict(rule="chain", stride=1, Win=32, rows_band=8)),
    ("chan_tail", dict(rule="s2", cin=0, Win=64, rows_band=2)),
    ("ld_ignored", dict(rule="ld", dtype="bf16", impl=0, stride=1, direction="fwd")),
    ("ld_ignored", dict(rule="ld", dtype="f32", stride=2, direction="fwd")),
    ("ld_ignored", dict(rule="ld", dtype="bf16", impl=1, stride=2, direction="bwd")),
    ("ld_ignored", dict(rule="chain_rc_ld")),
]


@pytest.mark.parametrize("mut,want", TEETH, ids=[f"{m}-{'-'.join(f'{k}{v}' for k, v in w.items())}" for m, w in TEETH])
def test_teeth_mutations_exceed_the_bound_and_change_the_exact_case(mut, want):
    for kind, cases in (("random", R.RANDOM_CASES), ("exact", R.EXACT_CASES)):
        c = _first(cases, **want)
        o = R.make_operands(c, CPU, kind)
        if c.direction == "fwd":
            ref, bound = R.forward_reference(o)
            bad = R.forward_reference(o, mut)[0]
        else:
            b = R.backward_reference(o)
            ref, bound = b["dh1"], b["dh1_bound"]
            bad = R.backward_reference(o, mut)["dh1"]
        if kind == "random":
            ratio, over = R.max_ratio(bad, ref, bound)
            print("DWS3-TEETH", mut, R.case_id(c), f"max_ratio={ratio:.1f} over={over}", flush=True)
            assert over > 0 and ratio > 2.0, (ratio, over)
        else:
            diff = (bad - ref).abs()
            assert not bool((diff < 0.5).all()), "the exact case does not notice"      # NaN (ld ignored) counts as noticed


def test_teeth_dw_lost_output():
    """One contributing output dropped from dW (a corner, whose taps reach the halo).  The bf16 dW bound is about 2^-7 SW and one
    term among the n contributing outputs is about SW / n: a random case sees a single lost term only while n stays below a few
    hundred, as in the cases here (ratios 4.5 to 23 in bf16); at 18 720 rows per column it does not.  The exact cases, whose dW
    must be bit-equal, see it at any size."""
    for want in (dict(rule="s1c", cin=0, Win=16, rows_band=4), dict(rule="s2", cin=64, Win=32, rows_band=2),
                 dict(rule="stride3", dtype="f32", direction="bwd"), dict(rule="tiny", dtype="bf16", direction="bwd", stride=1, Win=2)):
        c = _first(R.EXACT_CASES, **want)
        o = R.make_operands(c, CPU, "exact")
        diff = (R.backward_reference(o, "lost_output")["dW"] - R.backward_reference(o)["dW"]).abs()
        assert float(diff.max()) >= 1.0, "the exact case does not notice"
        c = _first(R.RANDOM_CASES, **want)
        o = R.make_operands(c, CPU)
        b = R.backward_reference(o)
        ratio, over = R.max_ratio(R.backward_reference(o, "lost_output")["dW"], b["dW"], b["dW_bound"])
        print("DWS3-TEETH lost_output dW", R.case_id(c), f"max_ratio={ratio:.3f} over={over}", flush=True)
        assert over > 0                              # at these sizes (n of a few hundred) the random case sees it too


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_teeth_u_w_is_a_necessary_term(direction):
    """Unrounded weights handed to the bf16 paths.  The float32 emulation of a path that rounds them (tile, taps and store all
    rounded) stays within the bound with u_w = 2^-8 on every such case, and exceeds the bound formed with u_w = 0 on the row-walk
    cases (not on every case: the worst-case sums leave room, 0.96 on the stride-2 pair kernel).  A mutation of the float64
    reference ALONE (taps rounded, nothing else) cannot exceed the u_w = 0 bound: it moves an output by at most 2^-8 S, which
    the bf16 tile's u_tile S already holds; its ratio is recorded."""
    total0 = 0
    for c in [c for c in R.RANDOM_CASES if c.rule == "w_unrounded" and c.direction == direction]:
        o = R.make_operands(c, CPU)
        o0 = R.make_operands(c._replace(wround=True), CPU)
        o0.__dict__.update({k: v for k, v in o.__dict__.items() if k != "case"})        # same operands, bound with u_w = 0
        assert not torch.equal(o.w, o.w.to(torch.bfloat16).float())
        if direction == "fwd":
            emu, bad = R.emulate_forward(o), R.forward_reference(o, "w_rounded")[0]
            (ref, b1), (_, b0) = R.forward_reference(o), R.forward_reference(o0)
        else:
            emu, bad = R.emulate_backward(o)[0], R.backward_reference(o, "w_rounded")["dh1"]
            r1, r0 = R.backward_reference(o), R.backward_reference(o0)
            ref, b1, b0 = r1["dh1"], r1["dh1_bound"], r0["dh1_bound"]
        assert bool((b1 > b0).all())
        (e0, over0), (e1, over1) = R.max_ratio(emu, ref, b0), R.max_ratio(emu, ref, b1)
        ratio0, _ = R.max_ratio(bad, ref, b0)
        print("DWS3-TEETH u_w", R.case_id(c), f"emulation: ratio_u_w_0={e0:.3f} over={over0} ratio_u_w={e1:.3f} over={over1}; "
              f"reference mutation alone: ratio_u_w_0={ratio0:.3f}", flush=True)
        assert over1 == 0
        assert bool(((bad - ref).abs() <= (b1 - b0) * (1 + 1e-9)).all()) and ratio0 <= 1.0
        if R.case_dispatch(c)[0] in R.DOT2_PATHS:
            total0 += over0
        else:
            assert over0 == 0                        # the generic kernels do not round the taps: u_w is slack for them
    assert total0 > 0

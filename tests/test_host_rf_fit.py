"""CPU tests of the host side of the parametric receptive-field fits: the three C-ABI entries are declared,
exported and bound with agreeing struct sizes under ABI 7, dwn_rf_fit.hip stands in both source lists, every argument check
answers before a device is entered, dwn_gauss2d_ws_bytes refuses what the entry refuses, GaussianFits converts units as
ReceptiveFields does, SpatialGain.set_positions inverts positions in all three units, and the Python entries refuse CPU tensors and
bad arguments.  No kernel runs here."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)
ENTRIES = (("dwn_gauss2d_ws_bytes", C.c_size_t, 1), ("dwn_gauss2d_fit", C.c_int, 3), ("dwn_gauss2d_profile", C.c_int, 3))


def test_symbols_structs_header_and_source_lists():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, nargs in ENTRIES:
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][0] is restype and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        assert header.index(name + "(") > header.index("int dwn_sta_finalize(")          # appended to the header
    for cname, struct, size in (("dwn_gauss2d_args", L.Gauss2dArgs, 96), ("dwn_gauss2d_profile_args", L.Gauss2dProfileArgs, 56)):
        assert L._STRUCTS[cname] is struct
        assert L.lib.dwn_sizeof(cname.encode()) == C.sizeof(struct) == size
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        for f, _ in struct._fields_:
            assert re.search(r"\b%s\b" % f, fields), (cname, f)
    assert (L.GAUSS_PARAMS, L.GAUSS_TABLE) == (7, 16)
    assert re.search(r"#define DWN_GAUSS_PARAMS 7\b", header) and re.search(r"#define DWN_GAUSS_TABLE 16\b", header)
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "dwn_rf_fit.hip" in srcs and [n for n in L.HASH_SRCS if n.endswith(".hip")] == srcs
    assert L.lib.dwn_source_hash().decode() == L.source_hash()
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n, _, _ in ENTRIES), doc
    assert "12r" in (ROOT / "DESIGN.md").read_text()


def _fit(**kw):
    import sensorium_amd._lib as L
    a = L.Gauss2dArgs()
    a.R, a.gh, a.gw, a.M = 40, 8, 12, 40
    a.fit_baseline, a.max_iter = 1, 100
    a.rel_threshold, a.xtol, a.ftol = 0.5, 1e-8, 1e-12
    a.maps = a.sel = a.params = a.table = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_GRID = [dict(gh=2), dict(gw=2), dict(gh=0), dict(gw=-3), dict(gh=17, gw=241), dict(gh=64, gw=65), dict(gh=4097, gw=3),
            dict(gh=1 << 16, gw=1 << 16)]


def test_ws_bytes_refusals():
    import sensorium_amd._lib as L
    wsb = L.lib.dwn_gauss2d_ws_bytes
    assert wsb(None) == 0
    for kw in BAD_GRID + [dict(M=0), dict(M=-1), dict(R=0), dict(M=1 << 20)]:
        assert wsb(C.byref(_fit(**kw))) == 0, kw
    assert wsb(C.byref(_fit())) == 40 * 8 * 8                    # the start vector and its S per fit
    assert wsb(C.byref(_fit(gh=3, gw=3, M=1))) == 64 and wsb(C.byref(_fit(gh=64, gw=64))) == 40 * 64
    assert wsb(C.byref(_fit(M=7863, R=7863 * 12))) == 7863 * 64
    assert wsb(C.byref(_fit(gh=36, gw=64))) == wsb(C.byref(_fit(gh=5, gw=7)))       # follows M, not the grid


def test_fit_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    fit, err = L.lib.dwn_gauss2d_fit, L.lib.dwn_last_error
    assert fit(None, NO_DEVICE, None) == -1
    bad = BAD_GRID + [dict(M=0), dict(M=-2), dict(R=0), dict(sel=None, M=41), dict(max_iter=-1), dict(rel_threshold=-0.1),
                      dict(rel_threshold=1.5), dict(rel_threshold=float("nan")), dict(xtol=-1e-9), dict(ftol=-1.0), dict(xtol=float("nan")),
                      dict(ftol=float("nan")), dict(params=PTR + 4), dict(table=PTR + 4)]
    for kw in bad:
        assert fit(C.byref(_fit(**kw)), NO_DEVICE, None) == -2, kw
        assert b"gauss2d" in err(), kw
    for field in ("maps", "params", "table", "ws"):
        assert fit(C.byref(_fit(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    need = L.lib.dwn_gauss2d_ws_bytes(C.byref(_fit()))
    assert fit(C.byref(_fit(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert fit(C.byref(_fit(ws=PTR + 4)), NO_DEVICE, None) == -3
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert fit(C.byref(_fit(ws_bytes=need)), NO_DEVICE, None) > 0
    assert fit(C.byref(_fit(sel=None, fit_baseline=0, max_iter=0, xtol=0.0, ftol=0.0, rel_threshold=1.0)), NO_DEVICE, None) > 0
    assert fit(C.byref(_fit(M=400, R=3)), NO_DEVICE, None) > 0    # a row table may name a row many times


def _profile(**kw):
    import sensorium_amd._lib as L
    a = L.Gauss2dProfileArgs()
    a.N, a.L, a.gh, a.gw, a.fit_baseline = 9, 5, 8, 12, 1
    a.params = a.maps = a.profile = a.separability = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_profile_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    prof, err = L.lib.dwn_gauss2d_profile, L.lib.dwn_last_error
    assert prof(None, NO_DEVICE, None) == -1
    for kw in BAD_GRID + [dict(N=0), dict(N=-1), dict(L=0), dict(L=65536), dict(params=PTR + 4), dict(profile=PTR + 4),
                          dict(separability=PTR + 4)]:
        assert prof(C.byref(_profile(**kw)), NO_DEVICE, None) == -2, kw
        assert b"gauss2d" in err(), kw
    for field in ("params", "maps", "profile", "separability"):
        assert prof(C.byref(_profile(**{field: None})), NO_DEVICE, None) == -1, field
    assert prof(C.byref(_profile()), NO_DEVICE, None) > 0 and prof(C.byref(_profile(fit_baseline=0, L=1)), NO_DEVICE, None) > 0


def _fits(window=(14, 4, 6, 8), cell=2, size=(64, 64)):
    from sensorium_amd import GaussianFits
    table = torch.zeros(3, 16, dtype=torch.float64)
    table[0, :14] = torch.tensor([0.0, 7.0, 0.1, 1.5, 1.0, 2.0, 1.5, 0.75, 0.25, 0.01, 0.9, 0.05, 0.2, 0.1], dtype=torch.float64)
    table[1, :14] = torch.tensor([1.0, 100.0, 0.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.5, 0.95, 0.01, 0.01, 0.1], dtype=torch.float64)
    table[2] = torch.tensor([2.0, 0.0, 0.3, 0.0] + [math.nan] * 5 + [0.0, 0.0] + [math.nan] * 3 + [0.0, 2.0], dtype=torch.float64)
    params = torch.zeros(3, 7, dtype=torch.float64)
    return GaussianFits(table, params, None, (3, 4), window, cell, size, True)


def test_gaussian_fits_unit_conversions():
    import sensorium_amd
    from sensorium_amd import GAUSS_FIT_COLUMNS, ReceptiveFields
    for name in ("GaussianFits", "GAUSS_FIT_COLUMNS", "fit_gaussian2d"):
        assert name in sensorium_amd.__all__ and hasattr(sensorium_amd, name)
    assert GAUSS_FIT_COLUMNS == ("status", "iterations", "baseline", "amplitude", "cy", "cx", "sigma_major", "sigma_minor", "theta", "sse",
                                 "r2", "se_cy", "se_cx", "se_amplitude", "lambda", "row")
    fits = _fits()
    assert fits.centres("cells")[0].tolist() == [1.0, 2.0]
    assert fits.centres("input")[:2].tolist() == [[14 + 2.5, 4 + 4.5], [14.5, 4.5]]          # the centre of a 2 x 2 cell, plus the origin
    assert fits.centres("normalised")[0].tolist() == pytest.approx([2 * 8.5 / 63 - 1, 2 * 16.5 / 63 - 1])      # (x, y)
    assert bool(torch.isnan(fits.centres("input")[2]).all()) and bool(torch.isnan(fits.centres("normalised")[2]).all())
    # the same conversions as the summary's centres
    summary = torch.zeros(3, 8, dtype=torch.float64)
    summary[:, 2:4] = fits.table[:, 4:6]
    rf = ReceptiveFields(torch.zeros(3, 1, 3, 4), None, summary, 10, (14, 4, 6, 8), 2, (64, 64))
    for units in ("cells", "input", "normalised"):
        assert torch.equal(fits.centres(units)[:2], rf.centres(units)[:2]), units
    assert fits.sigmas("cells")[0].tolist() == [1.5, 0.75] and fits.sigmas("input")[0].tolist() == [3.0, 1.5]
    assert fits.theta[0].item() == 0.25 and fits.r2.tolist()[:2] == [0.9, 0.95] and fits.converged.tolist() == [True, False, False]
    assert fits.good(0.5).tolist() == [0] and fits.good(0.95).tolist() == [] and fits.good(0.5, max_se=0.1).tolist() == []
    assert fits.good(0.5, max_se=0.2).tolist() == [0] and fits.column("sse")[1].item() == 0.5
    for call in (lambda: fits.centres("pixels"), lambda: fits.sigmas("normalised")):
        with pytest.raises(ValueError):
            call()
    # render: the model on the grid
    fits.params[0] = torch.tensor([0.5, 2.0, 1.0, 2.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    img = fits.render()
    assert img.shape == (3, 3, 4) and img[0, 1, 2].item() == 2.5 and img[0, 1, 3].item() == pytest.approx(0.5 + 2 * math.exp(-0.5))


def test_set_positions_round_trip_in_all_units():
    from sensorium_amd import SpatialGain
    gain = SpatialGain([6, 4], 8, features=4, stride=4, seed=3)
    size = (5, 9)
    gen = torch.Generator().manual_seed(1)
    want = (torch.rand(6, 2, generator=gen) * 2 - 1) * 0.9
    gain.set_positions(0, want)
    assert torch.equal(gain.positions(0), want)
    for units in ("cells", "input"):
        cur = gain.positions(0, units, map_size=size)
        gain.heads[0].pos.data.zero_()
        gain.set_positions(0, cur, units, map_size=size)
        back = gain.positions(0, units, map_size=size)
        print(units, "round trip: max deviation", float((back - cur).abs().max()))
        assert torch.allclose(back, cur, rtol=0, atol=4 * 2.0 ** -24 * float(cur.abs().max()))
        assert torch.allclose(gain.positions(0), want, rtol=0, atol=4 * 2.0 ** -24)
    # known values: the last cell of a 9-wide map at stride 4 is pixel 32
    gain.set_positions(1, torch.tensor([[32.0, 0.0], [16.0, 8.0]]), "input", neurons=[2, 0], map_size=size)
    assert gain.heads[1].pos[2].tolist() == [1.0, -1.0] and gain.heads[1].pos[0].tolist() == [0.0, 0.0]
    before = gain.heads[1].pos.detach().clone()
    gain.set_positions(1, torch.tensor([[100.0, -5.0]]), "cells", neurons=torch.tensor([3]), map_size=size)           # clamped
    assert gain.heads[1].pos[3].tolist() == [1.0, -1.0] and torch.equal(gain.heads[1].pos[:3], before[:3])
    assert gain.heads[1].pos.requires_grad and gain.heads[1].pos.grad is None
    gain.set_positions(1, torch.tensor([[3.0, 2.0]]), "cells", neurons=[1], map_size=(1, 9))          # a side of one cell: 0
    assert gain.heads[1].pos[1].tolist() == [-0.25, 0.0]
    for bad, exc in ((dict(xy=torch.tensor([[float("nan"), 0.0]]), neurons=[0]), ValueError),
                     (dict(xy=torch.tensor([[float("inf"), 0.0]]), neurons=[0]), ValueError),
                     (dict(xy=torch.zeros(3, 2)), ValueError), (dict(xy=torch.zeros(4, 2), units="pixels"), ValueError),
                     (dict(xy=torch.zeros(4, 2), units="cells"), RuntimeError)):
        with pytest.raises(exc):
            gain.set_positions(1, **bad)


def test_python_entries_refuse_cpu_tensors_and_bad_arguments():
    from sensorium_amd import ReceptiveFields, fit_gaussian2d, ops
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        fit_gaussian2d(torch.zeros(2, 5, 7))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.gauss2d_fit(torch.zeros(2, 5, 7))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.gauss2d_profile(torch.zeros(2, 7, dtype=torch.float64), torch.zeros(2, 3, 5, 7))
    assert ops.gauss2d_ws_numel(5, 8, 12) == 40
    for bad in ((0, 8, 12), (5, 2, 12), (5, 8, 2), (5, 64, 65)):
        with pytest.raises(ValueError):
            ops.gauss2d_ws_numel(*bad)
    rf = ReceptiveFields(torch.zeros(2, 3, 3, 4), None, torch.zeros(2, 8, dtype=torch.float64), 10, (0, 0, 3, 4), 1, (3, 4))
    assert rf.fits is None
    for bad in (dict(lag="best"), dict(lag=3), dict(lag=-1), dict(lag=torch.zeros(3, dtype=torch.long)), dict(lag=torch.zeros(2))):
        with pytest.raises(ValueError):
            rf.fit(**bad)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        rf.fit()

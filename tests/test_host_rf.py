"""CPU tests of the host side of the receptive-field mapping: the five C-ABI entries are declared,
exported and bound with agreeing struct sizes under ABI 7, dwn_rf.hip stands in both source lists after dwn_trial_score.hip and
before dwn_corr.hip, every argument check answers before a device is entered, the state and workspace sizes are monotone in the
geometry, and NoiseStimulus / StaAccumulator / attribution.receptive_fields refuse CPU tensors and bad arguments.  No kernel runs
here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)
ENTRIES = (("dwn_noise_forward", C.c_int, 3), ("dwn_sta_state_bytes", C.c_size_t, 1), ("dwn_sta_ws_bytes", C.c_size_t, 1),
           ("dwn_sta_accumulate", C.c_int, 3), ("dwn_sta_finalize", C.c_int, 3))


def test_symbols_structs_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, nargs in ENTRIES:
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][0] is restype and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert list(L.SYMBOLS)[-5:] == [n for n, _, _ in ENTRIES]            # appended under ABI 7
    for cname, struct, size in (("dwn_noise_args", L.NoiseArgs, 104), ("dwn_sta_args", L.StaArgs, 152)):
        assert L._STRUCTS[cname] is struct
        assert L.lib.dwn_sizeof(cname.encode()) == C.sizeof(struct) == size
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        for f, _ in struct._fields_:
            assert re.search(r"\b%s\b" % f, fields), (cname, f)
    assert (L.NOISE_BINARY, L.NOISE_SPARSE) == (0, 1) and re.search(r"DWN_NOISE_BINARY = 0, DWN_NOISE_SPARSE = 1", header)
    assert L.STA_SUMMARY == 8 and re.search(r"#define DWN_STA_SUMMARY 8\b", header)
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n, _, _ in ENTRIES), doc
    assert "12q" in (ROOT / "DESIGN.md").read_text()


def test_source_lists():
    import sensorium_amd._lib as L
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    i = srcs.index("dwn_rf.hip")
    assert srcs[i - 1] == "dwn_trial_score.hip" and srcs[i + 1:] == ["dwn_corr.hip", "dwn_stim.hip"]
    hip = [n for n in L.HASH_SRCS if n.endswith(".hip")]
    assert hip == srcs
    assert L.lib.dwn_source_hash().decode() == L.source_hash()
    assert "$(SRCS:%.hip=build_det/%.o)" in mk


def _noise(**kw):
    import sensorium_amd._lib as L
    a = L.NoiseArgs()
    a.B, a.Cin, a.T, a.H, a.W, a.video_channel = 2, 5, 3, 8, 12, 0
    a.kind, a.cell, a.hold = L.NOISE_BINARY, 2, 1
    a.y0, a.x0, a.wh, a.ww = 1, 2, 6, 8
    a.background, a.contrast, a.density, a.pad = 127.5, 64.0, 0.1, 0.0
    a.seed, a.first_clip = 7, 0
    a.x = a.out = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_PLANE = [dict(B=0), dict(B=-3), dict(Cin=0), dict(T=0), dict(T=-1), dict(H=0), dict(W=0), dict(W=-2), dict(H=1 << 16, W=1 << 15),
             dict(wh=0), dict(ww=0), dict(wh=-2), dict(ww=-4), dict(y0=-1), dict(x0=-1), dict(y0=3), dict(x0=5), dict(wh=8, y0=1),
             dict(ww=12, x0=2), dict(y0=2 ** 31 - 1), dict(wh=2 ** 31 - 2, y0=1), dict(cell=0), dict(cell=-1), dict(cell=4),
             dict(cell=3), dict(cell=2, wh=5), dict(cell=2, ww=7)]


def test_noise_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    fwd, err = L.lib.dwn_noise_forward, L.lib.dwn_last_error
    assert fwd(None, NO_DEVICE, None) == -1
    bad = BAD_PLANE + [dict(video_channel=-1), dict(video_channel=5), dict(kind=2), dict(kind=-1), dict(hold=0), dict(hold=-2),
                       dict(density=-0.01), dict(density=1.5), dict(density=float("nan")), dict(first_clip=-1),
                       dict(first_clip=2 ** 32 - 1), dict(first_clip=2 ** 32), dict(B=3, first_clip=2 ** 32 - 2)]
    for kw in bad:
        assert fwd(C.byref(_noise(**kw)), NO_DEVICE, None) == -2, kw
        assert b"noise" in err(), kw
    assert b"first_clip" in (fwd(C.byref(_noise(first_clip=2 ** 32 - 1)), NO_DEVICE, None), err())[1]
    assert b"cell" in (fwd(C.byref(_noise(cell=4)), NO_DEVICE, None), err())[1]
    for field in ("x", "out"):
        assert fwd(C.byref(_noise(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert fwd(C.byref(_noise()), NO_DEVICE, None) > 0
    assert fwd(C.byref(_noise(first_clip=2 ** 32 - 2, seed=2 ** 64 - 1, kind=L.NOISE_SPARSE, density=1.0, hold=9)), NO_DEVICE, None) > 0
    assert fwd(C.byref(_noise(y0=0, x0=0, wh=8, ww=12, cell=1, density=0.0)), NO_DEVICE, None) > 0


def _sta(**kw):
    import sensorium_amd._lib as L
    a = L.StaArgs()
    a.B, a.Cin, a.T, a.H, a.W, a.N = 2, 5, 9, 8, 12, 67
    a.channel, a.y0, a.x0, a.wh, a.ww, a.cell = 0, 1, 2, 6, 8, 2
    a.lags, a.skip, a.s0 = 4, 0, 127.5
    a.samples, a.rel_threshold = 12, 0.5
    a.x = a.r = a.r0 = a.state = a.cov = a.z = a.summary = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_accumulate_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    acc, err = L.lib.dwn_sta_accumulate, L.lib.dwn_last_error
    assert acc(None, NO_DEVICE, None) == -1
    bad = BAD_PLANE + [dict(N=0), dict(N=-1), dict(channel=-1), dict(channel=5), dict(lags=0), dict(lags=-1), dict(lags=65536),
                       dict(skip=-1), dict(lags=10), dict(lags=11), dict(skip=9), dict(skip=100), dict(T=4, lags=5), dict(T=3)]
    for kw in bad:
        assert acc(C.byref(_sta(**kw)), NO_DEVICE, None) == -2, kw
        assert b"sta" in err(), kw
    assert b"no valid frame" in (acc(C.byref(_sta(skip=9)), NO_DEVICE, None), err())[1]
    for field in ("x", "r", "state"):
        assert acc(C.byref(_sta(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert acc(C.byref(_sta(state=PTR + 4)), NO_DEVICE, None) == -2
    # r0 and what the finaliser uses are optional here; complete arguments reach the device
    assert acc(C.byref(_sta(r0=None, cov=None, z=None, summary=None, ws=None, ws_bytes=0, samples=0, rel_threshold=7.0)), NO_DEVICE, None) > 0
    assert acc(C.byref(_sta(lags=9, T=9 + 1)), NO_DEVICE, None) > 0 and acc(C.byref(_sta(skip=8)), NO_DEVICE, None) > 0


def test_finalize_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    fin, err, wsb = L.lib.dwn_sta_finalize, L.lib.dwn_last_error, L.lib.dwn_sta_ws_bytes
    assert fin(None, NO_DEVICE, None) == -1 and wsb(None) == 0 and L.lib.dwn_sta_state_bytes(None) == 0
    bad = [dict(N=0), dict(N=-1), dict(lags=0), dict(lags=-3), dict(cell=0), dict(cell=4), dict(wh=0), dict(ww=-8), dict(samples=0),
           dict(samples=-5), dict(samples=1 << 52), dict(rel_threshold=-0.1), dict(rel_threshold=1.5), dict(rel_threshold=float("nan"))]
    for kw in bad:
        assert fin(C.byref(_sta(**kw)), NO_DEVICE, None) == -2, kw
        assert b"sta" in err(), kw
    for kw in bad[:8]:
        assert wsb(C.byref(_sta(**kw))) == 0 and L.lib.dwn_sta_state_bytes(C.byref(_sta(**kw))) == 0, kw
    for field in ("state", "cov", "summary", "ws"):
        assert fin(C.byref(_sta(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    need = wsb(C.byref(_sta()))
    assert need == 2 * 4 * 12 * 8                                 # V1 / K and var_v: lags * cells doubles each
    assert fin(C.byref(_sta(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert fin(C.byref(_sta(ws=PTR + 4)), NO_DEVICE, None) == -3
    assert fin(C.byref(_sta(summary=PTR + 4)), NO_DEVICE, None) == -2
    # z is optional, the plane and the batch are the accumulate's business
    assert fin(C.byref(_sta(ws_bytes=need, z=None)), NO_DEVICE, None) > 0
    assert fin(C.byref(_sta(B=0, T=0, H=0, W=0, Cin=0, x=None, r=None, r0=None, skip=-1, y0=99)), NO_DEVICE, None) > 0


def test_state_and_workspace_bytes_are_monotone():
    import sensorium_amd._lib as L

    def state(**kw):
        return L.lib.dwn_sta_state_bytes(C.byref(_sta(**kw)))

    def ws(**kw):
        return L.lib.dwn_sta_ws_bytes(C.byref(_sta(**kw)))
    assert state() == 8 * (67 * 4 * 12 + 2 * 67 + 2 * 4 * 12)
    for field, values in (("N", (1, 2, 31, 67, 7863)), ("lags", (1, 2, 5, 12))):
        sizes = [state(**{field: n}) for n in values]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), field
    grids = [state(H=64, W=64, y0=0, x0=0, wh=h, ww=w, cell=c) for h, w, c in ((2, 2, 2), (6, 8, 2), (6, 8, 1), (36, 64, 2), (36, 64, 1), (64, 64, 1))]
    assert grids == sorted(grids) and len(set(grids)) == len(grids)
    # the workspace follows lags and the grid, not N
    assert [ws(lags=n) for n in (1, 2, 5, 12)] == [2 * n * 12 * 8 for n in (1, 2, 5, 12)] and ws(N=1) == ws(N=7863)
    assert ws(cell=1) == 4 * ws(cell=2)
    # the metric shape: 7863 neurons, 12 lags, 36 x 64 cells of one pixel: 1.7 GB; cells of two: 0.43 GB
    big = state(N=7863, lags=12, H=64, W=64, y0=14, x0=0, wh=36, ww=64, cell=1)
    assert big == 8 * (7863 * 12 * 2304 + 2 * 7863 + 2 * 12 * 2304) and 1.7e9 < big < 1.8e9
    assert 0.43e9 < state(N=7863, lags=12, H=64, W=64, y0=14, x0=0, wh=36, ww=64, cell=2) < 0.44e9


def test_python_classes_refuse_cpu_tensors_and_bad_arguments():
    import sensorium_amd
    from sensorium_amd import NoiseStimulus, ReceptiveFields, StaAccumulator, attribution, ops, receptive_fields
    for name in ("NoiseStimulus", "StaAccumulator", "ReceptiveFields", "receptive_fields"):
        assert name in sensorium_amd.__all__ and hasattr(sensorium_amd, name)
    assert sensorium_amd.receptive_fields is receptive_fields and receptive_fields.StaAccumulator is StaAccumulator
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        NoiseStimulus(2, 3, (6, 8))()
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.noise_stimulus(torch.zeros(1, 5, 2, 4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        StaAccumulator(3, 2, (6, 8), device="cpu")
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.sta_accumulate(torch.zeros(10, dtype=torch.float64), torch.zeros(1, 1, 4, 2, 2), torch.zeros(1, 1, 4), lags=1, window=(0, 0, 2, 2))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.sta_finalize(torch.zeros(10, dtype=torch.float64), 3, N=1, lags=1, window=(0, 0, 2, 2))
    s = NoiseStimulus(3, 4, (64, 64), window=(14, 0, 36, 64), cell=2, behavior=(1.0, 2.0), pupil_center=(3.0, 4.0))
    assert not list(s.parameters()) and s.grid == (18, 32) and s.template.shape == (3, 5, 4, 64, 64)
    assert [float(s.template[0, c, 0, 0, 0]) for c in range(5)] == [0.0, 1.0, 2.0, 3.0, 4.0]
    for bad in (dict(kind="gaussian"), dict(cell=0), dict(cell=5), dict(cell=1.5), dict(hold=0), dict(contrast=-1.0), dict(contrast=128.0),
                dict(background=200.0), dict(density=1.5), dict(density=-0.1), dict(seed=-1), dict(seed=1 << 64), dict(window=(0, 0, 9, 8)),
                dict(window=(0, 0, 4)), dict(video_channel=5), dict(video_range=(1.0, 0.0)), dict(behavior=(0.0,)),
                dict(window=(0, 0, 6, 7), cell=2)):
        with pytest.raises(ValueError):
            NoiseStimulus(3, 2, (8, 8), **bad)
    NoiseStimulus(3, 2, (8, 8), contrast=500.0, video_range=None)                # no range: nothing to leave
    for batch, frames, size in ((0, 2, (4, 8)), (3, 0, (4, 8)), (3, 2, (0, 8)), (3, 2, (4,))):
        with pytest.raises(ValueError):
            NoiseStimulus(batch, frames, size)
    assert ops.sta_state_numel(67, 4, (1, 2, 6, 8), 2) == 67 * 4 * 12 + 2 * 67 + 2 * 4 * 12
    for bad in (dict(N=0), dict(lags=0), dict(cell=4), dict(window=(0, 0, 0, 8))):
        with pytest.raises(ValueError):
            ops.sta_state_numel(**{**dict(N=3, lags=2, window=(0, 0, 6, 8), cell=2), **bad})
    model = torch.nn.Linear(1, 1)
    for bad in (dict(clips=0), dict(batch=0), dict(lags=0), dict(lags=9), dict(skip=8), dict(skip=-1), dict(noise=dict(seed=3)),
                dict(noise=dict(window=(0, 0, 2, 2)))):
        with pytest.raises(ValueError):
            attribution.receptive_fields(model, 0, **{**dict(clips=4, frames=8, lags=3), **bad})
    rf = ReceptiveFields(torch.zeros(2, 1, 3, 4), None, torch.tensor([[0.0, 5.0, 1.0, 2.0, 0.5, 0.5, 1.0, 3.0],
                                                                      [0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0]], dtype=torch.float64),
                         10, (14, 4, 6, 8), 2, (64, 64))
    assert rf.peak_lag.tolist() == [0, 0] and rf.polarity.tolist() == [1.0, -1.0] and rf.significant(2.0).tolist() == [0]
    assert rf.centres("cells").tolist() == [[1.0, 2.0], [0.0, 0.0]]
    assert rf.centres("input").tolist() == [[14 + 2.5, 4 + 4.5], [14.5, 4.5]]       # the centre of a 2 x 2 cell, plus the origin
    assert rf.centres("normalised")[0].tolist() == pytest.approx([2 * 8.5 / 63 - 1, 2 * 16.5 / 63 - 1])      # (x, y)
    with pytest.raises(ValueError):
        rf.centres("pixels")

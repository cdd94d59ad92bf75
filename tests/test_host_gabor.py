"""CPU tests of the host side of the drifting-Gabor stimulus: the three C-ABI entries are declared,
exported and bound with agreeing struct sizes under ABI 7, dwn_stim.hip is in both source lists, every argument check answers
before a device is entered, the workspace size is monotone in the geometry, and DriftingGabor / GaborFn / the two attribution
functions refuse CPU tensors and bad arguments.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)


def test_symbols_struct_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, nargs in (("dwn_gabor_workspace_bytes", C.c_size_t, 1), ("dwn_gabor_forward", C.c_int, 3),
                                 ("dwn_gabor_backward", C.c_int, 3)):
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][0] is restype and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert L._STRUCTS["dwn_gabor_args"] is L.GaborArgs
    assert L.lib.dwn_sizeof(b"dwn_gabor_args") == C.sizeof(L.GaborArgs) == 120
    fields = re.search(r"typedef struct dwn_gabor_args \{(.*?)\} dwn_gabor_args;", header, re.S).group(1)
    for f, _ in L.GaborArgs._fields_:
        assert re.search(r"\b%s\b" % f, fields), f
    assert (L.GABOR_GAUSSIAN, L.GABOR_NONE) == (0, 1) and re.search(r"DWN_GABOR_GAUSSIAN = 0, DWN_GABOR_NONE = 1", header)
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n in ("dwn_gabor_forward", "dwn_gabor_backward", "dwn_gabor_workspace_bytes")), doc


def test_source_lists():
    import sensorium_amd._lib as L
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert srcs[-2:] == ["dwn_corr.hip", "dwn_stim.hip"]
    hip = [n for n in L.HASH_SRCS if n.endswith(".hip")]
    assert hip == srcs and L.HASH_SRCS[len(hip) - 1] == "dwn_stim.hip"
    assert L.lib.dwn_source_hash().decode() == L.source_hash()


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.GaborArgs()
    a.B, a.Cin, a.T, a.H, a.W, a.video_channel = 2, 5, 3, 8, 12, 0
    a.envelope, a.clamp, a.background, a.lo, a.hi, a.pad = L.GABOR_GAUSSIAN, 1, 127.5, 0.0, 255.0, 0.0
    a.x = a.params = a.out = a.dout = a.dparams = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_GEOMETRY = [dict(B=0), dict(B=-3), dict(Cin=0), dict(T=0), dict(T=-1), dict(H=0), dict(W=0), dict(W=-2),
                dict(video_channel=-1), dict(video_channel=5), dict(H=1 << 16, W=1 << 15), dict(envelope=2), dict(envelope=-1),
                dict(clamp=2), dict(lo=1.0, hi=0.5), dict(lo=float("nan")), dict(hi=float("nan")),
                dict(y0=1), dict(x0=2), dict(wh=4), dict(ww=6), dict(y0=-1, wh=4, ww=6), dict(x0=-1, wh=4, ww=6),
                dict(y0=5, wh=4, ww=6), dict(x0=7, wh=4, ww=6), dict(wh=9, ww=6), dict(wh=4, ww=13), dict(wh=-4, ww=6),
                dict(y0=2 ** 31 - 1, wh=4, ww=6), dict(wh=2 ** 31 - 1, ww=6, y0=1)]


def test_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    fwd, bwd, wsb = lib.dwn_gabor_forward, lib.dwn_gabor_backward, lib.dwn_gabor_workspace_bytes
    assert fwd(None, NO_DEVICE, None) == -1 and bwd(None, NO_DEVICE, None) == -1 and wsb(None) == 0
    for bad in BAD_GEOMETRY:
        for f in (fwd, bwd):
            assert f(C.byref(_args(**bad)), NO_DEVICE, None) == -2, bad
            assert b"gabor:" in err(), bad
        assert wsb(C.byref(_args(**bad))) == 0, bad
    assert b"window not inside the plane" in (fwd(C.byref(_args(wh=9, ww=6)), NO_DEVICE, None), err())[1]
    assert b"lo <= hi" in (fwd(C.byref(_args(lo=2.0, hi=1.0)), NO_DEVICE, None), err())[1]
    # lo > hi is only an error where the range is used
    assert fwd(C.byref(_args(clamp=0, lo=2.0, hi=1.0)), NO_DEVICE, None) > 0
    for field in ("x", "params", "out"):
        assert fwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    for field in ("params", "dout", "dparams", "ws"):
        assert bwd(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    need = wsb(C.byref(_args()))
    assert need > 0
    assert bwd(C.byref(_args(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert bwd(C.byref(_args(ws=PTR + 4)), NO_DEVICE, None) == -3
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert fwd(C.byref(_args(dout=None, dparams=None, ws=None)), NO_DEVICE, None) > 0
    assert bwd(C.byref(_args(x=None, out=None, ws_bytes=need)), NO_DEVICE, None) > 0
    assert fwd(C.byref(_args(y0=2, x0=3, wh=4, ww=6)), NO_DEVICE, None) > 0
    assert fwd(C.byref(_args(y0=0, x0=0, wh=8, ww=12, envelope=L.GABOR_NONE)), NO_DEVICE, None) > 0


def test_workspace_size_is_monotone_in_the_geometry():
    import sensorium_amd._lib as L
    wsb = L.lib.dwn_gabor_workspace_bytes

    def need(**kw):
        return wsb(C.byref(_args(**kw)))
    base = need()
    assert base == 2 * 3 * 1 * 8 * 8                           # B * T * chunks * 8 sums * sizeof(double)
    for field in ("B", "T"):
        sizes = [need(**{field: n}) for n in (1, 2, 3, 7, 64)]
        assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), field
    planes = [need(H=h, W=w) for h, w in ((1, 1), (8, 12), (32, 32), (36, 64), (64, 64), (128, 128))]
    assert planes == sorted(planes) and planes[2] == base and planes[3] == 3 * base and planes[4] == 4 * base
    # the window, not the plane, sizes the partial sums; the channels do not enter
    assert need(H=64, W=64, y0=14, x0=0, wh=36, ww=64) == need(H=36, W=64) < need(H=64, W=64)
    assert need(Cin=1) == need(Cin=9) == base and need(envelope=L.GABOR_NONE, clamp=0) == base


def test_functions_refuse_cpu_tensors():
    from sensorium_amd import DriftingGabor, ops
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.GaborFn.apply(torch.zeros(1, 8), torch.zeros(1, 5, 2, 4, 6))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        DriftingGabor(2, 3, (5, 7))()


def test_drifting_gabor_arguments():
    import sensorium_amd
    from sensorium_amd import PARAM_NAMES, DriftingGabor, stimuli
    assert PARAM_NAMES == ("cy", "cx", "sigma", "theta", "sf", "tf", "phase", "amplitude") == stimuli.PARAM_NAMES
    for name in ("DriftingGabor", "PARAM_NAMES", "tuning_curve", "optimal_gabor"):
        assert name in sensorium_amd.__all__ and hasattr(sensorium_amd, name)
    g = DriftingGabor(3, 4, (36, 64))
    assert isinstance(g, torch.nn.Module) and [n for n, _ in g.named_parameters()] == ["params"]
    assert g.params.shape == (3, 8) and g.params.dtype == torch.float32 and not g.state_dict().keys() - {"params"}
    assert g.cy.tolist() == [17.5] * 3 and g.cx.tolist() == [31.5] * 3 and g.sigma.tolist() == [6.0] * 3
    assert not g.theta.requires_grad and g.theta.shape == (3,)
    with pytest.raises(AttributeError):
        g.theta = torch.zeros(3)
    g = DriftingGabor(3, 4, (64, 64), window=(14, 0, 36, 64), init=dict(theta=[0.1, 0.2, 0.3], sf=0.05), behavior=(1.0, 2.0),
                      pupil_center=(3.0, 4.0), video_range=None)
    assert g.cy.tolist() == [31.5] * 3 and torch.allclose(g.theta, torch.tensor([0.1, 0.2, 0.3]))
    assert g.sf.tolist() == pytest.approx([0.05] * 3) and g.amplitude.tolist() == [1.0] * 3
    assert [float(g.template[0, c, 0, 0, 0]) for c in range(5)] == [0.0, 1.0, 2.0, 3.0, 4.0] and g.template.shape == (3, 5, 4, 64, 64)
    g = DriftingGabor(1, 2, (4, 4), in_channels=6, video_channel=2, behavior=(1.0, 2.0), pupil_center=(3.0, 4.0))
    assert [float(g.template[0, c, 0, 0, 0]) for c in range(6)] == [1.0, 2.0, 0.0, 3.0, 4.0, 0.0]
    for bad in (dict(envelope="box"), dict(window=(0, 0, 5, 8)), dict(window=(2, 0, 3, 8)), dict(window=(0, 0, 0, 4)),
                dict(window=(0, 0, 4)), dict(window=(-1, 0, 2, 2)), dict(learn=("theta", "speed")), dict(init=dict(speed=1.0)),
                dict(init=dict(theta=[0.0, 1.0])), dict(init=dict(theta=torch.zeros(3, 1))), dict(video_range=(1.0, 0.0)),
                dict(video_channel=5), dict(video_channel=-1), dict(behavior=(0.0,)), dict(pupil_center=(0.0, 0.0, 0.0))):
        with pytest.raises(ValueError):
            DriftingGabor(3, 2, (4, 8), **bad)
    for batch, frames, size in ((0, 2, (4, 8)), (3, 0, (4, 8)), (3, 2, (0, 8)), (3, 2, (4,))):
        with pytest.raises(ValueError):
            DriftingGabor(batch, frames, size)


def test_attribution_arguments():
    from sensorium_amd import attribution
    model = torch.nn.Linear(1, 1)
    base = dict(frames=4, size=(8, 8), theta=0.0)
    for bad_base, sweep in ((base, {}), (base, dict(theta=[0.0], sf=[0.1])), (base, dict(speed=[1.0])), (base, dict(theta=[])),
                            (dict(size=(8, 8)), dict(theta=[0.0])), (dict(base, batch=2), dict(theta=[0.0])),
                            (dict(base, sf=[0.1, 0.2]), dict(theta=[0.0]))):
        with pytest.raises(ValueError):
            attribution.tuning_curve(model, 0, bad_base, sweep)
    with pytest.raises(ValueError):
        attribution.tuning_curve(model, 0, base, dict(theta=[0.0]), chunk=0)
    for kw in (dict(starts=dict(theta=0.0)), dict(starts=torch.zeros(3, 7)), dict(starts=torch.zeros(2, 8), scales=dict(speed=1.0)),
               dict(starts=torch.zeros(2, 8), scales=dict(theta=0.0)), dict(starts=torch.zeros(2, 8), bounds=dict(sigma=1.0)),
               dict(starts=dict(theta=[0.0, 1.0], sf=[0.1, 0.2, 0.3]))):
        with pytest.raises(ValueError):
            attribution.optimal_gabor(model, 0, [0], steps=1, lr=0.1, shape=(2, 8, 8), **kw)
    lo, hi = attribution.gabor_bounds(__import__("sensorium_amd").DriftingGabor(1, 2, (64, 64), window=(14, 0, 36, 64)))
    assert lo.tolist()[:3] == [14.0, 0.0, 1.0] and hi.tolist()[:2] == [49.0, 63.0] and hi.tolist()[4] == 0.5 and hi.tolist()[7] == 127.5

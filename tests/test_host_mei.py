"""CPU tests of the host side of the regularised-MEI kernels: the five C-ABI entries are declared,
exported and bound with agreeing struct sizes under ABI 7, dwn_mei.hip is in both source lists, every argument check answers
before a device is entered, the workspace sizes follow the geometry, and the Python layer refuses CPU tensors and bad arguments.
No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)
ENTRIES = (("dwn_blur3d_ws_bytes", C.c_size_t, 1), ("dwn_clip_moments_ws_bytes", C.c_size_t, 1), ("dwn_blur3d", C.c_int, 3),
           ("dwn_clip_moments", C.c_int, 3), ("dwn_mei_update", C.c_int, 3))


def test_symbols_structs_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, nargs in ENTRIES:
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][0] is restype and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    for cname, struct, size in (("dwn_blur3d_args", L.Blur3dArgs, 104), ("dwn_clip_moments_args", L.ClipMomentsArgs, 72),
                                ("dwn_mei_update_args", L.MeiUpdateArgs, 120)):
        assert L._STRUCTS[cname] is struct
        assert L.lib.dwn_sizeof(cname.encode()) == C.sizeof(struct) == size
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        for f, _ in struct._fields_:
            assert re.search(r"\b%s\b" % f, fields), (cname, f)
    assert re.search(r"#define DWN_BLUR_MAX_RADIUS 16\b", header) and L.BLUR_MAX_RADIUS == 16 and L.BLUR_TAPS_STRIDE == 33
    assert re.search(r"#define DWN_MOMENTS_CHUNK 4096\b", header) and L.MOMENTS_CHUNK == 4096
    assert (L.MEI_STEP, L.MEI_PROJECT) == (0, 1) and re.search(r"DWN_MEI_STEP = 0, DWN_MEI_PROJECT = 1", header)
    assert (L.MEI_CONTRAST_MAX, L.MEI_CONTRAST_FIXED) == (0, 1) and re.search(r"DWN_MEI_CONTRAST_MAX = 0, DWN_MEI_CONTRAST_FIXED = 1", header)
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n, _, _ in ENTRIES), doc


def test_source_lists():
    import sensorium_amd._lib as L
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "dwn_mei.hip" in srcs
    hip = [n for n in L.HASH_SRCS if n.endswith(".hip")]
    assert hip == srcs
    assert L.lib.dwn_source_hash().decode() == L.source_hash()


def _blur(**kw):
    import sensorium_amd._lib as L
    a = L.Blur3dArgs()
    a.B, a.T, a.H, a.W, a.Cin_src, a.c_src, a.Cin_dst, a.c_dst = 2, 3, 8, 12, 5, 0, 1, 0
    a.Rt, a.Rh, a.Rw = 1, 2, 3
    a.src = a.dst = a.taps = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _moments(**kw):
    import sensorium_amd._lib as L
    a = L.ClipMomentsArgs()
    a.B, a.Cin, a.T, a.H, a.W, a.c = 2, 5, 3, 8, 12, 0
    a.x = a.stat = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _update(**kw):
    import sensorium_amd._lib as L
    a = L.MeiUpdateArgs()
    a.mode, a.B, a.Cin, a.T, a.H, a.W, a.c, a.Cin_g, a.c_g = L.MEI_STEP, 2, 5, 3, 8, 12, 0, 1, 0
    a.lo, a.hi = 0.0, 255.0
    a.x = a.g = a.stat = a.lr = PTR
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_WINDOW = [dict(y0=1), dict(x0=2), dict(wh=4), dict(ww=6), dict(y0=-1, wh=4, ww=6), dict(x0=-1, wh=4, ww=6),
              dict(y0=5, wh=4, ww=6), dict(x0=7, wh=4, ww=6), dict(wh=9, ww=6), dict(wh=4, ww=13), dict(wh=-4, ww=6),
              dict(y0=2 ** 31 - 1, wh=4, ww=6), dict(wh=2 ** 31 - 1, ww=6, y0=1)]
BAD_SIZES = [dict(B=0), dict(B=-3), dict(T=0), dict(T=-1), dict(H=0), dict(W=0), dict(W=-2), dict(H=1 << 16, W=1 << 15),
             dict(T=1 << 12, H=1 << 10, W=1 << 10)]


def test_blur_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    assert lib.dwn_blur3d(None, NO_DEVICE, None) == -1 and lib.dwn_blur3d_ws_bytes(None) == 0
    bad = BAD_SIZES + BAD_WINDOW + [dict(Cin_src=0), dict(Cin_dst=0), dict(c_src=-1), dict(c_src=5), dict(c_dst=1), dict(c_dst=-1),
                                    dict(Rt=17), dict(Rh=17), dict(Rw=17), dict(Rt=-1), dict(Rh=-1), dict(Rw=-1), dict(Rw=2 ** 31 - 1)]
    for kw in bad:
        assert lib.dwn_blur3d(C.byref(_blur(**kw)), NO_DEVICE, None) == -2, kw
        assert b"blur3d:" in err(), kw
        assert lib.dwn_blur3d_ws_bytes(C.byref(_blur(**kw))) == 0, kw
    assert b"radius" in (lib.dwn_blur3d(C.byref(_blur(Rh=17)), NO_DEVICE, None), err())[1]
    assert b"window not inside the plane" in (lib.dwn_blur3d(C.byref(_blur(wh=9, ww=6)), NO_DEVICE, None), err())[1]
    for field in ("src", "dst", "taps", "ws"):
        assert lib.dwn_blur3d(C.byref(_blur(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    need = lib.dwn_blur3d_ws_bytes(C.byref(_blur()))
    assert need == 2 * 3 * 8 * 12 * 4                               # one intermediate the size of the channel block
    assert need == lib.dwn_blur3d_ws_bytes(C.byref(_blur(Cin_src=1, Cin_dst=7, c_dst=3, Rt=0, Rh=16, Rw=16, y0=1, x0=2, wh=5, ww=7)))
    assert lib.dwn_blur3d(C.byref(_blur(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert lib.dwn_blur3d(C.byref(_blur(ws=PTR + 2)), NO_DEVICE, None) == -3
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    assert lib.dwn_blur3d(C.byref(_blur(ws_bytes=need)), NO_DEVICE, None) > 0
    assert lib.dwn_blur3d(C.byref(_blur(Rt=16, Rh=16, Rw=16, y0=1, x0=2, wh=5, ww=7, ws=PTR + 4)), NO_DEVICE, None) > 0
    assert lib.dwn_blur3d(C.byref(_blur(Rt=0, Rh=0, Rw=0, Cin_dst=5, c_dst=4)), NO_DEVICE, None) > 0


def test_moments_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    assert lib.dwn_clip_moments(None, NO_DEVICE, None) == -1 and lib.dwn_clip_moments_ws_bytes(None) == 0
    for kw in BAD_SIZES + BAD_WINDOW + [dict(Cin=0), dict(c=-1), dict(c=5)]:
        assert lib.dwn_clip_moments(C.byref(_moments(**kw)), NO_DEVICE, None) == -2, kw
        assert b"clip_moments:" in err(), kw
        assert lib.dwn_clip_moments_ws_bytes(C.byref(_moments(**kw))) == 0, kw
    for field in ("x", "stat", "ws"):
        assert lib.dwn_clip_moments(C.byref(_moments(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()

    def need(**kw):
        return lib.dwn_clip_moments_ws_bytes(C.byref(_moments(**kw)))
    assert need() == 2 * 1 * 3 * 8                                  # B * chunks * 3 sums * sizeof(double)
    assert need(T=16, H=64, W=64) == 2 * 16 * 24 and need(T=16, H=64, W=64, y0=14, wh=36, ww=64) == 2 * 9 * 24
    assert need(T=1, H=64, W=64) == need(T=1, H=65, W=64) - 2 * 24 == need(Cin=9, c=8, T=1, H=64, W=64)
    assert lib.dwn_clip_moments(C.byref(_moments(ws_bytes=need() - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert lib.dwn_clip_moments(C.byref(_moments(ws=PTR + 4)), NO_DEVICE, None) == -3
    assert lib.dwn_clip_moments(C.byref(_moments(ws_bytes=need())), NO_DEVICE, None) > 0
    assert lib.dwn_clip_moments(C.byref(_moments(y0=2, x0=3, wh=4, ww=6)), NO_DEVICE, None) > 0


def test_update_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    upd = lib.dwn_mei_update
    assert upd(None, NO_DEVICE, None) == -1
    for mode in (L.MEI_STEP, L.MEI_PROJECT):
        for kw in BAD_SIZES + BAD_WINDOW + [dict(Cin=0), dict(c=-1), dict(c=5)]:
            assert upd(C.byref(_update(mode=mode, **kw)), NO_DEVICE, None) == -2, (mode, kw)
            assert b"mei_update:" in err(), kw
    for mode in (2, -1, 7):
        assert upd(C.byref(_update(mode=mode)), NO_DEVICE, None) == -2 and b"mode" in err()
    for kw in (dict(Cin_g=0), dict(c_g=1), dict(c_g=-1)):
        assert upd(C.byref(_update(**kw)), NO_DEVICE, None) == -2, kw
    P = L.MEI_PROJECT
    for kw in (dict(lo=1.0, hi=0.5), dict(lo=float("nan")), dict(hi=float("nan")), dict(has_contrast=1, contrast=1.0, contrast_mode=2),
               dict(has_contrast=1, contrast=-1.0), dict(has_contrast=1, contrast=float("nan")), dict(has_mean=1, mean_target=float("inf"))):
        assert upd(C.byref(_update(mode=P, **kw)), NO_DEVICE, None) == -2, kw
    assert b"lo <= hi" in (upd(C.byref(_update(mode=P, lo=2.0, hi=1.0)), NO_DEVICE, None), err())[1]
    # what a mode does not use is not checked
    assert upd(C.byref(_update(lo=2.0, hi=1.0)), NO_DEVICE, None) > 0
    assert upd(C.byref(_update(mode=P, Cin_g=0, g=None, lr=None, contrast_mode=9, contrast=-1.0)), NO_DEVICE, None) > 0
    for field in ("x", "g", "stat", "lr"):
        assert upd(C.byref(_update(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    for field in ("x", "stat"):
        assert upd(C.byref(_update(mode=P, **{field: None})), NO_DEVICE, None) == -1, field
    assert upd(C.byref(_update()), NO_DEVICE, None) > 0
    assert upd(C.byref(_update(mode=P, has_mean=1, mean_target=127.5, has_contrast=1, contrast=20.0, contrast_mode=1, y0=1, x0=2, wh=5,
                               ww=7)), NO_DEVICE, None) > 0
    assert upd(C.byref(_update(mode=P, lo=float("-inf"), hi=float("inf"))), NO_DEVICE, None) > 0


def test_python_layer_refuses_cpu_tensors_and_bad_arguments():
    from sensorium_amd import attribution, ops
    x = torch.zeros(1, 5, 2, 4, 6)
    table, radii = ops.blur_taps_table([ops.gaussian_taps(0.5), ops.gaussian_taps(1.0), ops.gaussian_taps(1.0)])
    assert table.shape == (3, 33) and radii == (2, 3, 3) and float(table[0, 5:].abs().sum()) == 0
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.blur3d(x, table, radii)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.clip_moments(x)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.mei_update(x, torch.zeros(1, 4, dtype=torch.float64), "project")
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.GaussianBlur3dFn.apply(x, table, radii)
    for bad in ([torch.ones(1)] * 2, [torch.ones(2)] * 3, [torch.ones(35)] * 3, [torch.ones(1, 1)] * 3):
        with pytest.raises(ValueError):
            ops.blur_taps_table(bad)
    model = torch.nn.Linear(1, 1)
    base = dict(steps=2, lr=1.0, shape=(2, 8, 8), device="cpu")
    for kw in (dict(contrast=10.0, norm_budget=5.0), dict(contrast_mode="rms"), dict(contrast=-1.0), dict(window=(0, 0, 9, 8)),
               dict(window=(0, 0, 8)), dict(window=(-1, 0, 4, 4)), dict(window=(2, 0, 0, 4)), dict(blur_sigma=(1.0, 1.0)),
               dict(blur_sigma=[[1.0, 1.0, 1.0]] * 3), dict(blur_sigma=(1.0, -1.0, 1.0)), dict(blur_sigma=(1.0, float("nan"), 1.0)),
               dict(lr=[1.0, 2.0, 3.0]), dict(lr=[1.0, float("inf")]), dict(neurons=[[0], [1, 2]], init=torch.zeros(3, 5, 2, 8, 8)),
               dict(neurons=[[0], []])):
        args = dict(base, neurons=[0], **kw) if "neurons" not in kw else dict(base, **kw)
        with pytest.raises(ValueError):
            attribution.most_exciting_input(model, 0, args.pop("neurons"), **args)
    lr, tables, radii = attribution.mei_schedules(3, [1.0, 0.5, 0.25], [[0.0, 2.0, 2.0], [1.0, 1.0, 1.0], [0.5, 0.0, 3.0]])
    assert lr.tolist() == [1.0, 0.5, 0.25] and radii == (3, 6, 9) and tables.shape == (3, 3, 33)
    assert tables[0, 0, :7].tolist() == [0, 0, 0, 1, 0, 0, 0] and float(tables[2, 1, 6]) == 1.0
    assert abs(float(tables[1].double().sum()) - 3.0) < 1e-6
    assert attribution.mei_schedules(2, 0.5, None)[0].tolist() == [0.5, 0.5] and attribution.mei_schedules(2, 0.5, None)[1] is None
    assert attribution._per_clip_sets([[0, 1], [2]]) and attribution._per_clip_sets(torch.zeros(2, 3, dtype=torch.long))
    assert not attribution._per_clip_sets([0, 1]) and not attribution._per_clip_sets(None) and not attribution._per_clip_sets(torch.zeros(3))
    idx, mask = attribution._padded_sets([[4, 1], [2], [0, 5, 6]], "cpu")
    assert idx.tolist() == [[4, 1, 0], [2, 0, 0], [0, 5, 6]] and mask.tolist() == [[1, 1, 0], [1, 0, 0], [1, 1, 1]]

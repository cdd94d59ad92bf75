"""CPU tests of the host side of the population-modes kernels: the eleven C-ABI entries are declared,
exported and bound under ABI 7, dwn_modes.hip is in both source lists, every argument check answers before a device is entered, the
size queries return 0 for what the entries refuse, and the Python layer refuses what it documents.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)
QUERIES = ("dwn_modes_moments_ws_bytes", "dwn_modes_ritz_ws_bytes", "dwn_modes_solve_ws_bytes", "dwn_modes_overlap_ws_bytes")
STAGES = ("dwn_modes_symm", "dwn_modes_moments", "dwn_modes_orth", "dwn_modes_small_eigh", "dwn_modes_ritz", "dwn_modes_solve",
          "dwn_modes_overlap")


def good():
    import sensorium_amd._lib as L
    a = L.ModesArgs()
    a.N, a.p, a.k, a.max_iters = 100, 24, 16, 64
    a.lda, a.ldq, a.ldy, a.ldv, a.scale, a.tol = 100, 32, 32, 32, 1.0, 1e-10
    for f in ("A", "Q", "Y", "V", "H", "W", "values", "residuals", "moments", "status", "ws"):
        setattr(a, f, PTR)
    a.ws_bytes = 1 << 30
    return a


def test_symbols_struct_and_sources():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name in QUERIES + STAGES:
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        restype, argtypes = L.SYMBOLS[name]
        assert restype is (C.c_size_t if name in QUERIES else C.c_int) and len(argtypes) == (1 if name in QUERIES else 3)
        assert re.search(r"(?:int|size_t) %s\(const dwn_modes_args\* a" % name, header), name
    assert L._STRUCTS["dwn_modes_args"] is L.ModesArgs and L.lib.dwn_sizeof(b"dwn_modes_args") == C.sizeof(L.ModesArgs) == 168
    fields = re.search(r"typedef struct dwn_modes_args \{(.*?)\} dwn_modes_args;", header, re.S).group(1)
    for f, _ in L.ModesArgs._fields_:
        assert re.search(r"\b%s\b" % f, fields), f
    assert re.search(r"#define DWN_MODES_MAXP 64\b", header) and L.MODES_MAXP == 64
    assert re.search(r"#define DWN_MODES_ORTH_C 8\.0\b", header) and L.MODES_ORTH_C == 8.0
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "dwn_modes.hip" in srcs and [n for n in L.HASH_SRCS if n.endswith(".hip")] == srcs and "dwn_philox.h" in L.HASH_SRCS
    src = (ROOT / "sensorium_amd" / "csrc" / "dwn_modes.hip").read_text()
    assert "DWN_DETERMINISTIC" not in src.replace("does not read DWN_DETERMINISTIC", "") and "atomic" not in src.replace("No atomics", "")


def call(name, a):
    import sensorium_amd._lib as L
    return L.lib[name](C.byref(a), NO_DEVICE, None) if name in STAGES else L.lib[name](C.byref(a))


def test_good_arguments_reach_the_device():
    for name in STAGES:
        assert call(name, good()) > 0, name             # a HIP error from hipSetDevice: every check before it passed
    import sensorium_amd._lib as L
    for name in QUERIES:
        assert call(name, good()) > 0 and L.lib[name](None) == 0


BAD = (
    ("N", 0, -2, tuple(n for n in STAGES if n != "dwn_modes_small_eigh")), ("N", 65536, -2, ("dwn_modes_symm", "dwn_modes_moments", "dwn_modes_orth", "dwn_modes_ritz", "dwn_modes_solve", "dwn_modes_overlap")),
    ("p", 0, -2, ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_small_eigh", "dwn_modes_ritz", "dwn_modes_solve")),
    ("p", 65, -2, ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_small_eigh", "dwn_modes_ritz", "dwn_modes_solve")),
    ("k", 0, -2, ("dwn_modes_ritz", "dwn_modes_solve", "dwn_modes_overlap")), ("k", 25, -2, ("dwn_modes_ritz", "dwn_modes_solve")),
    ("lda", 99, -2, ("dwn_modes_symm", "dwn_modes_moments", "dwn_modes_solve", "dwn_modes_overlap")),
    ("ldq", 31, -2, ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_ritz")), ("ldy", 24, -2, ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_ritz")),
    ("ldv", 31, -2, ("dwn_modes_ritz", "dwn_modes_solve")), ("max_iters", 0, -2, ("dwn_modes_solve",)),
    ("scale", float("nan"), -2, ("dwn_modes_symm", "dwn_modes_moments", "dwn_modes_solve", "dwn_modes_overlap")),
    ("tol", -1.0, -2, ("dwn_modes_ritz", "dwn_modes_solve")), ("tol", float("inf"), -2, ("dwn_modes_ritz", "dwn_modes_solve")),
    ("A", None, -1, ("dwn_modes_symm", "dwn_modes_moments", "dwn_modes_solve")), ("Q", None, -1, ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_ritz", "dwn_modes_overlap")),
    ("Y", None, -1, ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_ritz", "dwn_modes_overlap")), ("V", None, -1, ("dwn_modes_ritz", "dwn_modes_solve")),
    ("H", None, -1, ("dwn_modes_small_eigh",)), ("W", None, -1, ("dwn_modes_small_eigh", "dwn_modes_ritz")),
    ("values", None, -1, ("dwn_modes_small_eigh", "dwn_modes_ritz", "dwn_modes_solve", "dwn_modes_overlap")),
    ("residuals", None, -1, ("dwn_modes_ritz", "dwn_modes_solve")), ("moments", None, -1, ("dwn_modes_moments", "dwn_modes_solve", "dwn_modes_overlap")),
    ("status", None, -1, ("dwn_modes_ritz", "dwn_modes_solve")), ("ws", None, -1, ("dwn_modes_moments", "dwn_modes_ritz", "dwn_modes_solve", "dwn_modes_overlap")),
    ("A", PTR + 4, -2, ("dwn_modes_symm", "dwn_modes_moments", "dwn_modes_solve")), ("status", PTR + 2, -2, ("dwn_modes_ritz", "dwn_modes_solve")),
    ("ws_bytes", 8, -3, ("dwn_modes_moments", "dwn_modes_ritz", "dwn_modes_solve", "dwn_modes_overlap")),
    ("ws", PTR + 8, -3, ("dwn_modes_moments", "dwn_modes_ritz", "dwn_modes_solve", "dwn_modes_overlap")),
)


@pytest.mark.parametrize("field,value,code,entries", BAD, ids=[f"{b[0]}={b[1]}" for b in BAD])
def test_refusals_answer_before_the_device(field, value, code, entries):
    import sensorium_amd._lib as L
    for name in entries:
        a = good()
        setattr(a, field, value)
        assert call(name, a) == code, (name, L.lib.dwn_last_error())
        assert name.replace("dwn_", "") in L.lib.dwn_last_error().decode()


def test_p_above_n_and_the_size_queries():
    import sensorium_amd._lib as L
    a = good()
    a.N, a.lda = 10, 10
    for name in ("dwn_modes_symm", "dwn_modes_orth", "dwn_modes_ritz", "dwn_modes_solve"):
        assert call(name, a) == -2
    assert L.lib.dwn_modes_solve_ws_bytes(C.byref(a)) == 0
    a.k = 11
    assert call("dwn_modes_overlap", a) == -2 and L.lib.dwn_modes_overlap_ws_bytes(C.byref(a)) == 0
    a = good()
    a.N = 0
    assert all(L.lib[q](C.byref(a)) == 0 for q in QUERIES)
    a = good()
    big, small = L.lib.dwn_modes_solve_ws_bytes(C.byref(a)), None
    a.p = 16
    small = L.lib.dwn_modes_solve_ws_bytes(C.byref(a))
    assert big > small >= 2 * 100 * 16 * 8


def test_python_layer_refusals():
    from sensorium_amd import population as P
    A = torch.eye(6, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="GPU"):
        P.modes(A, 2)

    class FakeCuda(torch.Tensor):                       # a tensor that claims to be on a GPU: the checks after the device check
        @property
        def is_cuda(self):
            return True

    def fake(*shape, dtype=torch.float64):
        return torch.zeros(*shape, dtype=dtype).as_subclass(FakeCuda)
    with pytest.raises(RuntimeError, match="float64"):
        P.modes(fake(6, 6, dtype=torch.float32), 2)
    with pytest.raises(ValueError, match="square"):
        P.modes(fake(6, 5), 2)
    for k in (0, 7):
        with pytest.raises(ValueError, match="k must lie"):
            P.modes(fake(6, 6), k)
    with pytest.raises(ValueError, match="oversample"):
        P.modes(fake(100, 100), 60, oversample=8)
    with pytest.raises(ValueError, match="oversample"):
        P.modes(fake(100, 100), 4, oversample=-1)
    cm = P.CorrelationMatrices({}, {"noise": torch.zeros(7, 6, dtype=torch.float64)}, {"noise": 0})
    with pytest.raises(ValueError, match="kind"):
        cm.modes("signal", k=2)
    with pytest.raises(ValueError, match="of must be"):
        cm.modes("noise", of="precision", k=2)
    with pytest.raises(ValueError, match="no sample"):
        cm.modes("noise", of="covariance", k=2)

"""CPU tests of the host side of the population-structure kernels: the eight C-ABI entries are declared,
exported and bound with agreeing struct sizes under ABI 7, dwn_pairwise.hip is in both source lists, every argument check answers
before a device is entered, the size queries return 0 for what the entries refuse, and the Python layer refuses what the device
tables could not be built from.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)
ENTRIES = (("dwn_pair_ldz", None, 1), ("dwn_pair_state_bytes", C.c_size_t, 1), ("dwn_pair_ws_bytes", C.c_size_t, 1),
           ("dwn_pair_compare_ws_bytes", C.c_size_t, 1), ("dwn_pair_stage", C.c_int, 3), ("dwn_pair_syrk", C.c_int, 3),
           ("dwn_pair_corr_finalize", C.c_int, 3), ("dwn_pair_compare", C.c_int, 3))


def test_symbols_structs_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, nargs in ENTRIES:
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        assert (restype is None or L.SYMBOLS[name][0] is restype) and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"(?:int|size_t|long long) %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    assert L.SYMBOLS["dwn_pair_ldz"][0] is C.c_longlong
    for cname, struct, size in (("dwn_pair_seg", L.PairSeg, 24), ("dwn_pair_args", L.PairArgs, 96),
                                ("dwn_pair_compare_args", L.PairCompareArgs, 88)):
        assert L._STRUCTS[cname] is struct
        assert L.lib.dwn_sizeof(cname.encode()) == C.sizeof(struct) == size
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        for f, _ in struct._fields_:
            assert re.search(r"\b%s\b" % f, fields), (cname, f)
    assert re.search(r"DWN_PAIR_TOTAL = 0, DWN_PAIR_SIGNAL = 1, DWN_PAIR_NOISE = 2", header)
    assert (L.PAIR_TOTAL, L.PAIR_SIGNAL, L.PAIR_NOISE) == (0, 1, 2)
    for macro, value in (("DWN_PAIR_TILE", L.PAIR_TILE), ("DWN_PAIR_KSTEP", L.PAIR_KSTEP), ("DWN_PAIR_SUMMARY", L.PAIR_SUMMARY),
                         ("DWN_PAIR_ROW_STATS", L.PAIR_ROW_STATS)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert "NO degrees-of-freedom correction" in header and "reaches only row i and column i" in header
    from sensorium_amd import ops
    assert ops._PAIR_SEG.itemsize == 24
    assert [ops._PAIR_SEG.fields[f][1] for f, _ in L.PairSeg._fields_] == [getattr(L.PairSeg, f).offset for f, _ in L.PairSeg._fields_]
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n, _, _ in ENTRIES), doc
    assert "12t" in (ROOT / "DESIGN.md").read_text()


def test_source_lists():
    import sensorium_amd._lib as L
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "dwn_pairwise.hip" in srcs
    hip = [n for n in L.HASH_SRCS if n.endswith(".hip")]
    assert hip == srcs
    assert L.lib.dwn_source_hash().decode() == L.source_hash()
    assert "$(SRCS:%.hip=build_det/%.o)" in mk and "$(SRCS:%.hip=build_asan/%.o)" in mk
    text = (ROOT / "sensorium_amd" / "csrc" / "dwn_pairwise.hip").read_text()
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in text and "atomic" not in text.replace("No atomics", "")
    assert "DWN_DETERMINISTIC" not in text.replace("does not read DWN_DETERMINISTIC", "")


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.PairArgs()
    a.N, a.kind, a.n_segs, a.n_groups, a.max_repeats, a.max_frames = 67, L.PAIR_NOISE, 9, 4, 3, 249
    a.cols, a.out_f32, a.n, a.eps = 1000, 0, 500, 1e-8
    a.segs = a.groups = a.state = a.out = a.ws = PTR
    a.ws_bytes = 1 << 30
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_STATE = [dict(N=0), dict(N=-5), dict(N=65536), dict(n=-1), dict(n=1 << 52)]
BAD_COLS = [dict(cols=0), dict(cols=-4), dict(cols=1001), dict(cols=1002)]


def test_size_queries():
    import sensorium_amd._lib as L
    lib = L.lib
    assert [lib.dwn_pair_ldz(n) for n in (-1, 0, 1, 63, 64, 65, 7863, 65535, 65536)] == [0, 0, 64, 64, 64, 128, 7872, 65536, 0]
    assert lib.dwn_pair_state_bytes(None) == 0 and lib.dwn_pair_ws_bytes(None) == 0 and lib.dwn_pair_compare_ws_bytes(None) == 0
    assert lib.dwn_pair_state_bytes(C.byref(_args())) == (67 * 67 + 67) * 8
    assert lib.dwn_pair_state_bytes(C.byref(_args(N=7863))) == (7863 * 7863 + 7863) * 8
    assert lib.dwn_pair_ws_bytes(C.byref(_args())) == 1000 * 128 * 8
    assert lib.dwn_pair_ws_bytes(C.byref(_args(N=7863, cols=4096))) == 4096 * 7872 * 8
    for kw in BAD_STATE[:3]:
        assert lib.dwn_pair_state_bytes(C.byref(_args(**kw))) == 0 and lib.dwn_pair_ws_bytes(C.byref(_args(**kw))) == 0, kw
    for kw in BAD_COLS:
        assert lib.dwn_pair_ws_bytes(C.byref(_args(**kw))) == 0, kw
    assert lib.dwn_pair_compare_ws_bytes(C.byref(_cmp())) == 9 * 8 * 8
    assert lib.dwn_pair_compare_ws_bytes(C.byref(_cmp(sel=None, M=67))) == 67 * 8 * 8
    for kw in (dict(N=0), dict(M=0), dict(M=-1), dict(sel=None, M=68), dict(M=(1 << 20) + 1), dict(N=65536)):
        assert lib.dwn_pair_compare_ws_bytes(C.byref(_cmp(**kw))) == 0, kw


def test_stage_and_syrk_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    stage, syrk = lib.dwn_pair_stage, lib.dwn_pair_syrk
    assert stage(None, NO_DEVICE, None) == -1 and syrk(None, NO_DEVICE, None) == -1
    for kw in BAD_STATE + BAD_COLS:
        assert stage(C.byref(_args(**kw)), NO_DEVICE, None) == -2 and b"pair_stage" in err(), kw
        assert syrk(C.byref(_args(**kw)), NO_DEVICE, None) == -2 and b"pair_syrk" in err(), kw
    for kw in (dict(kind=3), dict(kind=-1), dict(n_segs=0), dict(n_groups=0), dict(n_groups=10), dict(max_repeats=0), dict(max_repeats=10),
               dict(max_frames=0), dict(max_frames=-1), dict(n=(1 << 52) - 2000)):
        assert stage(C.byref(_args(**kw)), NO_DEVICE, None) == -2, kw
        assert b"pair_stage" in err(), kw
    for field in ("segs", "groups", "state", "ws"):
        assert stage(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1 and b"null pointer" in err(), field
    for field in ("state", "ws"):
        assert syrk(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1 and b"null pointer" in err(), field
    need = lib.dwn_pair_ws_bytes(C.byref(_args()))
    for fn in (stage, syrk):
        assert fn(C.byref(_args(state=PTR + 4)), NO_DEVICE, None) == -2
        assert fn(C.byref(_args(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
        assert fn(C.byref(_args(ws=PTR + 8)), NO_DEVICE, None) == -3
        # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
        assert fn(C.byref(_args(ws_bytes=need)), NO_DEVICE, None) > 0
    # what the product does not use is not checked
    assert syrk(C.byref(_args(kind=9, segs=None, groups=None, n_segs=0, n_groups=0, max_repeats=0, max_frames=0, out=None, eps=0.0)),
                NO_DEVICE, None) > 0
    assert stage(C.byref(_args(out=None, eps=0.0, n=0)), NO_DEVICE, None) > 0


def test_finalize_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    fin = lib.dwn_pair_corr_finalize
    assert fin(None, NO_DEVICE, None) == -1
    for kw in BAD_STATE + [dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan"))]:
        assert fin(C.byref(_args(**kw)), NO_DEVICE, None) == -2 and b"pair_corr_finalize" in err(), kw
    for field in ("state", "out"):
        assert fin(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1 and b"null pointer" in err(), field
    assert fin(C.byref(_args(out=PTR + 4)), NO_DEVICE, None) == -2
    assert fin(C.byref(_args(out=PTR + 4, out_f32=1)), NO_DEVICE, None) > 0            # fp32 output: 4-byte alignment
    assert fin(C.byref(_args(out=PTR + 2, out_f32=1)), NO_DEVICE, None) == -2
    # the tables, the operand and the workspace are not the finaliser's business; n = 0 is legal (NaN everywhere)
    assert fin(C.byref(_args(segs=None, groups=None, ws=None, ws_bytes=0, cols=0, n_segs=0, n_groups=0, kind=7, n=0)), NO_DEVICE, None) > 0


def _cmp(**kw):
    import sensorium_amd._lib as L
    a = L.PairCompareArgs()
    a.N, a.M, a.lda, a.ldb, a.eps = 67, 9, 67, 70, 1e-8
    a.A = a.B = a.sel = a.per_neuron = a.summary = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_compare_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    cmp_ = lib.dwn_pair_compare
    assert cmp_(None, NO_DEVICE, None) == -1
    for kw in (dict(N=0), dict(N=65536), dict(M=0), dict(M=-2), dict(M=(1 << 20) + 1), dict(sel=None, M=68), dict(lda=66), dict(ldb=0),
               dict(eps=0.0), dict(eps=float("nan")), dict(A=PTR + 4), dict(B=PTR + 4), dict(per_neuron=PTR + 4), dict(summary=PTR + 4),
               dict(sel=PTR + 2)):
        assert cmp_(C.byref(_cmp(**kw)), NO_DEVICE, None) == -2 and b"pair_compare" in err(), kw
    for field in ("A", "B", "per_neuron", "summary", "ws"):
        assert cmp_(C.byref(_cmp(**{field: None})), NO_DEVICE, None) == -1 and b"null pointer" in err(), field
    need = lib.dwn_pair_compare_ws_bytes(C.byref(_cmp()))
    assert cmp_(C.byref(_cmp(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert cmp_(C.byref(_cmp(ws=PTR + 4)), NO_DEVICE, None) == -3
    assert cmp_(C.byref(_cmp(ws_bytes=need)), NO_DEVICE, None) > 0
    assert cmp_(C.byref(_cmp(sel=None, M=67)), NO_DEVICE, None) > 0 and cmp_(C.byref(_cmp(M=500)), NO_DEVICE, None) > 0


def test_python_layer_refuses_what_the_tables_cannot_be_built_from():
    import sensorium_amd
    from sensorium_amd import ops, population
    from sensorium_amd.evaluation import FrameCut
    from sensorium_amd.population import PairwiseCorrelation, compare
    assert sensorium_amd.PairwiseCorrelation is PairwiseCorrelation and sensorium_amd.population_structure is population.population_structure
    N = 4
    x = torch.zeros(N, 30)
    state = torch.zeros(N + 1, N, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.pair_accumulate(state, "total", None)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.pair_corr(state, 10)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.pair_compare(torch.zeros(N, N, dtype=torch.float64), torch.zeros(N, N, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.pair_tables([(x, 0, 30)], [(0, 1, 30)], N, torch.device("cuda", 0))
    with pytest.raises(ValueError, match="no trials"):
        ops.pair_tables([], [], N, torch.device("cuda", 0))
    assert [ops.pair_chunk_cols(k, 5, 249) for k in population.KINDS] == [5 * 252, 252, 1248]
    assert [ops.pair_chunk_cols(k, 1, 3) for k in population.KINDS] == [4, 0, 0] and ops.pair_chunk_cols("noise", 2, 2) == 8
    assert [ops.pair_samples(k, 5, 249) for k in population.KINDS] == [1245, 249, 1245] and ops.pair_samples("signal", 1, 9) == 0
    with pytest.raises(RuntimeError, match="GPU"):
        PairwiseCorrelation(N, "cpu")
    for kw in (dict(kinds=()), dict(kinds=("total", "partial")), dict(kinds=("noise", "noise")), dict(eps=0.0), dict(flush_frames=0)):
        with pytest.raises(ValueError):
            PairwiseCorrelation(N, "cuda:0", **kw)
    with pytest.raises(ValueError, match="positive"):
        PairwiseCorrelation(0, "cuda:0")
    acc = PairwiseCorrelation(N, "cuda:0", cut=FrameCut(2, 20, 1))      # naming a device enters none
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        acc.add(x)
    with pytest.raises(RuntimeError, match="fp32"):
        acc.add(x.double())
    with pytest.raises(ValueError, match="unit stride"):
        acc.add(torch.zeros(30, N).t())
    with pytest.raises(ValueError, match=r"\[N = 4, L\]"):
        acc.add(torch.zeros(N + 1, 30))
    with pytest.raises(ValueError, match=r"\[N = 4, L\]"):
        acc.add(x[0])
    with pytest.raises(ValueError, match="keeps no frame"):
        acc.add(x[:, :3])
    with pytest.raises(ValueError, match="keeps no frame"):
        acc.add(x, length=3)
    with pytest.raises(ValueError, match="length 31"):
        acc.add(x, length=31)
    assert not acc._pending
    acc._pending.append(("video 7", x, 2, 17))
    with pytest.raises(ValueError, match="group 'video 7' keeps 17 frames per trial, this trial keeps 9"):
        acc.add(x[:, :12], group="video 7")
    acc._pending.clear()
    acc._flushed_groups.add("video 3")
    with pytest.raises(ValueError, match="group 'video 3' was already flushed"):
        acc.add(x, group="video 3")
    with pytest.raises(ValueError, match="no trial"):
        acc.compute()
    A = torch.zeros(N, N, dtype=torch.float64)
    with pytest.raises(ValueError, match="integer indices"):
        compare(A, A, neurons=[0.5, 1.0])
    with pytest.raises(ValueError, match="empty"):
        compare(A, A, neurons=[])
    with pytest.raises(ValueError, match="no trials"):
        population.population_structure(type("P", (), {"model": type("M", (), {"device": "cuda:0"})()})(), [], 0)

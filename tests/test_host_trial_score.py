"""CPU tests of the host side of the trial-score kernels: the three C-ABI entries are declared, exported and
bound with agreeing struct sizes under ABI 7, dwn_trial_score.hip is in both source lists, every argument check answers before a
device is entered, and the Python layer refuses what the device tables could not be built from.  No kernel runs here."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)
ENTRIES = (("dwn_trial_score_ws_bytes", C.c_size_t, 1), ("dwn_trial_moments", C.c_int, 3), ("dwn_trial_score_finalize", C.c_int, 3))


def test_symbols_structs_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, nargs in ENTRIES:
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        assert L.SYMBOLS[name][0] is restype and len(L.SYMBOLS[name][1]) == nargs
        decl = re.search(r"(?:int|size_t) %s\(([^;]*)\);" % name, header)
        assert decl and len(decl.group(1).split(",")) == nargs, name
    for cname, struct, size in (("dwn_trial_desc", L.TrialDesc, 40), ("dwn_trial_group", L.TrialGroup, 12),
                                ("dwn_trial_score_args", L.TrialScoreArgs, 120)):
        assert L._STRUCTS[cname] is struct
        assert L.lib.dwn_sizeof(cname.encode()) == C.sizeof(struct) == size
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, re.S).group(1)
        for f, _ in struct._fields_:
            assert re.search(r"\b%s\b" % f, fields), (cname, f)
    for macro, value in (("DWN_TRIAL_STATE_ROWS", L.TRIAL_STATE_ROWS), ("DWN_TRIAL_SCORE_ROWS", L.TRIAL_SCORE_ROWS),
                         ("DWN_TRIAL_SUMMARY", L.TRIAL_SUMMARY), ("DWN_TRIAL_TILE", L.TRIAL_TILE)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert (L.TRIAL_STATE_ROWS, L.TRIAL_SCORE_ROWS, L.TRIAL_SUMMARY, L.TRIAL_TILE) == (17, 5, 8, 4)
    from sensorium_amd import ops
    assert ops._TRIAL_DESC.itemsize == 40 and ops._TRIAL_GROUP.itemsize == 12
    assert [ops._TRIAL_DESC.fields[f][1] for f, _ in L.TrialDesc._fields_] == [getattr(L.TrialDesc, f).offset for f, _ in L.TrialDesc._fields_]
    assert [ops._TRIAL_GROUP.fields[f][1] for f, _ in L.TrialGroup._fields_] == [getattr(L.TrialGroup, f).offset for f, _ in L.TrialGroup._fields_]
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n, _, _ in ENTRIES), doc


def test_source_lists():
    import sensorium_amd._lib as L
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "dwn_trial_score.hip" in srcs
    hip = [n for n in L.HASH_SRCS if n.endswith(".hip")]
    assert hip == srcs
    assert L.lib.dwn_source_hash().decode() == L.source_hash()
    assert "$(SRCS:%.hip=build_det/%.o)" in mk                      # the ordered-reduction build compiles the same list


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.TrialScoreArgs()
    a.N, a.n_trials, a.n_groups, a.max_repeats, a.max_frames = 67, 9, 4, 3, 249
    a.n_all, a.n_repeat, a.n_group_frames = 1000, 600, 200
    a.eps, a.fev_threshold = 1e-8, 0.15
    a.trials = a.groups = a.state = a.scores = a.summary = a.ws = PTR
    a.ws_bytes = 1 << 20
    for k, v in kw.items():
        setattr(a, k, v)
    return a


BAD_COUNTS = [dict(N=0), dict(N=-5), dict(n_all=-1), dict(n_repeat=-1), dict(n_group_frames=-1), dict(n_repeat=1001),
              dict(n_group_frames=301), dict(n_repeat=0), dict(n_group_frames=0), dict(n_all=1 << 52, n_repeat=0, n_group_frames=0)]


def test_moments_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    mom = lib.dwn_trial_moments
    assert mom(None, NO_DEVICE, None) == -1
    bad = BAD_COUNTS + [dict(n_trials=0), dict(n_trials=-1), dict(n_groups=0), dict(n_groups=10), dict(max_repeats=0),
                        dict(max_repeats=10), dict(max_repeats=-2), dict(max_frames=0), dict(max_frames=-1),
                        dict(n_all=(1 << 52) - 2000, n_repeat=0, n_group_frames=0)]
    for kw in bad:
        assert mom(C.byref(_args(**kw)), NO_DEVICE, None) == -2, kw
        assert b"trial_" in err(), kw
    assert b"contradict" in (mom(C.byref(_args(n_group_frames=301)), NO_DEVICE, None), err())[1]
    assert b"max_repeats" in (mom(C.byref(_args(max_repeats=10)), NO_DEVICE, None), err())[1]
    for field in ("trials", "groups", "state"):
        assert mom(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    assert mom(C.byref(_args(state=PTR + 4)), NO_DEVICE, None) == -2
    # what the moments do not use is not checked; complete arguments get past the checks: the answer is then the runtime's about
    # the device, a HIP error code
    assert mom(C.byref(_args()), NO_DEVICE, None) > 0
    assert mom(C.byref(_args(eps=0.0, fev_threshold=float("nan"), scores=None, summary=None, ws=None, ws_bytes=0)), NO_DEVICE, None) > 0
    assert mom(C.byref(_args(n_all=0, n_repeat=0, n_group_frames=0, n_trials=1, n_groups=1, max_repeats=1, max_frames=1, N=1)),
               NO_DEVICE, None) > 0


def test_finalize_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    fin = lib.dwn_trial_score_finalize
    assert fin(None, NO_DEVICE, None) == -1 and lib.dwn_trial_score_ws_bytes(None) == 0
    for kw in BAD_COUNTS + [dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(fev_threshold=float("nan"))]:
        assert fin(C.byref(_args(**kw)), NO_DEVICE, None) == -2, kw
        assert b"trial_score" in err(), kw
    assert lib.dwn_trial_score_ws_bytes(C.byref(_args(N=0))) == 0
    for field in ("state", "scores", "summary", "ws"):
        assert fin(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
        assert b"null pointer" in err()
    need = lib.dwn_trial_score_ws_bytes(C.byref(_args()))
    assert need == 1 * 5 * 8                                          # one workgroup of 256 neurons, five partial sums
    assert lib.dwn_trial_score_ws_bytes(C.byref(_args(N=256))) == 40 and lib.dwn_trial_score_ws_bytes(C.byref(_args(N=257))) == 80
    assert lib.dwn_trial_score_ws_bytes(C.byref(_args(N=7863))) == 31 * 40
    assert fin(C.byref(_args(ws_bytes=need - 1)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert fin(C.byref(_args(ws=PTR + 4)), NO_DEVICE, None) == -3
    assert fin(C.byref(_args(scores=PTR + 4)), NO_DEVICE, None) == -2
    assert fin(C.byref(_args(ws_bytes=need)), NO_DEVICE, None) > 0
    # the tables and their sizes are the moments' business; no repeat group and a threshold of -inf are legal
    assert fin(C.byref(_args(trials=None, groups=None, n_trials=0, n_groups=0, max_repeats=0, max_frames=0)), NO_DEVICE, None) > 0
    assert fin(C.byref(_args(n_repeat=0, n_group_frames=0, fev_threshold=float("-inf"))), NO_DEVICE, None) > 0
    assert fin(C.byref(_args(n_all=0, n_repeat=0, n_group_frames=0)), NO_DEVICE, None) > 0


def test_python_layer_refuses_what_the_tables_cannot_be_built_from():
    from sensorium_amd import ops
    from sensorium_amd.evaluation import FrameCut, TrialScorer, summarise
    N = 4
    x = torch.zeros(N, 30)
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.trial_moments(torch.zeros(17, N, dtype=torch.float64), [(x, x, 0, 30)], [(0, 1, 30)])
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        ops.trial_scores(torch.zeros(17, N, dtype=torch.float64), (30, 0, 0))
    with pytest.raises(RuntimeError, match="GPU"):
        TrialScorer(N, "cpu")
    sc = TrialScorer(N, "cuda:0", cut=FrameCut(2, 20, 1))             # naming a device enters none
    with pytest.raises(RuntimeError, match="must be on a GPU"):
        sc.add(x, x)
    with pytest.raises(RuntimeError, match="fp32"):
        sc.add(x.double(), x)
    with pytest.raises(RuntimeError, match="fp32"):
        sc.add(x, x.to(torch.bfloat16))
    with pytest.raises(ValueError, match="unit stride"):
        sc.add(torch.zeros(30, N).t(), x)
    with pytest.raises(ValueError, match="unit stride"):
        sc.add(x, torch.zeros(N, 60)[:, ::2])
    with pytest.raises(ValueError, match=r"\[N = 4, L\]"):
        sc.add(torch.zeros(N + 1, 30), x)
    with pytest.raises(ValueError, match=r"\[N = 4, L\]"):
        sc.add(x[0], x[0])
    with pytest.raises(ValueError, match="keeps no frame"):           # an empty cut: [2, min(3, 20) - 1)
        sc.add(x[:, :3], x)
    with pytest.raises(ValueError, match="keeps no frame"):
        sc.add(x, x, length=3)
    with pytest.raises(ValueError, match="length 31"):
        sc.add(x, x, length=31)
    assert not sc._pending
    # unequal kept lengths inside a group: the error names the group (lengths are host integers, nothing is launched)
    sc._pending.append(("video 7", x, x, 2, 17))
    with pytest.raises(ValueError, match="group 'video 7' keeps 17 frames per trial, this trial keeps 9"):
        sc.add(x[:, :12], x, group="video 7")
    sc._pending.clear()
    sc._flushed_groups.add("video 3")
    with pytest.raises(ValueError, match="group 'video 3' was already flushed"):
        sc.add(x, x, group="video 3")
    with pytest.raises(ValueError, match="no trial"):
        sc.compute()
    assert summarise({}) == {"correlations": {}, "mean_correlation": pytest.approx(float("nan"), nan_ok=True)}

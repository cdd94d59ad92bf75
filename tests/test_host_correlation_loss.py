"""CPU tests of the host side of the correlation objective: the two losses are exported and registered in
MouseModel, their constructors validate, CPU tensors are refused with the usual error, the four C-ABI entries are declared, exported
and bound with the struct of include/dwn.h, and every argument check answers before a device is entered.  No kernel runs here."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
TINY = dict(readout_outputs=(7, 10), core_features=(8, 8, 16), spatial_strides=(2, 1, 2), expansion_ratio=3, se_reduce_ratio=4,
            cortex_features=(32, 64))
PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has: an entry that reached the device would answer a HIP error (> 0)


def test_exports_and_registry_names():
    import sensorium_amd
    from sensorium_amd import MiceCorrelationLoss, MicePoissonCorrelationLoss, MicePoissonLoss, losses
    from sensorium_amd.argus_models import MouseModel
    assert {"MiceCorrelationLoss", "MicePoissonCorrelationLoss", "MicePoissonLoss"} <= set(sensorium_amd.__all__)
    assert MouseModel.loss == {"mice_poisson": MicePoissonLoss, "mice_correlation": MiceCorrelationLoss,
                               "mice_poisson_correlation": MicePoissonCorrelationLoss}
    assert losses.MiceCorrelationLoss is MiceCorrelationLoss
    base = dict(nn_module=("dwiseneuro", TINY), optimizer=("AdamW", {"lr": 1e-3}), device="cpu")
    assert isinstance(MouseModel(dict(base)).loss, MicePoissonLoss)                       # the default is the parent's
    m = MouseModel(dict(base, loss=("mice_correlation", {"reduction": "sum"})))
    assert isinstance(m.loss, MiceCorrelationLoss) and m.loss.reduction == "sum" and m.loss.eps == 1e-8
    m = MouseModel(dict(base, loss=("mice_poisson_correlation", {"correlation_weight": 2.5})))
    assert isinstance(m.loss, MicePoissonCorrelationLoss) and m.loss.correlation_weight == 2.5 and m.loss.poisson_weight == 1.0
    assert isinstance(m.loss.poisson, MicePoissonLoss) and isinstance(m.loss.correlation, MiceCorrelationLoss)
    assert not list(m.loss.parameters()) and not list(m.loss.buffers())                   # nothing for a checkpoint or the optimizer


def test_constructor_validation():
    from sensorium_amd import MiceCorrelationLoss, MicePoissonCorrelationLoss
    d = {k: p.default for k, p in inspect.signature(MiceCorrelationLoss.__init__).parameters.items() if k != "self"}
    assert d == dict(eps=1e-8, reduction="mean")
    names = list(inspect.signature(MicePoissonCorrelationLoss.__init__).parameters)[1:]
    assert names[:4] == ["poisson_weight", "correlation_weight", "eps", "reduction"]
    assert inspect.signature(MicePoissonCorrelationLoss.__init__).parameters["poisson_weight"].default == 1.0
    for cls in (MiceCorrelationLoss, MicePoissonCorrelationLoss):
        for bad in ("none", "batchmean", None, 1):
            with pytest.raises(ValueError, match="reduction"):
                cls(reduction=bad)
        for bad in (0.0, -1e-8, float("nan")):
            with pytest.raises(ValueError, match="eps"):
                cls(eps=bad)
        assert cls(eps=1e-6, reduction="sum") is not None
    for kw in (dict(poisson_weight=-1.0), dict(correlation_weight=-0.5), dict(poisson_weight=float("inf")),
               dict(correlation_weight=float("nan")), dict(poisson_weight=0.0, correlation_weight=0.0)):
        with pytest.raises(ValueError, match="weight"):
            MicePoissonCorrelationLoss(**kw)
    both = MicePoissonCorrelationLoss(poisson_weight=0.0, correlation_weight=3.0, eps=1e-6, reduction="sum")
    assert both.correlation.eps == 1e-6 and both.correlation.reduction == "sum" and both.poisson.eps == 1e-8


def test_cpu_tensors_are_refused():
    from sensorium_amd import MiceCorrelationLoss, MicePoissonCorrelationLoss, ops
    from sensorium_amd.metrics import CorrelationMetric
    p, t, w = torch.rand(3, 5, 4), torch.rand(3, 5, 4), torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]])
    with pytest.raises(RuntimeError, match="must be on a GPU.*no CPU fallback"):
        ops.CorrelationLossFn.apply(p, t, w[:, 0], torch.tensor(0.5), 1e-8, "mean")
    with pytest.raises(RuntimeError, match="must be on a GPU.*no CPU fallback"):
        ops.corr_moments(p, t, w[:, 0])
    for loss in (MiceCorrelationLoss(), MicePoissonCorrelationLoss()):
        with pytest.raises(RuntimeError, match="must be on a GPU.*no CPU fallback"):
            loss([p, p], ([t, t], w))
    out = {"prediction": [p, p], "target": ([t, t], w)}
    with pytest.raises(RuntimeError, match="must be on a GPU.*no CPU fallback"):
        CorrelationMetric(fused=True).update(out)
    plain = CorrelationMetric()                                    # the default keeps working on any device
    plain.update(out)
    assert sorted(plain.compute()) == [0, 1] and plain.fused is False
    assert list(inspect.signature(CorrelationMetric.__init__).parameters) == ["self", "fused"]
    assert inspect.signature(CorrelationMetric.__init__).parameters["fused"].default is False


def test_symbols_struct_and_header():
    import sensorium_amd._lib as L
    header = (ROOT / "include" / "dwn.h").read_text()
    assert re.search(r"#define DWN_ABI_VERSION 7\b", header) and L.lib.dwn_abi_version() == 7
    for name, restype, ret in (("dwn_corr_moments", C.c_int, "int"), ("dwn_corr_loss_finalize", C.c_int, "int"),
                               ("dwn_corr_loss_backward", C.c_int, "int"), ("dwn_corr_ws_bytes", C.c_size_t, "size_t")):
        assert hasattr(L.lib, name) and name in L.SYMBOLS
        got_restype, argtypes = L.SYMBOLS[name]
        decl = re.search(r"%s %s\(([^;]*)\);" % (ret, name), header)
        assert got_restype is restype and decl and len(decl.group(1).split(",")) == len(argtypes), name
    # appended: the new declarations stand behind everything the parent declared
    assert header.index("dwn_corr_args") > header.index("int dwn_plane_mean(")
    assert L._STRUCTS["dwn_corr_args"] is L.CorrArgs
    assert L.lib.dwn_sizeof(b"dwn_corr_args") == C.sizeof(L.CorrArgs) == 120
    fields = re.search(r"typedef struct dwn_corr_args \{(.*?)\} dwn_corr_args;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f for f, _ in L.CorrArgs._fields_]                                   # the same fields in the same order
    assert int(re.search(r"#define DWN_CORR_STAT_ROWS (\d+)", header).group(1)) == L.CORR_STAT_ROWS
    assert int(re.search(r"#define DWN_CORR_TILE (\d+)", header).group(1)) == L.CORR_TILE <= 32
    assert re.search(r"DWN_CORR_MEAN = 0, DWN_CORR_SUM = 1", header) and (L.CORR_MEAN, L.CORR_SUM) == (0, 1)
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        assert all(n in text for n in ("dwn_corr_moments", "dwn_corr_loss_finalize", "dwn_corr_loss_backward", "dwn_corr_ws_bytes")), doc
    # the new source is hashed in the same position in both lists (the stale-binary check)
    mk = (ROOT / "sensorium_amd" / "csrc" / "Makefile").read_text()
    srcs = re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split()
    assert "dwn_corr.hip" in srcs and list(L.HASH_SRCS[:len(srcs)]) == srcs


def _args(**kw):
    import sensorium_amd._lib as L
    a = L.CorrArgs()
    a.B, a.N, a.T, a.reduction, a.eps, a.w_stride = 3, 70, 8, L.CORR_MEAN, 1e-8, 1
    a.pred = a.target = a.w = a.stat = a.count = a.share = a.loss_acc = a.gscale = a.dpred = a.ws = PTR
    a.ws_bytes = 4096
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_answer_without_a_device():
    import sensorium_amd._lib as L
    lib, err = L.lib, L.lib.dwn_last_error
    entries = (lib.dwn_corr_moments, lib.dwn_corr_loss_finalize, lib.dwn_corr_loss_backward)
    for f in entries:
        assert f(None, NO_DEVICE, None) == -1 and b"null arguments" in err()
        for field in ("B", "N", "T"):
            for bad in (0, -3):
                assert f(C.byref(_args(**{field: bad})), NO_DEVICE, None) == -2, field
                assert b"must be positive" in err()
        assert f(C.byref(_args(N=1 << 20, T=1 << 11)), NO_DEVICE, None) == -2 and b"2^31" in err()
        assert f(C.byref(_args(w_stride=0)), NO_DEVICE, None) == -2 and b"w_stride" in err()
        for bad in (0.0, -1.0, float("nan")):
            assert f(C.byref(_args(eps=bad)), NO_DEVICE, None) == -2 and b"eps" in err()
        assert f(C.byref(_args(reduction=2)), NO_DEVICE, None) == -2 and b"reduction" in err()
        assert f(C.byref(_args(B=1 << 20)), NO_DEVICE, None) > 0        # B is no grid dimension: a large batch is not refused
    needs = ((lib.dwn_corr_moments, ("pred", "target", "w", "stat", "count")),
             (lib.dwn_corr_loss_finalize, ("stat", "count", "share", "loss_acc", "ws")),
             (lib.dwn_corr_loss_backward, ("pred", "target", "w", "stat", "share", "dpred")))
    for f, fields in needs:
        for field in fields:
            assert f(C.byref(_args(**{field: None})), NO_DEVICE, None) == -1, field
            assert b"null pointer" in err()
    assert lib.dwn_corr_loss_backward(C.byref(_args(gscale=None)), NO_DEVICE, None) > 0      # a null gscale means 1
    # the workspace: one double per 256 neurons
    assert lib.dwn_corr_ws_bytes(None) == 0
    for n, want in ((1, 8), (256, 8), (257, 16), (7863, 31 * 8)):
        assert lib.dwn_corr_ws_bytes(C.byref(_args(N=n))) == want
    assert lib.dwn_corr_loss_finalize(C.byref(_args(N=257, ws_bytes=8)), NO_DEVICE, None) == -3 and b"workspace" in err()
    assert lib.dwn_corr_loss_finalize(C.byref(_args(ws=PTR + 4)), NO_DEVICE, None) == -3
    # complete arguments get past the checks: the answer is then the runtime's about the device, a HIP error code
    for f in entries:
        assert f(C.byref(_args()), NO_DEVICE, None) > 0

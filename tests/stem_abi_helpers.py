"""The stem through the C-ABI with batch statistics, and its float64 autograd reference (imported by
tests/test_gpu_train_input_grad.py and tests/det_input_grad_worker.py).

Inputs are in production ranges: grey levels 0..255 in channel 0, small / offset traces in the others (what the stem sees, and
what stresses x - xbar).  The reference is torch on the CPU in float64: conv1x1 -> batch_norm(training=True), differentiated by
autograd; nothing of the code under test enters it."""
import ctypes as C

import torch
import torch.nn.functional as F

EPS = 1e-5
# the five shapes of tests/test_gpu_frozen_bn.py::test_stem_input_grad_c_abi: (B, S, Cin, C0)
SHAPES = {"metric": (2, 16 * 64 * 64, 5, 64), "odd": (3, 7 * 9 * 11, 5, 64), "tiny": (1, 61, 5, 8), "wide8": (2, 1000, 8, 128),
          "ragged": (2, 333, 3, 24)}
TRACE_SCALE = (10.0, 5.0, 20.0, 20.0, 1.0, 2.0, 3.0)
TRACE_SHIFT = (30.0, 5.0, 100.0, 70.0, 0.5, 1.0, 2.0)


def make_case(shape, dtype, kind="mixed"):
    """kind: 'mixed' dout = r + 0.5 zhat + c (r ~ N(0,1), c a per-channel constant of order one: the batch-statistics terms
    matter), 'const' dout = c, 'zhat' dout = zhat (the two directions BatchNorm's backward annihilates)."""
    B, S, Cin, C0 = shape
    if dtype == torch.float32:
        C0 = min(C0, 64)                      # fp32 rows: at most 64 channels are built (dwn.h)
    g = torch.Generator().manual_seed(B + S + Cin)
    x = torch.empty(B, Cin, S)
    x[:, 0] = torch.randint(0, 256, (B, S), generator=g).float()
    for k in range(1, Cin):
        x[:, k] = (torch.randn(B, S, generator=g) * TRACE_SCALE[k - 1] + TRACE_SHIFT[k - 1]).clamp_min(0)
    w = torch.randn(C0, Cin, generator=g) * 0.02
    gamma = torch.rand(C0, generator=g) + 0.5
    beta = torch.randn(C0, generator=g) * 0.2
    M = B * S
    x64 = x.double().requires_grad_(True)
    w64, g64, b64 = (t.double().requires_grad_(True) for t in (w, gamma, beta))
    z = x64.permute(0, 2, 1).reshape(M, Cin) @ w64.t()
    y = F.batch_norm(z, None, None, g64, b64, True, 0.1, EPS)
    with torch.no_grad():
        invstd = 1.0 / torch.sqrt(z.var(0, unbiased=False) + EPS)
        zhat = (z - z.mean(0)) * invstd
        c = 1.0 + torch.rand(C0, generator=g).double()
        if kind == "mixed":
            d = torch.randn(M, C0, generator=g).double() + 0.5 * zhat + c
        elif kind == "const":
            d = c.expand(M, C0).clone()
        else:
            d = zhat.clone()
        dout = d.to(dtype)                    # the reference sees the rounded values: dout is exact in both dtypes
        d = dout.double()
        # the frozen-mode formula alone, W0^T diag(gamma invstd) dout, in float64
        first = torch.einsum("ck,c,bsc->bks", w64, g64 * invstd, d.view(B, S, C0))
    (y * d).sum().backward()
    return dict(shape=(B, S, Cin, C0), dtype=dtype, x=x, w=w, gamma=gamma, beta=beta, dout=dout, first=first, invstd=invstd,
                dx=x64.grad, dw=w64.grad, dgamma=g64.grad, dbeta=b64.grad)


def run_stem(case, entry, device=None):
    """dwn_stem_forward (DWN_BN_TRAIN) and then `entry` ('backward_input' or 'backward') on the case's tensors.
    Returns dict(dx (None for 'backward'), dw, dgamma, dbeta) on the GPU."""
    from sensorium_amd import _lib as L
    dev = device or torch.device("cuda", 0)
    B, S, Cin, C0 = case["shape"]
    dtype = case["dtype"]
    x, w, gamma, beta, dout = (case[k].to(dev).contiguous() for k in ("x", "w", "gamma", "beta", "dout"))
    rm, rv = torch.zeros(C0, device=dev), torch.ones(C0, device=dev)
    nbt = torch.zeros((), dtype=torch.int64, device=dev)
    coef = torch.empty(4 * C0, device=dev)
    xmom = torch.empty(72, dtype=torch.float64, device=dev)
    out = torch.empty(B * S, C0, dtype=dtype, device=dev)
    nan = float("nan")
    dw, dgamma, dbeta = torch.full((C0, Cin), nan, device=dev), torch.full((C0,), nan, device=dev), torch.full((C0,), nan, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    a = L.StemArgs()
    a.dtype = L.DWN_F32 if dtype == torch.float32 else L.DWN_BF16
    a.training = L.BN_TRAIN; a.B = B; a.Cin = Cin; a.C0 = C0; a.S = S; a.eps = EPS; a.momentum = 0.1
    a.x = x.data_ptr(); a.w = w.data_ptr(); a.out = out.data_ptr(); a.xmom = xmom.data_ptr()
    a.bn.gamma = gamma.data_ptr(); a.bn.beta = beta.data_ptr(); a.bn.running_mean = rm.data_ptr(); a.bn.running_var = rv.data_ptr()
    a.bn.num_batches_tracked = nbt.data_ptr(); a.bn.coef = coef.data_ptr()
    ws = torch.empty(L.lib.dwn_stem_workspace_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
    L.check(L.lib.dwn_stem_forward(C.byref(a), dev.index, stream), "dwn_stem_forward")
    a.bn.dgamma = dgamma.data_ptr(); a.bn.dbeta = dbeta.data_ptr(); a.dout = dout.data_ptr(); a.dw = dw.data_ptr()
    dx = None
    if entry == "backward_input":
        dx = torch.full((B, Cin, S), nan, device=dev)
        L.check(L.lib.dwn_stem_backward_input(C.byref(a), dx.data_ptr(), dev.index, stream), "dwn_stem_backward_input")
    else:
        L.check(L.lib.dwn_stem_backward(C.byref(a), dev.index, stream), "dwn_stem_backward")
    torch.cuda.synchronize()
    return dict(dx=dx, dw=dw, dgamma=dgamma, dbeta=dbeta)

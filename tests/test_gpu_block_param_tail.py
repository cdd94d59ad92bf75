"""The parameter-gradient tail of dwn_block_backward: the SE MLP's parameter gradients and conv_pw's weight-gradient fold run as ONE
launch at the end of the block (csrc/dwn_elementwise.hip block_param_tail_kernel) instead of two stream-ordered ones inside it.

The block is InvertedResidual3d (src/models/dwiseneuro.py:70-144); the two gradients are those of SqueezeExcite3d's 1x1x1 convs
(:25-43) and of conv_pw (:90-93).  Checked through dwn_block_backward itself, on tiny geometries (B = 2, T = 2):

  * dw_pw must be BIT-IDENTICAL to what the public dwn_pw_backward entry — which still folds in a launch of its own — writes for the
    same dh1, a0 and BatchNorm-1 backward coefficients (at these sizes at most two workgroups add to an element of the raw products,
    and a + b = b + a, so the raw products themselves are reproducible);
  * dse_wr / dse_br / dse_we / dse_be must match their closed form in float64, dwe[c][r] = sum_b dgp[b][c] silu(hid[b][r]),
    dwr[r][c] = sum_b dhp[b][r] pmean[b][c], dbe = sum_b dgp, dbr = sum_b dhp, within the bounds tests/test_gpu_block.py holds these
    gradients to (norm-relative 1e-3 in fp32, 8e-2 in bf16).

dh1, the coefficients and (dgp, dhp) are internals of the call: the test hands dwn_block_backward a workspace and a scratch buffer of
its own and reads them back from the places carve_block (csrc/dwn_api.hip) gives them; a layout change fails the sanity check on the
coefficients' first row (A1 = BatchNorm-1's scale) before anything else."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_helpers import dev, rel, stream  # noqa: E402
from tests.test_gpu_block import make_block  # noqa: E402

CASES = [
    # cin, cout, stride, exp, se_ratio, B, T, H, W        (fold tile width / se_r / what else the case is for)
    (64, 64, 1, 7, 32, 2, 2, 4, 4),          # 64 / 14
    (128, 128, 1, 7, 32, 2, 2, 5, 3),        # 128 / 28
    (256, 256, 1, 7, 32, 2, 2, 4, 4),        # 256 / 56
    (64, 128, 2, 7, 32, 2, 2, 5, 3),         # stride 2
    (64, 64, 1, 7, 64, 2, 2, 4, 4),          # se_r = 7: odd, the SE kernels that are not the rows variant
    (64, 64, 1, 7, 32, 2, 2, 4, 8),          # 128 input rows: the one-pass conv_pw backward with the shortcut folded in (dx written by
                                             # it, the early return of old), and in bf16 the y1-free forward (the streaming Gram kernel)
]


def _carve_backward(a, ts):
    """byte offsets of (abc1, dgp, dhp) in the backward workspace: csrc/dwn_api.hip carve_block, backward = 1"""
    off = 0

    def take(nbytes):
        nonlocal off
        off = (off + 255) & ~255
        p = off
        off += nbytes
        return p
    take(a.Cmid * a.Cin * ts); take(a.Cout * a.Cmid * ts); take(a.ks * a.ks * a.Cmid * 4); take(a.kt * a.Cmid * 4); take(0)
    nstat = 32 * 2 * 8                           # DWN_NREP replicas of (sum, sum of squares), doubles
    for c in (a.Cmid, a.Cmid, a.Cmid, a.Cout, a.Cout):
        take(nstat * c)
    take(a.B * a.Cmid * 8)
    abc1 = take(12 * a.Cmid); take(12 * a.Cmid); take(12 * a.Cmid); take(12 * a.Cout); take(12 * a.Cout); take(12 * a.Cmid)
    dgp = take(4 * a.B * a.Cmid)
    dhp = take(4 * a.B * a.se_r)
    return abc1, dgp, dhp


@pytest.mark.parametrize("pwl_bwd", [1, 2], ids=["per-sample", "materialised-du"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bfloat16", "float32"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_block_backward_parameter_tail(monkeypatch, case, dtype, pwl_bwd):
    import sensorium_amd._lib as L
    from sensorium_amd import ops
    cin, cout, stride, exp, ser, B, T, H, W = case
    blk, pe = make_block(cin, cout, stride, exp, ser, seed=cin + stride)
    blk, pe = blk.to(dev()).train(), pe.to(dev())
    blk._capture = True
    Cmid, R = blk.mid_features, blk.se.conv_reduce.out_channels
    assert R == Cmid // ser
    ts = 2 if dtype == torch.bfloat16 else 4

    held = {}
    real = L.lib.dwn_block_backward

    def block_backward(ref, device, s):
        a = ref._obj                              # the dwn_block_args ops.BlockFn.backward filled: swap in buffers the test keeps
        m_in, m_out = a.B * a.T * a.Hin * a.Win, a.B * a.T * a.Hout * a.Wout
        held["buf_a"] = torch.empty(max(m_in, m_out) * a.Cmid, dtype=dtype, device=dev())
        held["ws"] = torch.empty(a.ws_bytes, dtype=torch.uint8, device=dev())
        a.buf_a, a.ws = held["buf_a"].data_ptr(), held["ws"].data_ptr()
        held["offsets"] = _carve_backward(a, ts)
        held["m_in"] = m_in
        return real(ref, device, s)

    monkeypatch.setattr(ops, "_PWL_BWD", pwl_bwd)
    monkeypatch.setattr(L.lib, "dwn_block_backward", block_backward)
    torch.manual_seed(1)
    x = (torch.randn(B, T, H, W, cin, device=dev()) * 1.5 + 0.3).to(dtype).requires_grad_(True)
    out = blk(x, pe, dtype, x_has_pe=True)        # x is the block input including its positional encoding: a0 itself
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(7)).to(dev()).to(dtype)
    out.backward(gout)
    torch.cuda.synchronize()
    assert held, "dwn_block_backward was not reached"

    ws, (o_abc, o_dgp, o_dhp), m_in = held["ws"], held["offsets"], held["m_in"]
    f32 = lambda o, n: ws[o:o + 4 * n].view(torch.float32).clone()
    abc1 = f32(o_abc, 3 * Cmid)
    coef1 = blk._captured["coefs"][0]
    assert torch.equal(abc1[:Cmid], coef1[:Cmid]), "the workspace layout this test reads is not carve_block's"

    # ---- dw_pw: the public entry, separate fold launch, same dh1 / a0 / coefficients
    dh1 = held["buf_a"][:m_in * Cmid]
    w_pw = blk.conv_pw[0].weight
    da0 = torch.empty(m_in * cin, dtype=dtype, device=dev())
    dw = torch.full((Cmid, cin), float("nan"), device=dev())
    dt = L.DWN_BF16 if dtype == torch.bfloat16 else L.DWN_F32
    nws = L.lib.dwn_pw_backward_workspace_bytes(Cmid, cin, dt)
    ws2 = torch.empty(nws, dtype=torch.uint8, device=dev())
    a = L.PwBwdArgs()
    a.dh1, a.a0, a.w_pw, a.abc = dh1.data_ptr(), x.data_ptr(), w_pw.data_ptr(), abc1.data_ptr()
    a.da0, a.dw, a.M, a.E, a.Cin, a.ws, a.ws_bytes = da0.data_ptr(), dw.data_ptr(), m_in, Cmid, cin, ws2.data_ptr(), nws
    L.check(L.lib.dwn_pw_backward(C.byref(a), dt, 0, stream()), "pw_backward")
    torch.cuda.synchronize()
    mine = w_pw.grad.reshape(Cmid, cin)
    assert torch.isfinite(mine).all() and float(mine.abs().max()) > 0
    assert torch.equal(mine, dw), f"dw_pw differs from the stand-alone fold: {float((mine - dw).abs().max()):.3e}"

    # ---- SE parameter gradients: closed form in float64 from what the kernel reads
    dgp = f32(o_dgp, B * Cmid).view(B, Cmid).double()
    dhp = f32(o_dhp, B * R).view(B, R).double()
    pmean, hid = blk._captured["pmean"].double(), blk._captured["hidpre"].double()
    want = {"we": dgp.t() @ (hid * torch.sigmoid(hid)), "wr": dhp.t() @ pmean, "be": dgp.sum(0), "br": dhp.sum(0)}
    got = {"we": blk.se.conv_expand.weight.grad.reshape(Cmid, R), "wr": blk.se.conv_reduce.weight.grad.reshape(R, Cmid),
           "be": blk.se.conv_expand.bias.grad, "br": blk.se.conv_reduce.bias.grad}
    bound = 1e-3 if dtype == torch.float32 else 8e-2
    for k in ("we", "wr", "be", "br"):
        assert float(want[k].abs().max()) > 0, k
        e = rel(got[k], want[k])
        assert e < bound, f"dse_{k}: rel err {e:.3e}"

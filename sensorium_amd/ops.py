"""torch.autograd.Function wrappers over the C-ABI composites of libdwiseneuro_hip.so.

One Function per reference module on the hot path (src/models/dwiseneuro.py): stem, [PositionalEncoding3d +
InvertedResidual3d], pool, ShuffleLayer, Readout, and MicePoissonLoss (src/losses.py).  PyTorch is plumbing
here: it owns device memory (every buffer, saved tensor and workspace is a torch tensor), the stream, and the
autograd graph; all arithmetic runs in the hand-written HIP kernels.  There is no fallback path: tensors must
live on a GPU and the shared library must be present.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from typing import Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib as L

_DT = {torch.float32: L.DWN_F32, torch.bfloat16: L.DWN_BF16}


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream(device: torch.device):
    return torch.cuda.current_stream(device).cuda_stream


def _require_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"sensorium_amd.{what}: tensors must be on a GPU (got {t.device}); "
                           "the HIP path has no CPU fallback")


def _bn_struct(bn: torch.nn.modules.batchnorm._BatchNorm, coef: torch.Tensor, dgamma=None, dbeta=None) -> L.BN:
    s = L.BN()
    s.gamma = bn.weight.data_ptr()
    s.beta = bn.bias.data_ptr()
    s.running_mean = bn.running_mean.data_ptr()
    s.running_var = bn.running_var.data_ptr()
    s.num_batches_tracked = bn.num_batches_tracked.data_ptr()
    s.coef = coef.data_ptr()
    s.dgamma = _ptr(dgamma)
    s.dbeta = _ptr(dbeta)
    return s


def _check_bn(bn):
    if bn.momentum is None or not bn.affine or not bn.track_running_stats:
        raise RuntimeError("sensorium_amd: BatchNorm must be affine with running stats and a fixed momentum")


def _f32_products(mod, inference_readout: bool = False) -> int:
    """How this module's fp32 GEMMs multiply (include/dwn.h DWN_F32_*).  ``DwiseNeuro.set_fp32_eval_products`` stamps the
    choice on its sub-modules: "bf16x3" (default: eval-mode forward as three bf16 products, 5.8e-7 from native; training always
    native) or "native" (fp32 MFMA everywhere)."""
    native = getattr(mod, "_dwn_fp32_native", False)
    if inference_readout:               # the readout's C struct has no training flag: the caller says what this forward is
        return L.F32_NATIVE if native else L.F32_SPLIT3
    return L.F32_NATIVE if native else L.F32_AUTO


# ------------------------------------------------------------------------------------------------
# BatchNorm mode of a forward (include/dwn.h DWN_BN_*)
# ------------------------------------------------------------------------------------------------
_EVAL_BACKWARD_ERROR = "sensorium_amd: backward through eval-mode BatchNorm is not built"


class _BnModeState(threading.local):
    override: Optional[int] = None      # set by DwiseNeuro.trunk for the modules it calls: the model decides once, from ITS input


_BN_MODE = _BnModeState()


class bn_mode_scope:
    """``with bn_mode_scope(mode):`` — the eval-mode modules called inside take ``mode`` (L.BN_EVAL or L.BN_FROZEN) instead of
    deciding from their own input.  DwiseNeuro uses it so that a whole forward runs in one mode: an inner activation requires
    grad whenever a parameter does, which says nothing about what the caller wants."""

    def __init__(self, mode: Optional[int]):
        self.mode = mode

    def __enter__(self):
        self.prev, _BN_MODE.override = _BN_MODE.override, self.mode
        return self

    def __exit__(self, *exc):
        _BN_MODE.override = self.prev
        return False


def wants_frozen(x: torch.Tensor, switch: bool = False) -> bool:
    """Does an eval-mode forward of ``x`` keep what a backward needs?  Only when autograd is recording AND (the input itself needs
    a gradient, or the caller asked for frozen-statistics fine-tuning).  Everything else — ``no_grad`` predictors, validation,
    hipGraph capture, eval forwards of plain data — stays on the eval kernels."""
    return torch.is_grad_enabled() and (bool(x.requires_grad) or switch)


def bn_mode(training: bool, x: torch.Tensor) -> int:
    """The BatchNorm mode of one module call; evaluated in the module's ``forward`` (inside an autograd Function grad mode is
    off and says nothing)."""
    if training:
        return L.BN_TRAIN
    if _BN_MODE.override is not None:
        return _BN_MODE.override
    return L.BN_FROZEN if wants_frozen(x) else L.BN_EVAL


def _ddp_flush() -> None:
    from . import ddp
    if ddp._LIVE:
        ddp.flush_ready_all()


def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


# conv_pwl backward implementation forced for a process (the block / model parity tests are re-run under both): "new" =
# per-sample products + recompute epilogue, "old" = materialised du; unset = the library chooses by shape
def _env_choice(name: str, table: dict) -> int:
    v = os.environ.get(name, "")
    if v not in table:
        raise ValueError(f"{name}={v!r}: expected one of {sorted(k for k in table if k)} (or unset)")
    return table[v]


_PWL_BWD = _env_choice("DWN_PWL_BWD", {"": 0, "new": 1, "old": 2})
# dwn_block_args.y1_mode: "" = the library leaves y1 (conv_pw's output) unmaterialised in bf16 training where both stencils rebuild it
# from the block input; DWN_Y1=materialise forces the stored-y1 path (the parity tests run both; same-box A/B runs)
_Y1_MODE = _env_choice("DWN_Y1", {"": 0, "free": 0, "materialise": 1, "all": 2})


def grad_out(param: torch.Tensor, zero: bool = False) -> torch.Tensor:
    """The fp32 tensor a backward kernel writes ``param``'s gradient into.  Under data parallelism ``GradBuckets`` gives
    every parameter a slice of a flat all-reduce bucket (``param._dwn_grad_slot``): the gradient is produced *there* — a
    fresh view object, so autograd adopts it as ``param.grad`` without a copy and the bucket needs no gather pass.  When a
    gradient is already being accumulated (``param.grad`` set: argus ``iter_size`` > 1) or no bucket exists, a new tensor in
    the parameter's own shape (same memory layout as the kernels' 2-D views, so autograd can take ownership)."""
    slot = getattr(param, "_dwn_grad_slot", None)
    if slot is not None and param.grad is None and not getattr(param, "_dwn_slot_out", False):
        # handed out ONCE per backward pass: a second producer of the same parameter's gradient (a module applied twice, two
        # forwards summed into one loss) gets a tensor of its own — two kernels writing the same slot before AccumulateGrad
        # adds them would leave 2x the last contribution.  GradBuckets' hook clears the mark when the gradient has arrived.
        param._dwn_slot_out = True
        flat, off = slot
        g = flat[off:off + param.numel()].view(param.shape)
        return g.zero_() if zero else g
    if zero:
        return torch.zeros_like(param, dtype=torch.float32)
    return torch.empty_like(param, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------
# index maps / positional-encoding tables (host side, cached by the modules)
# ------------------------------------------------------------------------------------------------
def nearest_src_index(out_size: int, in_size: int) -> np.ndarray:
    """F.interpolate(mode='nearest') source index (reference: dwiseneuro.py:127-129)."""
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(src, in_size - 1).astype(np.int32)


def inverse_index(src: np.ndarray, in_size: int) -> np.ndarray:
    inv = np.full(in_size, -1, dtype=np.int32)
    inv[src] = np.arange(len(src), dtype=np.int32)
    if len(np.unique(src)) != len(src):
        raise RuntimeError("nearest-neighbour shortcut map is not injective (stride < 1?)")
    return inv


def pe_axis_tables(channels: int, inv_freq: torch.Tensor, t: int, h: int, w: int):
    """Separable positional-encoding tables PT[t][C], PH[h][C], PW[w][C] (reference: dwiseneuro.py:163-182):
    enc[c](t,h,w) = PT[t][c] + PH[h][c] + PW[w][c] where every channel depends on exactly one axis."""
    ch = int(math.ceil(channels / 6) * 2)
    if ch % 2:
        ch += 1
    inv = inv_freq.detach().float().cpu()
    tabs = []
    for axis, size in enumerate((t, h, w)):
        arg = inv[:, None] * torch.arange(size).float()[None, :]
        emb = torch.cat([arg.sin(), arg.cos()], dim=0)              # [ch, size]
        tab = torch.zeros(size, channels, dtype=torch.float32)
        lo = axis * ch
        n = max(0, min(ch, channels - lo))
        if n > 0:
            tab[:, lo:lo + n] = emb[:n].t()
        tabs.append(tab.contiguous())
    return tabs


# ------------------------------------------------------------------------------------------------
# stem
# ------------------------------------------------------------------------------------------------
class StemFn(torch.autograd.Function):
    """Conv3d(C_in->C0, 1x1x1, bias=False) + BatchNorm3d on the NCDHW fp32 input (dwiseneuro.py:306-309).
    Returns the channels-last activation [B,T,H,W,C0] in the compute dtype."""

    @staticmethod
    def forward(ctx, x, weight, gamma, beta, mod, dtype, pe=None, mode=None):
        _require_gpu(x, "StemFn")
        conv, bn = mod.stem[0], mod.stem[1].bn
        _check_bn(bn)
        if mode is None:             # direct callers: training -> batch statistics, eval -> running statistics, no backward
            mode = int(bn.training)
        x = x.contiguous().float()
        B, Cin, T, H, W = x.shape
        C0 = weight.shape[0]
        dev = x.device
        out = torch.empty(B, T, H, W, C0, dtype=dtype, device=dev)
        coef = torch.empty(4 * C0, dtype=torch.float32, device=dev)
        # the input moments (sum x, sum x x^T): what the backward needs instead of the raw conv output (never materialised)
        xmom = torch.empty(72, dtype=torch.float64, device=dev)
        a = L.StemArgs()
        a.dtype = _DT[dtype]; a.training = mode; a.B = B; a.Cin = Cin; a.C0 = C0; a.S = T * H * W
        a.eps = bn.eps; a.momentum = bn.momentum
        a.x = x.data_ptr(); a.w = weight.data_ptr(); a.bn = _bn_struct(bn, coef)
        a.out = out.data_ptr(); a.xmom = xmom.data_ptr()
        if pe is not None:       # positional encoding of the first block, folded into the stem's output pass
            a.pe_t, a.pe_h, a.pe_w = (t.data_ptr() for t in pe)
        a.T, a.H, a.W = T, H, W
        ws = _ws(L.lib.dwn_stem_workspace_bytes(C.byref(a)), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_stem_forward(C.byref(a), dev.index, _stream(dev)), "dwn_stem_forward")
        ctx.mod = mod; ctx.dtype = dtype; ctx.mode = mode
        ctx.save_for_backward(x, weight, xmom, coef)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, weight, xmom, coef = ctx.saved_tensors
        if ctx.mode == L.BN_EVAL:
            raise RuntimeError(_EVAL_BACKWARD_ERROR)
        bn = ctx.mod.stem[1].bn
        dev = x.device
        B, Cin, T, H, W = x.shape
        C0 = weight.shape[0]
        dout = dout.contiguous()
        dx = None
        if ctx.needs_input_grad[0] and ctx.mode == L.BN_FROZEN:
            dx = torch.empty_like(x)
            g = L.StemInputGradArgs()
            g.dtype = _DT[ctx.dtype]; g.training = ctx.mode; g.B = B; g.Cin = Cin; g.C0 = C0; g.S = T * H * W
            g.w = weight.data_ptr(); g.coef = coef.data_ptr(); g.dout = dout.data_ptr(); g.dx = dx.data_ptr()
            L.check(L.lib.dwn_stem_input_grad(C.byref(g), dev.index, _stream(dev)), "dwn_stem_input_grad")
            if not any(ctx.needs_input_grad[1:4]):      # input gradient only (parameters frozen by the caller)
                return dx, None, None, None, None, None, None, None
        dw = grad_out(ctx.mod.stem[0].weight)
        dgamma = grad_out(bn.weight)
        dbeta = grad_out(bn.bias)
        a = L.StemArgs()
        a.dtype = _DT[ctx.dtype]; a.training = ctx.mode; a.B = B; a.Cin = Cin; a.C0 = C0; a.S = T * H * W
        a.eps = bn.eps; a.momentum = bn.momentum
        a.x = x.data_ptr(); a.w = weight.data_ptr(); a.bn = _bn_struct(bn, coef, dgamma, dbeta)
        a.xmom = xmom.data_ptr(); a.dout = dout.data_ptr(); a.dw = dw.data_ptr()
        ws = _ws(L.lib.dwn_stem_workspace_bytes(C.byref(a)), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        if ctx.needs_input_grad[0] and ctx.mode == L.BN_TRAIN:
            # through the batch statistics: parameter gradients and dx from one accumulation pass over dout (with the stem's
            # parameters frozen by the caller, dw / dgamma / dbeta above are temporaries that autograd drops)
            dx = torch.empty_like(x)
            L.check(L.lib.dwn_stem_backward_input(C.byref(a), dx.data_ptr(), dev.index, _stream(dev)), "dwn_stem_backward_input")
        else:
            L.check(L.lib.dwn_stem_backward(C.byref(a), dev.index, _stream(dev)), "dwn_stem_backward")
        return dx, dw, dgamma, dbeta, None, None, None, None


# ------------------------------------------------------------------------------------------------
# PositionalEncoding3d + InvertedResidual3d
# ------------------------------------------------------------------------------------------------
_BLOCK_PARAMS = ("w_pw", "g1", "b1", "w_dws", "g2", "b2", "w_dwt", "g3", "b3", "se_wr", "se_br", "se_we", "se_be",
                 "w_pwl", "g4", "b4", "gsc", "bsc")


def _block_args(blk, geom, x, dtype, training, coefs, saved, drop_scale, x_has_pe, a0):
    """Fill the fields shared by forward and backward."""
    B, T, Hin, Win, Cin = x.shape
    a = L.BlockArgs()
    a.dtype = _DT[dtype]; a.training = int(training)
    a.B = B; a.T = T; a.Hin = Hin; a.Win = Win
    a.Hout = (Hin - 1) // blk.spatial_stride + 1
    a.Wout = (Win - 1) // blk.spatial_stride + 1
    a.Cin = Cin; a.Cmid = blk.mid_features; a.Cout = blk.out_features
    a.stride = blk.spatial_stride; a.ks = blk.spatial_kernel; a.kt = blk.temporal_kernel
    a.se_r = blk.se.conv_reduce.out_channels
    bn1 = blk.conv_pw[1].bn
    a.eps = bn1.eps; a.momentum = bn1.momentum
    a.x = x.data_ptr()
    a.x_has_pe = int(x_has_pe)
    a.a0 = _ptr(a0)
    pe_t, pe_h, pe_w, hsrc, wsrc, hinv, winv = geom
    a.pe_t = pe_t.data_ptr(); a.pe_h = pe_h.data_ptr(); a.pe_w = pe_w.data_ptr()
    a.hsrc = hsrc.data_ptr(); a.wsrc = wsrc.data_ptr(); a.hinv = hinv.data_ptr(); a.winv = winv.data_ptr()
    a.w_pw = blk.conv_pw[0].weight.data_ptr()
    a.w_dws = blk.spat_covn_dw[0].weight.data_ptr()
    a.w_dwt = blk.temp_covn_dw[0].weight.data_ptr()
    a.w_pwl = blk.conv_pwl[0].weight.data_ptr()
    a.se_wr = blk.se.conv_reduce.weight.data_ptr(); a.se_br = blk.se.conv_reduce.bias.data_ptr()
    a.se_we = blk.se.conv_expand.weight.data_ptr(); a.se_be = blk.se.conv_expand.bias.data_ptr()
    a.drop_scale = _ptr(drop_scale)
    a.se_pmean = saved["pmean"].data_ptr(); a.se_hidpre = saved["hidpre"].data_ptr()
    a.se_gate = saved["gate"].data_ptr()
    a.f32_products = _f32_products(blk)
    a.y1_mode = getattr(blk, "_dwn_y1_mode", _Y1_MODE)
    return a


class BlockFn(torch.autograd.Function):
    """x -> InvertedResidual3d(x + PositionalEncoding3d) (dwiseneuro.py:136-144, 184-192), channels-last."""

    @staticmethod
    def forward(ctx, x, drop_scale, blk, geom, dtype, x_has_pe, out_pe, mode, *params):
        _require_gpu(x, "BlockFn")
        x = x.contiguous()
        dev = x.device
        B, T, Hin, Win, Cin = x.shape
        s = blk.spatial_stride
        Hout, Wout = (Hin - 1) // s + 1, (Win - 1) // s + 1
        Cmid, Cout = blk.mid_features, blk.out_features
        bns = blk.bn_modules()
        for bn in bns:
            _check_bn(bn)
        # mode: include/dwn.h DWN_BN_*, decided by the module's forward (bn_mode: grad mode is not visible in here)
        training = mode          # the C struct's `training` field
        f32 = dict(dtype=torch.float32, device=dev)
        y2 = torch.empty(B, T, Hout, Wout, Cmid, dtype=dtype, device=dev)
        z3 = torch.empty_like(y2)
        a0 = None if x_has_pe else torch.empty_like(x)
        y4 = torch.empty(B, T, Hout, Wout, Cout, dtype=dtype, device=dev)
        out = torch.empty_like(y4)
        coefs = [torch.empty(4 * c, **f32) for c in (Cmid, Cmid, Cmid, Cout, Cout)]
        R = blk.se.conv_reduce.out_channels
        saved = dict(pmean=torch.empty(B, Cmid, **f32), hidpre=torch.empty(B, R, **f32),
                     gate=torch.empty(B, Cmid, **f32))
        a = _block_args(blk, geom, x, dtype, training, coefs, saved, drop_scale, x_has_pe, a0)
        a.out = out.data_ptr()
        # y1 is not written where the stencils rebuild it (eval; bf16 training where both directions are built: the backward then
        # gets no y1 either), y3 not where the eval-mode temporal pass emits z3 directly
        writes = L.lib.dwn_block_forward_writes(C.byref(a))
        L.check(min(writes, 0), "dwn_block_forward_writes")      # a refused geometry answers its negative code, not a write set
        y1 = torch.empty(B, T, Hin, Win, Cmid, dtype=dtype, device=dev) if writes & 1 else None
        y3 = torch.empty_like(y2) if writes & 2 else None
        a.y1 = _ptr(y1); a.y2 = y2.data_ptr(); a.y3 = _ptr(y3); a.y4 = y4.data_ptr()
        a.z3 = z3.data_ptr()
        if out_pe is not None:   # next block's positional encoding, folded into this block's residual pass
            a.out_pe_t, a.out_pe_h, a.out_pe_w = (t.data_ptr() for t in out_pe)
        a.bn1, a.bn2, a.bn3, a.bn4, a.bnsc = (_bn_struct(bn, cf) for bn, cf in zip(bns, coefs))
        ws = _ws(L.lib.dwn_block_workspace_bytes(C.byref(a), 0), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_block_forward(C.byref(a), dev.index, _stream(dev)), "dwn_block_forward")
        ctx.blk = blk; ctx.geom = geom; ctx.dtype = dtype; ctx.mode = mode
        if getattr(blk, "_capture", False):        # test hook: expose the raw intermediates
            blk._captured = dict(y1=y1, y2=y2, y3=y3, y4=y4, z3=z3, coefs=coefs, **saved)
        ctx.has_drop = drop_scale is not None
        # the block input *including* its positional encoding is what backward needs
        if mode == L.BN_EVAL:         # no backward through eval-mode BatchNorm: nothing to keep
            return out
        tensors = [x if x_has_pe else a0, y1, y2, y3, y4, *coefs, saved["pmean"], saved["hidpre"], saved["gate"], z3]
        if drop_scale is not None:
            tensors.append(drop_scale)
        ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.mode == L.BN_EVAL:
            raise RuntimeError(_EVAL_BACKWARD_ERROR)
        blk, dtype = ctx.blk, ctx.dtype
        t = ctx.saved_tensors
        x, y1, y2, y3, y4 = t[:5]
        coefs = list(t[5:10])
        saved = dict(pmean=t[10], hidpre=t[11], gate=t[12])
        z3 = t[13]
        drop_scale = t[14] if ctx.has_drop else None
        dev = x.device
        dout = dout.contiguous()
        B, T, Hin, Win, Cin = x.shape
        Hout, Wout = y2.shape[2], y2.shape[3]
        Cmid, Cout = blk.mid_features, blk.out_features
        f32 = dict(dtype=torch.float32, device=dev)
        a = _block_args(blk, ctx.geom, x, dtype, ctx.mode, coefs, saved, drop_scale, True, None)
        a.y1 = _ptr(y1); a.y2 = y2.data_ptr(); a.y3 = y3.data_ptr(); a.y4 = y4.data_ptr()      # (y1 is None on a y1-free block)
        a.z3 = z3.data_ptr()
        bns = blk.bn_modules()
        dg = [grad_out(bn.weight) for bn in bns]
        db = [grad_out(bn.bias) for bn in bns]
        a.bn1, a.bn2, a.bn3, a.bn4, a.bnsc = (_bn_struct(bn, cf, g_, b_) for bn, cf, g_, b_ in zip(bns, coefs, dg, db))
        m_in, m_out = B * T * Hin * Win, B * T * Hout * Wout
        buf_a = torch.empty(max(m_in, m_out) * Cmid, dtype=dtype, device=dev)
        buf_b = torch.empty(m_out * Cmid, dtype=dtype, device=dev)
        dy4 = torch.empty(m_out * Cout, dtype=dtype, device=dev)
        da0 = torch.empty(m_in * Cin, dtype=dtype, device=dev)
        dx = torch.empty_like(x)
        R = blk.se.conv_reduce.out_channels
        # gradients are allocated in the parameters' own shapes (same memory layout as the kernels' 2-D views) so
        # that autograd can take ownership instead of cloning a view
        # (dwn_block_backward clears the four atomically accumulated weight gradients itself, in its prep launch)
        # ... or, under data parallelism, straight into the parameters' slices of the all-reduce buckets (grad_out)
        dw_pw = grad_out(blk.conv_pw[0].weight)
        dw_dws = grad_out(blk.spat_covn_dw[0].weight)
        dw_dwt = grad_out(blk.temp_covn_dw[0].weight)
        dw_pwl = grad_out(blk.conv_pwl[0].weight)
        dse_wr = grad_out(blk.se.conv_reduce.weight); dse_br = grad_out(blk.se.conv_reduce.bias)
        dse_we = grad_out(blk.se.conv_expand.weight); dse_be = grad_out(blk.se.conv_expand.bias)
        a.dout = dout.data_ptr(); a.dx = dx.data_ptr()
        a.buf_a = buf_a.data_ptr(); a.buf_b = buf_b.data_ptr(); a.dy4 = dy4.data_ptr(); a.da0 = da0.data_ptr()
        a.dw_pw = dw_pw.data_ptr(); a.dw_dws = dw_dws.data_ptr(); a.dw_dwt = dw_dwt.data_ptr()
        a.dw_pwl = dw_pwl.data_ptr()
        a.dse_wr = dse_wr.data_ptr(); a.dse_br = dse_br.data_ptr(); a.dse_we = dse_we.data_ptr()
        a.dse_be = dse_be.data_ptr()
        a.pwl_bwd = _PWL_BWD                       # before the workspace is sized: the per-sample path carves B x Cout x Cmid floats
        ws = _ws(L.lib.dwn_block_workspace_bytes(C.byref(a), 1), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_block_backward(C.byref(a), dev.index, _stream(dev)), "dwn_block_backward")
        _ddp_flush()            # this block's kernels are queued: a good moment for the host to start pending gradient exchanges
        grads = (dw_pw, dg[0], db[0], dw_dws, dg[1], db[1], dw_dwt, dg[2], db[2], dse_wr, dse_br, dse_we, dse_be,
                 dw_pwl, dg[3], db[3], dg[4], db[4])
        return (dx, None, None, None, None, None, None, None) + grads


# ------------------------------------------------------------------------------------------------
# pool
# ------------------------------------------------------------------------------------------------
class PoolFn(torch.autograd.Function):
    """AdaptiveAvgPool3d((None,1,1)) + squeeze (dwiseneuro.py:374,400): [B,T,H,W,C] -> [B,T,C]."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x, "PoolFn")
        x = x.contiguous()
        B, T, H, W, Cc = x.shape
        out = torch.empty(B, T, Cc, dtype=x.dtype, device=x.device)
        a = L.PoolArgs()
        a.dtype = _DT[x.dtype]; a.BT = B * T; a.HW = H * W; a.C = Cc; a.x = x.data_ptr(); a.out = out.data_ptr()
        L.check(L.lib.dwn_pool_forward(C.byref(a), x.device.index, _stream(x.device)), "dwn_pool_forward")
        ctx.shape = (B, T, H, W, Cc)
        return out

    @staticmethod
    def backward(ctx, dout):
        B, T, H, W, Cc = ctx.shape
        dout = dout.contiguous()
        dx = torch.empty(B, T, H, W, Cc, dtype=dout.dtype, device=dout.device)
        a = L.PoolArgs()
        a.dtype = _DT[dout.dtype]; a.BT = B * T; a.HW = H * W; a.C = Cc; a.dout = dout.data_ptr(); a.dx = dx.data_ptr()
        L.check(L.lib.dwn_pool_backward(C.byref(a), dout.device.index, _stream(dout.device)), "dwn_pool_backward")
        return dx


# ------------------------------------------------------------------------------------------------
# cortex ShuffleLayer
# ------------------------------------------------------------------------------------------------
class CortexFn(torch.autograd.Function):
    """ShuffleLayer.forward (dwiseneuro.py:228-234) on [B,T,C_in] -> [B,T,C]."""

    @staticmethod
    def forward(ctx, x, drop_scale, layer, dtype, mode, weight, g, b, gsc, bsc):
        _require_gpu(x, "CortexFn")
        x = x.contiguous()
        dev = x.device
        B, T, Cin = x.shape
        Cc = layer.out_features
        bn, bnsc = layer.bn.bn, layer.bn_sc.bn
        _check_bn(bn); _check_bn(bnsc)
        y = torch.empty(B, T, Cc, dtype=dtype, device=dev)
        out = torch.empty_like(y)
        coef = torch.empty(4 * Cc, dtype=torch.float32, device=dev)
        coefsc = torch.empty(4 * Cc, dtype=torch.float32, device=dev)
        a = L.CortexArgs()
        a.dtype = _DT[dtype]; a.training = mode; a.B = B; a.T = T; a.Cin = Cin; a.C = Cc
        a.groups = layer.groups; a.eps = bn.eps; a.momentum = bn.momentum
        a.x = x.data_ptr(); a.out = out.data_ptr(); a.y = y.data_ptr(); a.w = weight.data_ptr()
        a.bn = _bn_struct(bn, coef); a.bnsc = _bn_struct(bnsc, coefsc); a.drop_scale = _ptr(drop_scale)
        a.f32_products = _f32_products(layer)
        ws = _ws(L.lib.dwn_cortex_workspace_bytes(C.byref(a), 0), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_cortex_forward(C.byref(a), dev.index, _stream(dev)), "dwn_cortex_forward")
        ctx.layer = layer; ctx.dtype = dtype; ctx.mode = mode; ctx.has_drop = drop_scale is not None
        tensors = [x, y, coef, coefsc, weight]
        if drop_scale is not None:
            tensors.append(drop_scale)
        ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.mode == L.BN_EVAL:
            raise RuntimeError(_EVAL_BACKWARD_ERROR)
        layer, dtype = ctx.layer, ctx.dtype
        t = ctx.saved_tensors
        x, y, coef, coefsc, weight = t[:5]
        drop_scale = t[5] if ctx.has_drop else None
        dev = x.device
        dout = dout.contiguous()
        B, T, Cin = x.shape
        Cc = layer.out_features
        bn, bnsc = layer.bn.bn, layer.bn_sc.bn
        f32 = dict(dtype=torch.float32, device=dev)
        dgm, dbm, dgs, dbs = grad_out(bn.weight), grad_out(bn.bias), grad_out(bnsc.weight), grad_out(bnsc.bias)
        dw = grad_out(layer.conv.weight)             # cleared by dwn_cortex_backward's prep launch
        dx = torch.empty_like(x)
        a = L.CortexArgs()
        a.dtype = _DT[dtype]; a.training = ctx.mode; a.B = B; a.T = T; a.Cin = Cin; a.C = Cc
        a.groups = layer.groups; a.eps = bn.eps; a.momentum = bn.momentum
        a.x = x.data_ptr(); a.y = y.data_ptr(); a.w = weight.data_ptr()
        a.bn = _bn_struct(bn, coef, dgm, dbm); a.bnsc = _bn_struct(bnsc, coefsc, dgs, dbs)
        a.drop_scale = _ptr(drop_scale)
        a.dout = dout.data_ptr(); a.dx = dx.data_ptr(); a.dw = dw.data_ptr()
        ws = _ws(L.lib.dwn_cortex_workspace_bytes(C.byref(a), 1), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_cortex_backward(C.byref(a), dev.index, _stream(dev)), "dwn_cortex_backward")
        return dx, None, None, None, None, dw, dgm, dbm, dgs, dbs


# ------------------------------------------------------------------------------------------------
# readout
# ------------------------------------------------------------------------------------------------
class ReadoutFn(torch.autograd.Function):
    """Readout.forward (dwiseneuro.py:283-287): Dropout1d -> grouped Conv1d(k=1)+bias -> [:N] -> Softplus(beta).
    x: [B,T,C] (compute dtype) -> [B,N,T] fp32.
    ``beta``: ``None`` (the module's fixed ``softplus_beta``) or a 0-d fp32 tensor on x's device, > 0: the kernels read it from
    device memory and backward returns its gradient (a float64 reduction fused into the dz pass)."""

    @staticmethod
    def forward(ctx, x, drop_mask, mod, weight, bias, beta=None):
        _require_gpu(x, "ReadoutFn")
        x = x.contiguous()
        dev = x.device
        beta_in = beta
        if beta is not None:
            if beta.dim() != 0 or beta.dtype != torch.float32 or beta.device != dev:
                raise RuntimeError("ReadoutFn: beta must be a 0-d fp32 tensor on the input's device")
            beta = beta.detach()
        B, T, Cin = x.shape
        n = mod.out_features
        out = torch.empty(B, n, T, dtype=torch.float32, device=dev)
        a = L.ReadoutArgs()
        a.dtype = _DT[x.dtype]; a.B = B; a.T = T; a.Cin = Cin; a.groups = mod.groups; a.n_out = n
        a.softplus_beta = mod.softplus_beta; a.beta_dev = _ptr(beta)
        a.x = x.data_ptr(); a.w = weight.data_ptr(); a.bias = bias.data_ptr(); a.drop_mask = _ptr(drop_mask)
        a.out = out.data_ptr()
        # eval-mode forward (the module is not training; a no_grad forward of a training module keeps the training numerics)
        a.f32_products = _f32_products(mod, inference_readout=True) if not mod.training else L.F32_NATIVE
        # a backward will follow: the pack pass also writes the weight in the data gradient's layout and backward reuses it
        # (the optimizer only touches the weight after backward)
        # (beta counts: with only the gate trainable the backward still forms dx and dW — as it always has for a frozen weight —
        # since dz, which dbeta rides on, is one pass with them; a dbeta-only backward is not built)
        wt = None
        if any(ctx.needs_input_grad):
            wt = torch.empty(L.lib.dwn_readout_wt_bytes(C.byref(a)), dtype=torch.uint8, device=dev)
            a.wt = wt.data_ptr()
        ws = _ws(L.lib.dwn_readout_workspace_bytes(C.byref(a), 0), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_readout_forward(C.byref(a), dev.index, _stream(dev)), "dwn_readout_forward")
        ctx.mod = mod; ctx.has_mask = drop_mask is not None
        ctx.wt = wt
        # samples whose loss weight for this mouse is not zero (MouseModel.train_step knows them on the host): the backward
        # then runs on those rows only — the gradient w.r.t. the other rows' predictions is exactly zero (losses.py:15-17)
        ctx.active = getattr(mod, "_dwn_active", None)
        tensors = [x, weight, bias, out]
        if drop_mask is not None:
            tensors.append(drop_mask)
        ctx.has_beta = beta is not None
        # the gate parameter itself (the "beta" form): its gradient is written straight into its all-reduce slot, like dw / db
        ctx.beta_param = beta_in if isinstance(beta_in, torch.nn.Parameter) else None
        if beta is not None:
            tensors.append(beta)
        ctx.save_for_backward(*tensors)
        return out

    @staticmethod
    def backward(ctx, dout):
        mod = ctx.mod
        t = ctx.saved_tensors
        x, weight, bias, out = t[:4]
        drop_mask = t[4] if ctx.has_mask else None
        beta = t[-1] if ctx.has_beta else None
        dev = x.device
        dout = dout.contiguous().float()
        B, T, Cin = x.shape
        n = mod.out_features
        conv = mod.layer[1]
        dw = grad_out(conv.weight)                   # overwritten by dwn_readout_backward (no 64 MB clear per readout)
        db = grad_out(conv.bias, zero=True)
        dbeta = None
        if beta is not None:                         # overwritten by dwn_readout_backward
            dbeta = grad_out(ctx.beta_param) if ctx.beta_param is not None else torch.empty((), dtype=torch.float32, device=dev)
        idx, dx_full = ctx.active, None
        if idx is not None and idx.numel() < B:
            # compact backward: the three products see nb x T rows instead of B x T (ten readouts with one-hot mouse
            # weights: 3-4 of 32 samples each); zero rows contribute exactly nothing to dW / dbias and get dx = 0
            dx_full = torch.zeros_like(x)
            if idx.numel() == 0:
                return dx_full, None, None, dw.zero_(), db, (None if dbeta is None else dbeta.zero_())
            x, out, dout = x.index_select(0, idx), out.index_select(0, idx), dout.index_select(0, idx)
            if drop_mask is not None:
                drop_mask = drop_mask.index_select(0, idx)
            B = idx.numel()
        dx = torch.empty_like(x)
        a = L.ReadoutArgs()
        a.dtype = _DT[x.dtype]; a.B = B; a.T = T; a.Cin = Cin; a.groups = mod.groups; a.n_out = n
        a.softplus_beta = mod.softplus_beta; a.beta_dev = _ptr(beta); a.dbeta = _ptr(dbeta)
        a.x = x.data_ptr(); a.w = weight.data_ptr(); a.bias = bias.data_ptr(); a.drop_mask = _ptr(drop_mask)
        a.out = out.data_ptr(); a.dout = dout.data_ptr(); a.dx = dx.data_ptr(); a.dw = dw.data_ptr()
        a.dbias = db.data_ptr()
        if ctx.wt is not None:
            a.wt = ctx.wt.data_ptr()
        ws = _ws(L.lib.dwn_readout_workspace_bytes(C.byref(a), 1), dev)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel()
        L.check(L.lib.dwn_readout_backward(C.byref(a), dev.index, _stream(dev)), "dwn_readout_backward")
        if dx_full is not None:
            dx_full.index_copy_(0, idx, dx)
            dx = dx_full
        return dx, None, None, dw, db, dbeta


# ------------------------------------------------------------------------------------------------
# MicePoissonLoss
# ------------------------------------------------------------------------------------------------
class PoissonLossFn(torch.autograd.Function):
    """sum_{b,n,t} w[b] * (x - y*log(x + eps)) for one mouse (losses.py:14-20); w already normalised.
    The reduction runs in a double accumulator on the device and is returned as an fp32 scalar."""

    @staticmethod
    def forward(ctx, pred, target, w, eps):
        _require_gpu(pred, "PoissonLossFn")
        pred = pred.contiguous().float()
        target = target.contiguous().float()
        w = w.contiguous().float()
        dev = pred.device
        acc = torch.zeros(1, dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        per_sample = pred[0].numel()
        L.check(L.lib.dwn_poisson_loss_forward(pred.data_ptr(), target.data_ptr(), w.data_ptr(), per_sample,
                                               pred.numel(), eps, acc.data_ptr(), dev.index, _stream(dev)),
                "dwn_poisson_loss_forward")
        L.check(L.lib.dwn_f64_to_f32(acc.data_ptr(), out.data_ptr(), 1, dev.index, _stream(dev)), "dwn_f64_to_f32")
        ctx.eps = eps
        ctx.save_for_backward(pred, target, w)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred, target, w = ctx.saved_tensors
        dev = pred.device
        gscale = gout.contiguous().float()
        dpred = torch.empty_like(pred)
        L.check(L.lib.dwn_poisson_loss_backward(pred.data_ptr(), target.data_ptr(), w.data_ptr(),
                                                gscale.data_ptr(), pred[0].numel(), pred.numel(), ctx.eps,
                                                dpred.data_ptr(), dev.index, _stream(dev)),
                "dwn_poisson_loss_backward")
        return dpred, None, None, None


# ------------------------------------------------------------------------------------------------
# correlation objective: MiceCorrelationLoss, CorrelationMetric(fused=True)
# ------------------------------------------------------------------------------------------------
CORR_REDUCTIONS = {"mean": L.CORR_MEAN, "sum": L.CORR_SUM}


def _corr_args(pred, target, w, stat, eps: float = 1e-8, reduction: str = "mean") -> L.CorrArgs:
    """pred / target (B, N, T) or (B, N) fp32 contiguous, w a (B,) fp32 view of any stride, stat the (8 * N + 1,) float64 buffer:
    DWN_CORR_STAT_ROWS rows of N and the count n behind them."""
    a = L.CorrArgs()
    a.B, a.N = int(pred.shape[0]), int(pred.shape[1])
    a.T = int(pred.shape[2]) if pred.dim() == 3 else 1
    a.reduction = CORR_REDUCTIONS[reduction]
    a.eps = float(eps)
    a.w_stride = max(int(w.stride(0)), 1)
    a.pred, a.target, a.w = pred.data_ptr(), target.data_ptr(), w.data_ptr()
    a.stat = stat.data_ptr()
    a.count = stat.data_ptr() + 8 * L.CORR_STAT_ROWS * a.N
    return a


def _corr_inputs(pred, target, w, what: str):
    _require_gpu(pred, what)
    if pred.dim() not in (2, 3) or pred.shape != target.shape or w.dim() != 1 or w.shape[0] != pred.shape[0]:
        raise ValueError(f"sensorium_amd.{what}: pred / target (B, N[, T]) of one shape and w (B,), got "
                         f"{tuple(pred.shape)}, {tuple(target.shape)}, {tuple(w.shape)}")
    return pred.contiguous().float(), target.contiguous().float(), w.float()


def corr_moments(pred, target, w) -> torch.Tensor:
    """dwn_corr_moments for one mouse: the (8 * N + 1,) float64 buffer whose rows 0-4 are mean_p, mean_t, M2p, M2t, C over the
    (sample, frame) values of the rows with w != 0 and whose last element is n (rows 5-7 are left to dwn_corr_loss_finalize).
    One launch, no read-back."""
    pred, target, w = _corr_inputs(pred, target, w, "corr_moments")
    dev = pred.device
    stat = torch.empty(L.CORR_STAT_ROWS * pred.shape[1] + 1, dtype=torch.float64, device=dev)
    a = _corr_args(pred, target, w, stat)
    L.check(L.lib.dwn_corr_moments(C.byref(a), dev.index, _stream(dev)), "dwn_corr_moments")
    return stat


class CorrelationLossFn(torch.autograd.Function):
    """share * red_j (1 - r_j) for one mouse: r_j the Pearson correlation of neuron j over the (sample, frame) values of the rows
    with w != 0 (the weights' magnitudes enter through ``share`` alone, a 0-d device tensor).  Moments, coefficients and the
    reduction run in float64 on the device; the value is returned as an fp32 scalar.  A mouse without a row gives exactly 0 and
    a zero gradient, decided on the device."""

    @staticmethod
    def forward(ctx, pred, target, w, share, eps, reduction):
        pred, target, w = _corr_inputs(pred, target, w, "CorrelationLossFn")
        share = share.float().reshape(())
        dev = pred.device
        stat = torch.empty(L.CORR_STAT_ROWS * pred.shape[1] + 1, dtype=torch.float64, device=dev)
        acc = torch.zeros(1, dtype=torch.float64, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        a = _corr_args(pred, target, w, stat, eps, reduction)
        L.check(L.lib.dwn_corr_moments(C.byref(a), dev.index, _stream(dev)), "dwn_corr_moments")
        ws = _ws(L.lib.dwn_corr_ws_bytes(C.byref(a)), dev)
        a.share, a.loss_acc, a.ws, a.ws_bytes = share.data_ptr(), acc.data_ptr(), ws.data_ptr(), ws.numel()
        L.check(L.lib.dwn_corr_loss_finalize(C.byref(a), dev.index, _stream(dev)), "dwn_corr_loss_finalize")
        L.check(L.lib.dwn_f64_to_f32(acc.data_ptr(), out.data_ptr(), 1, dev.index, _stream(dev)), "dwn_f64_to_f32")
        ctx.eps, ctx.reduction = eps, reduction
        ctx.save_for_backward(pred, target, w, share, stat)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred, target, w, share, stat = ctx.saved_tensors
        dev = pred.device
        gscale = gout.contiguous().float()
        dpred = torch.empty_like(pred)
        a = _corr_args(pred, target, w, stat, ctx.eps, ctx.reduction)
        a.share, a.gscale, a.dpred = share.data_ptr(), gscale.data_ptr(), dpred.data_ptr()
        L.check(L.lib.dwn_corr_loss_backward(C.byref(a), dev.index, _stream(dev)), "dwn_corr_loss_backward")
        return dpred, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# gaze shifter (sensorium_amd/shifter.py)
# ------------------------------------------------------------------------------------------------
def _gaze_args(x_shape, video_channel: int, fill: float) -> L.GazeArgs:
    a = L.GazeArgs()
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in x_shape)
    a.video_channel = int(video_channel)
    a.fill = float(fill)
    return a


class GazeShiftFn(torch.autograd.Function):
    """Per-frame translation of channel ``video_channel`` of the NCDHW fp32 input by ``shift`` [B][T][2] = (dy, dx) pixels,
    bilinear, constant ``fill`` outside the frame; every other channel is copied (include/dwn.h dwn_gaze_args).  Gradients
    w.r.t. the input (an adjoint gather) and w.r.t. the shift (one float64 reduction per frame), both without atomics."""

    @staticmethod
    def forward(ctx, x, shift, video_channel=0, fill=0.0):
        _require_gpu(x, "GazeShiftFn")
        _require_gpu(shift, "GazeShiftFn")
        if x.dim() != 5 or shift.shape != (x.shape[0], x.shape[2], 2):
            raise RuntimeError("sensorium_amd.GazeShiftFn: x must be [B][C][T][H][W] and shift [B][T][2]")
        x = x.contiguous().float()
        shift = shift.contiguous().float()
        dev = x.device
        out = torch.empty_like(x)
        a = _gaze_args(x.shape, video_channel, fill)
        a.x = x.data_ptr(); a.shift = shift.data_ptr(); a.out = out.data_ptr()
        L.check(L.lib.dwn_gaze_shift_forward(C.byref(a), dev.index, _stream(dev)), "dwn_gaze_shift_forward")
        ctx.geom = (tuple(x.shape), int(video_channel), float(fill))
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, shift)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, shift = ctx.saved_tensors
        shape, video_channel, fill = ctx.geom
        dev = dout.device
        dout = dout.contiguous().float()
        dx = torch.empty(shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        dshift = torch.empty_like(shift) if ctx.needs_input_grad[1] else None
        if dx is None and dshift is None:
            return None, None, None, None
        a = _gaze_args(shape, video_channel, fill)
        a.x = _ptr(x); a.shift = shift.data_ptr(); a.dout = dout.data_ptr(); a.dx = _ptr(dx); a.dshift = _ptr(dshift)
        L.check(L.lib.dwn_gaze_shift_backward(C.byref(a), dev.index, _stream(dev)), "dwn_gaze_shift_backward")
        return dx, dshift, None, None


class PlaneMeanFn(torch.autograd.Function):
    """mean over H x W of channels [c0, c0 + nc) of the NCDHW fp32 input -> [B][T][nc] (dwn_plane_mean: float64 accumulation in a
    fixed order, a constant plane returns its constant bit for bit).  The backward — a broadcast of dmean / (H W) into the chosen
    channels — is plain torch: it runs only when the caller's input requires a gradient (attribution)."""

    @staticmethod
    def forward(ctx, x, c0, nc):
        _require_gpu(x, "PlaneMeanFn")
        if x.dim() != 5:
            raise RuntimeError("sensorium_amd.PlaneMeanFn: x must be [B][C][T][H][W]")
        x = x.contiguous().float()
        B, Cin, T, H, W = x.shape
        dev = x.device
        mean = torch.empty(B, T, int(nc), dtype=torch.float32, device=dev)
        L.check(L.lib.dwn_plane_mean(x.data_ptr(), B, Cin, T, H, W, int(c0), int(nc), mean.data_ptr(), dev.index, _stream(dev)),
                "dwn_plane_mean")
        ctx.geom = (tuple(x.shape), int(c0), int(nc))
        return mean

    @staticmethod
    @once_differentiable
    def backward(ctx, dmean):
        shape, c0, nc = ctx.geom
        dx = torch.zeros(shape, dtype=torch.float32, device=dmean.device)
        dx[:, c0:c0 + nc] = (dmean.float().permute(0, 2, 1) / float(shape[3] * shape[4]))[..., None, None]
        return dx, None, None


# ------------------------------------------------------------------------------------------------
# in-silico stimuli (sensorium_amd/stimuli.py)
# ------------------------------------------------------------------------------------------------
GABOR_ENVELOPES = {"gaussian": L.GABOR_GAUSSIAN, "none": L.GABOR_NONE}


def _gabor_args(shape, video_channel, envelope, background, video_range, window, pad) -> L.GaborArgs:
    if envelope not in GABOR_ENVELOPES:
        raise ValueError(f"envelope: one of {tuple(GABOR_ENVELOPES)} (got {envelope!r})")
    a = L.GaborArgs()
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in shape)
    a.video_channel = int(video_channel)
    a.envelope = GABOR_ENVELOPES[envelope]
    a.background = float(background)
    a.pad = float(pad)
    if video_range is not None:
        a.clamp, a.lo, a.hi = 1, float(video_range[0]), float(video_range[1])
    if window is not None:
        a.y0, a.x0, a.wh, a.ww = (int(n) for n in window)
    return a


class GaborFn(torch.autograd.Function):
    """``GaborFn.apply(params, template, video_channel, envelope, background, video_range, window, pad) -> input``: a drifting
    Gabor per clip (``params`` [B][8]: cy, cx, sigma, theta, sf, tf, phase, amplitude) rendered into channel ``video_channel`` of
    a copy of ``template`` [B][C][T][H][W] (include/dwn.h dwn_gabor_args).  The gradient w.r.t. ``params`` is one float64
    fixed-order reduction of the video channel of the incoming gradient; the gradient w.r.t. ``template`` passes through on the
    copied channels and is zero on the video channel."""

    @staticmethod
    def forward(ctx, params, template, video_channel=0, envelope="gaussian", background=127.5, video_range=(0.0, 255.0),
                window=None, pad=0.0):
        _require_gpu(params, "GaborFn")
        _require_gpu(template, "GaborFn")
        if template.dim() != 5 or params.shape != (template.shape[0], 8):
            raise RuntimeError("sensorium_amd.GaborFn: template must be [B][C][T][H][W] and params [B][8]")
        template = template.contiguous().float()
        params = params.contiguous().float()
        dev = template.device
        geom = (tuple(template.shape), int(video_channel), envelope, float(background),
                None if video_range is None else (float(video_range[0]), float(video_range[1])),
                None if window is None else tuple(int(n) for n in window), float(pad))
        a = _gabor_args(*geom)
        out = torch.empty_like(template)
        a.x = template.data_ptr(); a.params = params.data_ptr(); a.out = out.data_ptr()
        L.check(L.lib.dwn_gabor_forward(C.byref(a), dev.index, _stream(dev)), "dwn_gabor_forward")
        ctx.geom = geom
        ctx.save_for_backward(params)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (params,) = ctx.saved_tensors
        dev = dout.device
        dout = dout.contiguous().float()
        dparams = dtemplate = None
        if ctx.needs_input_grad[0]:
            a = _gabor_args(*ctx.geom)
            nbytes = L.lib.dwn_gabor_workspace_bytes(C.byref(a))
            ws = torch.empty(max(int(nbytes), 8) // 8, dtype=torch.float64, device=dev)
            dparams = torch.empty_like(params)
            a.params = params.data_ptr(); a.dout = dout.data_ptr(); a.dparams = dparams.data_ptr()
            a.ws = ws.data_ptr(); a.ws_bytes = ws.numel() * 8
            L.check(L.lib.dwn_gabor_backward(C.byref(a), dev.index, _stream(dev)), "dwn_gabor_backward")
        if ctx.needs_input_grad[1]:
            dtemplate = dout.clone()
            dtemplate[:, ctx.geom[1]] = 0
        return dparams, dtemplate, None, None, None, None, None, None


# ------------------------------------------------------------------------------------------------
# behaviour modulator (sensorium_amd/modulator.py)
# ------------------------------------------------------------------------------------------------
def _modulator_args(y, h, u, c, max_log_gain: float) -> L.ModulatorArgs:
    a = L.ModulatorArgs()
    a.B, a.N, a.T = (int(n) for n in y.shape)
    a.K = int(h.shape[2])
    a.max_log_gain = float(max_log_gain)
    a.y = y.data_ptr(); a.h = h.data_ptr(); a.u = u.data_ptr(); a.c = c.data_ptr()
    return a


class ModulatorFn(torch.autograd.Function):
    """``ModulatorFn.apply(y, h, u, c, max_log_gain) -> y * exp(max_log_gain * tanh(c[n] + h[b,t,:] . u[n,:]))`` for a readout's
    output ``y`` [B][N][T], the behaviour features ``h`` [B][T][K], the per-neuron weights ``u`` [N][K] and offsets ``c`` [N]
    (include/dwn.h dwn_modulator_args).  The backward asks the kernels only for the gradients autograd needs; the three
    reductions (du, dc over the rows, dh over the neurons) are float64 sums in a fixed order, without atomics."""

    @staticmethod
    def forward(ctx, y, h, u, c, max_log_gain=2.0):
        for t in (y, h, u, c):
            _require_gpu(t, "ModulatorFn")
        if y.dim() != 3 or h.dim() != 3 or h.shape[:2] != (y.shape[0], y.shape[2]) or u.shape != (y.shape[1], h.shape[2]) \
                or c.shape != (y.shape[1],):
            raise RuntimeError("sensorium_amd.ModulatorFn: y must be [B][N][T], h [B][T][K], u [N][K] and c [N]")
        y = y.contiguous().float(); h = h.contiguous().float(); u = u.contiguous().float(); c = c.contiguous().float()
        dev = y.device
        out = torch.empty_like(y)
        a = _modulator_args(y, h, u, c, max_log_gain)
        a.out = out.data_ptr()
        L.check(L.lib.dwn_modulator_forward(C.byref(a), dev.index, _stream(dev)), "dwn_modulator_forward")
        ctx.max_log_gain = float(max_log_gain)
        ctx.save_for_backward(y, h, u, c)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        y, h, u, c = ctx.saved_tensors
        need = ctx.needs_input_grad[:4]
        if not any(need):
            return None, None, None, None, None
        dev = dout.device
        dout = dout.contiguous().float()
        dy, dh, du, dc = (torch.empty_like(t) if n else None for t, n in zip((y, h, u, c), need))
        a = _modulator_args(y, h, u, c, ctx.max_log_gain)
        nbytes = L.lib.dwn_modulator_ws_bytes(C.byref(a))
        ws = torch.empty(max(int(nbytes), 8) // 8, dtype=torch.float64, device=dev)
        a.dout = dout.data_ptr(); a.dy = _ptr(dy); a.dh = _ptr(dh); a.du = _ptr(du); a.dc = _ptr(dc)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel() * 8
        L.check(L.lib.dwn_modulator_backward(C.byref(a), dev.index, _stream(dev)), "dwn_modulator_backward")
        return dy, dh, du, dc, None


# ------------------------------------------------------------------------------------------------
# regularised MEI synthesis (sensorium_amd/attribution.py most_exciting_input)
# ------------------------------------------------------------------------------------------------
MEI_CONTRAST_MODES = {"max": L.MEI_CONTRAST_MAX, "fixed": L.MEI_CONTRAST_FIXED}


def gaussian_taps(sigma: float, radius: Optional[int] = None) -> torch.Tensor:
    """The ``2 * radius + 1`` taps of a sampled Gaussian: float64 ``exp(-k^2 / (2 sigma^2))`` normalised to sum 1 in float64, then
    rounded to fp32.  ``radius`` defaults to ``ceil(3 sigma)`` and is capped at ``DWN_BLUR_MAX_RADIUS``; ``sigma == 0`` gives the
    single tap 1.0 (with a given radius: the centred delta).  Pure host code; returns a CPU tensor."""
    sigma = float(sigma)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError(f"gaussian_taps: sigma must be finite and not negative (got {sigma})")
    if radius is None:
        radius = min(int(math.ceil(3.0 * sigma)), L.BLUR_MAX_RADIUS)
    radius = int(radius)
    if radius < 0 or radius > L.BLUR_MAX_RADIUS:
        raise ValueError(f"gaussian_taps: radius outside [0, {L.BLUR_MAX_RADIUS}]")
    k = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma)) if sigma > 0.0 else (k == 0).astype(np.float64)
    return torch.from_numpy((w / w.sum()).astype(np.float32))


def blur_taps_table(taps, device=None):
    """``taps``: three 1-D sequences of odd length (frames, rows, columns) -> (the table [3][DWN_BLUR_TAPS_STRIDE] fp32 that
    ``dwn_blur3d`` reads, the radii).  Entries past ``2 * radius`` are zero and never read."""
    if len(taps) != 3:
        raise ValueError("taps: three sequences (frames, rows, columns)")
    table = torch.zeros(3, L.BLUR_TAPS_STRIDE, dtype=torch.float32)
    radii = []
    for a, t in enumerate(taps):
        t = torch.as_tensor(t, dtype=torch.float32).detach().cpu()
        if t.dim() != 1 or t.numel() % 2 != 1 or t.numel() > L.BLUR_TAPS_STRIDE:
            raise ValueError(f"taps[{a}]: a 1-D sequence of odd length, at most {L.BLUR_TAPS_STRIDE}")
        table[a, :t.numel()] = t
        radii.append(t.numel() // 2)
    return (table if device is None else table.to(device)), tuple(radii)


def _window4(window):
    if window is None:
        return (0, 0, 0, 0)
    if len(window) != 4:
        raise ValueError("window: (y0, x0, height, width)")
    return tuple(int(n) for n in window)


def _video5(t: torch.Tensor, what: str) -> torch.Tensor:
    _require_gpu(t, what)
    if t.dim() != 5 or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"sensorium_amd.{what}: a contiguous fp32 tensor [B][C][T][H][W]")
    return t


def blur3d(src: torch.Tensor, table: torch.Tensor, radii, *, c_src: int = 0, out: Optional[torch.Tensor] = None, c_dst: int = 0,
           window=None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Separable blur of channel ``c_src`` of ``src`` [B][C][T][H][W] into channel ``c_dst`` of ``out`` (default: a new
    [B][1][T][H][W]) with the DEVICE taps ``table`` [3][DWN_BLUR_TAPS_STRIDE] and the integer ``radii`` (frames, rows, columns);
    include/dwn.h dwn_blur3d.  ``ws``: a fp32 workspace of at least B T H W elements (allocated when not given)."""
    src = _video5(src, "blur3d")
    B, _, T, H, W = src.shape
    if out is None:
        out = torch.empty(B, 1, T, H, W, dtype=torch.float32, device=src.device)
    out = _video5(out, "blur3d")
    if (out.shape[0], *out.shape[2:]) != (B, T, H, W):
        raise RuntimeError("sensorium_amd.blur3d: src and out differ in B, T, H or W")
    _require_gpu(table, "blur3d")
    if table.shape != (3, L.BLUR_TAPS_STRIDE) or table.dtype != torch.float32 or not table.is_contiguous():
        raise RuntimeError(f"sensorium_amd.blur3d: table must be contiguous fp32 [3][{L.BLUR_TAPS_STRIDE}]")
    if ws is None:
        ws = torch.empty(B * T * H * W, dtype=torch.float32, device=src.device)
    a = L.Blur3dArgs()
    a.B, a.T, a.H, a.W = B, T, H, W
    a.Cin_src, a.c_src, a.Cin_dst, a.c_dst = int(src.shape[1]), int(c_src), int(out.shape[1]), int(c_dst)
    a.Rt, a.Rh, a.Rw = (int(r) for r in radii)
    a.y0, a.x0, a.wh, a.ww = _window4(window)
    a.src = src.data_ptr(); a.dst = out.data_ptr(); a.taps = table.data_ptr()
    a.ws = ws.data_ptr(); a.ws_bytes = ws.numel() * ws.element_size()
    L.check(L.lib.dwn_blur3d(C.byref(a), src.device.index, _stream(src.device)), "dwn_blur3d")
    return out


def clip_moments_ws(shape, window=None) -> int:
    """float64 elements of the workspace of ``clip_moments`` for a tensor of ``shape`` (at least 1)."""
    a = L.ClipMomentsArgs()
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in shape)
    a.y0, a.x0, a.wh, a.ww = _window4(window)
    return max(int(L.lib.dwn_clip_moments_ws_bytes(C.byref(a))) // 8, 1)


def clip_moments(x: torch.Tensor, *, c: int = 0, window=None, out: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-clip float64 statistics [B][4] = (n, mean, M2, S2) of channel ``c`` of ``x`` [B][C][T][H][W] over the window
    (include/dwn.h dwn_clip_moments)."""
    x = _video5(x, "clip_moments")
    dev = x.device
    if out is None:
        out = torch.empty(x.shape[0], 4, dtype=torch.float64, device=dev)
    if ws is None:
        ws = torch.empty(clip_moments_ws(x.shape, window), dtype=torch.float64, device=dev)
    a = L.ClipMomentsArgs()
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in x.shape)
    a.c = int(c)
    a.y0, a.x0, a.wh, a.ww = _window4(window)
    a.x = x.data_ptr(); a.stat = out.data_ptr(); a.ws = ws.data_ptr(); a.ws_bytes = ws.numel() * 8
    L.check(L.lib.dwn_clip_moments(C.byref(a), dev.index, _stream(dev)), "dwn_clip_moments")
    return out


def mei_update(x: torch.Tensor, stat: torch.Tensor, mode: str, *, c: int = 0, window=None, g: Optional[torch.Tensor] = None,
               c_g: int = 0, lr: Optional[torch.Tensor] = None, mean: Optional[float] = None, contrast: Optional[float] = None,
               contrast_mode: str = "max", video_range=(0.0, 255.0)) -> torch.Tensor:
    """In place on the window of channel ``c`` of ``x`` (include/dwn.h dwn_mei_update).  ``mode="step"``: ``x += lr * g / rms(g)``
    per clip with ``stat`` the moments of channel ``c_g`` of ``g`` and ``lr`` a one-element fp32 device tensor.
    ``mode="project"``: the mean / RMS-contrast projection and the clamp to ``video_range`` with ``stat`` the moments of ``x``."""
    x = _video5(x, "mei_update")
    dev = x.device
    _require_gpu(stat, "mei_update")
    if stat.shape != (x.shape[0], 4) or stat.dtype != torch.float64 or not stat.is_contiguous():
        raise RuntimeError("sensorium_amd.mei_update: stat must be contiguous float64 [B][4]")
    if mode not in ("step", "project"):
        raise ValueError("mode: 'step' or 'project'")
    if contrast_mode not in MEI_CONTRAST_MODES:
        raise ValueError(f"contrast_mode: one of {tuple(MEI_CONTRAST_MODES)} (got {contrast_mode!r})")
    a = L.MeiUpdateArgs()
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in x.shape)
    a.c = int(c)
    a.y0, a.x0, a.wh, a.ww = _window4(window)
    a.x = x.data_ptr(); a.stat = stat.data_ptr()
    if mode == "step":
        if g is None or lr is None:
            raise ValueError("mode 'step' needs g and lr")
        g = _video5(g, "mei_update")
        _require_gpu(lr, "mei_update")
        if (g.shape[0], *g.shape[2:]) != (x.shape[0], *x.shape[2:]) or lr.dtype != torch.float32 or lr.numel() != 1:
            raise RuntimeError("sensorium_amd.mei_update: g must match x in B, T, H, W and lr be one fp32 element")
        a.mode, a.Cin_g, a.c_g = L.MEI_STEP, int(g.shape[1]), int(c_g)
        a.g = g.data_ptr(); a.lr = lr.data_ptr()
    else:
        a.mode = L.MEI_PROJECT
        a.lo, a.hi = float(video_range[0]), float(video_range[1])
        if mean is not None:
            a.has_mean, a.mean_target = 1, float(mean)
        if contrast is not None:
            a.has_contrast, a.contrast, a.contrast_mode = 1, float(contrast), MEI_CONTRAST_MODES[contrast_mode]
    L.check(L.lib.dwn_mei_update(C.byref(a), dev.index, _stream(dev)), "dwn_mei_update")
    return x


class GaussianBlur3dFn(torch.autograd.Function):
    """``GaussianBlur3dFn.apply(x, table, radii, channel, window) -> [B][1][T][H][W]``: ``blur3d`` of one channel of ``x`` with
    a gradient.  The operator is (window mask) K (window mask), so its adjoint is the same kernel with each axis' taps reversed:
    the backward blurs the incoming gradient with the reversed table into ``channel`` of a zero tensor shaped like ``x``.  The
    table gets no gradient."""

    @staticmethod
    def forward(ctx, x, table, radii, channel=0, window=None):
        x = x.contiguous().float()
        ctx.geom = (tuple(x.shape), tuple(int(r) for r in radii), int(channel), window)
        ctx.save_for_backward(table)
        return blur3d(x, table, radii, c_src=channel, window=window)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (table,) = ctx.saved_tensors
        shape, radii, channel, window = ctx.geom
        rev = torch.zeros_like(table)
        for a, r in enumerate(radii):
            rev[a, :2 * r + 1] = table[a, :2 * r + 1].flip(0)
        dx = torch.zeros(shape, dtype=torch.float32, device=dout.device)
        blur3d(dout.contiguous().float(), rev, radii, c_src=0, out=dx, c_dst=channel, window=window)
        return dx, None, None, None, None


# ------------------------------------------------------------------------------------------------
# trial-level evaluation (sensorium_amd/evaluation.py)
# ------------------------------------------------------------------------------------------------
_TRIAL_DESC = np.dtype([("pred", "<u8"), ("target", "<u8"), ("ld_pred", "<i8"), ("ld_target", "<i8"), ("first", "<i4"),
                        ("frames", "<i4")])
_TRIAL_GROUP = np.dtype([("first_trial", "<i4"), ("repeats", "<i4"), ("frames", "<i4")])
assert _TRIAL_DESC.itemsize == C.sizeof(L.TrialDesc) and _TRIAL_GROUP.itemsize == C.sizeof(L.TrialGroup)


def _trial_rows(t: torch.Tensor, N: int, first: int, frames: int, dev, what: str):
    """The row stride of one side of a trial after the checks the device tables rely on: every row the kernel reads lies inside
    the tensor."""
    _require_gpu(t, what)
    if t.dtype != torch.float32:
        raise RuntimeError(f"sensorium_amd.{what}: trials must be fp32 (got {t.dtype})")
    if t.dim() != 2 or t.shape[0] != N or t.device != dev:
        raise ValueError(f"sensorium_amd.{what}: a trial is an [N = {N}, L] tensor on {dev}, got {tuple(t.shape)} on {t.device}")
    if t.shape[1] > 1 and t.stride(1) != 1:
        raise ValueError(f"sensorium_amd.{what}: frames must have unit stride (got {t.stride(1)})")
    if frames < 1 or first < 0 or first + frames > t.shape[1]:
        raise ValueError(f"sensorium_amd.{what}: frames [{first}, {first + frames}) are not inside a trial of length {t.shape[1]}")
    ld = int(t.stride(0))
    if ld < 0:
        raise ValueError(f"sensorium_amd.{what}: negative row stride")
    return ld


def trial_moments(state: torch.Tensor, trials, groups, counts=(0, 0, 0)):
    """dwn_trial_moments: merges trials into ``state`` (float64 ``[TRIAL_STATE_ROWS, N]``, zero before the first call) in place.
    ``trials``: a sequence of ``(pred, target, first, frames)`` with ``pred`` / ``target`` GPU fp32 ``[N, L]`` tensors of unit
    stride along frames and any row stride, of which the frames ``[first, first + frames)`` count; ``groups``: a sequence of
    ``(first_trial, repeats, frames)`` that covers the trials in order (a trial that repeats nothing is a group of 1).
    ``counts`` = ``(n_all, n_repeat, n_group_frames)`` of the state before the call; returns them after it.  Builds the two device
    tables and launches; the tensors must stay alive until the launch has run (stream order)."""
    _require_gpu(state, "trial_moments")
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[0] != L.TRIAL_STATE_ROWS or not state.is_contiguous():
        raise RuntimeError(f"sensorium_amd.trial_moments: state must be contiguous float64 [{L.TRIAL_STATE_ROWS}, N]")
    dev, N = state.device, int(state.shape[1])
    trials, groups = list(trials), list(groups)
    if not trials or not groups:
        raise ValueError("sensorium_amd.trial_moments: no trials")
    td = np.zeros(len(trials), dtype=_TRIAL_DESC)
    for i, (p, y, first, frames) in enumerate(trials):
        first, frames = int(first), int(frames)
        ldp = _trial_rows(p, N, first, frames, dev, "trial_moments")
        ldy = _trial_rows(y, N, first, frames, dev, "trial_moments")
        td[i] = (p.data_ptr(), y.data_ptr(), ldp, ldy, first, frames)
    gd = np.zeros(len(groups), dtype=_TRIAL_GROUP)
    n_all, n_rep, n_gf = (int(c) for c in counts)
    at = 0
    for i, (first_trial, repeats, frames) in enumerate(groups):
        first_trial, repeats, frames = int(first_trial), int(repeats), int(frames)
        if first_trial != at or repeats < 1 or at + repeats > len(trials):
            raise ValueError(f"sensorium_amd.trial_moments: group {i} does not continue the trial table")
        if any(int(td[k]["frames"]) != frames for k in range(at, at + repeats)):
            raise ValueError(f"sensorium_amd.trial_moments: group {i}: its trials do not all have {frames} frames")
        gd[i] = (first_trial, repeats, frames)
        at += repeats
        n_all += repeats * frames
        if repeats >= 2:
            n_rep += repeats * frames
            n_gf += frames
    if at != len(trials):
        raise ValueError("sensorium_amd.trial_moments: the groups do not cover every trial")
    tt = torch.from_numpy(td.view(np.uint8)).to(dev)
    gt = torch.from_numpy(gd.view(np.uint8)).to(dev)
    a = L.TrialScoreArgs()
    a.N, a.n_trials, a.n_groups = N, len(trials), len(groups)
    a.max_repeats, a.max_frames = int(gd["repeats"].max()), int(gd["frames"].max())
    a.n_all, a.n_repeat, a.n_group_frames = (int(c) for c in counts)
    a.trials, a.groups, a.state = tt.data_ptr(), gt.data_ptr(), state.data_ptr()
    L.check(L.lib.dwn_trial_moments(C.byref(a), dev.index, _stream(dev)), "dwn_trial_moments")
    return n_all, n_rep, n_gf


def trial_scores(state: torch.Tensor, counts, eps: float = 1e-8, fev_threshold: float = 0.15):
    """dwn_trial_score_finalize: ``(scores, summary)`` — float64 ``[TRIAL_SCORE_ROWS, N]`` (single_trial_corr, corr_to_average,
    fev, feve, oracle_corr) and ``[TRIAL_SUMMARY]`` (include/dwn.h) — from the state and its counts.  No read-back."""
    _require_gpu(state, "trial_scores")
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[0] != L.TRIAL_STATE_ROWS or not state.is_contiguous():
        raise RuntimeError(f"sensorium_amd.trial_scores: state must be contiguous float64 [{L.TRIAL_STATE_ROWS}, N]")
    dev, N = state.device, int(state.shape[1])
    scores = torch.empty(L.TRIAL_SCORE_ROWS, N, dtype=torch.float64, device=dev)
    summary = torch.empty(L.TRIAL_SUMMARY, dtype=torch.float64, device=dev)
    a = L.TrialScoreArgs()
    a.N = N
    a.n_all, a.n_repeat, a.n_group_frames = (int(c) for c in counts)
    a.eps, a.fev_threshold = float(eps), float(fev_threshold)
    ws = torch.empty(max(int(L.lib.dwn_trial_score_ws_bytes(C.byref(a))) // 8, 1), dtype=torch.float64, device=dev)
    a.state, a.scores, a.summary, a.ws, a.ws_bytes = state.data_ptr(), scores.data_ptr(), summary.data_ptr(), ws.data_ptr(), ws.numel() * 8
    L.check(L.lib.dwn_trial_score_finalize(C.byref(a), dev.index, _stream(dev)), "dwn_trial_score_finalize")
    return scores, summary


# ------------------------------------------------------------------------------------------------
# population structure (sensorium_amd/population.py)
# ------------------------------------------------------------------------------------------------
_PAIR_SEG = np.dtype([("x", "<u8"), ("ld", "<i8"), ("first", "<i4"), ("frames", "<i4")])
assert _PAIR_SEG.itemsize == C.sizeof(L.PairSeg)
PAIR_KINDS = {"total": L.PAIR_TOTAL, "signal": L.PAIR_SIGNAL, "noise": L.PAIR_NOISE}


def pair_chunk_cols(kind: str, repeats: int, frames: int) -> int:
    """The columns of Z the chunks of one group take (include/dwn.h): per chunk its values and the merge column, rounded up to
    the k-step.  ``total``: one chunk per trial; ``signal`` / ``noise``: one per group of at least two repeats."""
    up = lambda n: -(-(n + 1) // L.PAIR_KSTEP) * L.PAIR_KSTEP      # noqa: E731
    if kind == "total":
        return repeats * up(frames)
    if repeats < 2:
        return 0
    return up(frames) if kind == "signal" else up(repeats * frames)


def pair_samples(kind: str, repeats: int, frames: int) -> int:
    """The samples the chunks of one group add to the state of ``kind``."""
    if kind == "total":
        return repeats * frames
    if repeats < 2:
        return 0
    return frames if kind == "signal" else repeats * frames


def _pair_state(state: torch.Tensor, what: str):
    _require_gpu(state, what)
    if state.dtype != torch.float64 or state.dim() != 2 or state.shape[0] != state.shape[1] + 1 or not state.is_contiguous():
        raise RuntimeError(f"sensorium_amd.{what}: state must be contiguous float64 [N + 1, N] (the co-moments, then the mean)")
    return state.device, int(state.shape[1])


def pair_tables(trials, groups, N: int, dev, what: str = "pair_accumulate"):
    """The device segment and group tables of ``trials`` (``(x, first, frames)`` with ``x`` a GPU fp32 ``[N, L]`` tensor of unit
    stride along frames) and ``groups`` (``(first_trial, repeats, frames)`` covering the trials in order), after the checks the
    kernels rely on.  Returns ``(segs, groups, host group table)``."""
    trials, groups = list(trials), list(groups)
    if not trials or not groups:
        raise ValueError(f"sensorium_amd.{what}: no trials")
    sd = np.zeros(len(trials), dtype=_PAIR_SEG)
    for i, (x, first, frames) in enumerate(trials):
        first, frames = int(first), int(frames)
        sd[i] = (x.data_ptr(), _trial_rows(x, N, first, frames, dev, what), first, frames)
    gd = np.zeros(len(groups), dtype=_TRIAL_GROUP)
    at = 0
    for i, (first_trial, repeats, frames) in enumerate(groups):
        first_trial, repeats, frames = int(first_trial), int(repeats), int(frames)
        if first_trial != at or repeats < 1 or at + repeats > len(trials):
            raise ValueError(f"sensorium_amd.{what}: group {i} does not continue the trial table")
        if any(int(sd[k]["frames"]) != frames for k in range(at, at + repeats)):
            raise ValueError(f"sensorium_amd.{what}: group {i}: its trials do not all have {frames} frames")
        gd[i] = (first_trial, repeats, frames)
        at += repeats
    if at != len(trials):
        raise ValueError(f"sensorium_amd.{what}: the groups do not cover every trial")
    return torch.from_numpy(sd.view(np.uint8)).to(dev), torch.from_numpy(gd.view(np.uint8)).to(dev), gd


def pair_accumulate(state: torch.Tensor, kind: str, tables, count: int = 0, ws: Optional[torch.Tensor] = None,
                    return_staged: bool = False):
    """dwn_pair_stage + dwn_pair_syrk: merges the chunks of ``tables`` (of ``pair_tables``) into ``state`` (float64 ``[N + 1, N]``:
    the centred co-moments ``C`` and, last row, the mean; zero before the first call) in place.  ``kind``: ``total`` / ``signal``
    / ``noise``; ``count``: the samples of the state before the call; returns the count after it.  ``ws``: a float64 tensor to
    stage ``Z`` in (at least ``cols * dwn_pair_ldz(N)`` elements), allocated when absent.  Tables without a chunk of this kind
    launch nothing.  ``return_staged`` also returns ``Z`` as a ``[cols, ldz]`` view (for measurements and tests)."""
    dev, N = _pair_state(state, "pair_accumulate")
    if kind not in PAIR_KINDS:
        raise ValueError(f"sensorium_amd.pair_accumulate: kind must be one of {tuple(PAIR_KINDS)}, got {kind!r}")
    segs, grps, gd = tables
    cols = sum(pair_chunk_cols(kind, int(g["repeats"]), int(g["frames"])) for g in gd)
    added = sum(pair_samples(kind, int(g["repeats"]), int(g["frames"])) for g in gd)
    if cols == 0:
        return (int(count), None) if return_staged else int(count)
    ldz = int(L.lib.dwn_pair_ldz(N))
    if ws is None:
        ws = torch.empty(cols * ldz, dtype=torch.float64, device=dev)
    _require_gpu(ws, "pair_accumulate")
    if ws.dtype != torch.float64 or not ws.is_contiguous() or ws.numel() < cols * ldz or ws.device != dev:
        raise ValueError(f"sensorium_amd.pair_accumulate: ws must be a contiguous float64 tensor of at least {cols * ldz} elements on {dev}")
    a = L.PairArgs()
    a.N, a.kind, a.n_segs, a.n_groups = N, PAIR_KINDS[kind], int(segs.numel()) // _PAIR_SEG.itemsize, len(gd)
    a.max_repeats, a.max_frames, a.cols, a.n = int(gd["repeats"].max()), int(gd["frames"].max()), cols, int(count)
    a.segs, a.groups, a.state, a.ws, a.ws_bytes = segs.data_ptr(), grps.data_ptr(), state.data_ptr(), ws.data_ptr(), ws.numel() * 8
    L.check(L.lib.dwn_pair_stage(C.byref(a), dev.index, _stream(dev)), "dwn_pair_stage")
    L.check(L.lib.dwn_pair_syrk(C.byref(a), dev.index, _stream(dev)), "dwn_pair_syrk")
    if return_staged:
        return int(count) + added, ws[:cols * ldz].view(cols, ldz)
    return int(count) + added


def pair_corr(state: torch.Tensor, count: int, eps: float = 1e-8, dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """dwn_pair_corr_finalize: the ``[N, N]`` correlation matrix of a state and its sample count, float64 or (rounded once)
    fp32.  The state is left as it is.  No read-back."""
    dev, N = _pair_state(state, "pair_corr")
    if dtype not in (torch.float64, torch.float32):
        raise ValueError(f"sensorium_amd.pair_corr: dtype must be float64 or float32, got {dtype}")
    out = torch.empty(N, N, dtype=dtype, device=dev)
    a = L.PairArgs()
    a.N, a.n, a.eps, a.out_f32 = N, int(count), float(eps), int(dtype == torch.float32)
    a.state, a.out = state.data_ptr(), out.data_ptr()
    L.check(L.lib.dwn_pair_corr_finalize(C.byref(a), dev.index, _stream(dev)), "dwn_pair_corr_finalize")
    return out


def pair_compare(A: torch.Tensor, B: torch.Tensor, sel: Optional[torch.Tensor] = None, eps: float = 1e-8):
    """dwn_pair_compare: ``(per_neuron [M], summary [PAIR_SUMMARY])`` float64 device tensors for two float64 ``[N, N]`` matrices
    (unit stride along columns, any row stride) and an optional int32 device selection ``sel [M]``.  No read-back."""
    for t in (A, B):
        _require_gpu(t, "pair_compare")
        if t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] != t.shape[1] or t.shape != A.shape or t.device != A.device:
            raise ValueError("sensorium_amd.pair_compare: A and B must be float64 [N, N] matrices of one size on one device")
        if t.shape[1] > 1 and t.stride(1) != 1 or t.stride(0) < t.shape[1]:
            raise ValueError("sensorium_amd.pair_compare: rows must have unit stride and must not overlap")
    dev, N = A.device, int(A.shape[0])
    M = N
    if sel is not None:
        _require_gpu(sel, "pair_compare")
        if sel.dtype != torch.int32 or sel.dim() != 1 or not sel.is_contiguous() or sel.numel() < 1 or sel.device != dev:
            raise ValueError("sensorium_amd.pair_compare: sel must be a non-empty contiguous 1-D int32 tensor on the matrices' device")
        M = int(sel.numel())
    per = torch.empty(M, dtype=torch.float64, device=dev)
    summary = torch.empty(L.PAIR_SUMMARY, dtype=torch.float64, device=dev)
    a = L.PairCompareArgs()
    a.N, a.M, a.lda, a.ldb, a.eps = N, M, int(A.stride(0)), int(B.stride(0)), float(eps)
    ws = torch.empty(max(int(L.lib.dwn_pair_compare_ws_bytes(C.byref(a))) // 8, 1), dtype=torch.float64, device=dev)
    a.A, a.B, a.sel = A.data_ptr(), B.data_ptr(), (sel.data_ptr() if sel is not None else None)
    a.per_neuron, a.summary, a.ws, a.ws_bytes = per.data_ptr(), summary.data_ptr(), ws.data_ptr(), ws.numel() * 8
    L.check(L.lib.dwn_pair_compare(C.byref(a), dev.index, _stream(dev)), "dwn_pair_compare")
    return per, summary


# ------------------------------------------------------------------------------------------------
# population modes (sensorium_amd/population.py)
# ------------------------------------------------------------------------------------------------
def modes_pad(p: int) -> int:
    """The columns a block of ``p`` columns is stored with: ``p`` rounded up to the MFMA tile width."""
    return -(-int(p) // 16) * 16


def _modes_matrix(A: torch.Tensor, what: str):
    _require_gpu(A, what)
    if A.dtype != torch.float64:
        raise RuntimeError(f"sensorium_amd.{what}: the matrix must be float64 (got {A.dtype})")
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError(f"sensorium_amd.{what}: the matrix must be square [N, N], got {tuple(A.shape)}")
    if (A.shape[1] > 1 and A.stride(1) != 1) or (A.shape[0] > 1 and A.stride(0) < A.shape[1]):
        raise ValueError(f"sensorium_amd.{what}: rows must have unit stride and must not overlap")
    return A.device, int(A.shape[0])


def _modes_block(X: torch.Tensor, N: int, dev, what: str, name: str) -> int:
    """A block ``[N, >= p]`` float64 whose row stride is at least the padded width; returns its row stride."""
    _require_gpu(X, what)
    if X.dtype != torch.float64 or X.dim() != 2 or X.shape[0] != N or X.device != dev:
        raise ValueError(f"sensorium_amd.{what}: {name} must be a float64 [N = {N}, p] tensor on {dev}")
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError(f"sensorium_amd.{what}: {name} must have unit stride along its columns")
    return int(X.stride(0)) if N > 1 else max(int(X.stride(0)), modes_pad(X.shape[1]))


def modes_block(N: int, p: int, dev) -> torch.Tensor:
    """A zeroed block of ``p`` columns: the ``[N, p]`` view of a ``[N, modes_pad(p)]`` tensor."""
    return torch.zeros(N, modes_pad(p), dtype=torch.float64, device=dev)[:, :p]


def _modes_args(N: int, p: int, k: int = 0) -> "L.ModesArgs":
    a = L.ModesArgs()
    a.N, a.p, a.k, a.scale = N, p, k, 1.0
    return a


def _modes_ws(a, query, dev) -> torch.Tensor:
    ws = torch.empty(max(int(query(C.byref(a))) // 8, 2), dtype=torch.float64, device=dev)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
    return ws


def modes_symm(A: torch.Tensor, Q: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """dwn_modes_symm: ``scale * A @ Q`` for a symmetric float64 ``[N, N]`` matrix (any row stride ``>= N``) and a block ``Q``
    (``modes_block``), as a new block."""
    dev, N = _modes_matrix(A, "modes_symm")
    ldq = _modes_block(Q, N, dev, "modes_symm", "Q")
    p = int(Q.shape[1])
    Y = modes_block(N, p, dev)
    a = _modes_args(N, p)
    a.lda, a.ldq, a.ldy, a.scale = int(A.stride(0)) if N > 1 else max(int(A.stride(0)), 1), ldq, modes_pad(p), float(scale)
    a.A, a.Q, a.Y = A.data_ptr(), Q.data_ptr(), Y.data_ptr()
    L.check(L.lib.dwn_modes_symm(C.byref(a), dev.index, _stream(dev)), "dwn_modes_symm")
    return Y


def modes_moments(A: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """dwn_modes_moments: float64 ``[2]`` device tensor, the trace and the squared Frobenius norm of ``scale * A``."""
    dev, N = _modes_matrix(A, "modes_moments")
    out = torch.zeros(4, dtype=torch.float64, device=dev)
    a = _modes_args(N, 1)
    a.lda, a.scale, a.A, a.moments = (int(A.stride(0)) if N > 1 else max(int(A.stride(0)), 1)), float(scale), A.data_ptr(), out.data_ptr()
    ws = _modes_ws(a, L.lib.dwn_modes_moments_ws_bytes, dev)       # noqa: F841  (alive until the launch is enqueued)
    L.check(L.lib.dwn_modes_moments(C.byref(a), dev.index, _stream(dev)), "dwn_modes_moments")
    return out[:2]


def modes_orth(Y: torch.Tensor) -> torch.Tensor:
    """dwn_modes_orth: an orthonormal basis of the columns of the block ``Y`` (a dependent column becomes an exact zero
    column), as a new block."""
    _require_gpu(Y, "modes_orth")
    dev, N = Y.device, int(Y.shape[0])
    ldy = _modes_block(Y, N, dev, "modes_orth", "Y")
    p = int(Y.shape[1])
    Q = modes_block(N, p, dev)
    a = _modes_args(N, p)
    a.ldq, a.ldy, a.Q, a.Y = modes_pad(p), ldy, Q.data_ptr(), Y.data_ptr()
    L.check(L.lib.dwn_modes_orth(C.byref(a), dev.index, _stream(dev)), "dwn_modes_orth")
    return Q


def modes_small_eigh(H: torch.Tensor):
    """dwn_modes_small_eigh: ``(values [p] descending, W [p, p])`` of a symmetric float64 ``[p, p]`` device matrix, ``p <= 64``."""
    _require_gpu(H, "modes_small_eigh")
    if H.dtype != torch.float64 or H.dim() != 2 or H.shape[0] != H.shape[1]:
        raise ValueError("sensorium_amd.modes_small_eigh: H must be a float64 [p, p] matrix")
    p, dev = int(H.shape[0]), H.device
    Hp = torch.zeros(max(p, 1), L.MODES_MAXP, dtype=torch.float64, device=dev)
    if 1 <= p <= L.MODES_MAXP:
        Hp[:, :p] = H
    W = torch.zeros_like(Hp)
    values = torch.zeros(L.MODES_MAXP, dtype=torch.float64, device=dev)
    a = _modes_args(1, p)
    a.H, a.W, a.values = Hp.data_ptr(), W.data_ptr(), values.data_ptr()
    L.check(L.lib.dwn_modes_small_eigh(C.byref(a), dev.index, _stream(dev)), "dwn_modes_small_eigh")
    return values[:p], W[:, :p]


def modes_ritz(Q: torch.Tensor, Y: torch.Tensor, theta: torch.Tensor, W: torch.Tensor, k: int, tol: float):
    """dwn_modes_ritz: ``(V, residuals [p], status int32 [4] = done, converged, rounds, 0)`` for the blocks ``Q`` and ``Y = A Q``
    and the eigenpairs ``theta [p]``, ``W [p, p]`` of ``Q^T Y``."""
    _require_gpu(Q, "modes_ritz")
    dev, N, p = Q.device, int(Q.shape[0]), int(Q.shape[1])
    ldq, ldy = _modes_block(Q, N, dev, "modes_ritz", "Q"), _modes_block(Y, N, dev, "modes_ritz", "Y")
    if Y.shape != Q.shape or tuple(theta.shape) != (p,) or tuple(W.shape) != (p, p):
        raise ValueError("sensorium_amd.modes_ritz: Q and Y [N, p], theta [p], W [p, p]")
    Wp = torch.zeros(p, L.MODES_MAXP, dtype=torch.float64, device=dev)
    Wp[:, :p] = W
    values = torch.zeros(L.MODES_MAXP, dtype=torch.float64, device=dev)
    values[:p] = theta
    residuals = torch.zeros(L.MODES_MAXP, dtype=torch.float64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    V = modes_block(N, p, dev)
    a = _modes_args(N, p, int(k))
    a.ldq, a.ldy, a.ldv, a.tol = ldq, ldy, modes_pad(p), float(tol)
    a.Q, a.Y, a.V, a.W, a.values, a.residuals, a.status = (Q.data_ptr(), Y.data_ptr(), V.data_ptr(), Wp.data_ptr(), values.data_ptr(),
                                                           residuals.data_ptr(), status.data_ptr())
    ws = _modes_ws(a, L.lib.dwn_modes_ritz_ws_bytes, dev)          # noqa: F841
    L.check(L.lib.dwn_modes_ritz(C.byref(a), dev.index, _stream(dev)), "dwn_modes_ritz")
    return V, residuals[:p], status


def modes_solve(A: torch.Tensor, k: int, p: int, max_iters: int = 64, tol: float = 1e-10, seed: int = 0, scale: float = 1.0):
    """dwn_modes_solve: block subspace iteration on ``scale * A`` with a block of ``p`` columns, stopping on the first ``k``.
    Returns ``(values [p], V [N, p], residuals [p], moments [2], status int32 [4])``, all on the device; nothing is read back."""
    dev, N = _modes_matrix(A, "modes_solve")
    k, p = int(k), int(p)
    V = modes_block(N, max(p, 1), dev)
    values = torch.zeros(L.MODES_MAXP, dtype=torch.float64, device=dev)
    residuals = torch.zeros(L.MODES_MAXP, dtype=torch.float64, device=dev)
    moments = torch.zeros(4, dtype=torch.float64, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    a = _modes_args(N, p, k)
    a.max_iters, a.tol, a.seed, a.scale = int(max_iters), float(tol), int(seed) & (2 ** 64 - 1), float(scale)
    a.lda, a.ldv = (int(A.stride(0)) if N > 1 else max(int(A.stride(0)), 1)), modes_pad(max(p, 1))
    a.A, a.V, a.values, a.residuals, a.moments, a.status = (A.data_ptr(), V.data_ptr(), values.data_ptr(), residuals.data_ptr(),
                                                            moments.data_ptr(), status.data_ptr())
    ws = _modes_ws(a, L.lib.dwn_modes_solve_ws_bytes, dev)         # noqa: F841
    L.check(L.lib.dwn_modes_solve(C.byref(a), dev.index, _stream(dev)), "dwn_modes_solve")
    return values[:p], V, residuals[:p], moments[:2], status


def modes_overlap(Va: torch.Tensor, Vb: torch.Tensor, B: Optional[torch.Tensor] = None, scale: float = 1.0):
    """dwn_modes_overlap: the singular values ``[k]`` of ``Va^T Vb`` (descending) for two blocks of ``k`` columns, and with ``B``
    also ``moments [3]`` = trace and squared Frobenius norm of ``scale * B`` and ``tr(Va^T (scale B) Va)``; else ``None``."""
    _require_gpu(Va, "modes_overlap")
    dev, N, k = Va.device, int(Va.shape[0]), int(Va.shape[1])
    lda_, ldb_ = _modes_block(Va, N, dev, "modes_overlap", "Va"), _modes_block(Vb, N, dev, "modes_overlap", "Vb")
    if Vb.shape != Va.shape:
        raise ValueError("sensorium_amd.modes_overlap: Va and Vb must have one shape")
    values = torch.zeros(L.MODES_MAXP, dtype=torch.float64, device=dev)
    moments = torch.zeros(4, dtype=torch.float64, device=dev)
    a = _modes_args(N, k, k)
    a.ldq, a.ldy, a.Q, a.Y, a.values, a.moments, a.scale = lda_, ldb_, Va.data_ptr(), Vb.data_ptr(), values.data_ptr(), moments.data_ptr(), float(scale)
    if B is not None:
        devb, Nb = _modes_matrix(B, "modes_overlap")
        if Nb != N or devb != dev:
            raise ValueError("sensorium_amd.modes_overlap: B must be [N, N] on the device of the blocks")
        a.A, a.lda = B.data_ptr(), (int(B.stride(0)) if N > 1 else max(int(B.stride(0)), 1))
    ws = _modes_ws(a, L.lib.dwn_modes_overlap_ws_bytes, dev)       # noqa: F841
    L.check(L.lib.dwn_modes_overlap(C.byref(a), dev.index, _stream(dev)), "dwn_modes_overlap")
    return values[:k], (moments[:3] if B is not None else None)


# ------------------------------------------------------------------------------------------------
# retinotopic readout gain (sensorium_amd/spatial.py)
# ------------------------------------------------------------------------------------------------
def _spatial_gain_args(y, g, pos, weight, bias, max_log_gain: float) -> L.SpatialGainArgs:
    a = L.SpatialGainArgs()
    a.B, a.N, a.T = (int(n) for n in y.shape)
    a.Hf, a.Wf, a.K = (int(n) for n in g.shape[2:])
    a.g_dtype = _DT[g.dtype]
    a.max_log_gain = float(max_log_gain)
    a.y = y.data_ptr(); a.g = g.data_ptr(); a.pos = pos.data_ptr(); a.weight = weight.data_ptr(); a.bias = bias.data_ptr()
    return a


class SpatialGainFn(torch.autograd.Function):
    """``SpatialGainFn.apply(y, g, pos, weight, bias, max_log_gain) -> y * exp(max_log_gain * tanh(bias[n] + weight[n,:] .
    sample(g[b,t], pos[n])))`` for a readout's output ``y`` [B][N][T], a channels-last map ``g`` [B][T][Hf][Wf][K] in fp32 or bf16,
    the per-neuron positions ``pos`` [N][2] = (x, y) in [-1, 1], weights [N][K] and offsets [N] (include/dwn.h
    dwn_spatial_gain_args).  ``sample`` is ``grid_sample(bilinear, border, align_corners=True)``.  The backward asks the kernels only
    for the gradients autograd needs; the map's gradient is a fixed-order float64 sum in fp32, cast to the map's dtype here."""

    @staticmethod
    def forward(ctx, y, g, pos, weight, bias, max_log_gain=1.0):
        for t in (y, g, pos, weight, bias):
            _require_gpu(t, "SpatialGainFn")
        if y.dim() != 3 or g.dim() != 5 or g.shape[:2] != (y.shape[0], y.shape[2]) or pos.shape != (y.shape[1], 2) \
                or weight.shape != (y.shape[1], g.shape[4]) or bias.shape != (y.shape[1],):
            raise RuntimeError("sensorium_amd.SpatialGainFn: y must be [B][N][T], g [B][T][Hf][Wf][K], pos [N][2], weight [N][K] "
                               "and bias [N]")
        if g.dtype not in _DT:
            raise RuntimeError("sensorium_amd.SpatialGainFn: the map must be fp32 or bf16")
        y = y.contiguous().float(); g = g.contiguous()
        pos = pos.contiguous().float(); weight = weight.contiguous().float(); bias = bias.contiguous().float()
        dev = y.device
        out = torch.empty_like(y)
        a = _spatial_gain_args(y, g, pos, weight, bias, max_log_gain)
        a.out = out.data_ptr()
        L.check(L.lib.dwn_spatial_gain_forward(C.byref(a), dev.index, _stream(dev)), "dwn_spatial_gain_forward")
        ctx.max_log_gain = float(max_log_gain)
        ctx.save_for_backward(y, g, pos, weight, bias)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        y, g, pos, weight, bias = ctx.saved_tensors
        need = ctx.needs_input_grad[:5]
        if not any(need):
            return None, None, None, None, None, None
        dev = dout.device
        dout = dout.contiguous().float()
        dy, dpos, dweight, dbias = (torch.empty_like(t) if n else None
                                    for t, n in zip((y, pos, weight, bias), (need[0], need[2], need[3], need[4])))
        dg = torch.empty(g.shape, dtype=torch.float32, device=dev) if need[1] else None
        a = _spatial_gain_args(y, g, pos, weight, bias, ctx.max_log_gain)
        nbytes = L.lib.dwn_spatial_gain_ws_bytes(C.byref(a))
        ws = torch.empty(max(int(nbytes), 16) // 8, dtype=torch.float64, device=dev)
        a.dout = dout.data_ptr(); a.dy = _ptr(dy); a.dg = _ptr(dg); a.dpos = _ptr(dpos); a.dweight = _ptr(dweight)
        a.dbias = _ptr(dbias)
        a.ws = ws.data_ptr(); a.ws_bytes = ws.numel() * 8
        L.check(L.lib.dwn_spatial_gain_backward(C.byref(a), dev.index, _stream(dev)), "dwn_spatial_gain_backward")
        if dg is not None and dg.dtype != g.dtype:
            dg = dg.to(g.dtype)
        return dy, dg, dpos, dweight, dbias, None


# ------------------------------------------------------------------------------------------------
# receptive-field mapping (sensorium_amd/receptive_fields.py, stimuli.NoiseStimulus)
# ------------------------------------------------------------------------------------------------
NOISE_KINDS = {"binary": L.NOISE_BINARY, "sparse": L.NOISE_SPARSE}


def noise_stimulus(template: torch.Tensor, *, kind: str = "binary", cell: int = 1, hold: int = 1, contrast: float = 64.0,
                   density: float = 0.1, background: float = 127.5, window=None, pad: float = 0.0, video_channel: int = 0,
                   seed: int = 0, first_clip: int = 0) -> torch.Tensor:
    """dwn_noise_forward: a copy of ``template`` [B][C][T][H][W] fp32 whose channel ``video_channel`` holds Philox noise cells
    inside ``window`` = (y0, x0, height, width) (default: the whole plane) and ``pad`` outside it.  Clip ``b`` is a function of
    ``(seed, first_clip + b)`` alone (include/dwn.h dwn_noise_args)."""
    _require_gpu(template, "noise_stimulus")
    if template.dim() != 5 or template.dtype != torch.float32:
        raise RuntimeError("sensorium_amd.noise_stimulus: template must be fp32 [B][C][T][H][W]")
    if kind not in NOISE_KINDS:
        raise ValueError(f"kind: one of {tuple(NOISE_KINDS)} (got {kind!r})")
    seed, first_clip = int(seed), int(first_clip)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must lie in [0, 2^64)")
    template = template.contiguous()
    dev = template.device
    a = L.NoiseArgs()
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in template.shape)
    if first_clip < 0 or first_clip + a.B > 1 << 32:
        raise ValueError("clip numbers must stay inside [0, 2^32): first_clip + batch <= 2^32")
    a.video_channel, a.kind, a.cell, a.hold = int(video_channel), NOISE_KINDS[kind], int(cell), int(hold)
    a.y0, a.x0, a.wh, a.ww = (int(n) for n in window) if window is not None else (0, 0, a.H, a.W)
    a.background, a.contrast, a.density, a.pad = float(background), float(contrast), float(density), float(pad)
    a.seed, a.first_clip = seed, first_clip
    out = torch.empty_like(template)
    a.x, a.out = template.data_ptr(), out.data_ptr()
    L.check(L.lib.dwn_noise_forward(C.byref(a), dev.index, _stream(dev)), "dwn_noise_forward")
    return out


def _sta_args(N: int, lags: int, window, cell: int) -> L.StaArgs:
    a = L.StaArgs()
    a.N, a.lags, a.cell = int(N), int(lags), int(cell)
    a.y0, a.x0, a.wh, a.ww = (int(n) for n in window)
    return a


def sta_state_numel(N: int, lags: int, window, cell: int) -> int:
    """float64 elements of the accumulator's state (dwn_sta_state_bytes / 8); raises for a geometry the entries refuse."""
    n = int(L.lib.dwn_sta_state_bytes(C.byref(_sta_args(N, lags, window, cell))))
    if n == 0:
        raise ValueError(f"sta: N = {N}, lags = {lags}, window = {tuple(window)}, cell = {cell} is not a geometry the kernels take")
    return n // 8


def sta_accumulate(state: torch.Tensor, x: torch.Tensor, r: torch.Tensor, *, lags: int, window, cell: int = 1, channel: int = 0,
                   skip: int = 0, s0: float = 127.5, r0: Optional[torch.Tensor] = None) -> int:
    """dwn_sta_accumulate: adds the lagged cross-sums and moments of one batch — ``x`` [B][C][T][H][W] fp32, ``r`` [B][N][T] fp32,
    ``r0`` [N] fp32 or None — to ``state`` (float64, ``sta_state_numel`` elements, zero before the first call) in place.  Returns
    the number of samples the call added, ``B * (T - max(skip, lags - 1))``.  No read-back."""
    for t in (state, x, r):
        _require_gpu(t, "sta_accumulate")
    if x.dim() != 5 or r.dim() != 3 or x.dtype != torch.float32 or r.dtype != torch.float32:
        raise RuntimeError("sensorium_amd.sta_accumulate: x must be fp32 [B][C][T][H][W] and r fp32 [B][N][T]")
    if r.shape[0] != x.shape[0] or r.shape[2] != x.shape[2]:
        raise ValueError(f"sensorium_amd.sta_accumulate: x {tuple(x.shape)} and r {tuple(r.shape)} disagree in batch or frames")
    x, r = x.contiguous(), r.contiguous()
    dev, N = x.device, int(r.shape[1])
    a = _sta_args(N, lags, window, cell)
    a.B, a.Cin, a.T, a.H, a.W = (int(n) for n in x.shape)
    a.channel, a.skip, a.s0 = int(channel), int(skip), float(s0)
    if state.dtype != torch.float64 or not state.is_contiguous() or state.numel() != sta_state_numel(N, lags, window, cell):
        raise RuntimeError("sensorium_amd.sta_accumulate: state must be contiguous float64 of sta_state_numel elements")
    if r0 is not None:
        _require_gpu(r0, "sta_accumulate")
        if r0.dtype != torch.float32 or r0.shape != (N,) or not r0.is_contiguous():
            raise RuntimeError("sensorium_amd.sta_accumulate: r0 must be contiguous fp32 [N]")
    a.x, a.r, a.r0, a.state = x.data_ptr(), r.data_ptr(), _ptr(r0), state.data_ptr()
    L.check(L.lib.dwn_sta_accumulate(C.byref(a), dev.index, _stream(dev)), "dwn_sta_accumulate")
    return a.B * (a.T - max(a.skip, a.lags - 1))


def sta_finalize(state: torch.Tensor, samples: int, *, N: int, lags: int, window, cell: int = 1, rel_threshold: float = 0.5,
                 z: bool = True):
    """dwn_sta_finalize: ``(cov, z or None, summary)`` — fp32 ``[N, lags, gh, gw]`` twice and float64 ``[N, STA_SUMMARY]``
    (include/dwn.h) — from the state and its sample count.  No read-back."""
    _require_gpu(state, "sta_finalize")
    if state.dtype != torch.float64 or not state.is_contiguous() or state.numel() != sta_state_numel(N, lags, window, cell):
        raise RuntimeError("sensorium_amd.sta_finalize: state must be contiguous float64 of sta_state_numel elements")
    dev = state.device
    a = _sta_args(N, lags, window, cell)
    a.samples, a.rel_threshold = int(samples), float(rel_threshold)
    gh, gw = a.wh // a.cell, a.ww // a.cell
    cov = torch.empty(N, lags, gh, gw, dtype=torch.float32, device=dev)
    zz = torch.empty_like(cov) if z else None
    summary = torch.empty(N, L.STA_SUMMARY, dtype=torch.float64, device=dev)
    ws = torch.empty(max(int(L.lib.dwn_sta_ws_bytes(C.byref(a))) // 8, 1), dtype=torch.float64, device=dev)
    a.state, a.cov, a.z, a.summary, a.ws, a.ws_bytes = state.data_ptr(), cov.data_ptr(), _ptr(zz), summary.data_ptr(), ws.data_ptr(), ws.numel() * 8
    L.check(L.lib.dwn_sta_finalize(C.byref(a), dev.index, _stream(dev)), "dwn_sta_finalize")
    return cov, zz, summary


def gauss2d_ws_numel(M: int, gh: int, gw: int, rows: int = 1) -> int:
    """float64 elements of the fit's workspace (dwn_gauss2d_ws_bytes / 8); raises for a geometry the entry refuses."""
    a = L.Gauss2dArgs()
    a.R, a.gh, a.gw, a.M = int(rows), int(gh), int(gw), int(M)
    n = int(L.lib.dwn_gauss2d_ws_bytes(C.byref(a)))
    if n == 0:
        raise ValueError(f"gauss2d: M = {M} maps of {gh} x {gw} cells is not a geometry the kernels take (3 <= gh, gw; gh gw <= 4096; M >= 1)")
    return n // 8


def gauss2d_fit(maps: torch.Tensor, sel: Optional[torch.Tensor] = None, *, fit_baseline: bool = True, rel_threshold: float = 0.5,
                max_iter: int = 100, xtol: float = 1e-8, ftol: float = 1e-12):
    """dwn_gauss2d_fit: ``(params, table, start)`` — float64 ``[M, GAUSS_PARAMS]``, ``[M, GAUSS_TABLE]`` and the workspace
    ``[M, 8]`` (the start vector and its S) — of the elliptical-Gaussian fits of the rows ``sel`` (an int32 device table, default
    all rows in order) of ``maps`` fp32 ``[R, gh, gw]`` (include/dwn.h).  One launch on the current stream; no read-back."""
    _require_gpu(maps, "gauss2d_fit")
    if maps.dim() != 3 or maps.dtype != torch.float32 or not maps.is_contiguous():
        raise RuntimeError("sensorium_amd.gauss2d_fit: maps must be contiguous fp32 [R][gh][gw]")
    dev = maps.device
    R, gh, gw = (int(n) for n in maps.shape)
    if sel is not None:
        _require_gpu(sel, "gauss2d_fit")
        if sel.dtype != torch.int32 or sel.dim() != 1 or not sel.is_contiguous() or sel.device != dev:
            raise RuntimeError("sensorium_amd.gauss2d_fit: sel must be a contiguous int32 [M] table on the maps' device")
    M = R if sel is None else int(sel.shape[0])
    a = L.Gauss2dArgs()
    a.R, a.gh, a.gw, a.M = R, gh, gw, M
    a.fit_baseline, a.max_iter = int(bool(fit_baseline)), int(max_iter)
    a.rel_threshold, a.xtol, a.ftol = float(rel_threshold), float(xtol), float(ftol)
    ws = torch.empty(gauss2d_ws_numel(M, gh, gw, R), dtype=torch.float64, device=dev)
    params = torch.empty(M, L.GAUSS_PARAMS, dtype=torch.float64, device=dev)
    table = torch.empty(M, L.GAUSS_TABLE, dtype=torch.float64, device=dev)
    a.maps, a.sel, a.params, a.table, a.ws, a.ws_bytes = maps.data_ptr(), _ptr(sel), params.data_ptr(), table.data_ptr(), ws.data_ptr(), ws.numel() * 8
    L.check(L.lib.dwn_gauss2d_fit(C.byref(a), dev.index, _stream(dev)), "dwn_gauss2d_fit")
    return params, table, ws.view(M, 8)


def gauss2d_profile(params: torch.Tensor, maps: torch.Tensor, *, fit_baseline: bool = True):
    """dwn_gauss2d_profile: ``(profile, separability)`` — float64 ``[N, L]`` and ``[N]`` — of ``maps`` fp32 ``[N, L, gh, gw]`` on the
    spatial shapes of ``params`` float64 ``[N, GAUSS_PARAMS]`` (include/dwn.h).  One launch on the current stream; no read-back."""
    _require_gpu(params, "gauss2d_profile")
    _require_gpu(maps, "gauss2d_profile")
    if maps.dim() != 4 or maps.dtype != torch.float32 or not maps.is_contiguous():
        raise RuntimeError("sensorium_amd.gauss2d_profile: maps must be contiguous fp32 [N][L][gh][gw]")
    N, lags, gh, gw = (int(n) for n in maps.shape)
    if params.dtype != torch.float64 or tuple(params.shape) != (N, L.GAUSS_PARAMS) or not params.is_contiguous() or params.device != maps.device:
        raise RuntimeError(f"sensorium_amd.gauss2d_profile: params must be contiguous float64 [{N}][{L.GAUSS_PARAMS}] on the maps' device")
    dev = maps.device
    a = L.Gauss2dProfileArgs()
    a.N, a.L, a.gh, a.gw, a.fit_baseline = N, lags, gh, gw, int(bool(fit_baseline))
    profile = torch.empty(N, lags, dtype=torch.float64, device=dev)
    sep = torch.empty(N, dtype=torch.float64, device=dev)
    a.params, a.maps, a.profile, a.separability = params.data_ptr(), maps.data_ptr(), profile.data_ptr(), sep.data_ptr()
    L.check(L.lib.dwn_gauss2d_profile(C.byref(a), dev.index, _stream(dev)), "dwn_gauss2d_profile")
    return profile, sep

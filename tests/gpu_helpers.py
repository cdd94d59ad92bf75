"""Helpers shared by the GPU parity tests (imported only by tests)."""
import ctypes as C
import math

import numpy as np
import torch

from oracle import dwiseneuro_oracle as orc


def rel(a, b):
    a = a.detach().double().cpu().reshape(-1)
    b = b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-30))


def tol(dtype, f32=1e-3, bf16=4e-2):
    return f32 if dtype == torch.float32 else bf16


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def stats_buffer(c):
    return torch.zeros(32 * 2 * c, dtype=torch.float64, device=dev())


def read_stats(buf, c):
    s = buf.view(32, 2, c).sum(0)
    return s[0], s[1]


def load_desc(L, p, ld, **kw):
    d = L.LoadDesc()
    d.p = p.data_ptr()
    d.ld = ld
    d.rows_per_sample = 1
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    return d


def sd_to_module(module, sd):
    missing = module.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return module


NUM_NEURONS_ALL = (7863, 7908, 8202, 7939, 8122, 7440, 7928, 8285, 7671, 7495)      # src/constants.py:18,26,38


def synth_inputs(rng, b, t, h, w, readout_outputs):
    """The synthetic clip generator of oracle/make_golden.py (same draw order), restated here because that script imports
    the reference and cannot run on the GPU box: ch0 video 0..255, ch1-4 per-(b,t) scalars broadcast over HxW."""
    x = np.zeros((b, 5, t, h, w), dtype=np.float32)
    x[:, 0] = rng.integers(0, 256, size=(b, t, h, w)).astype(np.float32)
    scale = np.array([10, 5, 20, 20], dtype=np.float32)
    shift = np.array([30, 5, 100, 70], dtype=np.float32)
    beh = np.clip(rng.normal(size=(b, 4, t)).astype(np.float32) * scale[None, :, None] + shift[None, :, None], 0, None)
    x[:, 1:] = beh[:, :, :, None, None]
    targets = [np.maximum(rng.normal(size=(b, n, t)), 0).astype(np.float32) * 10 for n in readout_outputs]
    weights = np.zeros((b, len(readout_outputs)), dtype=np.float32)
    for i in range(b):
        weights[i, i % len(readout_outputs)] = 1.0
    return x, targets, weights


def analytically_zero_grad(name: str) -> bool:
    """The 21 parameters whose gradient is identically zero: a per-channel bias whose only consumers are
    BatchNorms reached through linear ops (stem BN bias; each block's two output BN biases; the shortcut BN bias of the first
    two cortex layers).  What the kernels compute for them is summation noise; relative comparisons skip them."""
    import re as _re
    return bool(name == "core.stem.1.bn.bias" or _re.fullmatch(r"core\.blocks\.\d+\.(conv_pwl\.1\.bn|bn_sc\.bn)\.bias", name)
                or _re.fullmatch(r"cortex\.layers\.[01]\.bn_sc\.bn\.bias", name))


# ------------------------------------------------------------------------------------------------
# inputs of the tail tests (pool ... AdamW/EMA): built here because tests/test_gpu_tail.py runs them on the device and
# tests/test_tail_reference_cpu.py checks on the CPU that the same inputs would catch the errors they are meant to catch
# ------------------------------------------------------------------------------------------------
EMA_DECAYS = (0.99, 0.999, 0.9999)
TAIL_F32_BOUND = 1e-3            # the standing fp32 bound (norm-relative, and per neuron in the low-rate readout case)
TAIL_BF16_NEURON_BOUND = 2.0 ** -8   # low-rate readout in bf16: every dz term is rounded to bf16 (8 significant bits: unit roundoff
                                     # 2^-8) before it is summed into dbias, so sum |error| <= 2^-8 sum |dz| (the fp32 part is 2e-6)
ADAMW_BOUND = 1e-6               # tests/test_gpu_model.py::test_adamw_ema_multi_matches_reference


def ema_int_pairs():
    """Every pair (ema, model) with ema in 0..2999 and model in {ema, ema + 1, ema + 7}: int64 [9000] each."""
    e = torch.arange(3000, dtype=torch.int64).repeat_interleave(3)
    m = e + torch.tensor([0, 1, 7], dtype=torch.int64).repeat(3000)
    return e, m


def ema_int_separate(ema, model, decay):
    """The reference's arithmetic spelled out (ema.py:47-55): two float32 products, each rounded, a rounded sum, truncation."""
    d, o = np.float32(decay), np.float32(1.0 - decay)
    a = (d * ema.numpy().astype(np.float32)).astype(np.float32)
    b = (o * model.numpy().astype(np.float32)).astype(np.float32)
    return torch.from_numpy((a + b).astype(np.float32).astype(np.int64))


def ema_int_contracted(ema, model, decay):
    """What a fused multiply-add makes of the same line (v_mul_f32 of one product, v_fmac_f32 of the other): decay * ema is not
    rounded before the sum.  float64 holds a 24 x 24 bit product exactly, so the float64 sum is rounded once."""
    d, o = np.float32(decay), np.float32(1.0 - decay)
    b = (o * model.numpy().astype(np.float32)).astype(np.float32)
    s = np.float64(d) * ema.numpy().astype(np.float64) + b.astype(np.float64)
    return torch.from_numpy(s.astype(np.float32).astype(np.int64))


def ema_trajectory(steps, decay, width=3):
    """Model counters of a run, [steps][width] int64: column 0 counts 1, 2, 3, ... (num_batches_tracked of a training run),
    the others count in other strides so that a multi-element tensor is not three copies of one value."""
    k = torch.arange(1, steps + 1, dtype=torch.int64)
    return torch.stack([k * (j + 1) + 5 * j for j in range(width)], dim=1).contiguous()


def low_rate_bias(beta):
    """Readout biases whose pre-activation beta * z runs over [-30, 25] in steps of 0.5 (across softplus' threshold at 20):
    with zero weights z is the bias itself.  float32 [111]."""
    bz = torch.arange(-30.0, 25.25, 0.5, dtype=torch.float64)
    return (bz / beta).float()


def adamw_case(seed, sizes, step0):
    """float32 inputs of one optimizer run: per tensor p, m, v, ema and ten gradients.  step0 > 1 starts from moments as a run has
    them (m of the gradients' scale, v positive); step0 == 1 from zero moments."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        p = torch.randn(n, generator=g) * 0.1
        grads = [torch.randn(n, generator=g) * 0.02 for _ in range(10)]
        if step0 == 1:
            m, v = torch.zeros(n), torch.zeros(n)
        else:
            m = torch.randn(n, generator=g) * 0.005
            v = (torch.randn(n, generator=g) * 0.02) ** 2 + 1e-6
        out.append(dict(p=p, m=m, v=v, ema=p.clone() + torch.randn(n, generator=g) * 0.001, grads=grads))
    return out


def adamw_reference(case, step0, lr, wd, decay, grad_scale, dtype=torch.float64, has_ema=None):
    """Ten steps of oracle.adamw_step + oracle.ema_update from `case`; dtype float64 is the reference, float32 the same
    formulas with every state rounded to float32 (what storing the state in float32 costs by itself)."""
    res = []
    for i, c in enumerate(case):
        p, m, v, e = (c[k].to(dtype) for k in ("p", "m", "v", "ema"))
        for s in range(10):
            gr = c["grads"][s].to(dtype) * grad_scale
            p, m, v = orc.adamw_step(p, gr, m, v, step0 + s, lr, weight_decay=wd)
            if has_ema is None or has_ema[i]:
                e = orc.ema_update(e, p, decay)
        res.append(dict(p=p, m=m, v=v, ema=e))
    return res


def qround(t, dtype):
    """t rounded to `dtype`, kept in float32: the value both the kernel (which stores / packs it in dtype) and the reference see."""
    return t.float().to(dtype).float()


def pool_reference(x64, dout64):
    """x [BT][HW][C] -> mean over HW (oracle.forward: x.mean(dim=(2, 3))), and its gradient by autograd."""
    x = x64.clone().requires_grad_()
    out = x.mean(dim=1)
    out.backward(dout64)
    return out.detach(), x.grad


def cortex_inputs(seed, dtype, B, T, Cin, Cc, groups, drop, mask, offset=0.0, keep=None):
    g = torch.Generator().manual_seed(seed)
    Kg = Cin // groups
    r = lambda *s: torch.randn(*s, generator=g)
    d = dict(x=qround(r(B, T, Cin) + offset, dtype), w=qround(r(Cc, Kg) / Kg ** 0.5, dtype), dout=qround(r(B, T, Cc), dtype))
    for p in ("bn", "bnsc"):
        d[p] = dict(weight=1 + 0.2 * r(Cc), bias=0.3 * r(Cc), running_mean=0.3 * r(Cc) + (offset if p == "bnsc" else 0.0),
                    running_var=0.5 + torch.rand(Cc, generator=g), num_batches_tracked=torch.tensor(5, dtype=torch.int64))
    d["drop_scale"] = d["dout_mask"] = None
    if drop:       # DropPath factor per sample (0 or 1/keep); sample 0 is dropped whenever there is a second one
        ds = (torch.rand(B, generator=g) < 0.7).float() / 0.7
        ds[0] = 0.0 if B > 1 else 1 / 0.7
        if keep is not None:       # (a sample that must stay: with two samples the draw may drop both)
            ds[keep] = 1 / 0.7
        d["drop_scale"] = ds
    if mask:       # the readout's Dropout1d factor on dout, [B][C], 0 or 1/keep
        d["dout_mask"] = (torch.rand(B, Cc, generator=g) < 0.6).float() / 0.6
    return d


def cortex_reference(d, groups, training):
    """oracle.cortex_layer in float64 and autograd through it.  training False is both the eval forward and the frozen-statistics
    backward (BatchNorm a fixed affine map)."""
    pre = "cortex.layers.0"
    sd, leaves = {}, {}
    leaves["w"] = d["w"].double()[:, :, None].clone().requires_grad_()
    sd[pre + ".conv.weight"] = leaves["w"]
    for p, name in (("bn", ".bn.bn"), ("bnsc", ".bn_sc.bn")):
        for k, v in d[p].items():
            t = v.double() if v.is_floating_point() else v.clone()
            if k in ("weight", "bias"):
                t = t.clone().requires_grad_()
                leaves[p + "." + k] = t
            sd[pre + name + "." + k] = t
    x = d["x"].double().clone().requires_grad_()
    ns = {}
    ds = None if d["drop_scale"] is None else d["drop_scale"].double()
    out = orc.cortex_layer(x, pre, sd, groups, training, ds, ns)
    gout = d["dout"].double()
    if d["dout_mask"] is not None:
        gout = gout * d["dout_mask"].double()[:, None, :]
    out.backward(gout)
    res = dict(out=out.detach(), dx=x.grad, dw=leaves["w"].grad[:, :, 0])
    for p in ("bn", "bnsc"):
        res[p + ".dgamma"], res[p + ".dbeta"] = leaves[p + ".weight"].grad, leaves[p + ".bias"].grad
    for p, name in (("bn", ".bn.bn"), ("bnsc", ".bn_sc.bn")):
        for k in ("running_mean", "running_var", "num_batches_tracked"):
            if pre + name + "." + k in ns:
                res[p + "." + k] = ns[pre + name + "." + k]
    return res


def readout_inputs(seed, dtype, B, T, Cin, groups, n_out, beta, mask):
    g = torch.Generator().manual_seed(seed)
    Kg, npad = Cin // groups, (n_out + groups - 1) // groups * groups
    r = lambda *s: torch.randn(*s, generator=g)
    zs = 2.0 / beta                # beta * z of a few units either way: the curved part of softplus, both tails reached
    d = dict(x=qround(r(B, T, Cin), dtype), w=qround(r(npad, Kg) * (zs / Kg ** 0.5), dtype), bias=r(npad) * zs,
             dout=r(B, n_out, T), drop_mask=None)
    if mask:                       # Dropout1d factor [B][Cin], 0 or 1/keep; channel 3 is dropped in every sample
        m = (torch.rand(B, Cin, generator=g) < 0.6).float() / 0.6
        m[:, 3] = 0.0
        d["drop_mask"] = m
    return d


def readout_reference(d, groups, n_out, beta):
    pre = "readouts.0"
    w = d["w"].double()[:, :, None].clone().requires_grad_()
    b = d["bias"].double().clone().requires_grad_()
    x = d["x"].double().clone().requires_grad_()
    dm = None if d["drop_mask"] is None else d["drop_mask"].double()
    out = orc.readout(x, pre, {pre + ".layer.1.weight": w, pre + ".layer.1.bias": b}, groups, n_out, beta, dm)
    out.backward(d["dout"].double())
    return dict(out=out.detach(), dx=x.grad, dw=w.grad[:, :, 0], dbias=b.grad)


def low_rate_reference(bias, beta, B, T, target=None, w=None):
    """Zero readout weights: z[b][t][n] = bias[n].  out = oracle.softplus(z); dout is the Poisson gradient (target None: a target
    of 0 with weights 1, which is 1 everywhere).  Returns out [B][N][T], dout, dz, dbias = sum dz and sum |dz| per neuron, float64."""
    z = bias.double()[None, None, :].expand(B, T, -1).clone().requires_grad_()
    out = orc.softplus(z, beta).permute(0, 2, 1)
    if target is None:
        loss = out.sum()
    else:
        loss = orc.mice_poisson_loss([out], [target.double()], w.double()[:, None])
    out.retain_grad()
    loss.backward()
    return dict(out=out.detach(), dout=out.grad, dbias=z.grad.sum((0, 1)), sumabs=z.grad.abs().sum((0, 1)))


def poisson_inputs(seed, B, per_sample, kind):
    """Predictions log-uniform over 1e-7 ... 1e3, targets with exact zeros, sample weights of one of three kinds (normalised)."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.exp(torch.empty(B, per_sample).uniform_(math.log(1e-7), math.log(1e3), generator=g))
    target = torch.clamp(torch.randn(B, per_sample, generator=g), min=0) * 10
    if kind == "equal":
        w = torch.ones(B)
    elif kind == "onehot":         # one mouse of ten: most samples carry weight exactly 0
        w = (torch.arange(B) % 10 == 0).float()
    else:
        w = torch.rand(B, generator=g) + 0.05
    return pred, target, (w / w.sum()).float()


def poisson_reference(pred, target, w, gscale=1.0):
    x = pred.double().clone().requires_grad_()
    loss = orc.mice_poisson_loss([x[:, :, None]], [target.double()[:, :, None]], w.double()[:, None])
    (loss * gscale).backward()
    return loss.detach() * float(w.double().sum()), x.grad * float(w.double().sum())

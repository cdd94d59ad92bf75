"""Float64 checker of the regularised-MEI kernels (include/dwn.h dwn_blur3d, dwn_clip_moments,
dwn_mei_update), in plain torch on the CPU.  Everything works on ONE channel: tensors are [B, T, H, W].

tests/test_mei_reference_cpu.py holds these functions to independent definitions (conv3d, numpy longdouble, a restatement);
the GPU tests hold the kernels to these functions."""
import torch

MAX_RADIUS = 16


def resolve_window(H, W, window):
    return (0, 0, H, W) if window is None else tuple(int(n) for n in window)


def _shifted_sum(x, k, axis):
    """out[..., p, ...] = sum_i k[i] x[..., p + i - R, ...] with zeros outside, R = len(k) // 2."""
    k = torch.as_tensor(k, dtype=torch.float64)
    R, L = k.numel() // 2, x.shape[axis]
    pad_shape = list(x.shape)
    pad_shape[axis] = R
    z = torch.zeros(pad_shape, dtype=torch.float64)
    xp = torch.cat([z, x, z], dim=axis)
    out = torch.zeros_like(x)
    for i in range(k.numel()):
        out = out + k[i] * xp.narrow(axis, i, L)
    return out


def blur3d_ref(src, taps, window=None, absolute=False):
    """[B, T, H, W] -> float64 [B, T, H, W]: the three-axis filter with the source zero outside the window and outside [0, T),
    and zero written outside the window.  ``absolute``: |taps| on |src| (the scale of the rounding bound)."""
    x = src.detach().cpu().to(torch.float64)
    y0, x0, wh, ww = resolve_window(x.shape[2], x.shape[3], window)
    v = x[:, :, y0:y0 + wh, x0:x0 + ww]
    if absolute:
        v = v.abs()
    for axis, k in zip((3, 2, 1), (taps[2], taps[1], taps[0])):
        k = torch.as_tensor(k, dtype=torch.float64)
        v = _shifted_sum(v, k.abs() if absolute else k, axis)
    out = torch.zeros_like(x)
    out[:, :, y0:y0 + wh, x0:x0 + ww] = v
    return out


def blur3d_bound(src, taps, window=None):
    """Per-element bound of |device - blur3d_ref|: (nt + nh + nw + 3) 2^-24 (|kt| x |kh| x |kw| |src|)."""
    n = sum(len(k) for k in taps) + 3
    return n * 2.0 ** -24 * blur3d_ref(src, taps, window, absolute=True)


def moments_ref(x, window=None):
    """[B, T, H, W] -> float64 [B, 4] = (n, mean, M2, S2) over the window: the mean first, then the centred sum."""
    x = x.detach().cpu().to(torch.float64)
    y0, x0, wh, ww = resolve_window(x.shape[2], x.shape[3], window)
    v = x[:, :, y0:y0 + wh, x0:x0 + ww].reshape(x.shape[0], -1)
    n = v.shape[1]
    mean = v.sum(dim=1) / n
    m2 = ((v - mean[:, None]) ** 2).sum(dim=1)
    s2 = (v * v).sum(dim=1)
    return torch.stack([torch.full_like(mean, n), mean, m2, s2], dim=1)


def _apply_window(x, new, window):
    y0, x0, wh, ww = resolve_window(x.shape[2], x.shape[3], window)
    out = x.detach().cpu().to(torch.float32).clone()
    out[:, :, y0:y0 + wh, x0:x0 + ww] = new[:, :, y0:y0 + wh, x0:x0 + ww]
    return out


def step_ref(x, g, stat_g, lr, window=None):
    """x += lr g / sqrt(S2 / n) per clip inside the window (no step where S2 == 0), evaluated in float64, rounded once to fp32.
    A clip with a non-finite S2 becomes NaN inside its window."""
    xd = x.detach().cpu().to(torch.float64)
    gd = g.detach().cpu().to(torch.float64)
    n, s2 = stat_g[:, 0], stat_g[:, 3]
    c = torch.where(s2 > 0, 1.0 / torch.sqrt(s2 / n), torch.zeros_like(s2))
    new = xd + float(lr) * gd * c.view(-1, 1, 1, 1)
    new = torch.where((s2 == 0).view(-1, 1, 1, 1), xd, new)
    new = torch.where(torch.isfinite(s2).view(-1, 1, 1, 1), new, torch.full_like(new, float("nan")))
    return _apply_window(x, new.to(torch.float32), window)


def project_scale(stat_x, mean, contrast, contrast_mode):
    """(m [B], s [B]) of the projection from the moments of the stepped clip."""
    n, mu, m2 = stat_x[:, 0], stat_x[:, 1], stat_x[:, 2]
    sd = torch.sqrt(m2 / n)
    m = mu.clone() if mean is None else torch.full_like(mu, float(mean))
    s = torch.ones_like(mu)
    if contrast is not None:
        ratio = float(contrast) / sd
        if contrast_mode == "fixed":
            s = torch.where(sd == 0, torch.zeros_like(sd), ratio)
        else:
            s = torch.where(sd == 0, torch.ones_like(sd), torch.minimum(torch.ones_like(sd), ratio))
    return m, s


def project_ref(x, stat_x, mean=None, contrast=None, contrast_mode="max", lo=0.0, hi=255.0, window=None, clamp=True):
    """x = clamp((float)(m + s (x - mu)), lo, hi) inside the window; a clip that the projection does not bind (s == 1, m == mu)
    is only clamped; a clip with a non-finite statistic becomes NaN.  ``clamp=False`` returns the value before the clamp."""
    xd = x.detach().cpu().to(torch.float64)
    mu = stat_x[:, 1]
    m, s = project_scale(stat_x, mean, contrast, contrast_mode)
    new = (m.view(-1, 1, 1, 1) + s.view(-1, 1, 1, 1) * (xd - mu.view(-1, 1, 1, 1))).to(torch.float32)
    free = ((s == 1) & (m == mu)).view(-1, 1, 1, 1)
    new = torch.where(free, x.detach().cpu().to(torch.float32), new)
    if clamp:
        new = new.clamp(lo, hi)
    fin = (torch.isfinite(mu) & torch.isfinite(stat_x[:, 2])).view(-1, 1, 1, 1)
    new = torch.where(fin, new, torch.full_like(new, float("nan")))
    return _apply_window(x, new, window)


def ulp32(v):
    """The spacing of fp32 at |v| (float64 tensor in, float64 out); the smallest normal's spacing below it."""
    a = v.abs().to(torch.float64).clamp_min(2.0 ** -126)
    return 2.0 ** (torch.floor(torch.log2(a)) - 23)

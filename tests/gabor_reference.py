"""Float64 checker of the drifting-Gabor stimulus (include/dwn.h dwn_gabor_args), in torch on the CPU.

``render`` evaluates the definition, ``param_jacobian`` the analytic derivatives of ``raw`` w.r.t. the eight parameters per element,
``dparams`` the reduction of an incoming gradient through the clamp mask.  tests/test_gabor_reference_cpu.py holds the analytic
derivatives to autograd of an independently written form and to central differences.  Parameters enter as given (float32 values
are converted exactly), so the checker sees the very numbers the kernels see.
"""
import math

import torch

PARAM_NAMES = ("cy", "cx", "sigma", "theta", "sf", "tf", "phase", "amplitude")
TAU = 2.0 * math.pi
U = 2.0 ** -24


def _grid(T, H, W):
    t = torch.arange(T, dtype=torch.float64).view(1, T, 1, 1)
    y = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    x = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    return t, y, x


def _cols(params):
    p = params.double()
    return [p[:, k].view(-1, 1, 1, 1) for k in range(8)]


def window_mask(H, W, window):
    m = torch.zeros(H, W, dtype=torch.bool)
    y0, x0, wh, ww = window if window is not None else (0, 0, H, W)
    m[y0:y0 + wh, x0:x0 + ww] = True
    return m


def healthy(params, envelope):
    """[B] bool: every parameter finite, and sigma > 0 under the Gaussian envelope."""
    p = params.double()
    ok = torch.isfinite(p).all(dim=1)
    if envelope == "gaussian":
        ok = ok & (p[:, 2] > 0)
    return ok


def parts(params, T, H, W, envelope="gaussian"):
    """The per-element pieces [B][T][H][W] in float64: dyp, dxp, u, q, envelope e, cos C, sin S of 2 pi q."""
    cy, cx, sigma, theta, sf, tf, phase, amp = _cols(params)
    t, y, x = _grid(T, H, W)
    dyp, dxp = (y - cy).expand(-1, T, H, W), (x - cx).expand(-1, T, H, W)
    u = dxp * torch.cos(theta) + dyp * torch.sin(theta)
    q = sf * u - tf * t + phase / TAU
    e = torch.exp(-(dxp ** 2 + dyp ** 2) / (2.0 * sigma ** 2)) if envelope == "gaussian" else torch.ones_like(q)
    return dyp, dxp, u, q, e, torch.cos(TAU * q), torch.sin(TAU * q)


def raw_video(params, T, H, W, envelope="gaussian", background=127.5):
    """raw [B][T][H][W] float64 (unclamped, window ignored)."""
    amp = _cols(params)[7]
    _, _, _, _, e, c, _ = parts(params, T, H, W, envelope)
    return background + amp * e * c


def render(params, template, video_channel=0, envelope="gaussian", background=127.5, video_range=(0.0, 255.0), window=None,
           pad=0.0):
    """The model input in float64: ``template`` with channel ``video_channel`` replaced by the stimulus."""
    B, Cin, T, H, W = template.shape
    raw = raw_video(params, T, H, W, envelope, background)
    vid = raw if video_range is None else raw.clamp(video_range[0], video_range[1])
    vid = torch.where(healthy(params, envelope).view(B, 1, 1, 1), vid, torch.full_like(vid, math.nan))
    vid = torch.where(window_mask(H, W, window), vid, torch.full_like(vid, float(pad)))
    out = template.double().clone()
    out[:, video_channel] = vid
    return out


def pass_mask(params, T, H, W, envelope="gaussian", background=127.5, video_range=(0.0, 255.0), window=None):
    """[B][T][H][W] bool: inside the window and lo <= raw <= hi (torch.clamp passes the gradient at equality)."""
    m = window_mask(H, W, window).expand(params.shape[0], T, H, W)
    if video_range is not None:
        raw = raw_video(params, T, H, W, envelope, background)
        m = m & (raw >= video_range[0]) & (raw <= video_range[1])
    return m


def param_jacobian(params, T, H, W, envelope="gaussian"):
    """d raw / d p_k, [B][8][T][H][W] float64 (unclamped, window ignored)."""
    cy, cx, sigma, theta, sf, tf, phase, amp = _cols(params)
    t, _, _ = _grid(T, H, W)
    dyp, dxp, u, q, e, c, s = parts(params, T, H, W, envelope)
    ct, st = torch.cos(theta), torch.sin(theta)
    aes = amp * e * s * TAU                      # -d raw / d q
    J = torch.zeros(params.shape[0], 8, T, H, W, dtype=torch.float64)
    J[:, 0] = aes * sf * st
    J[:, 1] = aes * sf * ct
    if envelope == "gaussian":
        aec = amp * e * c
        J[:, 0] += aec * dyp / sigma ** 2
        J[:, 1] += aec * dxp / sigma ** 2
        J[:, 2] = aec * (dxp ** 2 + dyp ** 2) / sigma ** 3
    J[:, 3] = -aes * sf * (dyp * ct - dxp * st)
    J[:, 4] = -aes * u
    J[:, 5] = aes * t
    J[:, 6] = -amp * e * s
    J[:, 7] = e * c
    return J


def q_magnitude(params, T, H, W):
    """Q = |sf| (|dxp| + |dyp|) + |tf| t + |phase| / (2 pi), [B][T][H][W]: the size of the terms whose roundings make up q."""
    cy, cx, sigma, theta, sf, tf, phase, amp = _cols(params)
    t, y, x = _grid(T, H, W)
    return sf.abs() * ((x - cx).abs() + (y - cy).abs()) + tf.abs() * t + phase.abs() / TAU


def forward_floor(params, out_video, T, H, W):
    """2^-24 |amplitude| (1 + 2 pi Q) + ulp(out) per element of the video channel (fp32 ulp of the float64 result)."""
    amp = _cols(params)[7]
    ulp = torch.ldexp(torch.ones_like(out_video), (torch.frexp(out_video.abs().clamp_min(2.0 ** -126))[1] - 24).to(torch.int32))
    return U * amp.abs() * (1.0 + TAU * q_magnitude(params, T, H, W)) + ulp


def dparams(dout, params, video_channel=0, envelope="gaussian", background=127.5, video_range=(0.0, 255.0), window=None,
            with_floor=False):
    """dparams [B][8] float64 = sum over t, y, x of dout * d out / d p_k; NaN rows for degenerate clips.  ``with_floor``: also
    sum (1 + 2 pi Q) |dout * d out / d p_k|, the magnitude the backward's bound is a multiple of (times 2^-24)."""
    B, Cin, T, H, W = dout.shape
    g = dout[:, video_channel].double()
    g = torch.where(pass_mask(params, T, H, W, envelope, background, video_range, window), g, torch.zeros_like(g))
    terms = param_jacobian(params, T, H, W, envelope) * g[:, None]
    ok = healthy(params, envelope).view(B, 1)
    dp = torch.where(ok, terms.sum(dim=(2, 3, 4)), torch.full((B, 8), math.nan, dtype=torch.float64))
    if not with_floor:
        return dp
    weight = (1.0 + TAU * q_magnitude(params, T, H, W))[:, None]
    return dp, (terms.abs() * weight).sum(dim=(2, 3, 4))

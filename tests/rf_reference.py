"""Float64 checker of the receptive-field mapping: the Philox noise stimulus bit for bit, the lagged
cross-sums and moments in float64 from operands formed exactly as the kernels form them (u and v in fp32), the finaliser, and the
a-priori error bounds the GPU tests assert at.  numpy only; written for this project and held to brute force by
tests/test_rf_reference_cpu.py.

Definitions (include/dwn.h): cell q = gy * gw + gx of frame t of clip b takes word q & 3 of
philox4x32-10(counter = (q >> 2, t // hold, first_clip + b, 0), key = (seed & 0xffffffff, seed >> 32));
u = r - r0 and v = (fp32 row-major sum of the cell's pixels) * (1 / cell^2) - s0, each step rounded to fp32;
valid frames t in [t0, T), t0 = max(skip, lags - 1); state Cuv, U1, U2, V1, V2; cov = (Cuv - U1 (V1 / K)) / K."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53          # unit roundoffs
KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                  (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox_scalar(counter, key):
    """Philox4x32-10 on Python integers: (c0, c1, c2, c3), (k0, k1) -> four 32-bit words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox(c0, c1, c2, c3, key):
    """The same on broadcastable integer arrays; returns uint32 [..., 4]."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3)))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m, s = np.uint64(MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> s) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def noise_words(batch, frames, gh, gw, *, hold=1, seed=0, first_clip=0):
    """uint32 [batch, frames, gh * gw]: the word of every cell."""
    G = gh * gw
    nblk = (G + 3) // 4
    key = (seed & MASK, (seed >> 32) & MASK)
    blk = np.arange(nblk, dtype=np.uint64)[None, None, :]
    step = (np.arange(frames, dtype=np.uint64) // np.uint64(hold))[None, :, None]
    clip = (np.uint64(first_clip) + np.arange(batch, dtype=np.uint64))[:, None, None]
    w = philox(blk, step, clip, np.uint64(0), key)              # [B, T, nblk, 4]
    return w.reshape(batch, frames, nblk * 4)[:, :, :G]


def noise_values(words, kind, background, contrast, density):
    """fp32 grey levels of the cells from their words."""
    bg, ct = np.float32(background), np.float32(contrast)
    lo, hi = np.float32(bg - ct), np.float32(bg + ct)
    w = words.astype(np.uint64)
    if kind == "binary":
        return np.where(w >> np.uint64(31) != 0, hi, lo).astype(np.float32)
    if kind != "sparse":
        raise ValueError(kind)
    thr = int(np.floor(float(np.float32(density)) * 2.0 ** 31))
    out = np.full(w.shape, bg, dtype=np.float32)
    out[w < np.uint64(thr)] = lo
    out[w >= np.uint64(2 ** 32 - thr)] = hi
    return out


def noise(batch, frames, size, *, kind="binary", cell=1, hold=1, contrast=64.0, density=0.1, background=127.5, window=None,
          pad=0.0, behavior=(0.0, 0.0), pupil_center=(0.0, 0.0), in_channels=5, video_channel=0, seed=0, first_clip=0):
    """The model input [batch, in_channels, frames, H, W] fp32 of stimuli.NoiseStimulus."""
    H, W = size
    y0, x0, wh, ww = window if window is not None else (0, 0, H, W)
    assert wh % cell == 0 and ww % cell == 0 and first_clip + batch <= 2 ** 32 and 0 <= seed < 2 ** 64
    gh, gw = wh // cell, ww // cell
    vals = noise_values(noise_words(batch, frames, gh, gw, hold=hold, seed=seed, first_clip=first_clip), kind, background, contrast,
                        density).reshape(batch, frames, gh, gw)
    x = np.zeros((batch, in_channels, frames, H, W), dtype=np.float32)
    others = [c for c in range(in_channels) if c != video_channel]
    for c, v in zip(others, (*behavior, *pupil_center)):
        x[:, c] = np.float32(v)
    x[:, video_channel] = np.float32(pad)
    x[:, video_channel, :, y0:y0 + wh, x0:x0 + ww] = np.repeat(np.repeat(vals, cell, axis=2), cell, axis=3)
    return x


# ------------------------------------------------------------------------------------------------------------------------------
def cell_values(x, channel, window, cell, s0):
    """v [B, T, gh * gw] fp32, formed as the kernel forms it."""
    y0, x0, wh, ww = window
    vid = np.asarray(x, dtype=np.float32)[:, channel, :, y0:y0 + wh, x0:x0 + ww]
    s = np.zeros(vid[:, :, ::cell, ::cell].shape, dtype=np.float32)
    for dy in range(cell):
        for dx in range(cell):
            s = (s + vid[:, :, dy::cell, dx::cell]).astype(np.float32)
    m = (s * (np.float32(1.0) / np.float32(cell * cell))).astype(np.float32)
    v = (m - np.float32(s0)).astype(np.float32)
    return v.reshape(v.shape[0], v.shape[1], -1)


class State:
    """The float64 state of the accumulator, with the sums of magnitudes the error bounds need."""

    def __init__(self, N, lags, gh, gw):
        self.N, self.L, self.gh, self.gw = N, lags, gh, gw
        G = gh * gw
        self.Cuv = np.zeros((N, lags, G)); self.U1 = np.zeros(N); self.U2 = np.zeros(N)
        self.V1 = np.zeros((lags, G)); self.V2 = np.zeros((lags, G))
        self.K = 0
        self.absC = np.zeros((N, lags, G)); self.absU = np.zeros(N); self.absV = np.zeros((lags, G))
        self.bound_C = np.zeros((N, lags, G))       # fp32 chain of the device, summed over calls
        self.bound_U1 = np.zeros(N); self.bound_U2 = np.zeros(N)
        self.bound_V1 = np.zeros((lags, G)); self.bound_V2 = np.zeros((lags, G))

    def flat(self):
        """The device layout: Cuv, U1, U2, V1, V2."""
        return np.concatenate([self.Cuv.ravel(), self.U1, self.U2, self.V1.ravel(), self.V2.ravel()])

    @classmethod
    def from_flat(cls, flat, N, lags, gh, gw, K):
        st = cls(N, lags, gh, gw)
        G, flat = gh * gw, np.asarray(flat, dtype=np.float64)
        o = N * lags * G
        st.Cuv = flat[:o].reshape(N, lags, G).copy(); st.U1 = flat[o:o + N].copy(); st.U2 = flat[o + N:o + 2 * N].copy()
        st.V1 = flat[o + 2 * N:o + 2 * N + lags * G].reshape(lags, G).copy()
        st.V2 = flat[o + 2 * N + lags * G:].reshape(lags, G).copy()
        st.K = K
        return st


def accumulate(st, x, r, *, channel=0, window=None, cell=1, skip=0, s0=127.5, r0=None):
    """One call of dwn_sta_accumulate in float64 on fp32 operands.  Also advances the bounds:
    cross term   (K_call + 2) 2^-24 sum |u| |v|     an fp32 fma chain of K_call terms (gamma_K), the conversion and the float64 add
    moments      (K_call + 2) 2^-53 sum |term|      float64 recursive or pairwise summation of K_call terms and the add"""
    x, r = np.asarray(x, dtype=np.float32), np.asarray(r, dtype=np.float32)
    B, _, T, H, W = x.shape
    window = window if window is not None else (0, 0, H, W)
    L = st.L
    t0 = max(skip, L - 1)
    assert t0 < T and r.shape == (B, st.N, T)
    v = cell_values(x, channel, window, cell, s0).astype(np.float64)
    c = np.zeros(st.N, dtype=np.float32) if r0 is None else np.asarray(r0, dtype=np.float32)
    u = (r - c[None, :, None]).astype(np.float32).astype(np.float64)
    kc = B * (T - t0)
    uu = u[:, :, t0:]
    for l in range(L):
        vv = v[:, t0 - l:T - l]
        st.Cuv[:, l] += np.einsum("bnt,btg->ng", uu, vv)
        a = np.einsum("bnt,btg->ng", np.abs(uu), np.abs(vv))
        st.absC[:, l] += a
        st.bound_C[:, l] += (kc + 2) * EPS32 * a
        st.V1[l] += vv.sum(axis=(0, 1)); st.V2[l] += (vv * vv).sum(axis=(0, 1))
        av = np.abs(vv).sum(axis=(0, 1))
        st.absV[l] += av
        st.bound_V1[l] += (kc + 2) * EPS64 * av; st.bound_V2[l] += (kc + 2) * EPS64 * (vv * vv).sum(axis=(0, 1))
    st.U1 += uu.sum(axis=(0, 2)); st.U2 += (uu * uu).sum(axis=(0, 2))
    au = np.abs(uu).sum(axis=(0, 2))
    st.absU += au
    st.bound_U1 += (kc + 2) * EPS64 * au; st.bound_U2 += (kc + 2) * EPS64 * (uu * uu).sum(axis=(0, 2))
    st.K += kc
    return st


def covariance(st):
    K = float(st.K)
    return (st.Cuv - st.U1[:, None, None] * (st.V1 / K)[None]) / K


def cov_f64_bound(st):
    """A-priori bound of the float64 evaluation of cov from exact operands: the three sums carry gamma_K each, the product, the
    quotient, the difference and the final quotient one rounding each:
    |d cov| <= 2^-53 [(K + 4) sum |u||v| + (2 K + 8) (sum |u|)(sum |v|) / K] / K."""
    K = float(st.K)
    return EPS64 * ((K + 4) * st.absC + (2 * K + 8) * st.absU[:, None, None] * st.absV[None] / K) / K


def finalize(st, rel_threshold=0.5):
    """(cov, z, summary) in float64 from the state, in the formulas of include/dwn.h."""
    K = float(st.K)
    N, L, gh, gw = st.N, st.L, st.gh, st.gw
    mv = st.V1 / K
    cov = (st.Cuv - st.U1[:, None, None] * mv[None]) / K
    var_u = (st.U2 - st.U1 * (st.U1 / K)) / K
    var_v = (st.V2 - st.V1 * mv) / K
    ok = (var_u[:, None, None] > 0) & (var_v[None] > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(ok, cov * np.sqrt(K) / np.sqrt(np.where(ok, var_u[:, None, None] * var_v[None], 1.0)), 0.0)
    summary = np.zeros((N, 8))
    gy, gx = np.divmod(np.arange(gh * gw), gw)
    for n in range(N):
        e = (cov[n] ** 2).sum(axis=1)
        if not e.sum() > 0:
            summary[n] = (0, 0, np.nan, np.nan, np.nan, np.nan, 0, 0)
            continue
        l = int(np.argmax(e))                                   # the first maximum: the lowest lag
        c = cov[n, l]
        i = int(np.argmax(np.abs(c)))                           # the lowest index
        keep = np.abs(c) >= rel_threshold * np.abs(c[i])
        w = np.where(keep, c * c, 0.0)
        sw = w.sum()
        cy, cx = (w * gy).sum() / sw, (w * gx).sum() / sw
        sy, sx = np.sqrt((w * (gy - cy) ** 2).sum() / sw), np.sqrt((w * (gx - cx) ** 2).sum() / sw)
        summary[n] = (l, z[n, l, i], cy, cx, sy, sx, e[l] / e.sum(), keep.sum())
    return cov.reshape(N, L, gh, gw), z.reshape(N, L, gh, gw), summary


def summary_tolerance(gh, gw):
    """Absolute tolerance of summary columns 2-6 between two float64 evaluations that differ in the order of their sums over the
    G cells: each weighted sum carries G 2^-53 relative (the weights are not negative, so nothing cancels), a centre is a
    quotient of two of them times a coordinate below max(gh, gw), and a spread is the square root of a quantity that carries
    that error absolutely: sqrt(4 G 2^-53) max(gh, gw)."""
    G = gh * gw
    return float(np.sqrt(4 * G * EPS64) * max(gh, gw))


def softplus(a):
    return np.logaddexp(0.0, a)


def planted_filter(gh=8, gw=12, centre=(3.0, 7.0), sigma=1.2, prof=(0.2, 0.6, 1.0, 0.5, 0.1)):
    """f [L, gh, gw] of the planted-filter case of the issue."""
    yy, xx = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    env = np.exp(-((yy - centre[0]) ** 2 + (xx - centre[1]) ** 2) / (2 * sigma ** 2))
    return np.asarray(prof)[:, None, None] * env[None]


def planted_response(stim, f, s0, gain):
    """r [B, 1, T] fp32 = softplus(0.5 + gain sum_l f_l . (s_{t-l} - s0)) for stim [B, T, gh, gw]; frames before the clip count
    as s0 (no drive)."""
    B, T = stim.shape[:2]
    d = stim.astype(np.float64) - s0
    drive = np.zeros((B, T))
    for l in range(f.shape[0]):
        drive[:, l:] += np.einsum("btyx,yx->bt", d[:, :T - l], f[l])
    return softplus(0.5 + gain * drive).astype(np.float32)[:, None, :]

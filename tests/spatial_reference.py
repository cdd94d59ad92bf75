"""float64 numpy checker of the retinotopic readout gain: forward, the five gradients and, for every output, the
rounding floor the GPU tests measure the kernels against.

    px = (clamp(x, -1, 1) + 1) / 2 (Wf - 1)   x0 = min(floor(px), max(Wf - 2, 0))   fx = px - x0   x1 = min(x0 + 1, Wf - 1)   (y alike)
    w00 = (1-fy)(1-fx)  w01 = (1-fy) fx  w10 = fy (1-fx)  w11 = fy fx          d_c = sum_k G[b,t,cell_c,k] weight[n,k]
    a = bias[n] + sum_c w_c d_c     gain = exp(m tanh(a))     out = y gain
    dy = dout gain     s = dout y gain m sech^2(a)     dbias = sum_{b,t} s     dweight[n,k] = sum_{b,t} s samp_k,  samp_k = sum_c w_c G_c,k
    dpos[n,0] = (Wf-1)/2 sum_{b,t} s ((1-fy)(d01 - d00) + fy (d11 - d10))   (0 for x strictly outside [-1, 1] or Wf = 1; y alike)
    dG[b,t,cell,k] = sum_{n, c: cell_c(n) = cell} s w_c weight[n,k]

which is ``grid_sample(bilinear, border, align_corners=True)`` followed by the behaviour modulator's gain
(tests/test_spatial_reference_cpu.py holds it to float64 grid_sample and autograd).  A position on a cell boundary takes the slope
of the cell it is assigned to: the cell to the right of (below) an interior cell centre, the last cell at +1.

Floors, in units of eps = 2^-24.  They are the modulator checker's (tests/modulator_reference.py: the constants c0 of the gain chain
are imported from there) with the error of ``a`` replaced by the one of this kernel:
  * a: four corner dots of K FMAs each and the combination with the four weights and the bias, 4K + 3 rounded operations over
    A = |bias| + sum_c w_c sum_k |G weight|;
  * the fp32 bilinear weights: px carries two roundings (|dpx| <= 2 eps (Wf - 1)), 1 - fx one more and each product one more, so every
    weight is off by at most WB eps absolutely, WB = 2 (Wf - 1) + 2 (Hf - 1) + 3: a moves by at most WB eps sum_c sum_k |G weight|;
  element:  floor = eps |value| (c0 + m sech^2(a) ((4K + 3) A + WB D)),        D = sum_c sum_k |G_c,k weight_k|
  reduced:  every term is a product of s (element floor above) and a factor with its own error, plus one rounding of the product;
            the float64 sums add nothing visible, and the one final rounding adds eps |result|:
              dbias    factor 1
              dweight  factor samp_k: 4 rounded operations over sum_c w_c |G_c,k| and the weights' WB eps sum_c |G_c,k|
              dpos     factor (1-fy)(d01 - d00) + fy (d11 - d10): dots of K operations, a difference, two products and a sum
                       ((K + 4) eps over the absolute dots) and the error of fy ((2 (Hf - 1) + 1) eps D)
              dG       factor w_c weight[n,k]: the weight's WB eps |weight[n,k]|
The checker reads G as it is stored (a bf16 map is passed in as the values bf16 holds), so bf16 storage adds no term."""
import numpy as np

from tests.modulator_reference import EPS, c0_element, sech2  # noqa: F401


def draw_positions(rng, N, Hf, Wf, lo=0.05, hi=0.95):
    """[N][2] float32 positions whose pixel coordinates have a fractional part in [lo, hi] (any value on a one-cell axis)."""
    def axis(n):
        if n == 1:
            return rng.uniform(-1.0, 1.0, size=N)
        p = rng.integers(0, n - 1, size=N) + rng.uniform(lo, hi, size=N)
        return p / (n - 1) * 2.0 - 1.0
    return np.stack([axis(Wf), axis(Hf)], axis=1).astype(np.float32)


def _axis(v, n):
    c = np.clip(v, -1.0, 1.0)
    p = (c + 1.0) / 2.0 * (n - 1)
    i0 = np.minimum(np.floor(p), max(n - 2, 0)).astype(np.int64)
    f = p - i0
    i1 = np.minimum(i0 + 1, n - 1)
    live = (v >= -1.0) & (v <= 1.0) & (n > 1)
    return i0, i1, f, live


def cells(pos, Hf, Wf):
    """pos [N][2] -> dict of the four corner cell indices (y * Wf + x), the four weights, fx, fy and the live flags."""
    pos = np.asarray(pos, dtype=np.float64)
    x0, x1, fx, lx = _axis(pos[:, 0], Wf)
    y0, y1, fy, ly = _axis(pos[:, 1], Hf)
    return dict(c=[y0 * Wf + x0, y0 * Wf + x1, y1 * Wf + x0, y1 * Wf + x1],
                w=[(1 - fy) * (1 - fx), (1 - fy) * fx, fy * (1 - fx), fy * fx], fx=fx, fy=fy, live_x=lx, live_y=ly)


def reference(y, g, pos, weight, bias, m, dout=None):
    """All arguments as arrays of any float type; computed in float64.  y [B][N][T], g [B][T][Hf][Wf][K], pos [N][2], weight [N][K],
    bias [N].  Returns a dict with out, gain, a (and with ``dout``: dy, s, dg, dpos, dweight, dbias) and ``floor``: a dict of arrays
    of the same shapes."""
    y, g, weight, bias = (np.asarray(v, dtype=np.float64) for v in (y, g, weight, bias))
    m = float(m)
    B, T, Hf, Wf, K = g.shape
    N = y.shape[1]
    ce = cells(pos, Hf, Wf)
    gf = g.reshape(B, T, Hf * Wf, K)
    G = [gf[:, :, c, :] for c in ce["c"]]                                   # four [B][T][N][K]
    d = [np.einsum("btnk,nk->bnt", Gc, weight) for Gc in G]
    dabs = [np.einsum("btnk,nk->bnt", np.abs(Gc), np.abs(weight)) for Gc in G]
    w = [wc[None, :, None] for wc in ce["w"]]
    a = bias[None, :, None] + sum(wc * dc for wc, dc in zip(w, d))
    A = np.abs(bias)[None, :, None] + sum(wc * dc for wc, dc in zip(w, dabs))
    D = sum(dabs)
    WB = 2.0 * (Wf - 1) + 2.0 * (Hf - 1) + 3.0
    gain = np.exp(m * np.tanh(a))
    sc = sech2(a)
    spread = m * sc * ((4 * K + 3) * A + WB * D)
    res = dict(a=a, gain=gain, out=y * gain, sech2=sc, cells=ce)
    floor = dict(out=EPS * np.abs(res["out"]) * (c0_element(m, "out") + spread))
    if dout is not None:
        dout = np.asarray(dout, dtype=np.float64)
        s = dout * y * gain * m * sc
        fs = EPS * np.abs(s) * (c0_element(m, "s") + spread)
        sa = np.abs(s)
        res.update(dy=dout * gain, s=s, dbias=s.sum(axis=(0, 2)))
        floor["dy"] = EPS * np.abs(res["dy"]) * (c0_element(m, "dy") + spread)
        floor["s"] = fs
        floor["dbias"] = fs.sum(axis=(0, 2)) + EPS * np.abs(res["dbias"])
        # dweight
        wn = [wc[None, None, :, None] for wc in ce["w"]]
        samp = sum(wc * Gc for wc, Gc in zip(wn, G))                        # [B][T][N][K]
        samp_abs = sum(wc * np.abs(Gc) for wc, Gc in zip(wn, G))
        g_abs = sum(np.abs(Gc) for Gc in G)
        res["dweight"] = np.einsum("bnt,btnk->nk", s, samp)
        floor["dweight"] = (np.einsum("bnt,btnk->nk", fs, np.abs(samp)) +
                            EPS * np.einsum("bnt,btnk->nk", sa, 4.0 * samp_abs + WB * g_abs + np.abs(samp)) +
                            EPS * np.abs(res["dweight"]))
        # dpos
        fx, fy = ce["fx"][None, :, None], ce["fy"][None, :, None]
        ax = (1 - fy) * (d[1] - d[0]) + fy * (d[3] - d[2])
        ay = (1 - fx) * (d[2] - d[0]) + fx * (d[3] - d[1])
        ax_abs = (1 - fy) * (dabs[1] + dabs[0]) + fy * (dabs[3] + dabs[2])
        ay_abs = (1 - fx) * (dabs[2] + dabs[0]) + fx * (dabs[3] + dabs[1])
        sx, sy = 0.5 * (Wf - 1), 0.5 * (Hf - 1)
        dpx = sx * (s * ax).sum(axis=(0, 2)) * ce["live_x"]
        dpy = sy * (s * ay).sum(axis=(0, 2)) * ce["live_y"]
        fpx = sx * (fs * np.abs(ax) + EPS * sa * ((K + 4) * ax_abs + (2.0 * (Hf - 1) + 1.0) * D + np.abs(ax))).sum(axis=(0, 2))
        fpy = sy * (fs * np.abs(ay) + EPS * sa * ((K + 4) * ay_abs + (2.0 * (Wf - 1) + 1.0) * D + np.abs(ay))).sum(axis=(0, 2))
        res["dpos"] = np.stack([dpx, dpy], axis=1)
        floor["dpos"] = np.stack([fpx * ce["live_x"], fpy * ce["live_y"]], axis=1) + EPS * np.abs(res["dpos"])
        # dG: scatter over the four corners
        dg = np.zeros((Hf * Wf, B, T, K))
        fdg = np.zeros((Hf * Wf, B, T, K))
        wabs = np.abs(weight)
        for c, wc in zip(ce["c"], ce["w"]):
            np.add.at(dg, c, np.einsum("bnt,n,nk->nbtk", s, wc, weight))
            np.add.at(fdg, c, np.einsum("bnt,n,nk->nbtk", fs, wc, wabs) + EPS * np.einsum("bnt,n,nk->nbtk", sa, wc + WB, wabs))
        res["dg"] = dg.transpose(1, 2, 0, 3).reshape(B, T, Hf, Wf, K)
        floor["dg"] = fdg.transpose(1, 2, 0, 3).reshape(B, T, Hf, Wf, K) + EPS * np.abs(res["dg"])
    res["floor"] = floor
    return res

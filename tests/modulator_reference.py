"""float64 numpy checker of the behaviour modulator: forward, the four gradients and, for every output, the
rounding floor the GPU tests measure the kernels against.

    a = c[n] + sum_k h[b,t,k] u[n,k]     gain = exp(m tanh(a))     out = y gain
    dy = dout gain     s = dout y gain m sech^2(a)     du = sum_{b,t} s h     dc = sum_{b,t} s     dh = sum_n s u

``sech2`` is 4 e / (1 + e)^2 with e = exp(-2 |a|): the form that does not cancel (``1 - tanh^2`` is exactly 0 in float64 from
|a| ~ 19, in fp32 from |a| ~ 9).

Floors, in units of eps = 2^-24 (the largest relative error of one fp32 rounding).  The fp32 chain of the kernels:
  * a: K FMAs from c[n]; its error is at most (K + 1) eps (|c| + sum_k |h u|) and enters log(gain) with the factor m sech^2(a);
  * gain: tanh(a) = (1 - e) / (1 + e) with e = exp(-2 |a|) from the hardware exponential (relative error 2 eps (1 + |x|); since
    |x| e^-|x| <= 1/e its ABSOLUTE effect on e, and through the quotient on tanh, stays below 2 eps), then the difference, the
    sum, the reciprocal (1 ulp = 2 eps) and the product: below 7 eps absolute, scaled by m into log(gain); the product m tanh
    (eps m); the hardware exponential of an argument of size <= m (2 eps (1 + m)): G = 10 m + 2;
  * out, dy: one more product: c0 = G + 1;
  * s: sech^2 = 4 e / (1 + e)^2 with e from expf (1 ulp = 2 eps for every |a|), the sum 1 + e, the square and the quotient
    (3 eps; 4 e is exact), and s is four more products: c0 = G + 5 + 4.
  element:  floor = eps |value| (c0 + m sech^2(a) (K + 1) (|c| + sum_k |h u|))
  reduced:  floor = eps c0 sum |terms| + eps |result|      (c0 of s, plus one for the fp32 product s h / s u; the float64 sums
            themselves add nothing visible; the last term is the one final rounding)
"""
import numpy as np

EPS = 2.0 ** -24


def sech2(a):
    e = np.exp(-2.0 * np.abs(a))
    return 4.0 * e / ((1.0 + e) * (1.0 + e))


def c0_element(m, which):
    gain = 10.0 * m + 2.0
    return gain + 1.0 if which in ("out", "dy") else gain + 9.0


def reference(y, h, u, c, m, dout=None):
    """All arguments as arrays of any float type; computed in float64.  Returns a dict with out, gain, a (and with ``dout``:
    dy, s, du, dc, dh) and ``floor``: a dict of arrays of the same shapes for out (dy, s, du, dc, dh)."""
    y, h, u, c = (np.asarray(v, dtype=np.float64) for v in (y, h, u, c))
    m = float(m)
    K = h.shape[2]
    a = np.einsum("btk,nk->bnt", h, u) + c[None, :, None]
    abs_a = np.einsum("btk,nk->bnt", np.abs(h), np.abs(u)) + np.abs(c)[None, :, None]
    gain = np.exp(m * np.tanh(a))
    sc = sech2(a)
    spread = m * sc * (K + 1) * abs_a
    res = dict(a=a, gain=gain, out=y * gain, sech2=sc)
    floor = dict(out=EPS * np.abs(res["out"]) * (c0_element(m, "out") + spread))
    if dout is not None:
        dout = np.asarray(dout, dtype=np.float64)
        s = dout * y * gain * m * sc
        res.update(dy=dout * gain, s=s, du=np.einsum("bnt,btk->nk", s, h), dc=s.sum(axis=(0, 2)),
                   dh=np.einsum("bnt,nk->btk", s, u))
        c0s = c0_element(m, "s")
        floor["dy"] = EPS * np.abs(res["dy"]) * (c0_element(m, "dy") + spread)
        floor["s"] = EPS * np.abs(s) * (c0s + spread)
        sa = np.abs(s)
        floor["du"] = EPS * (c0s + 1) * np.einsum("bnt,btk->nk", sa, np.abs(h)) + EPS * np.abs(res["du"])
        floor["dc"] = EPS * c0s * sa.sum(axis=(0, 2)) + EPS * np.abs(res["dc"])
        floor["dh"] = EPS * (c0s + 1) * np.einsum("bnt,nk->btk", sa, np.abs(u)) + EPS * np.abs(res["dh"])
    res["floor"] = floor
    return res

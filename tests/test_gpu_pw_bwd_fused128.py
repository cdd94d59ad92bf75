"""conv_pw backward at 128 input channels through the one-pass kernel (csrc/dwn_pw_bwd.hip pw_bwd_fused128_kernel: bf16, Cin = 128,
E = 896, two workgroups per 64-row tile, each owning 64 columns), through the public entry dwn_pw_backward.

Shapes: M = 128 (two row tiles, a grid smaller than the chip, the "prefetch this tile again" path), 128 * 3 (six tiles on eight
row-tile owners: unequal work, idle workgroups), 128 * 129 (258 tiles on 128 owners: three rounds, the last with two tiles).
Bounds: those of tests/test_gpu_gemm.py::test_pw_backward_without_y1 for the same quantities.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_helpers import dev, rel, stream  # noqa: E402

E, CIN = 896, 128
BF = torch.bfloat16
SHAPES = [128, 128 * 3, 128 * 129]


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    return lib


class Call:
    """one dwn_pw_bwd_args with its buffers"""

    def __init__(self, L, dh1, a0, w1, abc, E_=E, Cin=CIN):
        M = dh1.shape[0]
        self.L, self.M, self.keep = L, M, (dh1, a0, w1, abc)
        self.da0 = torch.full((M, Cin), float("nan"), device=dev()).to(BF)
        self.dw = torch.full((E_, Cin), float("nan"), device=dev())
        self.nws = L.lib.dwn_pw_backward_workspace_bytes(E_, Cin, L.DWN_BF16)
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=dev())
        a = self.a = L.PwBwdArgs()
        a.dh1, a.a0, a.w_pw, a.abc = dh1.data_ptr(), a0.data_ptr(), w1.data_ptr(), abc.data_ptr()
        a.da0, a.dw, a.M, a.E, a.Cin, a.ws, a.ws_bytes = self.da0.data_ptr(), self.dw.data_ptr(), M, E_, Cin, self.ws.data_ptr(), self.nws

    def rc(self):
        return self.L.lib.dwn_pw_backward(C.byref(self.a), self.L.DWN_BF16, 0, stream())

    def run(self):
        self.L.check(self.rc(), "pw_backward")
        torch.cuda.synchronize()
        return self.da0, self.dw


@functools.lru_cache(maxsize=None)
def case(M):
    """inputs and their float64 products, made once per shape and read only"""
    g = torch.Generator(device="cuda").manual_seed(M + E)
    dh1 = torch.randn(M, E, generator=g, device=dev()).to(BF)
    a0 = (torch.randn(M, CIN, generator=g, device=dev()) + 0.3).to(BF)               # a non-zero column mean: the A3 term counts
    w1 = (torch.randn(E, CIN, generator=g, device=dev()) * 0.1).contiguous()
    abc = torch.randn(3, E, generator=g, device=dev()).contiguous()
    res = torch.randn(M, 2 * CIN, generator=g, device=dev()).to(BF)
    rabc = torch.randn(3, 2 * CIN, generator=g, device=dev()).contiguous()
    w1r = w1.to(BF).double()
    y1 = a0.double() @ w1r.t()
    return dict(dh1=dh1, a0=a0, w1=w1, abc=abc, res=res, rabc=rabc, w1r=w1r, y1=y1)


def dy_of(c, abc):
    return abc[0].double() * c["dh1"].double() + abc[1].double() * c["y1"] + abc[2].double()


@pytest.mark.parametrize("M", SHAPES)
def test_against_float64(L, M):
    """dy1 = A1*dh1 + A2*(a0 W1^T) + A3; da0 = dy1 W1; dW = dy1^T a0, W1 as rounded to bf16; then each abc term alone"""
    assert L.lib.dwn_pw_bwd_fused_supported(L.DWN_BF16, M, E, CIN) == 1
    c = case(M)
    k = Call(L, c["dh1"], c["a0"], c["w1"], c["abc"])
    da0, dw = k.run()
    dy = dy_of(c, c["abc"])
    assert torch.isfinite(da0.float()).all() and torch.isfinite(dw).all()
    e_da, e_dw = rel(da0, dy @ c["w1r"]), rel(dw, dy.t() @ c["a0"].double())
    print(f"M={M}: da0 {e_da:.3e} dW {e_dw:.3e}")
    assert e_da < 8e-3
    assert e_dw < 2e-4
    for sel in range(3):
        ab = torch.zeros_like(c["abc"]); ab[sel] = c["abc"][sel]
        k.a.abc = ab.data_ptr()
        _, dw = k.run()
        e = rel(dw, dy_of(c, ab).t() @ c["a0"].double())
        print(f"M={M}: abc term {sel} alone: dW {e:.3e}")
        assert e < 2e-3, sel


@pytest.mark.parametrize("mult", [1, 2])
@pytest.mark.parametrize("M", SHAPES)
def test_identity_shortcut(L, M, mult):
    """res_C = Cin and 2 Cin: da0 += sum_j A1sc*res + A2sc*a0 + A3sc over the channel tiles; dW does not see it"""
    c = case(M)
    rc = mult * CIN
    res = c["res"][:, :rc].contiguous()
    rabc = c["rabc"][:, :rc].contiguous()
    k = Call(L, c["dh1"], c["a0"], c["w1"], c["abc"])
    k.a.res, k.a.res_abc, k.a.res_C = res.data_ptr(), rabc.data_ptr(), rc
    da0, dw = k.run()
    dy = dy_of(c, c["abc"])
    want = dy @ c["w1r"]
    for j in range(mult):
        sl = slice(j * CIN, (j + 1) * CIN)
        want = want + rabc[0, sl].double() * res[:, sl].double() + rabc[1, sl].double() * c["a0"].double() + rabc[2, sl].double()
    e_da, e_dw = rel(da0, want), rel(dw, dy.t() @ c["a0"].double())
    print(f"M={M} res_C={rc}: da0 {e_da:.3e} dW {e_dw:.3e}")
    assert e_da < 8e-3
    assert e_dw < 2e-4


def gathered_inputs(F, Hin, Win, Hout, Wout, seed, rc=CIN):
    g = torch.Generator(device="cuda").manual_seed(seed)
    M = F * Hin * Win
    dh1 = torch.randn(M, E, generator=g, device=dev()).to(BF)
    a0 = (torch.randn(M, CIN, generator=g, device=dev()) + 0.3).to(BF)
    w1 = (torch.randn(E, CIN, generator=g, device=dev()) * 0.1).contiguous()
    abc = torch.randn(3, E, generator=g, device=dev()).contiguous()
    res = torch.randn(F * Hout * Wout, rc, generator=g, device=dev()).to(BF)
    rabc = torch.randn(3, rc, generator=g, device=dev()).contiguous()
    return dh1, a0, w1, abc, res, rabc


@pytest.mark.parametrize("mult", [1, 2])
def test_gathered_shortcut(L, mult):
    """the shortcut of a strided block: 4 frames of 8 x 16 (two 64-row tiles per frame), stride-2 nearest maps, res_C = Cin (and
    2 Cin, which the block plan also folds: the second channel tile of the top-of-tile and epilogue terms) — only the
    sampled rows get A1sc*dout[rout] + A2sc*a0 + A3sc (tests/test_gpu_gemm.py::test_pw_backward_gathered_shortcut at 128 channels)"""
    F, Hin, Win, Hout, Wout = 4, 8, 16, 4, 8
    M = F * Hin * Win
    rc = mult * CIN
    dh1, a0, w1, abc, res, rabc = gathered_inputs(F, Hin, Win, Hout, Wout, 5 + mult, rc)
    hinv = torch.full((Hin,), -1, dtype=torch.int32); hinv[::2] = torch.arange(Hout, dtype=torch.int32)
    winv = torch.full((Win,), -1, dtype=torch.int32); winv[::2] = torch.arange(Wout, dtype=torch.int32)
    hinv_d, winv_d = hinv.to(dev()), winv.to(dev())
    k = Call(L, dh1, a0, w1, abc)
    a = k.a
    a.res, a.res_abc, a.res_C = res.data_ptr(), rabc.data_ptr(), rc
    a.res_hinv, a.res_winv = hinv_d.data_ptr(), winv_d.data_ptr()
    a.res_Hin, a.res_Win, a.res_Hout, a.res_Wout = Hin, Win, Hout, Wout
    da0, dw = k.run()
    w1r = w1.to(BF).double()
    dy = abc[0].double() * dh1.double() + abc[1].double() * (a0.double() @ w1r.t()) + abc[2].double()
    want = (dy @ w1r).view(F, Hin, Win, CIN).clone()
    resv = res.double().view(F, Hout, Wout, rc)
    for j in range(mult):
        sl = slice(j * CIN, (j + 1) * CIN)
        want[:, ::2, ::2] += (rabc[0, sl].double() * resv[..., sl]
                              + rabc[1, sl].double() * a0.double().view(F, Hin, Win, CIN)[:, ::2, ::2] + rabc[2, sl].double())
    assert torch.isfinite(da0.float()).all()
    e = rel(da0, want.view(M, CIN))
    print(f"gathered res_C={rc}: da0 {e:.3e}")
    assert e < 8e-3
    # the rows the map skips are the plain data gradient, the sampled rows are not
    da_g = da0.clone()
    a.res = None
    da1, _ = k.run()
    skip = torch.ones(F, Hin, Win, dtype=torch.bool, device=dev()); skip[:, ::2, ::2] = False
    assert rel(da_g.view(F, Hin, Win, CIN)[skip], da1.view(F, Hin, Win, CIN)[skip].double()) < 2e-3
    assert rel(da_g.view(F, Hin, Win, CIN)[~skip], da1.view(F, Hin, Win, CIN)[~skip].double()) > 5e-2
    assert rel(dw, dy.t() @ a0.double()) < 2e-4


def test_exact_integers(L):
    """Indexing: fragment layouts, column halves, chunk order.  dh1 rows one-hot in E with values in {-2 .. 2}, the position walking
    through all 896 columns (every one of the 14 chunks, every column of a chunk); W1 in {-1, 0, 1}; a0 small integers; A1 = 1,
    A2 = A3 = 0.  da0 = dh1 W1 and dW = dh1^T a0 are small integers: da0 must equal the int64 product exactly (bf16 holds it), dW
    exactly in fp32."""
    M = 1024
    g = torch.Generator().manual_seed(3)
    m = torch.arange(M)
    pos = (m * 5 + m // E) % E                                     # gcd(5, 896) = 1: 1024 rows visit every column of E
    assert len(set(pos.tolist())) == E and set((pos // 64).tolist()) == set(range(14))
    val = torch.randint(-2, 3, (M,), generator=g)
    val[val == 0] = 1
    dh1_i = torch.zeros(M, E, dtype=torch.int64); dh1_i[m, pos] = val
    w1_i = torch.randint(-1, 2, (E, CIN), generator=g)
    a0_i = torch.randint(-3, 4, (M, CIN), generator=g)
    abc = torch.zeros(3, E); abc[0] = 1.0
    k = Call(L, dh1_i.to(dev()).to(BF), a0_i.to(dev()).to(BF), w1_i.float().to(dev()).contiguous(), abc.to(dev()))
    da0, dw = k.run()
    want_da, want_dw = dh1_i @ w1_i, dh1_i.t() @ a0_i
    assert want_da.abs().max() <= 2 and (want_da[:, :64] != 0).any() and (want_da[:, 64:] != 0).any()
    assert torch.equal(da0.float().cpu(), want_da.float())
    assert torch.equal(dw.cpu(), want_dw.float())


def test_two_launches_are_bit_identical(L):
    """da0 has no atomics in the kernel.  The entry's prep kernel does add G = W1^T diag(A2) W1 and r3 = A3 W1 with fp32 atomics
    in arrival order, so W1, A2 and A3 are dyadic here (multiples of 1/8 and 1/4: every partial sum is exact in fp32, the order
    cannot matter); dh1, a0 and A1 are arbitrary."""
    M = 128 * 129
    c = case(M)
    g = torch.Generator(device="cuda").manual_seed(9)
    w1 = (torch.randint(-1, 2, (E, CIN), generator=g, device=dev()).float() * 0.125).contiguous()
    abc = c["abc"].clone()
    abc[1] = torch.randint(-2, 3, (E,), generator=g, device=dev()).float() * 0.25
    abc[2] = torch.randint(-2, 3, (E,), generator=g, device=dev()).float() * 0.25
    k = Call(L, c["dh1"], c["a0"], w1, abc)
    first = k.run()[0].clone()
    k.da0.fill_(float("nan"))
    second = k.run()[0]
    assert torch.isfinite(first.float()).all() and float(first.float().abs().max()) > 0
    assert torch.equal(first.view(torch.int16), second.view(torch.int16))


def test_refusals_match_the_64_channel_path(L):
    """res_C = 3 Cin, a gathered map with Hin + Win > 512, a workspace one byte short: the error code of the 64-channel analogue"""
    codes = {}
    for E_, Cin in ((448, 64), (E, CIN)):
        F, Hin, Win, Hout, Wout = 1, 1, 512, 1, 256                # Hin + Win = 513
        M = F * Hin * Win
        assert L.lib.dwn_pw_bwd_fused_supported(L.DWN_BF16, M, E_, Cin) == 1
        dh1 = torch.zeros(M, E_, device=dev()).to(BF)
        a0 = torch.zeros(M, Cin, device=dev()).to(BF)
        w1 = torch.zeros(E_, Cin, device=dev())
        abc = torch.zeros(3, E_, device=dev())
        res = torch.zeros(M, 3 * Cin, device=dev()).to(BF)
        rabc = torch.zeros(3, 3 * Cin, device=dev())
        hinv = torch.zeros(Hin, dtype=torch.int32, device=dev())
        winv = torch.full((Win,), -1, dtype=torch.int32, device=dev())
        got = []
        k = Call(L, dh1, a0, w1, abc, E_, Cin)
        k.a.res, k.a.res_abc, k.a.res_C = res.data_ptr(), rabc.data_ptr(), 3 * Cin
        got.append(k.rc())
        k.a.res_C = Cin
        k.a.res_hinv, k.a.res_winv = hinv.data_ptr(), winv.data_ptr()
        k.a.res_Hin, k.a.res_Win, k.a.res_Hout, k.a.res_Wout = Hin, Win, Hout, Wout
        got.append(k.rc())
        k.a.res, k.a.res_abc, k.a.res_C, k.a.res_hinv, k.a.res_winv = None, None, 0, None, None
        k.a.ws_bytes = k.nws - 1
        got.append(k.rc())
        k.a.ws_bytes = k.nws
        assert k.rc() == 0                                         # the same arguments, unrefused
        torch.cuda.synchronize()
        codes[Cin] = got
    assert all(rc < 0 for rc in codes[64]), codes
    assert codes[CIN] == codes[64], codes
    assert codes[CIN][2] == -6

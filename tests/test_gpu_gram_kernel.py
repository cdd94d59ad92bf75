"""The streaming Gram kernel behind BatchNorm-1's batch statistics (csrc/dwn_gram.hip), through dwn_conv_pw_bn_stats.

y1 = a0 . W1^T is never computed in the y1-free training forward (src/models/dwiseneuro.py:90-93 is conv_pw + BatchNorm3d): its
batch mean and variance come from G = a0^T a0 and s = 1^T a0.  Here the inputs are integer-valued bf16 with |v| <= 8, so every
product and every partial sum is exact in fp32 and in fp64, and

  * the raw sums (sum a0, sum a0^2: row Cin and the diagonal of G) read back from the shortcut statistics buffer must EQUAL float64;
  * every off-diagonal G[i][j] is exposed through a W1 whose rows are e_i + e_j (and e_i): mean = (s_i + s_j) / M,
    var = (G_ii + G_jj + 2 G_ij) / M - mean^2, compared with float64 to 1e-6 relative — the fp32 rounding of the coefficients
    (unit roundoff 6e-8) is the only error an exact G leaves, and 1e-6 is the bound tests/test_gpu_gemm.py holds this entry to.

Shapes: fewer rows than one 32-row step, ragged steps, fewer steps than waves, more than one workgroup (M = 5000), both widths
the forward uses (64: the streaming kernel; 128: the gemm_tn route it falls back to), one width neither specialises (192), and a
row stride larger than the width."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_helpers import dev, stream  # noqa: E402

EPS = 1e-5


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    return lib


def _pair_weights(Cin):
    """rows e_i (Cin of them), then e_i + e_j for every i < j: float32 [Cin + Cin (Cin - 1) / 2][Cin]"""
    iu = torch.triu_indices(Cin, Cin, offset=1)
    n = iu.shape[1]
    w = torch.zeros(Cin + n, Cin)
    w[torch.arange(Cin), torch.arange(Cin)] = 1.0
    w[Cin + torch.arange(n), iu[0]] = 1.0
    w[Cin + torch.arange(n), iu[1]] = 1.0
    return w


def _run(L, a0, ld, M, Cin, w, dtype=None):
    E = w.shape[0]
    gamma, beta = torch.ones(E, device=dev()), torch.zeros(E, device=dev())
    rm, rv = torch.zeros(E, device=dev()), torch.ones(E, device=dev())
    nbt = torch.zeros(1, dtype=torch.int64, device=dev())
    coef = torch.full((4 * E,), float("nan"), device=dev())
    sc = torch.zeros(32 * 2 * Cin, dtype=torch.float64, device=dev())
    ws = torch.empty(L.lib.dwn_conv_pw_bn_stats_workspace_bytes(Cin), dtype=torch.uint8, device=dev())
    bn = L.BN()
    bn.gamma = gamma.data_ptr(); bn.beta = beta.data_ptr(); bn.running_mean = rm.data_ptr(); bn.running_var = rv.data_ptr()
    bn.num_batches_tracked = nbt.data_ptr(); bn.coef = coef.data_ptr()
    L.check(L.lib.dwn_conv_pw_bn_stats(a0.data_ptr(), ld, M, w.data_ptr(), E, Cin, C.byref(bn), 0.1, EPS, sc.data_ptr(),
                                       ws.data_ptr(), ws.numel(), L.DWN_BF16 if dtype is None else dtype, 0, stream()),
            "conv_pw_bn_stats")
    torch.cuda.synchronize()
    return coef.view(4, E).double(), sc.view(32, 2, Cin).sum(0)


def _integer_input(M, Cin, ld, seed):
    g = torch.Generator().manual_seed(seed)
    buf = torch.full((M, ld), 7.0)                       # (columns past Cin: a value a wrong row stride would pick up)
    # asymmetric over the channels: an offset that grows with the channel index, so that a swapped (row, column) map of the
    # accumulators or a permuted channel block changes s and the off-diagonal of G
    v = torch.randint(-8, 9, (M, Cin), generator=g).float()
    v = torch.clamp(v + (torch.arange(Cin) % 5 - 2).float(), -8, 8)
    buf[:, :Cin] = v
    return buf.to(torch.bfloat16).to(dev()), v.double().to(dev())


def _check_exact(L, M, Cin, ld, seed):
    a0, v = _integer_input(M, Cin, ld, seed)
    w = _pair_weights(Cin).to(dev())
    coef, sums = _run(L, a0, ld, M, Cin, w)
    s = v.sum(0)
    G = v.t() @ v                                        # integers below 2^53: exact
    assert torch.equal(sums[0], s), "sum a0 is not exact"
    assert torch.equal(sums[1], torch.diagonal(G)), "sum a0^2 is not exact"
    wd = w.double()
    mean = (wd @ s) / M
    var = torch.einsum("ei,ij,ej->e", wd, G, wd) / M - mean ** 2
    sigma = var.clamp_min(0).sqrt()
    invstd = 1.0 / (var.clamp_min(0) + EPS).sqrt()
    err_mean = float(((coef[2] - mean).abs() / torch.maximum(mean.abs(), sigma).clamp_min(1e-30)).max())
    err_inv = float(((coef[3] - invstd).abs() / invstd).max())
    print(f"M={M} Cin={Cin} ld={ld}: mean rel err {err_mean:.2e}, invstd rel err {err_inv:.2e}")
    assert err_mean < 1e-6 and err_inv < 1e-6, (M, Cin, err_mean, err_inv)


@pytest.mark.parametrize("Cin", [64, 128])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 257, 5000])
def test_gram_sums_exact_on_integer_inputs(L, M, Cin):
    _check_exact(L, M, Cin, Cin, 1000 * Cin + M)


def test_gram_width_without_a_specialised_kernel(L):
    """192 channels: neither the streaming kernel (64) nor a tile-width case of its own — the gemm_tn route, unchanged."""
    _check_exact(L, 257, 192, 192, 3)


@pytest.mark.parametrize("Cin", [64, 128])
def test_gram_row_stride_larger_than_the_width(L, Cin):
    _check_exact(L, 1031, Cin, Cin + 8, 4)


def test_gram_fp32_input_keeps_the_gemm_tn_route(L):
    """fp32 activations are not built into the streaming kernel: same entry, same answers."""
    M, Cin = 257, 64
    _, v = _integer_input(M, Cin, Cin, 6)
    w = _pair_weights(Cin).to(dev())
    coef, sums = _run(L, v.float().contiguous(), Cin, M, Cin, w, dtype=L.DWN_F32)
    assert torch.equal(sums[0], v.sum(0)) and torch.equal(sums[1], (v * v).sum(0))


def test_gram_repeated_calls_agree_to_the_order_of_fp64_adds(L):
    """The workgroups' fp64 partials meet in fp64 atomics (8 replicas, summed in replica order by the finaliser): the order of the
    adds into one replica is the only thing that varies between calls, so 50 calls on the same non-integer inputs agree to 1e-12 on
    the fp64 sums (2^-53 per add, a few hundred adds) — and to one fp32 rounding on the coefficients made from them."""
    torch.manual_seed(9)
    M, Cin, E = 5000, 64, 448
    a0 = (torch.randn(M, Cin, device=dev()) * (0.5 + torch.rand(Cin, device=dev())) + torch.randn(Cin, device=dev())).to(torch.bfloat16)
    w = torch.randn(E, Cin, device=dev()) / Cin ** 0.5
    coef0, sums0 = _run(L, a0, Cin, M, Cin, w)
    ref = a0.double()
    # against float64: the matrix cores sum up to 256 rows in fp32 before the fold into fp64 — 256 additions of unit roundoff 2^-24
    # each, relative to sum |terms|, is the bound of that part (the fp64 part is 1e-16)
    fp32_part = 256 * 2.0 ** -24
    assert float(((sums0[0] - ref.sum(0)).abs() / ref.abs().sum(0)).max()) < fp32_part
    assert float(((sums0[1] - (ref * ref).sum(0)).abs() / (ref * ref).sum(0)).max()) < fp32_part
    scale = torch.stack([ref.abs().sum(0), (ref * ref).sum(0)])          # (a channel's sum may cancel: measure against sum |a0|)
    sigma0 = 1.0 / coef0[3]
    worst = 0.0
    for _ in range(49):
        coef, sums = _run(L, a0, Cin, M, Cin, w)
        worst = max(worst, float(((sums - sums0).abs() / scale).max()))
        assert float(((coef[3] - coef0[3]).abs() / coef0[3]).max()) <= 2.0 ** -22
        assert float(((coef[2] - coef0[2]).abs() / torch.maximum(coef0[2].abs(), sigma0)).max()) <= 2.0 ** -22
    print(f"50 calls: largest relative difference of the fp64 sums {worst:.2e}")
    assert worst < 1e-12

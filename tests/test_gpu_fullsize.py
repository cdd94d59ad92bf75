"""Size-independent properties at BASELINE.json's full metric shape (B=32, T=32, 36x64, expansion 7, one readout of
7863 neurons, bf16 storage) — sizes the CPU oracle cannot run in seconds, so parity is asserted through invariants:

* the point-wise GEMM on small-integer data is exact: column checksums and the fused BatchNorm sums equal the
  integer results (a checksum of checksums over the 2.36 M-row operand of block 0);
* the weight-gradient GEMM on small-integer data is exact;
* eval forward is per-sample independent: a batch slice run alone equals the slice of the full-batch run;
* the backward pass is linear in the loss scale: scaling the loss by 2 scales every gradient by 2 (a power-of-two
  scale is exact in bf16/fp32, so only the atomic summation order may differ);
* the depth-wise stencils (spatial and temporal, forward and backward) on small-integer data are exact.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.gpu_helpers import dev, load_desc, read_stats, rel, stats_buffer, stream  # noqa: E402

B, T, H, W = 32, 32, 36, 64


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    return lib


def test_fullsize_pointwise_gemm_checksums_exact(L):
    """conv_pw of block 0 at full size: M = 32*32*36*64 rows, K = 64, N = 448, entries in {-1, 0, 1}."""
    M, K, N = B * T * H * W, 64, 448
    g = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(-1, 2, (M, K), generator=g, device=dev(), dtype=torch.int8)
    b = torch.randint(-1, 2, (N, K), generator=g, device=dev(), dtype=torch.int8)
    a16, b16 = a.to(torch.bfloat16), b.to(torch.bfloat16)
    c = torch.empty(M, N, dtype=torch.bfloat16, device=dev())
    st = stats_buffer(N)
    args = L.GemmNNArgs()
    args.a = load_desc(L, a16, K); args.a_kind = L.LD_PLAIN
    args.b = b16.data_ptr(); args.ldb = K; args.c = c.data_ptr(); args.ldc = N
    args.M, args.N, args.K, args.groups = M, N, K, 1
    args.stats = st.data_ptr(); args.stat_nchan = N; args.epi = L.EPI_STORE
    L.check(L.lib.dwn_gemm_nn(C.byref(args), L.DWN_BF16, 0, stream()), "gemm_nn")
    torch.cuda.synchronize()
    # column checksum: sum_m C[m][n] == (sum_m A[m][:]) . B[n][:]   (all integers, |C| <= 64 exact in bf16)
    col_a = a.to(torch.int64).sum(0)                                   # [K]
    want_sum = (b.to(torch.int64) * col_a[None, :]).sum(1)             # [N]
    got_sum = torch.zeros(N, dtype=torch.float64, device=dev())
    for r0 in range(0, M, 1 << 18):                                    # chunked fp64 reduction of the bf16 output
        got_sum += c[r0:r0 + (1 << 18)].double().sum(0)
    assert torch.equal(got_sum.to(torch.int64), want_sum)
    s0, s1 = read_stats(st, N)
    assert torch.equal(s0.to(torch.int64), want_sum)                   # fused BN sum: integers in fp64
    # sum of squares: exact integer too; checked on a 64 K-row prefix against int64 arithmetic plus globally vs the output
    sq = torch.zeros(N, dtype=torch.float64, device=dev())
    for r0 in range(0, M, 1 << 18):
        blk = c[r0:r0 + (1 << 18)].double()
        sq += (blk * blk).sum(0)
    assert torch.equal(s1.to(torch.int64), sq.to(torch.int64))
    rows = 1 << 16
    ref = a[:rows].to(torch.float32) @ b.to(torch.float32).t()        # exact in fp32
    assert torch.equal(c[:rows].float(), ref)
    tail = a[-rows:].to(torch.float32) @ b.to(torch.float32).t()
    assert torch.equal(c[-rows:].float(), tail)


def test_fullsize_weight_gradient_gemm_exact(L):
    """dW = P^T Q over the full 2.36 M rows with entries in {-1, 0, 1}: |dW| <= M < 2^24, exact in fp32 atomics."""
    M, R, Cc = B * T * H * W, 448, 64
    g = torch.Generator(device="cuda").manual_seed(6)
    p = torch.randint(-1, 2, (M, R), generator=g, device=dev(), dtype=torch.int8)
    q = torch.randint(-1, 2, (M, Cc), generator=g, device=dev(), dtype=torch.int8)
    p16, q16 = p.to(torch.bfloat16), q.to(torch.bfloat16)
    dw = torch.zeros(R, Cc, dtype=torch.float32, device=dev())
    args = L.GemmTNArgs()
    args.p = load_desc(L, p16, R); args.p_kind = L.LD_PLAIN
    args.q = load_desc(L, q16, Cc); args.q_kind = L.LD_PLAIN
    args.M, args.R, args.Cc = M, R, Cc
    args.dw = dw.data_ptr(); args.lddw = Cc; args.groups = 1; args.nsplit = 0
    L.check(L.lib.dwn_gemm_tn(C.byref(args), L.DWN_BF16, 0, stream()), "gemm_tn")
    torch.cuda.synchronize()
    want = torch.zeros(R, Cc, dtype=torch.int64, device=dev())
    for r0 in range(0, M, 1 << 18):
        want += (p[r0:r0 + (1 << 18)].to(torch.float32).t() @ q[r0:r0 + (1 << 18)].to(torch.float32)).to(torch.int64)
    assert torch.equal(dw.to(torch.int64), want)


def _model():
    from sensorium_amd import DwiseNeuro
    torch.manual_seed(0)
    m = DwiseNeuro(readout_outputs=(7863,), expansion_ratio=7, drop_rate=0.0, drop_path_rate=0.0,
                   compute_dtype=torch.bfloat16)
    return m.to(dev())


def _inputs():
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.zeros(B, 5, T, H, W, device=dev())
    x[:, 0] = torch.randint(0, 256, (B, T, H, W), generator=g, device=dev()).float()
    x[:, 1:] = torch.rand(B, 4, T, 1, 1, generator=g, device=dev()) * 50
    return x


def test_fullsize_eval_forward_is_per_sample():
    model = _model().eval()
    x = _inputs()
    with torch.no_grad():
        full = model(x)[0]
        part = model(x[8:12].contiguous())[0]
    torch.cuda.synchronize()
    assert full.shape == (B, 7863, T) and torch.isfinite(full).all()
    # eval BatchNorm uses running statistics: samples do not interact.  The two runs differ only in summation order
    # (fp32 atomics of the SE pooling sums; different tile partition for a different batch), which bf16 storage turns
    # into 1-ulp flips (2^-8) that propagate through 9 blocks: observed 2e-4 .. 1.2e-3, bound 1e-2 (the bf16 forward
    # tolerance used against the oracle elsewhere is 4e-2)
    assert rel(part, full[8:12]) < 1e-2


def test_fullsize_backward_is_linear_in_loss_scale():
    """One forward, three backward passes over the same saved activations (scales 1, 1, 2).

    A power-of-two loss scale is exact in bf16/fp32, so 2*g(1) and g(2) may differ only through the order of atomic
    accumulations.  Readout and cortex gradients have no such order dependence left and must match bit for bit; in the
    core that noise (~1e-6 at the last block) is amplified block by block on this random-init / random-target problem
    (BatchNorm-backward projections attenuate the signal, not the noise), so the linearity error is bounded by the
    run-to-run noise of two identical passes measured in the same test.
    """
    from sensorium_amd import MicePoissonLoss
    model = _model().train()
    x = _inputs()
    g = torch.Generator(device="cuda").manual_seed(2)
    target = torch.rand(B, 7863, T, generator=g, device=dev()) * 5
    w = torch.ones(B, 1, device=dev())
    loss = MicePoissonLoss()(model(x), ([target], w))
    grads = []
    for scale in (1.0, 1.0, 2.0):
        model.zero_grad(set_to_none=True)
        (loss * scale).backward(retain_graph=True)
        torch.cuda.synchronize()
        grads.append({k: p.grad.detach().double() / scale for k, p in model.named_parameters()})
    assert all(torch.isfinite(v).all() for v in grads[2].values())
    gn = sum(float(v.norm()) ** 2 for v in grads[0].values()) ** 0.5

    def err(a, b2, k):
        return float((a[k] - b2[k]).norm()) / (float(b2[k].norm()) + 1e-3 * gn)

    for k in grads[0]:
        if k.startswith("readouts.") or k.startswith("cortex."):
            assert torch.equal(grads[0][k], grads[2][k]), k
        else:
            noise = err(grads[0], grads[1], k)
            lin = err(grads[0], grads[2], k)
            assert lin <= 3.0 * noise + 1e-3, (k, lin, noise)
        if k.startswith("core.blocks.17."):
            assert err(grads[0], grads[2], k) < 1e-3, k


# ---- depth-wise stencils at the metric batch, exact-integer data (round-5 verdict, item 7a) ------------------------------------------
# spat_covn_dw forward / backward (src/models/dwiseneuro.py:96-102) of blocks 0, 1 and 4 at B = 32, T = 32, stored-y1 AND rebuilt-y1
# forms, on data chosen so that every intermediate is a small integer that bf16 holds exactly:
#   a0 in {0, 1}; W1 rows with exactly 16 ones  ->  y1 = a0 . W1^T in 0 .. 16 (integers; the rebuilt forms compute them by MFMA)
#   BatchNorm-1 scale 1, shift 17  ->  h = y1 + 17 >= 17, where the fp32 SiLU is the identity to the last bit that bf16 keeps
#     (exp2(-17 log2 e) < 2^-24: sigmoid = 1 within an ulp) and SiLU' = 1  ->  z1 = h in 17 .. 33
#   three non-zero taps of +-1 per channel  ->  |y2| <= 99; gradient rows g = dh2 in {-1, 0, 1} (A1 = 1, A2 = A3 = 0)  ->  |dh1| <= 3
# so y2, dh1, the 9-tap weight gradient and the BatchNorm-1 backward sums must EQUAL float64 arithmetic on the same integers.
def _exact_stencil_case(L, planes, Hin, Win, cin, E, stride):
    from tests.dw_reference import _dw3x3
    d = dev()
    s = stream()
    BF = torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(planes + Hin + cin + stride)
    Hout, Wout = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    Min, Mout = planes * Hin * Win, planes * Hout * Wout
    a0 = torch.randint(0, 2, (Min, cin), generator=g, device=d, dtype=torch.int8).to(BF)
    w1 = torch.zeros(E, cin, device=d)
    w1.scatter_(1, torch.rand(E, cin, generator=g, device=d).argsort(1)[:, :16], 1.0)
    w1 = w1.to(BF)
    taps = torch.zeros(E, 9, device=d)
    taps.scatter_(1, torch.rand(E, 9, generator=g, device=d).argsort(1)[:, :3], 1.0)
    taps = (taps * (torch.randint(0, 2, (E, 9), generator=g, device=d) * 2 - 1)).t().contiguous()          # [9][E], +-1 / 0
    dh2 = torch.randint(-1, 2, (Mout, E), generator=g, device=d, dtype=torch.int8).to(BF)
    y2in = torch.zeros(Mout, E, dtype=BF, device=d)                                                      # weighted with A2 = 0
    y1 = (a0.float() @ w1.float().t()).to(BF)                                                           # exact: integers 0 .. 16
    ones, zeros = torch.ones(E, device=d), torch.zeros(E, device=d)
    shift = torch.full((E,), 17.0, device=d)
    # float64 reference on the integers (linear activation: z1 = h, SiLU' = 1)
    h = (y1.double().view(planes, Hin, Win, E) + 17.0).requires_grad_(True)
    wd = taps.double().clone().requires_grad_(True)
    y2_ref = _dw3x3(h, wd, stride)
    y2_ref.backward(dh2.double().view(planes, Hout, Wout, E))
    y2_ref = y2_ref.detach().reshape(Mout, E)
    dh1_ref = h.grad.reshape(Min, E)
    dw_ref = wd.grad.t().contiguous()                                                                   # [E][9]
    sum_dh1 = dh1_ref.sum(0)
    sum_dh1_y1 = (dh1_ref * y1.double()).sum(0)
    del h
    for mode in ("stored", "rebuilt"):
        # ---- forward
        y2 = torch.full((Mout, E), float("nan"), dtype=BF, device=d)
        st = torch.zeros(32 * 2 * E, dtype=torch.float64, device=d)
        f = L.DwSpatialFwdArgs()
        di = L.LoadDesc()
        di.p = y1.data_ptr() if mode == "stored" else None
        di.ld = E; di.rows_per_sample = 1; di.v1 = ones.data_ptr(); di.v2 = shift.data_ptr(); di.act = 1
        f.inp = di
        f.w = taps.data_ptr(); f.out = y2.data_ptr(); f.planes = planes; f.Hin = Hin; f.Win = Win; f.Hout = Hout; f.Wout = Wout
        f.C = E; f.stride = stride; f.ks = 3; f.stats = st.data_ptr()
        if mode == "rebuilt":
            f.a0 = a0.data_ptr(); f.a0_ld = cin; f.w1 = w1.data_ptr(); f.Cin = cin
            assert L.lib.dwn_dw_spatial_fwd_rc_supported(C.byref(f), L.DWN_BF16) == 1
        L.check(L.lib.dwn_dw_spatial_fwd(C.byref(f), L.DWN_BF16, 0, s), "dwn_dw_spatial_fwd")
        torch.cuda.synchronize()
        assert torch.equal(y2.double(), y2_ref), (mode, "y2")
        s0, s1 = read_stats(st, E)
        assert torch.equal(s0, y2_ref.sum(0)), (mode, "sum y2")                        # integers below 2^24 in every partial sum
        assert rel(s1, (y2_ref ** 2).sum(0)) < 1e-6, (mode, "sum y2^2")                 # fp32 partial sums beyond 2^24: rounded
        del y2
        # ---- backward
        dh1 = torch.full((Min, E), float("nan"), dtype=BF, device=d)
        dw = torch.zeros(E, 9, device=d)
        st = torch.zeros(32 * 2 * E, dtype=torch.float64, device=d)
        b = L.DwSpatialBwdArgs()
        b.dy = load_desc(L, dh2, E, q=y2in, v1=ones, v2=zeros, v3=zeros)
        b.y1 = load_desc(L, y1, E, v1=ones, v2=shift, v3=zeros, v4=ones)                # mean 0, invstd 1: yhat1 = y1
        b.w = taps.data_ptr(); b.dh1 = dh1.data_ptr(); b.dw = dw.data_ptr(); b.planes = planes; b.Hin = Hin; b.Win = Win
        b.Hout = Hout; b.Wout = Wout; b.C = E; b.stride = stride; b.ks = 3; b.stats = st.data_ptr()
        if mode == "rebuilt":
            b.y1.p = None
            b.a0 = a0.data_ptr(); b.a0_ld = cin; b.w1 = w1.data_ptr(); b.Cin = cin
            assert L.lib.dwn_dw_spatial_bwd_rc_supported(C.byref(b), L.DWN_BF16) == 1
        L.check(L.lib.dwn_dw_spatial_bwd(C.byref(b), L.DWN_BF16, 0, s), "dwn_dw_spatial_bwd")
        torch.cuda.synchronize()
        assert torch.equal(dh1.double(), dh1_ref), (mode, "dh1")
        assert torch.equal(dw.double(), dw_ref), (mode, "dW")
        s0, s1 = read_stats(st, E)
        assert torch.equal(s0, sum_dh1) and torch.equal(s1, sum_dh1_y1), (mode, "BatchNorm-1 backward sums")
        del dh1


@pytest.mark.parametrize("geom", [(36, 64, 64, 448, 2), (18, 32, 64, 448, 1), (18, 32, 128, 896, 2)], ids=["block0", "block1", "block4"])
def test_fullsize_depthwise_stencils_exact(L, geom):
    _exact_stencil_case(L, B * T, *geom)


@pytest.mark.parametrize("geom", [(9, 16, 128, 896, 1), (5, 8, 64, 448, 1), (9, 16, 64, 448, 2)], ids=["block5", "w8", "w16s2"])
def test_depthwise_stencils_exact_other_plane_widths(L, geom):
    """The narrower plane widths (several planes side by side in one tile) with a ragged plane count."""
    _exact_stencil_case(L, 131, *geom)


# ---- temp_covn_dw at the metric batch, exact-integer data ------------------------------------------------------------------------------
# The temporal forward and the y3-recomputing backward (DWN_LD_PLAIN, what the block backward runs; src/models/dwiseneuro.py:105-111)
# of blocks 0, 4 and 8 at B = 32, T = 32, on data built like the spatial cases above so that every intermediate is a small integer:
#   y2 in 0 .. 3; BatchNorm-2 scale 1, shift 17  ->  z2 = h = y2 + 17 in 17 .. 20 and SiLU' = 1 (1 + exp(-h) rounds to 1.0f: see above)
#   exactly three (kt = 5) / two (kt = 3) non-zero taps of +-1 per channel  ->  |y3| <= 60
#   dh3 in {-1, 0, 1}, A1 = 1, A2 = 1, A3 = 0: dy3 = dh3 + y3, so the RECOMPUTED y3 matters  ->  |dy3| <= 61, |dh2| <= 183
# bf16 holds all of them exactly, so y3 and dh2 must EQUAL float64 arithmetic on the same integers — what a tolerance cannot see: a wrong
# frame at a boundary, an index that wraps at 2.6e8 elements, a lost atomic.
def _exact_temporal_case(L, Bn, Tn, HW, E, kt, dtype):
    from tests.dw_reference import _dwt
    d = dev()
    s = stream()
    dt = L.DWN_BF16 if dtype == torch.bfloat16 else L.DWN_F32
    g = torch.Generator(device="cuda").manual_seed(HW + E + kt)
    M = Bn * Tn * HW
    y2 = torch.randint(0, 4, (M, E), generator=g, device=d, dtype=torch.int8).to(dtype)
    taps = torch.zeros(E, kt, device=d)
    taps.scatter_(1, torch.rand(E, kt, generator=g, device=d).argsort(1)[:, :(3 if kt == 5 else 2)], 1.0)
    taps = (taps * (torch.randint(0, 2, (E, kt), generator=g, device=d) * 2 - 1)).t().contiguous()        # [kt][E], +-1 / 0
    dh3 = torch.randint(-1, 2, (M, E), generator=g, device=d, dtype=torch.int8).to(dtype)
    ones, zeros = torch.ones(E, device=d), torch.zeros(E, device=d)
    shift = torch.full((E,), 17.0, device=d)
    # float64 reference on the integers (linear activation: z2 = h, SiLU' = 1)
    h = (y2.double().view(Bn, Tn, HW, E) + 17.0).requires_grad_(True)
    wd = taps.double().clone().requires_grad_(True)
    y3_ref = _dwt(h, wd)
    y3_ref.backward(dh3.double().view(Bn, Tn, HW, E) + y3_ref.detach())
    y3_ref = y3_ref.detach().reshape(M, E)
    dh2_ref = h.grad.reshape(M, E)
    dw_ref = wd.grad.t().contiguous()                                                                   # [E][kt]
    del h
    assert float(y3_ref.abs().max()) <= 60 and float(dh2_ref.abs().max()) <= 183
    # ---- forward
    y3 = torch.full((M, E), float("nan"), dtype=dtype, device=d)
    st = stats_buffer(E)
    f = L.DwTemporalFwdArgs()
    f.inp = load_desc(L, y2, E, v1=ones, v2=shift, act=1)
    f.w = taps.data_ptr(); f.out = y3.data_ptr(); f.B = Bn; f.T = Tn; f.HW = HW; f.C = E; f.kt = kt; f.stats = st.data_ptr()
    L.check(L.lib.dwn_dw_temporal_fwd(C.byref(f), dt, 0, s), "dwn_dw_temporal_fwd")
    torch.cuda.synchronize()
    assert torch.equal(y3.double(), y3_ref), "y3"
    s0, s1 = read_stats(st, E)
    # fp32 partial sums end at the workgroup (the replicas are doubles).  The persistent grid has at least 2 * 256 / slices workgroups per
    # channel slice, so a workgroup sums at most 8192 elements of a channel (block 0: 16 rounds of 16 positions, 32 frames; fewer at the
    # other widths).  sum y3: 8192 * 60 < 2^24: exact.  sum y3^2: 8192 * 3600 > 2^24: rounded
    assert torch.equal(s0, y3_ref.sum(0)), "sum y3"
    assert rel(s1, (y3_ref ** 2).sum(0)) < 1e-6, "sum y3^2"
    del y3
    # ---- backward, y3 recomputed
    dh2 = torch.full((M, E), float("nan"), dtype=dtype, device=d)
    dw = torch.zeros(E, kt, device=d)
    st = stats_buffer(E)
    b = L.DwTemporalBwdArgs()
    b.dy = load_desc(L, dh3, E, v1=ones, v2=ones, v3=zeros); b.dy_kind = L.LD_PLAIN
    b.y2 = load_desc(L, y2, E, v1=ones, v2=shift, v3=zeros, v4=ones)                    # mean 0, invstd 1: yhat2 = y2
    b.w = taps.data_ptr(); b.dh2 = dh2.data_ptr(); b.dw = dw.data_ptr()
    b.B = Bn; b.T = Tn; b.HW = HW; b.C = E; b.kt = kt; b.stats = st.data_ptr()
    L.check(L.lib.dwn_dw_temporal_bwd(C.byref(b), dt, 0, s), "dwn_dw_temporal_bwd")
    torch.cuda.synchronize()
    assert torch.equal(dh2.double(), dh2_ref), "dh2"
    s0, s1 = read_stats(st, E)
    # sum dh2 (<= 183 per element) and sum dh2 * y2 (<= 549): 8192 * 549 < 2^24: exact
    assert torch.equal(s0, dh2_ref.sum(0)), "sum dh2"
    assert torch.equal(s1, (dh2_ref * y2.double()).sum(0)), "sum dh2 * y2"
    # dW[k] = sum z2(t) dy3(t - k + P): terms up to 20 * 61, of one sign where the taps do not cancel; a workgroup's share is exact
    # (8192 * 1220 < 2^24) but the workgroups add into one fp32 word per (channel, tap), |dW| up to 6e8 > 2^24: rounded
    assert rel(dw, dw_ref) < 1e-6, "dW"


@pytest.mark.parametrize("geom", [(576, 448, 5, torch.bfloat16), (144, 896, 5, torch.bfloat16), (40, 1792, 5, torch.bfloat16),
                                  (576, 448, 3, torch.bfloat16), (40, 1792, 5, torch.float32)],
                         ids=["block0", "block4", "block8", "block0-kt3", "block8-fp32"])
def test_fullsize_temporal_depthwise_exact(L, geom):
    _exact_temporal_case(L, B, T, *geom)

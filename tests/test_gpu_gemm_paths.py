"""dwn_gemm_nn / dwn_gemm_tn through the C-ABI on every dispatch path, element by element (reference, bound and case lists:
tests/gemm_reference.py, itself checked by tests/test_gemm_reference_cpu.py; the table of paths: DESIGN.md 12j).

  exact   integer operands: the stored product, dW, dg and both BatchNorm sums equal the float64 reference BIT FOR BIT.
  random  Gaussian operands: |got - ref| <= elem_bound on EVERY element (no share may exceed).

Every output buffer is NaN-filled first and must come back finite; buffers the header says the caller zeroes are zeroed.  Each test
prints `GEMM <path> <case> max_ratio=...` before it asserts.  Default library only: the deterministic build routes around the
256-row kernel and the DG epilogue."""
import ctypes as C

import pytest
import torch

from tests import gemm_reference as R
from tests.gemm_reference import BF16, F32
from tests.gpu_helpers import dev, load_desc, read_stats, stats_buffer, stream

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import sensorium_amd._lib as lib
    if lib.DETERMINISTIC:
        pytest.skip("the default library only: the deterministic build routes around the 256-row kernel and the DG epilogue")
    return lib


def _dt(L, dtype):
    return L.DWN_BF16 if dtype == BF16 else L.DWN_F32


def _report(path, case, **kw):
    """One line per figure, printed before anything is asserted (pytest -s or a failure shows them)."""
    print("GEMM", path, case, " ".join(f"{k}={v:.4e}" if isinstance(v, float) else f"{k}={v}" for k, v in kw.items()), flush=True)


def _finish(L, rc, what):
    """Check the return code and wait for the kernel.  A device error (not a wrong result) ends the session: after a fault nothing
    further is launched on that device."""
    try:
        L.check(rc, what)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if rc > 0 or "HIP" in str(e) or "hip" in str(e):
            pytest.exit(f"{what}: device error, stopping: {e}", returncode=3)
        raise


def _desc(L, o):
    """dwn_load_desc of a gemm_reference.Operand (whose tensors stay alive with it)."""
    cols = o.p.shape[1]
    if o.kind == R.LD_PE:
        return load_desc(L, o.p, cols, pe_t=o.pe_t, pe_h=o.pe_h, pe_w=o.pe_w, pT=o.T, pH=o.H, pW=o.W, pe_ld=cols)
    if o.kind == R.LD_BNACT:
        kw = dict(gate=o.gate, gate_ld=cols, rows_per_sample=o.rows_per_sample) if o.gate is not None else {}
        return load_desc(L, o.p, cols, v1=o.v1, v2=o.v2, act=o.act, **kw)
    if o.kind == R.LD_AFFINE2:
        return load_desc(L, o.p, cols, q=o.q, v1=o.v1, v2=o.v2, v3=o.v3)
    if o.kind == R.LD_GATE:
        return load_desc(L, o.p, cols, gate=o.gate, gate_ld=cols, rows_per_sample=o.rows_per_sample)
    if o.kind == R.LD_CAT1:
        return load_desc(L, o.p, cols, q=o.q, ld2=o.q.shape[1], cat_c1=cols, cat_c2=o.q.shape[1])
    return load_desc(L, o.p, cols)


def _ratio(got, ref, bound):
    """(elements over the bound, largest |got - ref| / bound); chunked so that the walking cases keep their temporaries small."""
    over, worst = 0, 0.0
    for r0 in range(0, got.shape[0], 65536):
        err = (got[r0:r0 + 65536].double() - ref[r0:r0 + 65536]).abs()
        b = bound[r0:r0 + 65536]
        over += int((err > b).sum())
        worst = max(worst, float((err / b.clamp_min(1e-300)).max()))
    return over, worst


def _run_nn(L, p):
    M, N, K, G = p.M, p.N, p.K, p.groups
    c = torch.full((M, G * N), float("nan"), dtype=p.dtype, device=dev())
    st = stats_buffer(G * N)
    g = L.GemmNNArgs()
    g.a = _desc(L, p.a); g.a_kind = p.a.kind
    g.b = p.b.data_ptr(); g.ldb = K; g.c = c.data_ptr(); g.ldc = G * N
    g.M, g.N, g.K, g.groups = M, N, K, G
    g.stats = st.data_ptr(); g.stat_nchan = G * N; g.epi = L.EPI_STORE
    g.f32_split = p.split
    g.variant = {"auto": L.NN_AUTO, "xl128": L.NN_XL128, "xl256": L.NN_XL256, "tile128": L.NN_TILE128, "kd": L.NN_KD}[p.case.get("variant", "auto")]
    dg = None
    if p.epi == "cat":
        g.epi = L.EPI_STORE_CAT; g.a2 = p.a2.data_ptr(); g.a2_ld = p.a2.shape[1]; g.K1 = p.K1; g.bias = p.bias.data_ptr()
    elif p.epi == "dg":
        dg = torch.zeros(M // p.rows, N, device=dev())                 # the caller zeroes dg (include/dwn.h: dg += ...)
        g.epi = L.EPI_DG; g.y3 = p.z3.data_ptr(); g.ldy3 = N; g.dg = dg.data_ptr(); g.dg_ld = N; g.rows_per_sample = p.rows
    if p.b_rows:
        g.b_sample_stride = N * K; g.b_rows_per_sample = p.b_rows
    _finish(L, L.lib.dwn_gemm_nn(C.byref(g), _dt(L, p.dtype), 0, stream()), "gemm_nn " + p.case["name"])
    s0, s1 = read_stats(st, G * N)
    return c, s0, s1, dg


def _check_nn(L, case, mode):
    p = R.NNProblem(case, mode, dev())
    path = R.nn_dispatch(case) + ("+split" if p.split else "") + ("+dg" if p.epi == "dg" else "")
    name = f"{case['name']}[{mode}]"
    c, s0, s1, dg = _run_nn(L, p)
    finite = bool(torch.isfinite(c.float()).all()) and bool(torch.isfinite(s0).all()) and bool(torch.isfinite(s1).all())
    if mode == "exact":
        ref, _ = p.reference()
        want = ref.to(p.dtype)
        r0, r1, _ = R.stats_reference(want)
        bad = int((c != want).sum())
        _report(path, name, max_ratio=0.0 if bad == 0 else float("inf"), mismatches=bad,
                stats_equal=bool(torch.equal(s0, r0) and torch.equal(s1, r1)))
        assert finite
        assert torch.equal(c, want)
        assert torch.equal(s0, r0) and torch.equal(s1, r1)
        if dg is not None:
            want_dg, _ = R.dg_reference(want, p.z3, p.rows)
            assert torch.isfinite(dg).all() and torch.equal(dg.double(), want_dg)
        return
    if p.computed_bf16:
        ref, S, mab = p.reference(want_maxab=True)
        bound = R.elem_bound(ref, S, p.n_terms, R.U[p.dtype], p.extra) + R.flip_allowance(mab)
    else:
        ref, S = p.reference()
        bound = R.elem_bound(ref, S, p.n_terms, R.U[p.dtype], p.extra)
    over, worst = _ratio(c, ref, bound)
    # the BatchNorm sums and dg are sums of the values the kernel stored: those are the operands, nothing is rounded on the way out
    r0, r1, a0 = R.stats_reference(c)
    o0, w0 = _ratio(s0, r0, R.elem_bound(r0, a0, p.M, 0.0))
    o1, w1 = _ratio(s1, r1, R.elem_bound(r1, r1, p.M, 0.0))
    og, wg = 0, 0.0
    if dg is not None:
        want_dg, Sg = R.dg_reference(c, p.z3, p.rows)
        og, wg = _ratio(dg, want_dg, R.elem_bound(want_dg, Sg, p.rows, 0.0))
        finite = finite and bool(torch.isfinite(dg).all())
    _report(path, name, max_ratio=worst, over=over, sum_ratio=w0, sumsq_ratio=w1, dg_ratio=wg)
    assert finite
    assert over == 0
    assert o0 == 0 and o1 == 0 and og == 0


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.NN_CASES, ids=R.case_id)
def test_gemm_nn_paths(L, case, mode):
    _check_nn(L, case, mode)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.DG_CASES, ids=R.case_id)
def test_gemm_nn_dg_epilogue(L, case, mode):
    _check_nn(L, case, mode)


def _tn_args(L, p, dw):
    case = p.case
    g = L.GemmTNArgs()
    g.p = _desc(L, p.p); g.p_kind = p.p.kind
    g.q = _desc(L, p.q); g.q_kind = p.q.kind
    g.M, g.R, g.Cc = p.M, p.R, p.Cc
    g.dw = dw.data_ptr(); g.lddw = p.Cc; g.groups = p.groups
    g.nsplit = case.get("nsplit", 0); g.rows_per_split = case.get("rows_per_split", 0)
    g.R_load = case.get("R_load", 0)
    g.overwrite = case.get("overwrite", 0); g.dw_f64 = case.get("dw_f64", 0)
    return g


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("case", R.TN_CASES, ids=R.case_id)
def test_gemm_tn_paths(L, case, mode):
    p = R.TNProblem(case, mode, dev())
    shape = (p.groups * p.R, p.Cc)
    if case.get("dw_f64"):
        dw = torch.zeros(shape, dtype=torch.float64, device=dev())       # accumulated into: the caller zeroes it
    elif case.get("overwrite"):
        dw = torch.full(shape, float("nan"), device=dev())               # dW = the product: need not be zeroed
    else:
        dw = torch.zeros(shape, device=dev())
    g = _tn_args(L, p, dw)
    _finish(L, L.lib.dwn_gemm_tn(C.byref(g), _dt(L, p.dtype), 0, stream()), "gemm_tn " + case["name"])
    name = f"{case['name']}[{mode}]"
    finite = bool(torch.isfinite(dw).all())
    if mode == "exact":
        ref, _ = p.reference()
        bad = int((dw.double() != ref).sum())
        _report("tn", name, max_ratio=0.0 if bad == 0 else float("inf"), mismatches=bad)
        assert finite
        assert torch.equal(dw.double(), ref)
        return
    if p.computed_bf16:
        ref, S, mab = p.reference(want_maxab=True)
        bound = R.elem_bound(ref, S, p.M, R.U[F32]) + R.flip_allowance(mab)
    else:
        ref, S = p.reference()
        bound = R.elem_bound(ref, S, p.M, R.U[F32])       # every M-split's partial tile is an fp32 accumulator, dw_f64 included
    over, worst = _ratio(dw, ref, bound)
    _report("tn", name, max_ratio=worst, over=over)
    assert finite
    assert over == 0


# ---- refusals: answered by the host before anything is enqueued --------------------------------------------------------------------------
SENTINEL = 7.0


def _refused(L, rc, want, out):
    torch.cuda.synchronize()
    assert rc == want, (rc, L.lib.dwn_last_error())
    assert L.lib.dwn_last_error()
    assert bool((out.float() == SENTINEL).all()), "a refused call wrote to its output"


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gemm_nn_refusals(L, dtype):
    M, N, K = 256, 64, 128
    kc = R.KC[dtype]
    a = torch.zeros(M, 2 * K, dtype=dtype, device=dev())
    b = torch.zeros(2 * N, K, dtype=dtype, device=dev())
    c = torch.full((M, 2 * N), SENTINEL, dtype=dtype, device=dev())
    f = torch.full((2 * N,), SENTINEL, device=dev())
    ones = torch.ones(2 * K, device=dev())
    out_nct = torch.full((M * 2 * N,), SENTINEL, device=dev())

    def base():
        g = L.GemmNNArgs()
        g.a = load_desc(L, a, 2 * K); g.a_kind = L.LD_PLAIN
        g.b = b.data_ptr(); g.ldb = K; g.c = c.data_ptr(); g.ldc = 2 * N
        g.M, g.N, g.K, g.groups = M, N, K, 1
        g.epi = L.EPI_STORE
        return g

    def call(g):
        return L.lib.dwn_gemm_nn(C.byref(g), _dt(L, dtype), 0, stream())

    g = base(); g.N = N - kc // 2                                         # N % vector != 0
    _refused(L, call(g), -2, c)
    g = base(); g.epi = L.EPI_DG; g.y3 = a.data_ptr(); g.ldy3 = 2 * K; g.dg = f.data_ptr(); g.dg_ld = N; g.rows_per_sample = 128
    g.groups = 2                                                          # DG with groups = 2
    _refused(L, call(g), -3, c); assert bool((f == SENTINEL).all())
    g.groups = 1; g.a_kind = L.LD_GATE; g.a.gate = ones.data_ptr(); g.a.gate_ld = K; g.a.rows_per_sample = 128     # DG, non-plain loader
    _refused(L, call(g), -3, c); assert bool((f == SENTINEL).all())
    g = base(); g.epi = L.EPI_STORE_CAT; g.a2 = a.data_ptr(); g.a2_ld = 2 * K; g.K1 = 64; g.bias = None                # K-concat, no bias
    _refused(L, call(g), -3, c)
    g.bias = f.data_ptr(); g.K1 = 64 + kc // 2                            # K-concat with K1 % vector != 0
    _refused(L, call(g), -3, c)
    g = base(); g.epi = L.EPI_READOUT; g.sp_beta_dev = ones.data_ptr(); g.out_nct = out_nct.data_ptr(); g.Tn = 16; g.n_valid = N
    g.a_kind = L.LD_BNACT; g.a.v1 = ones.data_ptr(); g.a.v2 = ones.data_ptr()      # readout with a device beta, non-plain loader
    _refused(L, call(g), -3, out_nct)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_gemm_tn_refusals(L, dtype):
    M, R_, Cc = 1100, 64, 72
    p = torch.zeros(M, 2 * R_, dtype=dtype, device=dev())
    q = torch.zeros(M, 2 * Cc, dtype=dtype, device=dev())
    dw = torch.full((2 * R_, 2 * Cc), SENTINEL, device=dev())
    ones = torch.ones(2 * R_, device=dev())

    def base():
        g = L.GemmTNArgs()
        g.p = load_desc(L, p, 2 * R_); g.p_kind = L.LD_PLAIN
        g.q = load_desc(L, q, 2 * Cc); g.q_kind = L.LD_PLAIN
        g.M, g.R, g.Cc = M, R_, Cc
        g.dw = dw.data_ptr(); g.lddw = Cc; g.groups = 1; g.nsplit = 0
        return g

    def call(g):
        return L.lib.dwn_gemm_tn(C.byref(g), _dt(L, dtype), 0, stream())

    g = base(); g.p_kind = L.LD_GATE; g.p.gate = ones.data_ptr(); g.p.gate_ld = R_; g.p.rows_per_sample = 100      # an unlisted pair
    _refused(L, call(g), -3, dw)
    g = base(); g.dw_f64 = 1; g.overwrite = 1                             # dw_f64 with overwrite
    _refused(L, call(g), -2, dw)
    g = base(); g.overwrite = 1; g.lddw = 2 * Cc                          # overwrite with lddw != Cc
    _refused(L, call(g), -2, dw)
    g = base(); g.p_kind = L.LD_CAT1; g.p.q = p.data_ptr(); g.p.ld2 = 2 * R_; g.p.cat_c1 = 32; g.p.cat_c2 = 24
    g.groups = 2                                                          # CAT1 with groups = 2
    _refused(L, call(g), -2, dw)
    g.groups = 1; g.p.cat_c1 = 48                                         # CAT1 with R < cat_c1 + cat_c2
    _refused(L, call(g), -2, dw)
    for overwrite in (0, 1):      # (with overwrite the library would zero dW before the launch: refused before that too)
        g = base(); g.overwrite = overwrite; g.nsplit = 3; g.rows_per_split = 0                    # caller's splits: no rows
        _refused(L, call(g), -2, dw)
        g.rows_per_split = -64
        _refused(L, call(g), -2, dw)
        g.rows_per_split = 320                                            # caller's splits: 3 * 320 < M, rows would be left out
        _refused(L, call(g), -2, dw)
        g.nsplit = 1; g.rows_per_split = M - 1
        _refused(L, call(g), -2, dw)

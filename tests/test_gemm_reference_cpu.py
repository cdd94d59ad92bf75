"""The checker of the GEMM kernel tests, checked on the CPU (tests/gemm_reference.py; the device tests are tests/test_gpu_gemm_paths.py):
  room         the same formulas in float32 on the rounded operands, rounded once, meet elem_bound on every element of every random
               case — the bound leaves room for a correct kernel;
  teeth        a result that is wrong in one of the ways these kernels can go wrong differs from the exact-integer reference;
  sensitivity  the bound of the bf16x3 products notices a dropped lo*hi term at small K (and, as computed, not at K = 1792);
  coverage     the case lists reach every dispatch path of launch_gemm_nn at least once per storage type the path is built for.
"""
import pytest
import torch

from tests import gemm_reference as R
from tests.gemm_reference import BF16, F32

CPU = torch.device("cpu")
BIG = 20000          # cases with more rows than this are built once per test at most (the walking cases)


def _ids(cases):
    return [R.case_id(c) for c in cases]


def _over(got, ref, bound):
    """(share of elements over the bound, largest |got - ref| / bound)."""
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    return float((err > bound).double().mean()), float(ratio.max())


# ---- room --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.NN_CASES + R.DG_CASES, ids=_ids(R.NN_CASES + R.DG_CASES))
def test_room_nn(case):
    p = R.NNProblem(case, "random", CPU)
    ref, S, mab = p.reference(want_maxab=True) if p.computed_bf16 else (*p.reference(), None)
    bound = R.elem_bound(ref, S, p.n_terms, R.U[p.dtype], p.extra)
    if mab is not None:
        bound = bound + R.flip_allowance(mab)
    c = p.emulate()
    share, worst = _over(c, ref, bound)
    print("ROOM nn", case["name"], f"max_ratio={worst:.3f}")
    assert share == 0.0
    # the sums of the stored values, added up in float32
    s0, s1, a0 = R.stats_reference(c)
    cf = c.float()
    assert _over(cf.sum(0), s0, R.elem_bound(s0, a0, p.M, 0.0))[0] == 0.0
    assert _over((cf * cf).sum(0), s1, R.elem_bound(s1, s1, p.M, 0.0))[0] == 0.0
    if p.z3 is not None:
        dg, Sg = R.dg_reference(c, p.z3, p.rows)
        got = (cf * p.z3.float()).view(-1, p.rows, p.N).sum(1)
        assert _over(got, dg, R.elem_bound(dg, Sg, p.rows, 0.0))[0] == 0.0


@pytest.mark.parametrize("case", R.TN_CASES, ids=_ids(R.TN_CASES))
def test_room_tn(case):
    p = R.TNProblem(case, "random", CPU)
    ref, S, mab = p.reference(want_maxab=True) if p.computed_bf16 else (*p.reference(), None)
    bound = R.elem_bound(ref, S, p.M, R.U[F32])
    if mab is not None:
        bound = bound + R.flip_allowance(mab)
    share, worst = _over(p.emulate(), ref, bound)
    print("ROOM tn", case["name"], f"max_ratio={worst:.3f}")
    assert share == 0.0


# ---- exact cases: the preconditions hold, and float32 arithmetic in another order gives the same bits -------------------------------------
@pytest.mark.parametrize("case", R.NN_CASES + R.DG_CASES, ids=_ids(R.NN_CASES + R.DG_CASES))
def test_exact_nn_is_order_independent(case):
    p = R.NNProblem(case, "exact", CPU)
    ref, S = p.reference()                       # asserts the preconditions
    c = ref.to(p.dtype)
    assert torch.equal(p.emulate(), c)
    cf = c.float()
    s0, s1, _ = R.stats_reference(c)
    assert torch.equal(cf.sum(0).double(), s0) and torch.equal((cf * cf).sum(0).double(), s1)
    if p.z3 is not None:
        dg, _ = R.dg_reference(c, p.z3, p.rows)
        assert torch.equal((cf * p.z3.float()).view(-1, p.rows, p.N).sum(1).double(), dg)


@pytest.mark.parametrize("case", R.TN_CASES, ids=_ids(R.TN_CASES))
def test_exact_tn_is_order_independent(case):
    p = R.TNProblem(case, "exact", CPU)
    ref, S = p.reference()
    assert torch.equal(p.emulate().double(), ref)


# ---- teeth -------------------------------------------------------------------------------------------------------------------------
_SMALL_NN = [c for c in R.NN_CASES if c["M"] <= BIG]


@pytest.mark.parametrize("case", _SMALL_NN + R.DG_CASES, ids=_ids(_SMALL_NN + R.DG_CASES))
def test_teeth_nn(case):
    p = R.NNProblem(case, "exact", CPU)
    ref, _ = p.reference()
    c = ref.to(p.dtype)
    # a dropped last k-vector
    assert not torch.equal(p.reference(mutate="drop_kvec")[0].to(p.dtype), c)
    # two output rows swapped
    sw = c.clone()
    sw[[0, 1]] = c[[1, 0]]
    assert not torch.equal(sw, c)
    # the last M row omitted: from the store (its row stays as the buffer was) and from the column sums
    s0, s1, _ = R.stats_reference(c)
    t0, t1, _ = R.stats_reference(c[:-1])
    assert c[-1].any() and not torch.equal(t1, s1)
    if p.groups > 1:         # group 1 reading group 0's columns
        assert not torch.equal(p.reference(mutate="group_cols")[0].to(p.dtype), c)
    if p.z3 is not None:     # a sample boundary shifted by one row; the last row left out of its sample's sum
        dg, _ = R.dg_reference(c, p.z3, p.rows)
        assert not torch.equal(R.dg_reference(c, p.z3, p.rows, shift=1)[0], dg)
        assert not torch.equal(R.dg_reference(c, p.z3, p.rows, shift=-1)[0], dg)
        last = c.clone()
        last[-1] = 0
        assert not torch.equal(R.dg_reference(last, p.z3, p.rows)[0], dg)


@pytest.mark.parametrize("case", R.TN_CASES, ids=_ids(R.TN_CASES))
def test_teeth_tn(case):
    p = R.TNProblem(case, "exact", CPU)
    ref, _ = p.reference()
    assert not torch.equal(p.reference(m_end=p.M - 1)[0], ref)                      # the last M row omitted
    sw = ref.clone()
    sw[[0, 1]] = ref[[1, 0]]
    assert not torch.equal(sw, ref)                                                 # two output rows swapped
    rps = case.get("rows_per_split", 0)
    if case.get("nsplit", 0) > 1:                                                   # the last split omitted
        assert not torch.equal(p.reference(m_end=(case["nsplit"] - 1) * rps)[0], ref)
    if p.p.kind == R.LD_CAT1:                                                       # the "1" columns read as 0
        assert not torch.equal(p.reference(mutate="ones_zero")[0], ref)
    if p.groups > 1:                                                                # group 1 reading group 0's columns
        assert not torch.equal(p.reference(mutate="group_cols")[0], ref)


def test_teeth_apply_somewhere():
    """Every mutation above has at least one case it fits."""
    assert any(c.get("groups", 1) > 1 for c in _SMALL_NN) and any(c.get("groups", 1) > 1 for c in R.TN_CASES)
    assert any(c.get("nsplit", 0) > 1 for c in R.TN_CASES)
    assert any(c.get("p_kind") == R.LD_CAT1 for c in R.TN_CASES)
    assert R.DG_CASES


# ---- sensitivity of the split bound ----------------------------------------------------------------------------------------------------
def _split_share(M, N, K):
    case = dict(name=f"sens-{M}x{N}x{K}", dtype=F32, M=M, N=N, K=K, split=1)
    p = R.NNProblem(case, "random", CPU)
    ref, S = p.reference()
    bound = R.elem_bound(ref, S, K, R.U[F32], R.SPLIT_EXTRA)
    assert _over(p.emulate(), ref, bound)[0] == 0.0                 # the full product has room ...
    return _over(p.emulate(drop_lohi=True), ref, bound)[0]         # ... the one without lo*hi: share of elements over the bound


def test_split_bound_notices_a_dropped_term_at_small_k():
    for K in (32, 40, 72):
        share = _split_share(300, 136, K)
        print("SENS split", K, f"share_over={share:.3f}")
        assert share > 0.5
    # at K = 1792 the summation term of the bound dominates and the dropped term hides under it: the reason the split cases
    # include K <= 72
    share = _split_share(64, 136, 1792)
    print("SENS split", 1792, f"share_over={share:.3f}")
    assert share < 0.5
    assert all(c["K"] <= 72 for c in R.NN_CASES if c.get("split"))


# ---- coverage of the dispatch ---------------------------------------------------------------------------------------------------------
def test_case_lists_reach_every_dispatch_path():
    reached = {}
    for c in R.NN_CASES + R.DG_CASES:
        key = (R.nn_dispatch(c), c["dtype"])
        reached.setdefault(key, []).append(c)
    tile_paths = [f"t{bn}.{k}" for bn in (64, 128) for k in ("single1", "single2", "kloop")]
    for dt in (BF16, F32):
        for path in tile_paths:
            assert (path, dt) in reached, (path, dt)
    for path in ("t64.dma", "t128.dma", "xl128", "xl256", "kd"):        # built for bf16 only
        assert (path, BF16) in reached, path
        assert (path, F32) not in reached, path

    def has(pred, dts=(BF16, F32)):
        return all(any(c["dtype"] == dt and pred(c) for c in R.NN_CASES + R.DG_CASES) for dt in dts)

    disp = R.nn_dispatch
    # loaders on the k-loop kernel, K-concat on the 128-row kernel, groups, per-sample weights
    for ld in (R.LD_PE, R.LD_BNACT, R.LD_AFFINE2, R.LD_GATE):
        assert has(lambda c: c.get("loader") == ld and disp(c) == "t128.kloop")
    assert has(lambda c: c.get("loader") == R.LD_BNACT and c.get("act") == 1 and c.get("gated"))
    assert has(lambda c: c.get("loader") == R.LD_BNACT and c.get("act") == 0 and not c.get("gated"))
    assert has(lambda c: c.get("epi") == "cat" and disp(c).startswith("t128"))
    assert has(lambda c: c.get("groups", 1) == 2 and disp(c).startswith("t"))
    assert has(lambda c: c.get("b_rows") == 128)
    assert has(lambda c: c.get("b_rows") == 128 and disp(c) == "t64.dma", (BF16,))
    # A-direct: plain, gate, K-concat; the 256-row kernel with groups
    assert has(lambda c: disp(c) == "kd" and c.get("loader") == R.LD_GATE, (BF16,))
    assert has(lambda c: disp(c) == "kd" and c.get("epi") == "cat", (BF16,))
    assert has(lambda c: disp(c) == "kd" and c.get("epi", "store") == "store" and c.get("loader", 0) == R.LD_PLAIN, (BF16,))
    for v in ("xl128", "xl256"):
        assert has(lambda c: disp(c) == v and c.get("groups", 1) == 2, (BF16,))
    # f32_split on each resident / k-loop form
    for k in ("single1", "single2", "kloop"):
        assert has(lambda c: c.get("split") and disp(c).endswith(k), (F32,))
    # the DG epilogue on each form it is built for
    for dt, forms in ((BF16, ("single1", "single2", "kloop")), (F32, ("single1", "single2", "kloop"))):
        for k in forms:
            assert has(lambda c: c.get("epi") == "dg" and disp(c).endswith(k), (dt,)), (dt, k)
    # a workgroup that walks two or more M-tiles: each resident form, the k-loop, the DMA ring, the 256-row kernel
    for k in ("t64.single1", "t64.single2", "t64.kloop", "t128.dma", "xl128"):
        assert has(lambda c: disp(c) == k and R.nn_walks_tiles(c), (BF16,)), k


def test_dispatch_restatement_on_the_shapes_the_issue_names():
    d = lambda dt, M, N, K, **kw: R.nn_dispatch(dict(dtype=dt, M=M, N=N, K=K, **kw))
    assert d(BF16, 40, 64, 64) == "t64.single1" and d(BF16, 300, 136, 64) == "t128.single1" and d(F32, 300, 136, 32) == "t128.single1"
    assert d(BF16, 257, 56, 128) == "t64.single2" and d(BF16, 300, 136, 72) == "t128.single2" and d(F32, 300, 136, 40) == "t128.single2"
    assert d(BF16, 300, 136, 200) == "t128.kloop" and d(BF16, 300, 264, 256) == "t128.kloop" and d(F32, 300, 136, 72) == "t128.kloop"
    assert d(BF16, 300, 136, 512) == "t128.dma" and d(BF16, 300, 56, 576) == "t64.dma"
    assert d(BF16, 384, 64, 192, b_rows=128) == "t64.dma" and d(F32, 384, 64, 192, b_rows=128) == "t64.kloop"
    assert d(BF16, 40960, 256, 1792) == "kd" and d(BF16, 147456, 1792, 256) == "xl256"        # the shapes the library routes by itself

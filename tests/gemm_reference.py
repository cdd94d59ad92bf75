"""float64 reference of the point-wise GEMM family (dwn_gemm_nn / dwn_gemm_tn, include/dwn.h; reference call sites
src/models/dwiseneuro.py:91,118,207,276 and their backward), its per-element error bound, and the case lists of the kernel-level
tests (tests/test_gpu_gemm_paths.py on the device, tests/test_gemm_reference_cpu.py for the checker itself).  Plain torch, on
whatever device the operands live on.  Test infrastructure only.

Two kinds of operands per case:
  exact   small integers (A in {-1, 0, 1}, B in {-2 .. 2}, integer loader coefficients, gates in {0.5, 1, 2}): every product, loader
          output and partial sum is an integer (or a multiple of 0.5) below 2^24, so ANY summation order gives the same bits and the
          kernel must equal the reference bit for bit.  The preconditions are asserted here, from the reference alone.
  random  Gaussian operands, B scaled by K^-1/2, fixed seed: every element within elem_bound of the float64 result.
"""
import zlib

import torch

BF16, F32 = torch.bfloat16, torch.float32
U = {BF16: 2.0 ** -8, F32: 2.0 ** -24}           # unit roundoff of the storage types
KC = {BF16: 8, F32: 4}                            # elements per 16-byte vector
BK = {BF16: 64, F32: 32}                          # k-tile of gemm_nn_kernel (dwn_gemm_nn.h: BK = 128 bytes / sizeof(T))
LD_PLAIN, LD_PE, LD_BNACT, LD_AFFINE2, LD_GATE, LD_CAT1 = 0, 1, 2, 3, 5, 6       # DWN_LD_* of include/dwn.h
SPLIT_EXTRA = 3 * 2.0 ** -16                      # f32_split: the dropped lo*lo term and the two split residuals
EXACT_LIMIT = 2.0 ** 24
ROW_CHUNK = 32768                                 # float64 products are formed in row chunks of this many rows


def elem_bound(ref, S, n, u_out, extra=0.0):
    """|got - ref| may reach  u_out*|ref| + (2*n*2^-24 + extra)*S  per element.
    S = sum |a_k||b_k| over the contracted index (float64), n = number of summed terms, u_out = unit roundoff of the store (0 where
    the stored value is itself the operand).  n*2^-24*S is the standard fp32 summation bound for any order; the factor 2 allows for
    the matrix cores' undocumented accumulate rounding."""
    return u_out * ref.abs() + (2.0 * n * 2.0 ** -24 + extra) * S


def flip_allowance(maxab):
    """Computed operands held in bf16 (PE, BNACT, AFFINE2, GATE on random data): the kernel's fp32 prologue and the float64 formula
    may round an operand to different bf16 neighbours.  Two such flips per output element: 2 * 2^-8 * max_k |a_k b_k|."""
    return 2.0 * 2.0 ** -8 * maxab


def _gen(name, device):
    g = torch.Generator(device=device)
    g.manual_seed(zlib.crc32(name.encode()))
    return g


def _ints(shape, lo, hi, g, device, density=1.0):
    v = torch.randint(lo, hi + 1, shape, generator=g, device=device).double()
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g, device=device) < density)
    return v


# ---- operands and their loaders -----------------------------------------------------------------------------------------------------
class Operand:
    """One operand [rows][cols] as the kernel reads it: the stored tensor(s) in `dtype`, the loader kind and its fp32 coefficients.
    f64(): the loader's formula in float64.  mfma(): that rounded to the storage type, "what the matrix cores get".
    f32(): the same formula carried out in float32 and rounded once (the emulation of the room test)."""

    def __init__(self, kind, dtype, p, **kw):
        self.kind, self.dtype, self.p = kind, dtype, p
        self.q = self.v1 = self.v2 = self.v3 = self.gate = self.pe_t = self.pe_h = self.pe_w = None
        self.act, self.rows_per_sample, self.T, self.H, self.W, self.ones = 0, 1, 1, 1, 1, 0
        self.__dict__.update(kw)

    @property
    def rows(self):
        return self.p.shape[0]

    @property
    def cols(self):
        return self.p.shape[1] + ((self.q.shape[1] + self.ones) if self.kind == LD_CAT1 else 0)

    def _formula(self, wt, r0, r1):
        p = self.p[r0:r1].to(wt)
        k = self.kind
        if k == LD_PLAIN:
            return p
        r = torch.arange(r0, r1, device=p.device)
        if k == LD_PE:        # p + pe_t[t] + pe_h[h] + pe_w[w], rows ordered (b, t, h, w)   (dwn_common.h load_op<LD_PE>)
            w, h, t = r % self.W, (r // self.W) % self.H, (r // (self.W * self.H)) % self.T
            return p + ((self.pe_t.to(wt)[t] + self.pe_h.to(wt)[h]) + self.pe_w.to(wt)[w])
        if k == LD_BNACT:     # act(v1 * p + v2) * gate[b]
            h = p * self.v1.to(wt) + self.v2.to(wt)
            if self.act:
                h = h * torch.sigmoid(h)
            return h if self.gate is None else h * self.gate.to(wt)[r // self.rows_per_sample]
        if k == LD_AFFINE2:   # v1 * p + v2 * q + v3
            return self.v1.to(wt) * p + (self.v2.to(wt) * self.q[r0:r1].to(wt) + self.v3.to(wt))
        if k == LD_GATE:      # p * gate[b]
            return p * self.gate.to(wt)[r // self.rows_per_sample]
        if k == LD_CAT1:      # [p | q | 1]
            return torch.cat([p, self.q[r0:r1].to(wt), torch.ones(r1 - r0, self.ones, dtype=wt, device=p.device)], 1)
        raise ValueError(k)

    def f64(self, r0=0, r1=None):
        return self._formula(torch.float64, r0, self.rows if r1 is None else r1)

    def mfma(self, r0=0, r1=None):
        return self.f64(r0, r1).to(self.dtype).double()

    def f32(self, r0=0, r1=None):
        return self._formula(torch.float32, r0, self.rows if r1 is None else r1).to(self.dtype).float()

    def assert_exact(self):
        v = self.f64()
        assert torch.equal(v, v.to(self.dtype).double()), "a loader output is not representable in the storage type"


def make_operand(kind, dtype, rows, cols, mode, g, device, mag=1, scale=1.0, density=1.0, rows_per_sample=1, act=0, gated=False,
                 pe_shape=None, cat=None):
    """mode "exact": integers in [-mag, mag] (thinned to `density`), integer coefficients; "random": scale * randn."""
    ex = mode == "exact"

    def data(c):
        v = _ints((rows, c), -mag, mag, g, device, density) if ex else torch.randn(rows, c, generator=g, device=device) * scale
        return v.to(dtype)

    def coef(c, lo, hi, rnd_scale, rnd_off=0.0, n=None):
        shape = (c,) if n is None else (n, c)
        if ex:
            return _ints(shape, lo, hi, g, device).float()
        return (torch.randn(shape, generator=g, device=device) * rnd_scale + rnd_off).float()

    def gates(c):
        nb = (rows + rows_per_sample - 1) // rows_per_sample
        if ex:
            return torch.tensor([0.5, 1.0, 2.0], device=device)[torch.randint(0, 3, (nb, c), generator=g, device=device)].float()
        return (torch.rand(nb, c, generator=g, device=device) + 0.25).float()

    if kind == LD_CAT1:
        c1, c2 = cat
        return Operand(kind, dtype, data(c1), q=data(c2), ones=cols - c1 - c2)
    o = Operand(kind, dtype, data(cols), rows_per_sample=rows_per_sample)
    if kind == LD_PE:
        o.T, o.H, o.W = pe_shape
        o.pe_t, o.pe_h, o.pe_w = (coef(cols, -1, 1, 0.5, n=s) for s in pe_shape)
    elif kind == LD_BNACT:
        o.act = 0 if ex else act
        o.v1 = coef(cols, 1, 2, 0.25, 1.0)
        o.v2 = coef(cols, -1, 1, 0.5)
        o.gate = gates(cols) if gated else None
    elif kind == LD_AFFINE2:
        o.q = data(cols)
        o.v1, o.v2, o.v3 = coef(cols, 1, 2, 0.5, 1.0), coef(cols, -1, 1, 0.5), coef(cols, -1, 1, 0.3)
    elif kind == LD_GATE:
        o.gate = gates(cols)
    if ex:
        o.assert_exact()
    return o


def _maxab(A, B):
    """max_k |A[m][k]| |B[n][k]|  ->  [M][N], in row chunks (the [M][N][K] tensor is never whole in memory)."""
    A, B = A.abs(), B.abs()
    step = max(1, (1 << 24) // max(1, B.shape[0] * B.shape[1]))
    return torch.cat([(A[i:i + step, None, :] * B[None]).amax(-1) for i in range(0, A.shape[0], step)])


def _split3(A, B):
    """hi*hi + hi*lo + lo*hi of the bf16 splits, in float32 (f32_split: dwn_gemm_nn.h x3_store, "small terms first")."""
    ah, bh = A.to(BF16).float(), B.to(BF16).float()
    al, bl = (A - ah).to(BF16).float(), (B - bh).to(BF16).float()
    return (ah @ bl.t() + al @ bh.t()) + ah @ bh.t()


# ---- NN: C[M][groups * N] = load(A)[M][groups * K] . B[groups * N][K]^T ---------------------------------------------------------------
class NNProblem:
    """Operands of one dwn_gemm_nn call.  a: Operand [M][groups * K1]; a2: plain [M][K - K1] (K-concat) with fp32 bias[N];
    b: [groups * N][K], or [nb][N][K] with per-sample weights (b_rows rows per sample); z3: [M][N] for the DG epilogue (rows rows
    per sample)."""

    def __init__(self, case, mode, device):
        self.case, self.mode, self.device = case, mode, device
        c = case
        self.dtype = dt = c["dtype"]
        self.M, self.N, self.K, self.groups = c["M"], c["N"], c["K"], c.get("groups", 1)
        self.K1 = c.get("K1", 0)
        self.rows = c.get("rows", 0)                 # rows per sample: gate loaders, DG epilogue
        self.b_rows = c.get("b_rows", 0)
        self.split = c.get("split", 0)
        self.epi = c.get("epi", "store")
        g = _gen(c["name"] + mode, device)
        M, N, K, G = self.M, self.N, self.K, self.groups
        Ka = self.K1 if self.K1 else K
        ex = mode == "exact"
        # exact: thin A until a column's sum of squares (M * K * density * E[a^2 b^2] ~ 2 M K density) stays under 2^22
        dens = min(1.0, 2.0 ** 22 / (2.0 * M * K)) if ex else 1.0
        self.a = make_operand(c.get("loader", LD_PLAIN), dt, M, G * Ka, mode, g, device, mag=1, density=dens,
                              rows_per_sample=max(1, self.rows), act=c.get("act", 0), gated=c.get("gated", False),
                              pe_shape=c.get("pe"))
        self.a2 = self.bias = self.z3 = None
        nb = M // self.b_rows if self.b_rows else 0
        bshape = (nb, N, K) if nb else (G * N, K)
        if ex:
            self.b = _ints(bshape, -2, 2, g, device).to(dt)
        else:
            self.b = (torch.randn(bshape, generator=g, device=device) / K ** 0.5).to(dt)
        if self.K1:
            self.a2 = (_ints((M, K - Ka), -1, 1, g, device, dens) if ex else torch.randn(M, K - Ka, generator=g, device=device)).to(dt)
            self.bias = (_ints((N,), -2, 2, g, device) if ex else torch.randn(N, generator=g, device=device)).float()
        if self.epi == "dg":
            self.z3 = (_ints((M, N), -2, 2, g, device) if ex else torch.randn(M, N, generator=g, device=device)).to(dt)

    # terms per element and the store's unit roundoff
    @property
    def n_terms(self):
        return self.K + (1 if self.K1 else 0)

    @property
    def extra(self):
        return SPLIT_EXTRA if self.split else 0.0

    @property
    def computed_bf16(self):
        return self.dtype == BF16 and self.a.kind != LD_PLAIN and self.mode == "random"

    def _a_rows(self, r0, r1, how):
        A = getattr(self.a, how)(r0, r1)
        if self.a2 is not None:
            A = torch.cat([A, self.a2[r0:r1].to(A.dtype)], 1)
        return A

    def _b_for(self, grp, r0):
        if self.b_rows:
            return self.b[r0 // self.b_rows]
        return self.b[grp * self.N:(grp + 1) * self.N]

    def _chunks(self):
        step = self.b_rows if self.b_rows else ROW_CHUNK
        return [(r0, min(self.M, r0 + step)) for r0 in range(0, self.M, step)]

    def reference(self, want_maxab=False, mutate=None):
        """float64 product of the operands the matrix cores get: (ref, S[, maxab]), each [M][groups * N].
        mutate (teeth): "drop_kvec" = the last 16-byte k-vector of every row left out; "group_cols" = group 1 reads group 0's
        columns of A."""
        M, N, K, G = self.M, self.N, self.K, self.groups
        ref = torch.empty(M, G * N, dtype=torch.float64, device=self.device)
        S = torch.empty_like(ref)
        mab = torch.empty_like(ref) if want_maxab else None
        for r0, r1 in self._chunks():
            A = self._a_rows(r0, r1, "mfma")
            for grp in range(G):
                src = 0 if mutate == "group_cols" else grp
                Ag = A[:, src * K:(src + 1) * K]
                if mutate == "drop_kvec":
                    Ag = Ag.clone()
                    Ag[:, K - KC[self.dtype]:] = 0
                Bg = self._b_for(grp, r0).double()
                sl = slice(grp * N, (grp + 1) * N)
                ref[r0:r1, sl] = Ag @ Bg.t()
                S[r0:r1, sl] = Ag.abs() @ Bg.abs().t()
                if want_maxab:
                    mab[r0:r1, sl] = _maxab(Ag, Bg)
        if self.bias is not None:
            ref += self.bias.double()
            S += self.bias.double().abs()
        if self.mode == "exact" and mutate is None:
            self.assert_exact_preconditions(ref, S)
        return (ref, S, mab) if want_maxab else (ref, S)

    def emulate(self, drop_lohi=False):
        """The same formulas in float32, operands rounded to the storage type, the result rounded once: [M][groups * N] in dtype."""
        M, N, K, G = self.M, self.N, self.K, self.groups
        out = torch.empty(M, G * N, dtype=self.dtype, device=self.device)
        for r0, r1 in self._chunks():
            A = self._a_rows(r0, r1, "f32")
            for grp in range(G):
                Ag, Bg = A[:, grp * K:(grp + 1) * K], self._b_for(grp, r0).float()
                if self.split:
                    acc = _split3(Ag, Bg)
                    if drop_lohi:
                        acc = acc - (Ag - Ag.to(BF16).float()).to(BF16).float() @ Bg.to(BF16).float().t()
                else:
                    acc = Ag @ Bg.t()
                if self.bias is not None:
                    acc = acc + self.bias
                out[r0:r1, grp * N:(grp + 1) * N] = acc.to(self.dtype)
        return out

    def assert_exact_preconditions(self, ref, S):
        assert self.mode == "exact"
        assert float(S.max()) < EXACT_LIMIT, "sum |a||b| reaches 2^24"
        c = ref.to(self.dtype).double()
        assert float((c * c).sum(0).max()) < EXACT_LIMIT and float(c.abs().sum(0).max()) < EXACT_LIMIT, "a column's sums reach 2^24"
        if self.z3 is not None:
            assert float((c * self.z3.double()).abs().sum(0).max()) < EXACT_LIMIT, "a column's sum |c z3| reaches 2^24"


def stats_reference(c):
    """BatchNorm sums of the STORED values: (sum c, sum c^2) and their S = (sum |c|, sum c^2), float64 [cols]."""
    cd = c.double()
    return cd.sum(0), (cd * cd).sum(0), cd.abs().sum(0)


def dg_reference(c, z3, rows, shift=0):
    """dg[b][n] = sum_{m in sample b} c_stored[m][n] * z3[m][n] and S = the same of |c z3|, float64 [B][N].
    shift (teeth): the sample boundaries moved by that many rows."""
    M, N = c.shape
    B = M // rows
    t = c.double() * z3.double()
    b = ((torch.arange(M, device=c.device) + shift) // rows).clamp(0, B - 1)
    dg = torch.zeros(B, N, dtype=torch.float64, device=c.device).index_add_(0, b, t)
    S = torch.zeros(B, N, dtype=torch.float64, device=c.device).index_add_(0, b, t.abs())
    return dg, S


# ---- TN: dW[groups * R][Cc] = sum_m load(P)[m][g * R_load + r] * load(Q)[m][g * Cc + c] -------------------------------------------------
class TNProblem:
    def __init__(self, case, mode, device):
        self.case, self.mode, self.device = case, mode, device
        c = case
        self.dtype = dt = c["dtype"]
        self.M, self.R, self.Cc, self.groups = c["M"], c["R"], c["Cc"], c.get("groups", 1)
        self.Rl = c.get("R_load", 0) or self.R
        g = _gen(c["name"] + mode, device)
        M, G = self.M, self.groups
        rows = c.get("rows", 1)
        pk, qk = c.get("p_kind", LD_PLAIN), c.get("q_kind", LD_PLAIN)
        self.p = make_operand(pk, dt, M, G * self.Rl, mode, g, device, mag=1, rows_per_sample=rows, cat=c.get("cat"))
        self.q = make_operand(qk, dt, M, G * self.Cc, mode, g, device, mag=2, scale=M ** -0.5, rows_per_sample=rows, act=1, gated=True,
                              pe_shape=c.get("pe"))
        if self.Rl != self.R:                         # the padding columns of P are zero (include/dwn.h: R_load)
            for grp in range(G):
                self.p.p[:, grp * self.Rl + self.R:(grp + 1) * self.Rl] = 0

    @property
    def computed_bf16(self):
        return self.dtype == BF16 and self.mode == "random" and (self.p.kind not in (LD_PLAIN, LD_CAT1) or self.q.kind != LD_PLAIN)

    def reference(self, want_maxab=False, mutate=None, m_end=None):
        """(ref, S[, maxab]) float64 [groups * R][Cc].  mutate (teeth): "ones_zero" = CAT1's 1 columns read as 0; "group_cols" =
        group 1 reads group 0's columns of P.  m_end: only rows [0, m_end) are summed (a row or a split left out)."""
        R, Cc, G, Rl = self.R, self.Cc, self.groups, self.Rl
        m_end = self.M if m_end is None else m_end
        P, Q = self.p.mfma(0, m_end), self.q.mfma(0, m_end)
        if mutate == "ones_zero":
            P = P.clone()
            P[:, P.shape[1] - self.p.ones:] = 0
        ref = torch.empty(G * R, Cc, dtype=torch.float64, device=self.device)
        S = torch.empty_like(ref)
        mab = torch.empty_like(ref) if want_maxab else None
        for grp in range(G):
            src = 0 if mutate == "group_cols" else grp
            Pg, Qg = P[:, src * Rl:src * Rl + R], Q[:, grp * Cc:(grp + 1) * Cc]
            sl = slice(grp * R, (grp + 1) * R)
            ref[sl] = Pg.t() @ Qg
            S[sl] = Pg.abs().t() @ Qg.abs()
            if want_maxab:
                mab[sl] = _maxab(Pg.t().contiguous(), Qg.t().contiguous())
        if self.mode == "exact" and mutate is None and m_end == self.M:
            self.assert_exact_preconditions(ref, S)
        return (ref, S, mab) if want_maxab else (ref, S)

    def emulate(self):
        R, Cc, G, Rl = self.R, self.Cc, self.groups, self.Rl
        P, Q = self.p.f32(), self.q.f32()
        return torch.cat([P[:, grp * Rl:grp * Rl + R].t() @ Q[:, grp * Cc:(grp + 1) * Cc] for grp in range(G)])

    def assert_exact_preconditions(self, ref, S):
        assert self.mode == "exact" and float(S.max()) < EXACT_LIMIT, "sum |p||q| reaches 2^24"


# ---- which kernel a call runs: a restatement of the host-side choice ---------------------------------------------------------------------
def nn_dispatch(case):
    """The kernel dwn_gemm_nn picks for `case`, restated from the launchers:
      launch_gemm_nn       (dwn_gemm.hip)     A-direct first, then the 256-row kernel, then the 128-row family
      gemm_nn_kd_eligible  (dwn_gemm_kd.hip)  kd_args_ok: bf16, groups 1, no per-sample weights, store / K-concat, plain / gate
                                              loader (rows per sample % 128), K % 128 == 0, N % 128 == 0, K1 % 32 == 0; forced by
                                              DWN_NN_KD, else K >= 512, M >= 8192 and N == 256 (128 with the gate loader)
      gemm_nn_xl_eligible  (dwn_gemm_xl.hip)  bf16, plain loader, store epilogue, no per-sample weights; forced by DWN_NN_XL128 /
                                              XL256, else K >= 256, N >= 512, M >= 8192; launch_gemm_nn_xl: 256 columns when forced
                                              or with >= 256 such tiles
      launch_nn_t          (dwn_gemm_nn.h)    n64 = N <= 64; HasSingle (plain or PE loader with store, plain with DG): K <= BK ->
                                              one resident k-tile; HasSingle2 (plain loader, store / DG): K <= 2 BK and no per-sample
                                              weights -> two; plain bf16: nn_use_dma -> the LDS-DMA ring; else the k-loop
      nn_use_dma           (dwn_gemm_nn.h)    K % 64 == 0, K >= 128, K1 % 64 == 0; per-sample weights, or K >= 512 with at most
                                              5 * 256 tiles
    Returns a name such as "t128.single1", "t64.dma", "xl256", "kd"."""
    dt, M, N, K = case["dtype"], case["M"], case["N"], case["K"]
    G, ld, epi = case.get("groups", 1), case.get("loader", LD_PLAIN), case.get("epi", "store")
    variant, K1, b_rows, rows = case.get("variant", "auto"), case.get("K1", 0), case.get("b_rows", 0), case.get("rows", 0)
    kd_ok = (dt == BF16 and G == 1 and not b_rows and epi in ("store", "cat") and K % 128 == 0 and N % 128 == 0
             and (ld == LD_PLAIN or (ld == LD_GATE and epi == "store" and rows > 0 and rows % 128 == 0 and K <= 4096))
             and (epi == "store" or K1 % 32 == 0))
    if variant not in ("tile128", "xl128", "xl256") and kd_ok:
        if variant == "kd" or (K >= 512 and M >= 8192 and (N == 256 or (N == 128 and ld == LD_GATE))):
            return "kd"
    xl_ok = dt == BF16 and ld == LD_PLAIN and epi == "store" and not b_rows and K % 8 == 0 and N % 8 == 0
    if variant != "tile128" and xl_ok:
        if variant in ("xl128", "xl256"):
            return variant
        if K >= 256 and N >= 512 and M >= 8192:
            return "xl256" if ((M + 255) // 256) * ((N + 255) // 256) * G >= 256 else "xl128"
    bn = 64 if N <= 64 else 128
    bk = BK[dt]
    has_single = (ld == LD_PLAIN and epi in ("store", "dg")) or (ld == LD_PE and epi == "store")
    has_single2 = ld == LD_PLAIN and epi in ("store", "dg")
    if has_single and K <= bk:
        return f"t{bn}.single1"
    if has_single2 and K <= 2 * bk and not b_rows:
        return f"t{bn}.single2"
    if ld == LD_PLAIN and dt == BF16:
        dma = K % 64 == 0 and K >= 128 and not (epi == "cat" and K1 % 64)
        if dma and (b_rows or (((M + 127) // 128) * ((N + bn - 1) // bn) * G <= 5 * 256 and K >= 512)):
            return f"t{bn}.dma"
    return f"t{bn}.kloop"


def nn_walks_tiles(case):
    """True where some workgroup of the persistent grid must walk >= 2 M-tiles: launch_nn_k caps the grid at the resident slots,
    at most 2 workgroups (__launch_bounds__(256, 2)) on each of 256 CUs; launch_gemm_nn_xl launches 256 workgroups."""
    path = nn_dispatch(case)
    if path == "kd":
        return False                     # one workgroup per tile
    if path.startswith("xl"):
        bn = 256 if path == "xl256" else 128
        return ((case["M"] + 255) // 256) * ((case["N"] + bn - 1) // bn) * case.get("groups", 1) > 256
    bn = 64 if case["N"] <= 64 else 128
    ntn = (case["N"] + bn - 1) // bn
    return (case["M"] + 127) // 128 > 512 // (ntn * case.get("groups", 1))


# ---- case lists ------------------------------------------------------------------------------------------------------------------------
_DT = {BF16: "bf16", F32: "f32"}
_LOADERS = (("pe", dict(loader=LD_PE, pe=(3, 5, 5))), ("bn", dict(loader=LD_BNACT, act=0)), ("bnsilu", dict(loader=LD_BNACT, act=1)),
            ("bngate", dict(loader=LD_BNACT, act=0, gated=True, rows=75)), ("bnsilugate", dict(loader=LD_BNACT, act=1, gated=True, rows=75)),
            ("affine2", dict(loader=LD_AFFINE2)), ("gate", dict(loader=LD_GATE, rows=75)))


def _nn(tag, dt, M, N, K, **kw):
    d = dict(dtype=dt, M=M, N=N, K=K, **kw)
    d["name"] = f"{tag}-{_DT[dt]}-{M}x{N * kw.get('groups', 1)}x{K}"
    return d


def _nn_cases():
    c = []
    for dt, shapes in ((BF16, [(40, 64, 64), (129, 24, 8), (300, 136, 64)]), (F32, [(40, 64, 32), (300, 136, 32)])):
        c += [_nn("single1", dt, *s) for s in shapes]
    for dt, shapes in ((BF16, [(257, 56, 128), (300, 136, 72)]), (F32, [(300, 136, 40), (257, 56, 40)])):
        c += [_nn("single2", dt, *s) for s in shapes]
    for dt, shapes in ((BF16, [(300, 136, 200), (300, 264, 256)]), (F32, [(300, 136, 72)])):
        c += [_nn("kloop", dt, *s) for s in shapes]
    for dt in (BF16, F32):
        c += [_nn("kloop-" + tag, dt, 300, 136, 72, **kw) for tag, kw in _LOADERS]
    c += [_nn("dma", BF16, 300, 136, 512), _nn("dma", BF16, 300, 56, 576)]
    c += [_nn("persample", dt, 384, 64, 192, b_rows=128) for dt in (BF16, F32)]
    for v in ("xl128", "xl256"):
        c += [_nn(v, BF16, 300, 264, 72, variant=v), _nn(v, BF16, 257, 24, 8, variant=v), _nn(v + "-groups2", BF16, 200, 48, 32, groups=2, variant=v)]
    c += [_nn("kd", BF16, 128, 128, 128, variant="kd"), _nn("kd", BF16, 1000, 256, 384, variant="kd"),
          _nn("kd-gate", BF16, 256, 128, 128, variant="kd", loader=LD_GATE, rows=128),
          _nn("kd-cat", BF16, 1000, 256, 512, variant="kd", epi="cat", K1=384)]
    for dt in (BF16, F32):
        c += [_nn("cat", dt, 1000, 256, 512, variant="tile128", epi="cat", K1=384),
              _nn("cat", dt, 300, 136, 112, variant="tile128", epi="cat", K1=72),
              _nn("groups2", dt, 200, 48, 32, groups=2)]
    # f32_split: the fp32 cases of the single-k-tile, two-k-tile and k-loop rows
    c += [dict(x, split=1, name=x["name"] + "-split") for x in list(c)
          if x["dtype"] == F32 and x["name"].split("-")[0] in ("single1", "single2", "kloop")]
    # a workgroup walking two or more M-tiles
    c += [_nn("walk", BF16, 128 * 2049 + 5, 64, K) for K in (64, 128, 200)]
    c += [_nn("walk-dma", BF16, 128 * 600 + 5, 128, 512), _nn("walk-xl", BF16, 256 * 300 + 5, 128, 64, variant="xl128")]
    return c


def _dg_cases():
    return [_nn("dg", dt, B * rows, N, K, epi="dg", rows=rows)
            for dt in (BF16, F32) for B, rows, N, K in ((4, 128, 136, 64), (3, 192, 64, 128), (5, 100, 448, 64), (7, 40, 136, 256), (9, 8, 24, 8))]


def _tn(tag, dt, M, R, Cc, **kw):
    d = dict(dtype=dt, M=M, R=R, Cc=Cc, **kw)
    d["name"] = f"{tag}-{_DT[dt]}-{M}x{R}x{Cc}"
    return d


TN_PAIRS = (("affine2-pe", dict(p_kind=LD_AFFINE2, q_kind=LD_PE, pe=(3, 3, 37))), ("plain-bnact", dict(q_kind=LD_BNACT, rows=111)),
            ("plain-gate", dict(q_kind=LD_GATE, rows=111)), ("plain-plain", dict()), ("affine2-plain", dict(p_kind=LD_AFFINE2)),
            ("cat1-plain", dict(p_kind=LD_CAT1, cat=(64, 64))))


def _tn_cases():
    c = []
    for dt in (BF16, F32):
        c += [_tn("plain", dt, *s) for s in ((40, 8, 8), (64, 24, 40), (65, 128, 136), (333, 136, 264), (1100, 64, 448), (4100, 256, 136))]
        c += [_tn("pair-" + tag, dt, 333, 136, 72, **kw) for tag, kw in TN_PAIRS]
        c += [_tn("groups2", dt, 200, 32, 48, groups=2), _tn("groups2-rload", dt, 200, 24, 48, groups=2, R_load=32),
              _tn("overwrite-1split", dt, 300, 64, 72, overwrite=1), _tn("overwrite-zeroed", dt, 1100, 64, 72, overwrite=1),
              _tn("f64", dt, 1100, 64, 64, dw_f64=1),
              _tn("split-1", dt, 1100, 64, 72, nsplit=1, rows_per_split=1100), _tn("split-3", dt, 1100, 64, 72, nsplit=3, rows_per_split=384)]
    return c


NN_CASES = _nn_cases()
DG_CASES = _dg_cases()
TN_CASES = _tn_cases()
MODES = ("exact", "random")


def case_id(case):
    return case["name"]

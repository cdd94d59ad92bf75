// C-ABI layer of libdwiseneuro_hip.so (declarations and contracts: include/dwn.h).
// Composites chain the fused kernels of one reference module; they enqueue on the caller's stream only,
// never allocate, never synchronise (hipGraph-capturable), and carve all scratch from the caller's workspace.
#include "dwn_internal.h"
#include "dwn_kernels.h"
#include <string.h>
#include <math.h>

static thread_local char g_err[512] = "";
#ifndef DWN_EVAL_CHAIN
#define DWN_EVAL_CHAIN 1      // eval forward: the chained stencil's rebuilt-input form where it is built (0: dwn_dwrc.hip everywhere; A/B builds)
#endif

bool dw_spatial_bwd_rc_supported(const DwSpatialBwd& a, int dtype);          // dwn_dwbwd.hip
bool dw_spatial_fwd_rc_walk_supported(const DwSpatialFwd& a, int dtype);     // dwn_dwfwd.hip

int dwn_set_error(int code, const char* msg) {
    snprintf(g_err, sizeof(g_err), "dwn error %d: %s", code, msg ? msg : "");
    return code;
}

#define TRY(x) do { int rc__ = (x); if (rc__ != 0) return rc__; } while (0)

// ---- opt-in kernel-family timer (HIP events on the launch stream).  Off by default: zero cost and no state.
// bench.py turns it on for the kernel family it reports a roofline for (dwn_profile_enable / _collect).
#include <vector>
#include <dlfcn.h>
namespace {
struct ProfFam { std::vector<hipEvent_t> beg, end; size_t used = 0; };
static unsigned long long g_prof_mask = 0;
static ProfFam g_prof[DWN_FAM_COUNT];
constexpr size_t PROF_POOL = 8192;
// roctx ranges per kernel family: resolved at run time so that the library has no link-time dependency
static const char* const FAM_NAMES[DWN_FAM_COUNT] = {
    "dwn:pw_fwd", "dwn:dws_fwd", "dwn:dwt_fwd", "dwn:se_pool", "dwn:pwl_fwd", "dwn:resid_fwd", "dwn:resid_bwd", "dwn:pwl_dgrad",
    "dwn:pwl_wgrad", "dwn:bn3_reduce", "dwn:dwt_bwd", "dwn:dws_bwd", "dwn:pw_dgrad", "dwn:pw_wgrad", "dwn:cortex_fwd",
    "dwn:cortex_bwd", "dwn:readout_fwd", "dwn:readout_bwd"};
typedef int (*roctx_push_t)(const char*);
typedef int (*roctx_pop_t)(void);
static roctx_push_t g_roctx_push = nullptr;
static roctx_pop_t g_roctx_pop = nullptr;
static bool roctx_resolve() {
    static int state = 0;                         // 0 untried, 1 ok, -1 absent
    if (state == 0) {
        state = -1;
        for (const char* lib : {"librocprofiler-sdk-roctx.so", "libroctx64.so"}) {
            void* h = dlopen(lib, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            g_roctx_push = (roctx_push_t)dlsym(h, "roctxRangePushA");
            g_roctx_pop = (roctx_pop_t)dlsym(h, "roctxRangePop");
            if (g_roctx_push && g_roctx_pop) { state = 1; break; }
        }
    }
    return state == 1;
}
struct ProfScope {
    int fam; hipStream_t s; bool on; bool range;
    ProfScope(int f, hipStream_t st) : fam(f), s(st), on(false), range(false) {
        if (g_prof_mask == 0) return;
        if ((g_prof_mask & DWN_PROF_ROCTX) && g_roctx_push) { g_roctx_push(FAM_NAMES[f]); range = true; }
        if (!((g_prof_mask >> f) & 1ull)) return;
        ProfFam& p = g_prof[f];
        if (p.used >= p.beg.size()) return;
        on = true;
        (void)hipEventRecord(p.beg[p.used], s);
    }
    ~ProfScope() {
        if (on) {
            ProfFam& p = g_prof[fam];
            (void)hipEventRecord(p.end[p.used], s);
            p.used++;
        }
        if (range) g_roctx_pop();
    }
};
}  // namespace
#define PROF(fam, call) do { ProfScope ps__((fam), s); TRY(call); } while (0)
#define HIP_TRY(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return dwn_set_error((int)e__, hipGetErrorString(e__)); } while (0)
#define ENTER(device) do { g_err[0] = 0; HIP_TRY(hipSetDevice(device)); } while (0)

// ---- every entry opens in one order (DESIGN.md "The entry contract"): ARGS and the null scalar arguments (-1), the mode refusals
// (-7), the family's *_geometry (-2 / -4), the required pointers (-1), the workspace, ENTER.  No argument check needs a device,
// nothing in front of ENTER calls the runtime, and a refused call has launched and written nothing.
// the prologue: clear the error, reject a null argument struct
#define ARGS(a, who) do { g_err[0] = 0; if (!(a)) return dwn_set_error(-1, who ": null arguments"); } while (0)
// ... of an entry that takes its arguments one by one: clear the error, reject the null ones among the pointers it cannot do without
#define NEEDS(ok, who_and_names) do { g_err[0] = 0; if (!(ok)) return dwn_set_error(-1, who_and_names); } while (0)
// the workspace a->ws / a->ws_bytes against `need` bytes (what `getter` answers) and an alignment.  The code is -3 everywhere but
// in the two *_backward entries of the gains (-2), and the alignment is the entry's own: both are part of the interface.  (The model's
// composites keep their older answer: -6 "workspace too small".)
#define WS_CHECK(a, code, who, need, getter, align) do { \
    if ((a)->ws_bytes < (need) || ((size_t)(a)->ws & ((align) - 1))) \
        return dwn_set_error(code, who ": workspace smaller than " getter " or not " #align "-byte aligned"); } while (0)
// a *_ws_bytes entry: 0 and no error left behind when the arguments are null or their geometry is bad
#define WS_BYTES_OR_0(a, geometry, bytes) do { if (!(a) || geometry(a) != 0) { g_err[0] = 0; return 0; } return (bytes); } while (0)
// the largest value of a product that the code below holds in an `int`
constexpr long long INT_LIMIT = 0x7fffffffLL;

namespace {

struct Carver {
    char* base; size_t off; size_t cap;
    explicit Carver(void* b, size_t c) : base((char*)b), off(0), cap(c) {}
    template <class U> U* take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        U* p = base ? (U*)(base + off) : (U*)nullptr;
        off += n * sizeof(U);
        return p;
    }
    bool ok() const { return base == nullptr || off <= cap; }
};

inline size_t tsize(int dtype) { return dtype == DWN_BF16 ? 2 : 4; }
inline size_t nstat(int C) { return (size_t)DWN_NREP * 2 * C; }

LoadDesc ld_plain(const void* p, i64 ld) {
    LoadDesc d; memset(&d, 0, sizeof(d));
    d.p = p; d.ld = ld;
    return d;
}
LoadDesc ld_bnact(const void* p, i64 ld, const float* coef, int C, int act, const float* gate, int gate_ld,
                  int rows_per_sample) {
    LoadDesc d = ld_plain(p, ld);
    d.v1 = coef; d.v2 = coef + C; d.act = act; d.gate = gate; d.gate_ld = gate_ld;
    d.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
    return d;
}
LoadDesc ld_affine2(const void* p, const void* q, i64 ld, const float* abc, int C) {
    LoadDesc d = ld_plain(p, ld);
    d.q = q; d.v1 = abc; d.v2 = abc + C; d.v3 = abc + 2 * C;
    return d;
}
LoadDesc ld_pe(const void* p, i64 ld, const float* pe_t, const float* pe_h, const float* pe_w, int T, int H, int W) {
    LoadDesc d = ld_plain(p, ld);
    d.pe_t = pe_t; d.pe_h = pe_h; d.pe_w = pe_w; d.pT = T; d.pH = H; d.pW = W; d.pe_ld = (int)ld;
    return d;
}
// p = raw y; v1..v4 = scale, shift, mean, invstd (used by the dw backward kernels)
LoadDesc ld_ycoef(const void* y, i64 ld, const float* coef, int C) {
    LoadDesc d = ld_plain(y, ld);
    d.v1 = coef; d.v2 = coef + C; d.v3 = coef + 2 * C; d.v4 = coef + 3 * C;
    return d;
}

BnFinJob fin_job(const double* stats, int stat_c, double count, const dwn_bn& bn, int C) {
    BnFinJob j; memset(&j, 0, sizeof(j));
    j.stats = stats; j.stat_c = stat_c; j.count = count; j.gamma = bn.gamma; j.beta = bn.beta;
    j.running_mean = bn.running_mean; j.running_var = bn.running_var; j.nbt = bn.num_batches_tracked; j.coef = bn.coef; j.C = C;
    return j;
}
BnBwdJob bwd_job(const double* stats, double count, const dwn_bn& bn, float* abc, int C, bool frozen) {
    BnBwdJob j; memset(&j, 0, sizeof(j));
    j.stats = stats; j.count = count; j.coef = bn.coef; j.dgamma = bn.dgamma; j.dbeta = bn.dbeta; j.abc = abc; j.C = C;
    j.frozen = frozen ? 1 : 0;
    return j;
}

int bn_finalize(const double* stats, int stat_c, double count, const dwn_bn& bn, int C, int training, float momentum,
                float eps, hipStream_t s) {
    if (training) return k_bn_finalize_train(fin_job(stats, stat_c, count, bn, C), BnFinJob{}, momentum, eps, s);
    return k_bn_finalize_eval(bn.gamma, bn.beta, bn.running_mean, bn.running_var, eps, bn.coef, C, s);
}

GemmNN nn_base(const LoadDesc& a, int a_kind, const void* b, i64 ldb, void* c, i64 ldc, int M, int N, int K, int groups) {
    GemmNN g; memset(&g, 0, sizeof(g));
    g.a = a; g.a_kind = a_kind; g.b = b; g.ldb = ldb; g.c = c; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.groups = groups; g.epi = EPI_STORE;
    return g;
}
GemmTN tn_base(const LoadDesc& p, int pk, const LoadDesc& q, int qk, int M, int R, int Cc, float* dw, i64 lddw, int groups) {
    GemmTN g; memset(&g, 0, sizeof(g));
    g.p = p; g.p_kind = pk; g.q = q; g.q_kind = qk; g.M = M; g.R = R; g.Cc = Cc; g.dw = dw; g.lddw = lddw;
    g.groups = groups; g.nsplit = 0;
    return g;
}

// ---------------------------------------------------------------- block workspace layout
struct BlockWs {
    void *wpw, *wpwl;            // forward: W1 [Cmid][Cin], W2 [Cout][Cmid] in T; backward: W1^T [Cin][Cmid], W2^T [Cmid][Cout]
    float *wdws, *wdwt;          // tap-major depth-wise weights
    double *st1, *st2, *st3, *st4, *stsc;
    long long* pooled;           // forward: SE pooled sums (64-bit fixed point, pool_fix); backward: the same slot holds dg (float)
    float *abc1, *abc2, *abc3, *abc4, *abcsc, *ident3;
    float *dgp, *dhp, *dps;
    void* bp; float* r3; float* gacc;                      // conv_pw data-gradient folding (see dwn_elementwise.hip)
    float* tacc;                                           // conv_pw weight gradient: raw products T1 / Ga / s (k_pw_wgrad_fold)
    void* wgated;                                          // [B][Cout][Cmid] W2 . diag(gate_b) (forward only)
    void* rcblob;                                          // forward: slice images of the y1-recomputing stencil
    double* gram;                                          // y1-free training forward: gram_nrep() x [(Cin + 8)][Cin] raw products a0^T a0, 1^T a0 (fp64 atomics)
    float* pb;                                             // [B][Cout][Cmid] per-sample dy4^T z3 (backward, BlockPlan::pwl_per_sample)
    char* zero_beg; char* zero_end;
    size_t bytes;
};
// ---------------------------------------------------------------- block plan
// Everything the block entries decide from the arguments alone, decided once: carve_block, dwn_block_forward, dwn_block_backward
// and dwn_block_forward_writes read a BlockPlan and ask no route predicate themselves.
enum PwRoute {                   // how conv_pw and the spatial stencil run (precedence: plan_block)
    PW_MATERIALISED,             // gemm_nn writes y1, then the stencil on y1
    PW_Y1_FREE,                  // training / frozen: the chained row-walk stencil rebuilds y1 from a0; a Gram pass only with batch statistics
    PW_EVAL_CHAIN,               // eval: the same stencil, BatchNorm-1 known
    PW_EVAL_RC,                  // eval: the tile-resident y1-recomputing stencil (dwn_dwrc.hip)
};
struct BlockPlan {
    i64 Min, Mout; int S_out;    // rows of the block's input / output; output rows per sample
    // tr: the training kernels and their saved intermediates (DWN_BN_TRAIN and DWN_BN_FROZEN); bs: batch statistics (DWN_BN_TRAIN).
    // Frozen: every BatchNorm's coefficients are known before the first launch (prep, as eval), so the Gram pass, the shortcut's
    // statistics pass and all finalisers go; the statistics epilogues of the GEMMs / stencils stay (same kernels, same arguments
    // as training: their sums land in the zeroed arena and nobody reads them).  Backward: BatchNorm triples (scale, 0, 0)
    bool tr, bs, frozen;
    bool identity_sc;            // the shortcut's nearest map is the identity
    PwRoute pw;
    bool rc_blob;                // the forward workspace holds dwn_dwrc.hip's slice images (eval, wherever that stencil is built)
    bool pwl_gated;              // conv_pwl forward on per-sample gated weights
    bool pwl_per_sample;         // conv_pwl backward through per-sample products (pwl_bwd_per_sample)
    bool dx_folded, sc_gathered; // backward: the shortcut's gradient folded into conv_pw's data gradient; ... through its nearest map
    bool eval_z3;                // eval: z3 and the SE pooling sums come straight from the temporal pass, y3 is never stored
    int writes;                  // dwn_block_forward_writes: bit 0 = y1, bit 1 = y3
};
#ifndef PWL_GATED_MIN_ROWS
#define PWL_GATED_MIN_ROWS 8192
#endif
// conv_pwl backward through per-sample products (k_pwl_bwd_reduce) + the recompute-du GEMM epilogue (EPI_DH3): saves
// three passes over a [Mout][Cmid] tensor at the price of zeroing / accumulating / reading B [Cout][Cmid] fp32 matrices,
// so it is used when those are small next to one such pass.  dwn_block_args.pwl_bwd = 1 | 2 forces a path (the parity
// tests run both).
static bool pwl_bwd_per_sample(const dwn_block_args& a) {
#ifdef DWN_DETERMINISTIC
    return true;                 // the other path's GEMM epilogue adds to dg from several waves of a workgroup, inside its tile loop
#endif
    if (a.pwl_bwd == 2) return false;
    if (a.pwl_bwd == 1) return true;
    const double pb = 4.0 * a.B * a.Cout * a.Cmid * sizeof(float);
    const double pass = (double)a.B * a.T * a.Hout * a.Wout * a.Cmid * tsize(a.dtype);
    return pb <= pass;
}
// The geometry of the block's spatial stencil (D: DwSpatialFwd / DwSpatialBwd) and, rebuilt: the rebuilt-input form's a0_ld / Cin.
// The support probes of plan_block and the launches start from the same descriptor; a launch adds its loaders (every row length
// is Cmid), pointers and statistics.
template <class D> static D dws_desc(const dwn_block_args& a, bool rebuilt) {
    D d; memset(&d, 0, sizeof(d));
    d.planes = a.B * a.T; d.Hin = a.Hin; d.Win = a.Win; d.Hout = a.Hout; d.Wout = a.Wout; d.C = a.Cmid; d.stride = a.stride; d.ks = a.ks;
    if (rebuilt) { d.a0_ld = a.Cin; d.Cin = a.Cin; }
    return d;
}
// Pure: no device call, no state; the same arguments give the same plan in every entry and on a host without a device.
static BlockPlan plan_block(const dwn_block_args& a) {
    BlockPlan p; memset(&p, 0, sizeof(p));
    p.Min = (i64)a.B * a.T * a.Hin * a.Win; p.Mout = (i64)a.B * a.T * a.Hout * a.Wout; p.S_out = a.T * a.Hout * a.Wout;
    p.tr = a.training != DWN_BN_EVAL; p.bs = a.training == DWN_BN_TRAIN; p.frozen = a.training == DWN_BN_FROZEN;
    p.identity_sc = a.stride == 1 && a.Hin == a.Hout && a.Win == a.Wout;
    // the one probe of each direction: is the row-walk stencil's rebuilt-input form built for this geometry?
    DwSpatialFwd f = dws_desc<DwSpatialFwd>(a, true); f.in.ld = a.Cmid;
    DwSpatialBwd b = dws_desc<DwSpatialBwd>(a, true); b.dy.ld = b.y1.ld = a.Cmid;
    const bool walk = a.dtype == DWN_BF16 && dw_spatial_fwd_rc_walk_supported(f, a.dtype);
    // Training WITHOUT a materialised y1 (round 5; dwn_block_args.y1_mode).  y1 = a0 . W1^T is the widest tensor of a block and a
    // Cin-deep product of one seven times narrower: the forward stencil rebuilds its rows on the matrix cores (dwn_dwfwd.hip, CIN > 0) with
    // BatchNorm-1's batch statistics taken from the Gram matrix of a0 (k_bn1_gram_finalize), the backward stencil rebuilds the rows it
    // needs the same way (dwn_dwbwd.hip, CIN > 0), and conv_pw's backward has not read y1 since round 4 — so y1 is neither written nor
    // read: three E-wide passes over M_in rows less per block.
    // y1_mode 0: where it is also the faster path — 64 input channels (blocks 0-3: -0.4 ms per step); with 128 (blocks 4-6: four k-steps
    // per MFMA tile, 256 B of a0 per pixel against 128 B of a y1 slice) the rebuilding stencils lose more than conv_pw costs
    // (stand-alone 508 vs 295 us forward, 614 vs 549 us backward on block 4's shape); y1_mode 2 takes every block that is built
    const bool y1_free = p.tr && walk && a.y1_mode != 1 && dw_spatial_bwd_rc_supported(b, a.dtype) && (a.y1_mode == 2 || a.Cin == 64);
    // eval-mode forward without conv_pw as its own pass (BatchNorm-1 is known): the tile-resident stencil of dwn_dwrc.hip
    p.rc_blob = !p.tr && dwn_dw_spatial_rc_supported(a.dtype, a.Cin, a.Cmid, a.ks, a.stride, a.Hin, a.Win) != 0;
    // eval, 64 or 128 input channels, row-walk plane widths: the chained stencil's rebuilt-input form is also the faster way to skip
    // conv_pw (623 vs 768 us on block 0's shape, 276 vs 308 us on blocks 1-3'; faster than the tile-resident kernel at 128 channels
    // too: profiles/r5_predict_bf16_kernel_stats.csv); the tile-resident kernel keeps the other geometries — and its slice of the
    // workspace (rc_blob) also where the chain wins and nothing reads it: a known leftover of the layout
    p.pw = DWN_EVAL_CHAIN && !p.tr && walk ? PW_EVAL_CHAIN : y1_free ? PW_Y1_FREE : p.rc_blob ? PW_EVAL_RC : PW_MATERIALISED;
    // conv_pwl forward with the SE gate folded into per-sample weights (plain A loader): needs whole tiles per sample and
    // the k-loop GEMM variant
    // ... and enough rows per sample to pay for writing B weight copies: with 18432 rows (blocks 0-3) the copies are 1.8 MB and the
    // plain-loader GEMM on its LDS-DMA ring wins; at 4608 / 1280 rows (blocks 4-8) the copies are 7-29 MB per block — written, then
    // re-read at 1.35-1.53x the activations' bytes — and the gate in the A loader is faster for the step although the GEMM itself is
    // slower (round 5, same box: pwl_fwd 1.085 -> 1.289 ms, step 24.27 -> 24.12 ms)
    // (bf16 only: fp32 keeps the per-sample weights everywhere — its eval-mode split products were validated in that form)
    p.pwl_gated = (p.S_out % 128) == 0 && a.Cmid > (a.dtype == DWN_BF16 ? 64 : 32) && (a.dtype != DWN_BF16 || p.S_out >= PWL_GATED_MIN_ROWS);
    p.pwl_per_sample = pwl_bwd_per_sample(a);
    // backward, conv_pw's data gradient IS dx: output channels = input channels tiled once or twice, the one-pass kernel (asked
    // first: it leaves no Cin to divide by but the one it is built for), and the shortcut's map the identity or, on a strided block,
    // gathered through hinv / winv
    p.dx_folded = pw_bwd_fused_supported(a.dtype, p.Min, a.Cmid, a.Cin) && a.Cout % a.Cin == 0 && a.Cout / a.Cin <= 2 &&
                  (p.identity_sc || (a.hinv && a.winv && a.Hin + a.Win <= 512));
    p.sc_gathered = p.dx_folded && !p.identity_sc;
    p.eval_z3 = !p.tr;
    // training writes y3 and, unless the stencils rebuild it, y1; eval never writes y3 and writes y1 on the materialised route only
    p.writes = p.tr ? (p.pw == PW_Y1_FREE ? 2 : 3) : (p.pw == PW_MATERIALISED ? 1 : 0);
    return p;
}
// floats of the conv_pw data-gradient folding scratch: G accumulator [Cin][Cin] and r3 [Cin]
static size_t pw_fold_floats(int Cin) { return (size_t)Cin * Cin + Cin; }
BlockWs carve_block(const dwn_block_args& a, const BlockPlan& p, int backward, void* base, size_t cap) {
    BlockWs w; memset(&w, 0, sizeof(w));
    Carver c(base, cap);
    const size_t ts = tsize(a.dtype);
    w.wpw = c.take<char>((size_t)a.Cmid * a.Cin * ts);
    w.wpwl = c.take<char>((size_t)a.Cout * a.Cmid * ts);
    w.wdws = c.take<float>((size_t)a.ks * a.ks * a.Cmid);
    w.wdwt = c.take<float>((size_t)a.kt * a.Cmid);
    if (!backward && p.pwl_gated) w.wgated = c.take<char>((size_t)a.B * a.Cout * a.Cmid * ts);
    if (!backward && p.rc_blob) w.rcblob = c.take<char>(dwn_dw_spatial_rc_blob_bytes(a.Cmid, a.Cin));      // eval only
    c.take<char>(0);
    size_t z0 = (c.off + 255) & ~(size_t)255;
    w.st1 = c.take<double>(nstat(a.Cmid));
    w.st2 = c.take<double>(nstat(a.Cmid));
    w.st3 = c.take<double>(nstat(a.Cmid));
    w.st4 = c.take<double>(nstat(a.Cout));
    w.stsc = c.take<double>(nstat(backward ? a.Cout : a.Cin));
    w.pooled = c.take<long long>((size_t)a.B * a.Cmid);
    if (!backward && p.pw == PW_Y1_FREE) w.gram = c.take<double>((size_t)gram_nrep(a.dtype, a.Cin) * (a.Cin + 8) * a.Cin);
    size_t z1 = c.off;
    if (backward) {
        w.abc1 = c.take<float>(3 * (size_t)a.Cmid);
        w.abc2 = c.take<float>(3 * (size_t)a.Cmid);
        w.abc3 = c.take<float>(3 * (size_t)a.Cmid);
        w.abc4 = c.take<float>(3 * (size_t)a.Cout);
        w.abcsc = c.take<float>(3 * (size_t)a.Cout);
        w.ident3 = c.take<float>(3 * (size_t)a.Cmid);
        w.dgp = c.take<float>((size_t)a.B * a.Cmid);
        w.dhp = c.take<float>((size_t)a.B * a.se_r);
        w.dps = c.take<float>((size_t)a.B * a.Cmid);
        w.bp = c.take<char>((size_t)a.Cin * (a.Cmid + a.Cin) * ts);
        w.gacc = c.take<float>(pw_fold_floats(a.Cin));                  // one zeroed range: G accumulator, r3
        w.r3 = w.gacc + (size_t)a.Cin * a.Cin;
        w.tacc = c.take<float>(pw_wgrad_tacc_floats(a.Cmid, a.Cin));
        if (p.pwl_per_sample) w.pb = c.take<float>((size_t)a.B * a.Cout * a.Cmid);
    }
    w.bytes = c.off + 256;
    if (base) { w.zero_beg = (char*)base + z0; w.zero_end = (char*)base + z1; }
    return w;
}

// dwn.h DWN_F32_*: does this fp32 GEMM run as three bf16 products?
static inline int f32_split_of(int policy, bool eval_forward) {
    return policy == DWN_F32_SPLIT3 ? 1 : policy == DWN_F32_NATIVE ? 0 : (eval_forward ? 1 : 0);
}

ResGeom geom_of(const dwn_block_args& a) {
    ResGeom gm;
    gm.BT = a.B * a.T; gm.T = a.T; gm.Hin = a.Hin; gm.Win = a.Win; gm.Hout = a.Hout; gm.Wout = a.Wout;
    gm.Cin = a.Cin; gm.Cout = a.Cout; gm.hsrc = a.hsrc; gm.wsrc = a.wsrc; gm.hinv = a.hinv; gm.winv = a.winv;
    return gm;
}

// does the product of these positive factors stay an int?  (no overflow on the way: the running product is cut at INT_LIMIT)
inline bool fits_int(std::initializer_list<long long> f) {
    long long p = 1;
    for (long long v : f) { if (v > INT_LIMIT) return false; p *= v; if (p > INT_LIMIT) return false; }
    return true;
}
inline bool dtype_ok(int dtype) { return dtype == DWN_F32 || dtype == DWN_BF16; }
inline bool bn_mode_ok(int training) { return training == DWN_BN_EVAL || training == DWN_BN_TRAIN || training == DWN_BN_FROZEN; }

// the block's geometry: the two size entries, the two route entries, forward and backward
int check_block(const dwn_block_args* ap) {
    const dwn_block_args& a = *ap;
    if (a.B <= 0 || a.T <= 0 || a.Hin <= 0 || a.Win <= 0 || a.Hout <= 0 || a.Wout <= 0 || a.Cin <= 0 || a.Cmid <= 0 || a.Cout <= 0 ||
        a.stride <= 0 || a.se_r <= 0)
        return dwn_set_error(-2, "block: B, T, Hin, Win, Hout, Wout, Cin, Cmid, Cout, stride, se_r must be positive");
    if (a.Cin % 8 || a.Cmid % 8 || a.Cout % 8) return dwn_set_error(-2, "block: channel counts must be multiples of 8");
    if (a.ks != 3 && a.ks != 5 && a.ks != 7) return dwn_set_error(-4, "block: spatial_kernel must be 3, 5 or 7 (the built set)");
    if (a.kt != 3 && a.kt != 5 && a.kt != 7 && a.kt != 9) return dwn_set_error(-4, "block: temporal_kernel must be 3, 5, 7 or 9 (the built set)");
    if (a.Hout != (a.Hin - 1) / a.stride + 1 || a.Wout != (a.Win - 1) / a.stride + 1)
        return dwn_set_error(-2, "block: Hout/Wout inconsistent with stride");
    if (!dtype_ok(a.dtype)) return dwn_set_error(-2, "block: dtype must be DWN_F32 or DWN_BF16");
    if (!bn_mode_ok(a.training)) return dwn_set_error(-2, "block: training must be DWN_BN_EVAL, DWN_BN_TRAIN or DWN_BN_FROZEN");
    // the rows of the block's input are an int wherever a GEMM takes them — (int)Min, (int)Mout as GemmNN::M / GemmTN::M — and bound
    // the other int products of the entries: planes and gm.BT (B * T), BlockPlan::S_out and rows_per_sample (T * Hout * Wout),
    // DwTemporalFwd::HW (Hout * Wout); Hout <= Hin and Wout <= Win by the line above
    if (!fits_int({a.B, a.T, a.Hin, a.Win})) return dwn_set_error(-2, "block: B * T * Hin * Win must stay below 2^31");
    return 0;
}

// the stem's geometry, from the fields its two argument structs share: the size entry, forward, backward and the two input-gradient
// entries (`who` keeps each entry's own message prefix)
int stem_geometry(const char* who, int dtype, int training, int B, int Cin, int C0, i64 S) {
    char msg[128];
    const char* bad = nullptr;
    if (C0 <= 0 || C0 % 8 || Cin <= 0 || B <= 0 || S <= 0) bad = "C0 must be a positive multiple of 8; B, Cin, S positive";
    else if (!dtype_ok(dtype)) bad = "dtype";
    else if (!bn_mode_ok(training)) bad = "training must be DWN_BN_EVAL, DWN_BN_TRAIN or DWN_BN_FROZEN";
    // the launchers (k_stem_out, k_stem_bwd_acc) refuse 2^31 rows and more: B * S, `M` in the entries
    else if (!fits_int({B, S})) bad = "B * S must stay below 2^31";
    if (!bad) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, bad);
    return dwn_set_error(-2, msg);
}
int stem_geometry(const dwn_stem_args* a) {
    TRY(stem_geometry("stem", a->dtype, a->training, a->B, a->Cin, a->C0, a->S));
    if (a->pe_t && (i64)a->T * a->H * a->W != a->S) return dwn_set_error(-2, "stem: T*H*W != S");
    return 0;
}
size_t stem_ws_bytes(const dwn_stem_args* a) {
    return ((size_t)DWN_NREP * stem_moment_count() * sizeof(double) + 256 +
            (size_t)DWN_NREP * a->C0 * stem_acc_stride() * sizeof(double) + 1024);
}

}  // namespace

extern "C" {

int dwn_abi_version(void) { return DWN_ABI_VERSION; }
int dwn_sizeof(const char* name) {
#define SZ(T) if (strcmp(name, #T) == 0) return (int)sizeof(T)
    SZ(dwn_load_desc); SZ(dwn_gemm_nn_args); SZ(dwn_gemm_tn_args); SZ(dwn_dw_spatial_fwd_args);
    SZ(dwn_dw_spatial_bwd_args); SZ(dwn_dw_temporal_fwd_args); SZ(dwn_dw_temporal_bwd_args); SZ(dwn_bn);
    SZ(dwn_stem_args); SZ(dwn_block_args); SZ(dwn_pool_args); SZ(dwn_cortex_args); SZ(dwn_readout_args);
    SZ(dwn_tensor_entry); SZ(dwn_clip_src); SZ(dwn_clip_desc); SZ(dwn_pw_bwd_args); SZ(dwn_dw_spatial_rc_fwd_args);
    SZ(dwn_stem_input_grad_args); SZ(dwn_guarded_entry); SZ(dwn_step_guard); SZ(dwn_gaze_args);
    SZ(dwn_corr_args); SZ(dwn_gabor_args); SZ(dwn_modulator_args); SZ(dwn_spatial_gain_args);
    SZ(dwn_blur3d_args); SZ(dwn_clip_moments_args); SZ(dwn_mei_update_args);
    SZ(dwn_trial_desc); SZ(dwn_trial_group); SZ(dwn_trial_score_args);
    SZ(dwn_noise_args); SZ(dwn_sta_args); SZ(dwn_gauss2d_args); SZ(dwn_gauss2d_profile_args);
    SZ(dwn_pair_seg); SZ(dwn_pair_args); SZ(dwn_pair_compare_args); SZ(dwn_modes_args);
#undef SZ
    return -1;
}
const char* dwn_last_error(void) { return g_err; }

int dwn_profile_enable(unsigned long long family_mask, int device) {
    ENTER(device);
    for (int f = 0; f < DWN_FAM_COUNT; ++f) {
        ProfFam& p = g_prof[f];
        p.used = 0;
        if (((family_mask >> f) & 1ull) && p.beg.empty()) {
            p.beg.resize(PROF_POOL); p.end.resize(PROF_POOL);
            for (size_t i = 0; i < PROF_POOL; ++i) { HIP_TRY(hipEventCreate(&p.beg[i])); HIP_TRY(hipEventCreate(&p.end[i])); }
        }
    }
    if (family_mask & DWN_PROF_ROCTX) (void)roctx_resolve();      // absent library: ranges are skipped, events still work
    g_prof_mask = family_mask;
    return 0;
}
int dwn_profile_collect(int family, double* total_ms, long long* launches) {
    if (family < 0 || family >= DWN_FAM_COUNT) return dwn_set_error(-2, "profile_collect: bad family");
    ProfFam& p = g_prof[family];
    double tot = 0;
    for (size_t i = 0; i < p.used; ++i) {
        HIP_TRY(hipEventSynchronize(p.end[i]));
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, p.beg[i], p.end[i]));
        tot += ms;
    }
    *total_ms = tot; *launches = (long long)p.used;
    p.used = 0;
    return 0;
}

// ---- the kernel families' thin entries: the null refusals and the entry's own checks here, every other refusal is the launcher's
int dwn_gemm_nn(const dwn_gemm_nn_args* a, int dtype, int device, void* stream) {
    ARGS(a, "gemm_nn");
    ENTER(device);
    return launch_gemm_nn(*a, dtype, (hipStream_t)stream);
}
int dwn_gemm_tn(const dwn_gemm_tn_args* a, int dtype, int device, void* stream) {
    ARGS(a, "gemm_tn");
    ENTER(device);
    return launch_gemm_tn(*a, dtype, (hipStream_t)stream);
}
int dwn_dw_spatial_fwd(const dwn_dw_spatial_fwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "dw_spatial_fwd");
    ENTER(device);
    return launch_dw_spatial_fwd(*a, dtype, (hipStream_t)stream);
}
int dwn_dw_spatial_bwd(const dwn_dw_spatial_bwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "dw_spatial_bwd");
    ENTER(device);
    return launch_dw_spatial_bwd(*a, dtype, (hipStream_t)stream);
}
// (the probes answer 0 / 1: null arguments are not supported)
int dwn_dw_spatial_bwd_rc_supported(const dwn_dw_spatial_bwd_args* a, int dtype) { return a && dw_spatial_bwd_rc_supported(*a, dtype) ? 1 : 0; }
int dwn_dw_spatial_fwd_rc_supported(const dwn_dw_spatial_fwd_args* a, int dtype) { return a && dw_spatial_fwd_rc_walk_supported(*a, dtype) ? 1 : 0; }
int dwn_dw_temporal_fwd(const dwn_dw_temporal_fwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "dw_temporal_fwd");
    // this entry's built set stays {3, 5}: the launcher behind it also serves the block path, where 7 and 9 go on to the wide kernels
    if (a->kt != 3 && a->kt != 5) return dwn_set_error(-4, "dw_temporal: only temporal_kernel 3 or 5 is built");
    ENTER(device);
    return launch_dw_temporal_fwd(*a, dtype, (hipStream_t)stream);
}
int dwn_dw_temporal_bwd(const dwn_dw_temporal_bwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "dw_temporal_bwd");
    if (a->kt != 3 && a->kt != 5) return dwn_set_error(-4, "dw_temporal: only temporal_kernel 3 or 5 is built");
    ENTER(device);
    return launch_dw_temporal_bwd(*a, dtype, (hipStream_t)stream);
}
int dwn_dw_temporal_wide_fwd(const dwn_dw_temporal_fwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "dw_temporal_wide_fwd");
    TRY(dw_temporal_wide_check(a->kt, a->C, LD_PLAIN));
    ENTER(device);
    return launch_dw_temporal_wide_fwd(*a, dtype, (hipStream_t)stream);
}
int dwn_dw_temporal_wide_bwd(const dwn_dw_temporal_bwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "dw_temporal_wide_bwd");
    TRY(dw_temporal_wide_check(a->kt, a->C, a->dy_kind));
    ENTER(device);
    return launch_dw_temporal_wide_bwd(*a, dtype, (hipStream_t)stream);
}
int dwn_bn_finalize(const double* stats, int stat_c, double count, const dwn_bn* bn, int C, int training,
                    float momentum, float eps, int device, void* stream) {
    NEEDS(bn && (stats || !training), "bn_finalize: null pointer (bn; stats in training mode)");
    ENTER(device);
    return bn_finalize(stats, stat_c, count, *bn, C, training, momentum, eps, (hipStream_t)stream);
}
int dwn_bn_bwd_finalize(const double* stats, double count, const dwn_bn* bn, float* abc, int C, int device,
                        void* stream) {
    NEEDS(stats && bn && abc, "bn_bwd_finalize: null pointer (stats, bn, abc)");
    ENTER(device);
    return k_bn_bwd_finalize(bwd_job(stats, count, *bn, abc, C, false), BnBwdJob{}, (hipStream_t)stream);
}
// BatchNorm-1 of conv_pw WITHOUT conv_pw's output (dwn.h): raw products [a0 | 1]^T a0 by one gemm_tn pass, then k_bn1_gram_finalize
// (sized for the replicas of the streaming kernel of dwn_gram.hip where either dtype has them)
size_t dwn_conv_pw_bn_stats_workspace_bytes(int Cin) {
    const int nrep = gram_nrep(DWN_BF16, Cin) > gram_nrep(DWN_F32, Cin) ? gram_nrep(DWN_BF16, Cin) : gram_nrep(DWN_F32, Cin);
    return (size_t)nrep * (Cin + 8) * Cin * sizeof(double) + 256;
}
int dwn_conv_pw_bn_stats(const void* a0, long long a0_ld, long long M, const float* w_pw, int E, int Cin, const dwn_bn* bn,
                         float momentum, float eps, double* sc_stats, void* ws, size_t ws_bytes, int dtype, int device, void* stream) {
    NEEDS(bn, "conv_pw_bn_stats: null pointer (bn)");
    if (Cin % 8 || E <= 0 || M <= 0 || M >= (1ll << 31)) return dwn_set_error(-2, "conv_pw_bn_stats: Cin % 8 == 0, 0 < M < 2^31");
    if (!a0 || !w_pw || !bn->coef || !ws) return dwn_set_error(-1, "conv_pw_bn_stats: null pointer (a0, w_pw, bn.coef, ws)");
    if (ws_bytes < dwn_conv_pw_bn_stats_workspace_bytes(Cin)) return dwn_set_error(-6, "conv_pw_bn_stats: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    double* gram = reinterpret_cast<double*>(((size_t)ws + 255) & ~(size_t)255);
    const int nrep = gram_nrep(dtype, Cin);
    TRY(k_zero(gram, (size_t)nrep * (Cin + 8) * Cin * sizeof(double), s));
    bool streamed = false;
    TRY(k_gram(a0, a0_ld, M, Cin, gram, dtype, &streamed, s));
    if (!streamed) {
        LoadDesc cat = ld_plain(a0, a0_ld);
        cat.cat_c1 = Cin; cat.cat_c2 = 0;
        GemmTN g = tn_base(cat, LD_CAT1, ld_plain(a0, a0_ld), LD_PLAIN, (int)M, Cin + 8, Cin, reinterpret_cast<float*>(gram), Cin, 1);
        g.dw_f64 = 1;
        TRY(launch_gemm_tn(g, dtype, s));
    }
    return k_bn1_gram_finalize(gram, streamed ? nrep : 1, w_pw, E, Cin, (double)M, bn->gamma, bn->beta, bn->running_mean, bn->running_var,
                               bn->num_batches_tracked, momentum, eps, bn->coef, sc_stats, dtype, s);
}
int dwn_pack_weight(const float* src, void* dst, int groups, int R, int C, int transpose, int Rd, int Cd, int dtype,
                    int device, void* stream) {
    NEEDS(src && dst, "pack_weight: null pointer (src, dst)");
    ENTER(device);
    return k_pack_weight(src, dst, groups, R, C, transpose, Rd, Cd, dtype, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ stem
size_t dwn_stem_workspace_bytes(const dwn_stem_args* a) {
    WS_BYTES_OR_0(a, stem_geometry, stem_ws_bytes(a));
}
// Conv3d(Cin -> C0, 1x1x1) + BatchNorm3d (dwiseneuro.py:306-309).  y0 = W0 x is linear in the Cin <= 8 input channels, so the
// batch statistics come from the input moments (xmom) and y0 is never written: a->y0 is ignored (kept in the struct for
// layout compatibility), a->xmom receives [8] sums + [8][8] second moments (doubles) that the backward reads.
int dwn_stem_forward(const dwn_stem_args* a, int device, void* stream) {
    ARGS(a, "stem_forward");
    TRY(stem_geometry(a));
    if (!a->x || !a->w || !a->bn.coef || !a->out || !a->ws) return dwn_set_error(-1, "stem_forward: null pointer (x, w, bn.coef, out, ws)");
    if (a->training == DWN_BN_TRAIN && !a->xmom) return dwn_set_error(-1, "stem_forward: xmom buffer required in training mode");
    if (a->ws_bytes < stem_ws_bytes(a)) return dwn_set_error(-6, "stem: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    Carver c(a->ws, a->ws_bytes);
    double* mom = c.take<double>((size_t)DWN_NREP * stem_moment_count());
    const i64 M = (i64)a->B * a->S;
    if (a->training == DWN_BN_TRAIN) {
        TRY(k_zero(mom, (size_t)DWN_NREP * stem_moment_count() * sizeof(double), s));
        TRY(k_stem_xmom(a->x, a->B, a->Cin, a->S, mom, s));
        TRY(k_stem_bn_finalize(mom, (double)M, a->w, a->bn.gamma, a->bn.beta, a->bn.running_mean, a->bn.running_var,
                               a->bn.num_batches_tracked, a->momentum, a->eps, a->bn.coef, a->xmom, a->C0, a->Cin, s));
    } else {      // eval and frozen: coefficients from the running statistics, which stay as they are
        TRY(bn_finalize(nullptr, a->C0, (double)M, a->bn, a->C0, 0, a->momentum, a->eps, s));
    }
    return k_stem_out(a->x, a->w, a->bn.coef, a->pe_t, a->pe_h, a->pe_w, a->T, a->H, a->W, a->B, a->Cin, a->S, a->C0, a->out,
                      a->dtype, s);
}
int dwn_stem_backward(const dwn_stem_args* a, int device, void* stream) {
    ARGS(a, "stem_backward");
    TRY(stem_geometry(a));
    const bool frozen = a->training == DWN_BN_FROZEN;
    if (!a->x || !a->w || !a->bn.coef || !a->dout || !a->dw || !a->ws)
        return dwn_set_error(-1, "stem_backward: null pointer (x, w, bn.coef, dout, dw, ws)");
    if (!frozen && !a->xmom) return dwn_set_error(-1, "stem_backward: xmom (saved by the forward) required");
    if (a->ws_bytes < stem_ws_bytes(a)) return dwn_set_error(-6, "stem: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    Carver c(a->ws, a->ws_bytes);
    double* mom = c.take<double>((size_t)DWN_NREP * stem_moment_count());
    double* acc = c.take<double>((size_t)DWN_NREP * a->C0 * stem_acc_stride());
    const i64 M = (i64)a->B * a->S;
    if (frozen) {
        // frozen statistics: the same accumulation pass with zero input means (the workspace's moment slot, cleared with the
        // accumulators: the two are adjacent) -> raw sums Σ dout x_k, Σ dout; the frozen finaliser needs no batch moments
        TRY(k_zero(mom, (size_t)((char*)(acc + (size_t)DWN_NREP * a->C0 * stem_acc_stride()) - (char*)mom), s));
        TRY(k_stem_bwd_acc(a->dout, a->x, mom, (double)M, a->B, a->Cin, a->S, a->C0, acc, a->dtype, s));
        return k_stem_bwd_finalize_frozen(acc, a->w, a->bn.coef, a->bn.dgamma, a->bn.dbeta, a->dw, a->C0, a->Cin, s);
    }
    TRY(k_zero(acc, (size_t)DWN_NREP * a->C0 * stem_acc_stride() * sizeof(double), s));
    TRY(k_stem_bwd_acc(a->dout, a->x, a->xmom, (double)M, a->B, a->Cin, a->S, a->C0, acc, a->dtype, s));
    return k_stem_bwd_finalize(acc, a->xmom, a->w, a->bn.coef, (double)M, a->bn.dgamma, a->bn.dbeta, a->dw, a->C0, a->Cin, s);
}

// dwn_stem_backward in training mode + dx through the batch statistics (dwn.h).  The first three launches are dwn_stem_backward's,
// argument for argument; Q, q0, x̄ (80 floats) go to the workspace's moment slot, which only the forward and the frozen backward
// use — dwn_stem_workspace_bytes does not grow.
int dwn_stem_backward_input(const dwn_stem_args* a, float* dx, int device, void* stream) {
    NEEDS(a && dx, "stem_backward_input: null pointer (args, dx)");
    if (a->training != DWN_BN_TRAIN)
        return dwn_set_error(-7, "stem_backward_input: built for batch statistics (DWN_BN_TRAIN) only; the frozen-statistics input "
                                 "gradient is dwn_stem_backward + dwn_stem_input_grad");
    TRY(stem_geometry("stem_backward_input", a->dtype, a->training, a->B, a->Cin, a->C0, a->S));
    if (a->C0 > (a->dtype == DWN_BF16 ? 128 : 64) || a->Cin > 8)
        return dwn_set_error(-4, "stem_backward_input: more than 128 (bf16) / 64 (fp32) stem channels or 8 input channels not built");
    if (!a->x || !a->w || !a->bn.coef || !a->dout || !a->dw || !a->xmom || !a->ws)
        return dwn_set_error(-1, "stem_backward_input: null pointer (x, w, bn.coef, dout, dw, xmom, ws)");
    if (a->ws_bytes < stem_ws_bytes(a)) return dwn_set_error(-6, "stem: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    Carver c(a->ws, a->ws_bytes);
    double* mom = c.take<double>((size_t)DWN_NREP * stem_moment_count());
    double* acc = c.take<double>((size_t)DWN_NREP * a->C0 * stem_acc_stride());
    float* qx = reinterpret_cast<float*>(mom);
    const i64 M = (i64)a->B * a->S;
    TRY(k_zero(acc, (size_t)DWN_NREP * a->C0 * stem_acc_stride() * sizeof(double), s));
    TRY(k_stem_bwd_acc(a->dout, a->x, a->xmom, (double)M, a->B, a->Cin, a->S, a->C0, acc, a->dtype, s));
    TRY(k_stem_bwd_finalize(acc, a->xmom, a->w, a->bn.coef, (double)M, a->bn.dgamma, a->bn.dbeta, a->dw, a->C0, a->Cin, s));
    TRY(k_stem_bwd_finalize_dx(acc, a->xmom, a->w, a->bn.coef, (double)M, qx, a->C0, a->Cin, s));
    return k_stem_input_grad_train(a->dout, a->w, a->bn.coef, a->x, qx, a->B, a->Cin, a->S, a->C0, dx, a->dtype, s);
}

// dx of the stem with BatchNorm as a fixed affine map (dwn.h): one streaming pass over dout
int dwn_stem_input_grad(const dwn_stem_input_grad_args* a, int device, void* stream) {
    ARGS(a, "stem_input_grad");
    if (a->training != DWN_BN_FROZEN)
        return dwn_set_error(-7, "stem_input_grad: this entry is the frozen-statistics (DWN_BN_FROZEN) input gradient; through batch "
                                 "statistics (DWN_BN_TRAIN) it is dwn_stem_backward_input");
    TRY(stem_geometry("stem_input_grad", a->dtype, a->training, a->B, a->Cin, a->C0, a->S));
    if (!a->w || !a->coef || !a->dout || !a->dx) return dwn_set_error(-1, "stem_input_grad: null pointer (w, coef, dout, dx)");
    ENTER(device);
    return k_stem_input_grad(a->dout, a->w, a->coef, a->B, a->Cin, a->S, a->C0, a->dx, a->dtype, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ block
size_t dwn_block_workspace_bytes(const dwn_block_args* a, int backward) {
    WS_BYTES_OR_0(a, check_block, carve_block(*a, plan_block(*a), backward, nullptr, 0).bytes);
}

// the pointers every route of a direction reads or writes (the SE biases, BatchNorm parameters and optional tables are the kernels' own)
static bool block_common_pointers(const dwn_block_args& a) {
    return a.y2 && a.y4 && a.z3 && a.w_pw && a.w_dws && a.w_dwt && a.w_pwl && a.se_wr && a.se_we && a.se_pmean && a.se_hidpre &&
           a.se_gate && a.bn1.coef && a.bn2.coef && a.bn3.coef && a.bn4.coef && a.bnsc.coef && a.ws;
}

int dwn_block_forward(const dwn_block_args* ap, int device, void* stream) {
    ARGS(ap, "block_forward");
    const dwn_block_args& a = *ap;
    TRY(check_block(ap));
    const BlockPlan p = plan_block(a);
    if (!block_common_pointers(a) || !a.x || !a.out || ((p.writes & 1) && !a.y1) || ((p.writes & 2) && !a.y3))
        return dwn_set_error(-1, "block_forward: null pointer (x, out, y2, y4, z3, the four weights, se_wr, se_we, se_pmean, se_hidpre, "
                                 "se_gate, the five bn coef, ws; y1 / y3 where dwn_block_forward_writes names them)");
    if (!a.x_has_pe && !a.a0) return dwn_set_error(-2, "block_forward: a0 buffer required when x_has_pe == 0");
    BlockWs w = carve_block(a, p, 0, a.ws, a.ws_bytes);
    if (w.bytes > a.ws_bytes) return dwn_set_error(-6, "block_forward: workspace too small");
    const int dt = a.dtype, S_out = p.S_out;
    const i64 Min = p.Min, Mout = p.Mout;
    PrepArgs pa;
    {   // ---- prep, one launch: zero the statistics arena, pack the four weights
        bool ok = pa.zero(w.zero_beg, ((size_t)(w.zero_end - w.zero_beg) + 15) & ~(size_t)15);
        ok = ok && pa.packw(a.w_pw, w.wpw, 1, a.Cmid, a.Cin, 0, a.Cmid, a.Cin);
        ok = ok && pa.packw(a.w_pwl, w.wpwl, 1, a.Cout, a.Cmid, 0, a.Cout, a.Cmid);
        ok = ok && pa.packdw(a.w_dws, w.wdws, a.Cmid, a.ks * a.ks);
        ok = ok && pa.packdw(a.w_dwt, w.wdwt, a.Cmid, a.kt);
        if (!p.bs) {    // eval / frozen: the five BatchNorm coefficient sets come from running statistics — same launch
            ok = ok && pa.bneval(a.bn1, a.Cmid, a.eps) && pa.bneval(a.bn2, a.Cmid, a.eps) && pa.bneval(a.bn3, a.Cmid, a.eps);
            ok = ok && pa.bneval(a.bn4, a.Cout, a.eps) && pa.bneval(a.bnsc, a.Cout, a.eps);
        }
        if (!ok) return dwn_set_error(-2, "block_forward: workspace arena must be 16-byte aligned");
    }
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    TRY(k_prep(pa, dt, s));
    // ---- PositionalEncoding3d (dwiseneuro.py:184-192): normally already folded into x by the producer (stem /
    // previous block's residual kernel); stand-alone callers get it materialised here
    const void* a0 = a.x;
    if (!a.x_has_pe) {
        TRY(k_ew_apply(ld_pe(a.x, a.Cin, a.pe_t, a.pe_h, a.pe_w, a.T, a.Hin, a.Win), LD_PE, a.a0, a.Cin, Min, a.Cin, dt, s));
        a0 = a.a0;
    }
    LoadDesc xin = ld_plain(a0, a.Cin);
    // ---- conv_pw (dwiseneuro.py:90-93) + spat_covn_dw (:96-102), by the plan's route
    // the chained / generic stencil: on the stored y1, or (rebuilt) on the y1 rows it rebuilds from a0 on the matrix cores
    auto spatial_fwd = [&](bool rebuilt) -> int {
        DwSpatialFwd d = dws_desc<DwSpatialFwd>(a, rebuilt);
        d.in = ld_bnact(rebuilt ? nullptr : a.y1, a.Cmid, a.bn1.coef, a.Cmid, 1, nullptr, 0, 1);
        if (rebuilt) { d.a0 = a0; d.w1 = w.wpw; }
        d.w = w.wdws; d.out = a.y2; d.stats = p.tr ? w.st2 : nullptr;
        PROF(DWN_FAM_DWS_FWD, launch_dw_spatial_fwd(d, dt, s));
        return 0;
    };
    switch (p.pw) {
    case PW_EVAL_CHAIN:
        TRY(spatial_fwd(true));
        break;
    case PW_Y1_FREE:
        // BatchNorm-1's batch statistics from the Gram matrix of a0 (one C-wide pass), then the stencil rebuilds the y1 rows it needs:
        // conv_pw is no pass, a.y1 is not written.  (Frozen: BatchNorm-1 is known, no Gram pass)
        if (p.bs) {
            // the streaming kernel of dwn_gram.hip where it is built (bf16, 64 channels: one read, gram_nrep replicas), else gemm_tn [a0 | 1]^T a0
            bool streamed = false;
            PROF(DWN_FAM_PW_FWD, k_gram(a0, a.Cin, Min, a.Cin, w.gram, dt, &streamed, s));
            if (!streamed) {
                LoadDesc cat = ld_plain(a0, a.Cin);
                cat.cat_c1 = a.Cin; cat.cat_c2 = 0;
                GemmTN g = tn_base(cat, LD_CAT1, xin, LD_PLAIN, (int)Min, a.Cin + 8, a.Cin, reinterpret_cast<float*>(w.gram), a.Cin, 1);
                g.dw_f64 = 1;                         // fp64 atomics: the variance is a difference of these sums
                PROF(DWN_FAM_PW_FWD, launch_gemm_tn(g, dt, s));
            }
            PROF(DWN_FAM_PW_FWD, k_bn1_gram_finalize(w.gram, streamed ? gram_nrep(dt, a.Cin) : 1, a.w_pw, a.Cmid, a.Cin, (double)Min,
                                                     a.bn1.gamma, a.bn1.beta, a.bn1.running_mean, a.bn1.running_var, a.bn1.num_batches_tracked,
                                                     a.momentum, a.eps, a.bn1.coef, p.identity_sc ? w.stsc : nullptr, dt, s));
        }
        TRY(spatial_fwd(true));
        break;
    case PW_EVAL_RC: {
        // BatchNorm-1 needs no batch statistics and nobody reads y1 again, so the stencil kernel rebuilds its y1 tiles from a0
        // (MFMA) and conv_pw disappears as a pass (a.y1 is not written)
        TRY(dwn_dw_spatial_rc_prep(a.w_pw, w.wdws, a.bn1.coef, a.Cmid, a.Cin, w.rcblob, device, stream));
        dwn_dw_spatial_rc_fwd_args r; memset(&r, 0, sizeof(r));
        r.a0 = a0; r.a0_ld = a.Cin; r.blob = w.rcblob; r.out = a.y2; r.planes = a.B * a.T; r.Hin = a.Hin; r.Win = a.Win;
        r.Hout = a.Hout; r.Wout = a.Wout; r.Cin = a.Cin; r.E = a.Cmid; r.stride = a.stride; r.stats = nullptr;
        r.rows_band = 0; r.round_y1 = 1;
        PROF(DWN_FAM_DWS_FWD, dwn_dw_spatial_fwd_rc(&r, device, stream));
        break;
    }
    case PW_MATERIALISED: {
        // y1 = a0 @ W1^T, Σ/Σ² for bn1
        GemmNN g = nn_base(xin, LD_PLAIN, w.wpw, a.Cin, a.y1, a.Cmid, (int)Min, a.Cmid, a.Cin, 1);
        g.f32_split = f32_split_of(a.f32_products, !p.tr);    // eval-mode fp32: bf16 hi/lo products (dwn_gemm_nn.h NN_F32_X3) unless NATIVE
        g.stats = p.tr ? w.st1 : nullptr; g.stat_nchan = a.Cmid;
        PROF(DWN_FAM_PW_FWD, launch_gemm_nn(g, dt, s));
        if (p.bs) TRY(bn_finalize(w.st1, a.Cmid, (double)Min, a.bn1, a.Cmid, 1, a.momentum, a.eps, s));
        TRY(spatial_fwd(false));
        break;
    }
    }
    if (p.bs) TRY(bn_finalize(w.st2, a.Cmid, (double)Mout, a.bn2, a.Cmid, 1, a.momentum, a.eps, s));
    {   // ---- temp_covn_dw (:105-111)
        DwTemporalFwd d; memset(&d, 0, sizeof(d));
        d.in = ld_bnact(a.y2, a.Cmid, a.bn2.coef, a.Cmid, 1, nullptr, 0, 1);
        d.w = w.wdwt; d.out = a.y3; d.B = a.B; d.T = a.T; d.HW = a.Hout * a.Wout; d.C = a.Cmid; d.kt = a.kt;
        d.stats = p.tr ? w.st3 : nullptr;
        if (p.eval_z3) {     // eval: BatchNorm-3 is known -> z3 and the SE pooling sums (integer sums: any order) straight from this pass
            d.out = a.z3; d.z_scale = a.bn3.coef; d.z_shift = a.bn3.coef + a.Cmid; d.pooled = w.pooled;
        }
        PROF(DWN_FAM_DWT_FWD, launch_dw_temporal_fwd(d, dt, s));
    }
    if (p.bs) TRY(bn_finalize(w.st3, a.Cmid, (double)Mout, a.bn3, a.Cmid, 1, a.momentum, a.eps, s));
    // ---- se (:38-43)
    if (!p.eval_z3) {
        LoadDesc z3 = ld_bnact(a.y3, a.Cmid, a.bn3.coef, a.Cmid, 1, nullptr, 0, S_out);
        PROF(DWN_FAM_SE_POOL, k_se_pool(z3, a.B, a.Cmid, S_out, w.pooled, a.z3, dt, s));
    }
    // (z3 * gate_b) @ W2^T == z3 @ (W2 . diag(gate_b))^T: where conv_pwl runs on per-sample weights the SE kernel writes them too
    int gate_folded = 0;
    TRY(k_se_mlp_fwd(w.pooled, 1.0f / (float)S_out, a.se_wr, a.se_br, a.se_we, a.se_be, a.B, a.Cmid, a.se_r,
                     a.se_pmean, a.se_hidpre, a.se_gate, p.pwl_gated ? a.w_pwl : nullptr, w.wgated, a.Cout, dt, &gate_folded, s));
    {   // ---- conv_pwl (:117-120): y4 = (silu(bn3(y3)) * gate) @ W2^T
        GemmNN g;
        if (p.pwl_gated) {
            if (!gate_folded) TRY(k_gate_weights(a.w_pwl, a.se_gate, w.wgated, a.B, a.Cout, a.Cmid, dt, s));
            g = nn_base(ld_plain(a.z3, a.Cmid), LD_PLAIN, w.wgated, a.Cmid, a.y4, a.Cout, (int)Mout, a.Cout, a.Cmid, 1);
            g.b_sample_stride = (i64)a.Cout * a.Cmid; g.b_rows_per_sample = S_out;
        } else {
            LoadDesc u = ld_plain(a.z3, a.Cmid);
            u.gate = a.se_gate; u.gate_ld = a.Cmid; u.rows_per_sample = S_out;
            g = nn_base(u, LD_GATE, w.wpwl, a.Cmid, a.y4, a.Cout, (int)Mout, a.Cout, a.Cmid, 1);
        }
        g.stats = p.tr ? w.st4 : nullptr; g.stat_nchan = a.Cout; g.f32_split = f32_split_of(a.f32_products, !p.tr);
        PROF(DWN_FAM_PWL_FWD, launch_gemm_nn(g, dt, s));
    }
    // ---- shortcut (:125-134) + residual (:143); the two linear BatchNorms (conv_pwl.1.bn, bn_sc.bn) finalise in one launch
    ResGeom gm = geom_of(a);
    if (p.bs) {
        // (y1-free on an identity-map block: the shortcut's sums came out of the Gram pass, k_bn1_gram_finalize)
        if (!(p.pw == PW_Y1_FREE && p.identity_sc)) PROF(DWN_FAM_RESID_FWD, k_shortcut_stats(xin, gm, w.stsc, dt, s));
        TRY(k_bn_finalize_train(fin_job(w.st4, a.Cout, (double)Mout, a.bn4, a.Cout),
                                 fin_job(w.stsc, a.Cin, (double)Mout, a.bnsc, a.Cout), a.momentum, a.eps, s));
    }
    PROF(DWN_FAM_RESID_FWD, k_residual_fwd(xin, a.y4, a.bn4.coef, a.bnsc.coef, a.drop_scale, gm, a.out_pe_t, a.out_pe_h,
                                           a.out_pe_w, a.out, dt, s));
    return 0;
}

// conv_pw backward from (dh1, a0, W1, BatchNorm-1 backward coefficients): da0 and dW1, y1 not read (see the comment at its call
// in dwn_block_backward).  gacc (pw_fold_floats) and tacc (pw_wgrad_tacc_floats) must be zero on entry.
// res / res_abc / res_C (optional, dwn.h dwn_pw_bwd_args): the stride-1 shortcut branch's gradient folded in — the A2 * a0 and A3
// terms into G / r3, the A1 * dout term as the data-gradient GEMM's residual epilogue — so that da0 is the block's input gradient.
// rg (optional, with res): the shortcut's nearest map when it is not the identity (stride-2 block) — hinv / winv and the two
// plane sizes; the x terms then stay in the kernel's epilogue (only sampled rows have them).
static int pw_backward(int dt, const void* dh1, const void* a0, const float* w_pw, const float* abc, int E, int Cin, i64 M,
                       void* bp, float* gacc, float* r3, float* tacc, void* da0, float* dw, const void* res,
                       const float* res_abc, int res_C, const ResGeom* rg, hipStream_t s, bool fold = true) {
    const int res_n = res ? res_C / Cin : 0;         // (dwn_pw_backward has checked the shortcut term; the block's plan grants it)
    const bool gathered = res && rg && rg->hinv;
    TRY(k_pw_bwd_prep(w_pw, abc, E, Cin, bp, gacc, r3, dt, (res && !gathered) ? res_abc : nullptr, res_C, s));
    if (pw_bwd_fused_supported(dt, M, E, Cin)) {
        // 64- and 128-channel blocks (0-3, 4-6): both products from ONE pass over dh1
        PROF(DWN_FAM_PW_DGRAD, launch_pw_bwd_fused(dh1, a0, bp, r3, da0, tacc, M, E, Cin, dt, res, res_abc, res_n,
                                                   gathered ? rg->hinv : nullptr, gathered ? rg->winv : nullptr, gathered ? rg->Hin : 0,
                                                   gathered ? rg->Win : 0, gathered ? rg->Hout : 0, gathered ? rg->Wout : 0, s));
    } else {
        {
            GemmNN g = nn_base(ld_plain(dh1, E), LD_PLAIN, bp, (i64)E + Cin, da0, Cin, (int)M, Cin, E + Cin, 1);
            g.epi = EPI_STORE_CAT; g.a2 = a0; g.a2_ld = Cin; g.K1 = E; g.bias = r3;
            PROF(DWN_FAM_PW_DGRAD, launch_gemm_nn(g, dt, s));
        }
        {   // raw products [dh1 | a0 | 1]^T a0 -> tacc
            LoadDesc cat = ld_plain(dh1, E);
            cat.q = a0; cat.ld2 = Cin; cat.cat_c1 = E; cat.cat_c2 = Cin;
            GemmTN g = tn_base(cat, LD_CAT1, ld_plain(a0, Cin), LD_PLAIN, (int)M, E + Cin + 8, Cin, tacc, Cin, 1);
            PROF(DWN_FAM_PW_WGRAD, launch_gemm_tn(g, dt, s));
        }
    }
    if (!fold) return 0;            // dwn_block_backward folds tacc in its parameter-gradient tail (k_block_param_tail)
    return k_pw_wgrad_fold(tacc, abc, w_pw, E, Cin, dw, dt, s);
}

int dwn_block_backward(const dwn_block_args* ap, int device, void* stream) {
    ARGS(ap, "block_backward");
    const dwn_block_args& a = *ap;
    if (a.training == DWN_BN_EVAL)
        return dwn_set_error(-7, "block_backward: only training-mode (batch-statistics) and frozen-statistics backward are built");
    TRY(check_block(ap));
    const BlockPlan p = plan_block(a);
    const bool y1_free = p.pw == PW_Y1_FREE;         // the forward of these arguments wrote no y1 (BlockPlan::writes)
    if (!block_common_pointers(a) || !(a.x_has_pe ? a.x : a.a0) || !a.y3 || !a.dout || !a.dx || !a.buf_a || !a.buf_b || !a.dy4 ||
        !a.dw_pw || !a.dw_dws || !a.dw_dwt || !a.dw_pwl || !a.dse_wr || !a.dse_br || !a.dse_we || !a.dse_be ||
        (!y1_free && !a.y1) || (!p.dx_folded && !a.da0))
        return dwn_set_error(-1, "block_backward: null pointer (the block input, y2, y3, y4, z3, dout, dx, buf_a, buf_b, dy4, the weights "
                                 "and saved SE tensors, the dw_* and dse_* gradients, the five bn coef, ws; y1 where the forward wrote it; "
                                 "da0 unless dwn_block_backward_route bit 0)");
    BlockWs w = carve_block(a, p, 1, a.ws, a.ws_bytes);
    if (w.bytes > a.ws_bytes) return dwn_set_error(-6, "block_backward: workspace too small");
    const int dt = a.dtype, S_out = p.S_out;
    const i64 Min = p.Min, Mout = p.Mout;
    float* dg = reinterpret_cast<float*>(w.pooled);
    PrepArgs pa;
    {   // ---- prep, one launch: zero the statistics arena, W2^T [Cmid][Cout], tap-major depth-wise weights, identity affine
        bool ok = pa.zero(w.zero_beg, ((size_t)(w.zero_end - w.zero_beg) + 15) & ~(size_t)15);
        ok = ok && pa.packw(a.w_pwl, w.wpwl, 1, a.Cout, a.Cmid, 1, a.Cmid, a.Cout);
        if (y1_free) ok = ok && pa.packw(a.w_pw, w.wpw, 1, a.Cmid, a.Cin, 0, a.Cmid, a.Cin);      // W1 as rounded: the stencil rebuilds y1 with it
        ok = ok && pa.packdw(a.w_dws, w.wdws, a.Cmid, a.ks * a.ks);
        ok = ok && pa.packdw(a.w_dwt, w.wdwt, a.Cmid, a.kt);
        ok = ok && pa.fill(w.ident3, 1.0f, a.Cmid);
        ok = ok && pa.fill(w.ident3 + a.Cmid, 0.0f, 2 * a.Cmid);
        // the atomically accumulated weight gradients are cleared here (callers pass uninitialised buffers); dw_pw is written
        // whole by k_pw_wgrad_fold from the raw products accumulated in tacc
        ok = ok && pa.zero(a.dw_dws, (size_t)a.Cmid * a.ks * a.ks * sizeof(float));
        ok = ok && pa.zero(a.dw_dwt, (size_t)a.Cmid * a.kt * sizeof(float));
        ok = ok && pa.zero(a.dw_pwl, (size_t)a.Cout * a.Cmid * sizeof(float));
        if (p.pwl_per_sample) ok = ok && pa.zero(w.pb, (size_t)a.B * a.Cout * a.Cmid * sizeof(float));
        ok = ok && pa.zero(w.gacc, pw_fold_floats(a.Cin) * sizeof(float));
        ok = ok && pa.zero(w.tacc, pw_wgrad_tacc_floats(a.Cmid, a.Cin) * sizeof(float));
        if (!ok) return dwn_set_error(-2, "block_backward: workspace arena and dw_* buffers must be 16-byte aligned");
    }
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    TRY(k_prep(pa, dt, s));
    // ---- residual + the two linear BNs (bn4 = conv_pwl.1.bn, bnsc = bn_sc.bn)
    LoadDesc xin = ld_plain(a.x_has_pe ? a.x : a.a0, a.Cin);     // block input including its positional encoding
    ResGeom gm = geom_of(a);
    PROF(DWN_FAM_RESID_BWD, k_residual_bwd_reduce(xin, a.y4, a.dout, a.bn4.coef, a.bnsc.coef, a.drop_scale, gm, w.st4, w.stsc, dt, s));
    TRY(k_bn_bwd_finalize(bwd_job(w.st4, (double)Mout, a.bn4, w.abc4, a.Cout, p.frozen),
                          bwd_job(w.stsc, (double)Mout, a.bnsc, w.abcsc, a.Cout, p.frozen), s));
    PROF(DWN_FAM_RESID_BWD, k_residual_bwd_dy4(a.y4, a.dout, w.abc4, a.drop_scale, gm, a.dy4, dt, s));
    // ---- conv_pwl + SE backward: du = dy4 @ W2 (+ SE gate gradient), dW2 = dy4^T @ u; both forms leave dh3 in du and its sums in st3
    void* du = a.buf_a;
    if (p.pwl_per_sample) {
        // per-sample products P_b = dy4_b^T z3_b -> dW2 and the SE gate gradient without touching du
        {
            GemmTN g = tn_base(ld_plain(a.dy4, a.Cout), LD_PLAIN, ld_plain(a.z3, a.Cmid), LD_PLAIN, (int)Mout, a.Cout,
                               a.Cmid, w.pb, a.Cmid, 1);
            g.rows_per_sample = S_out; g.dw_sample_stride = (i64)a.Cout * a.Cmid;
            PROF(DWN_FAM_PWL_WGRAD, launch_gemm_tn(g, dt, s));
        }
        PROF(DWN_FAM_PWL_WGRAD, k_pwl_bwd_reduce(w.pb, a.se_gate, a.w_pwl, a.B, a.Cout, a.Cmid, a.dw_pwl, dg, s));
        TRY(k_se_mlp_bwd(dg, a.se_gate, a.se_hidpre, a.se_pmean, a.se_wr, a.se_we, a.B, a.Cmid, a.se_r,
                         1.0f / (float)S_out, w.dgp, w.dhp, w.dps, a.dse_wr, a.dse_br, a.dse_we, a.dse_be, s, false));
        // dh3 = (du*gate + dpS) * silu'(bn3(y3)) with du = dy4 . W2 recomputed in the GEMM, plus the bn3 backward sums
        GemmNN g = nn_base(ld_plain(a.dy4, a.Cout), LD_PLAIN, w.wpwl, a.Cout, du, a.Cmid, (int)Mout, a.Cmid, a.Cout, 1);
        g.epi = EPI_DH3; g.y3 = a.y3; g.ldy3 = a.Cmid; g.gate3 = a.se_gate; g.dps3 = w.dps; g.dg_ld = a.Cmid;
        g.coef3 = a.bn3.coef; g.coef3_ld = a.Cmid; g.rows_per_sample = S_out;
        g.stats = w.st3; g.stat_nchan = a.Cmid;
        PROF(DWN_FAM_PWL_DGRAD, launch_gemm_nn(g, dt, s));
    } else {
        // the materialised du
        {
            GemmNN g = nn_base(ld_plain(a.dy4, a.Cout), LD_PLAIN, w.wpwl, a.Cout, du, a.Cmid, (int)Mout, a.Cmid, a.Cout, 1);
            g.epi = EPI_DG; g.y3 = a.z3; g.ldy3 = a.Cmid; g.s3 = nullptr; g.t3 = nullptr; g.dg = dg;
            g.dg_ld = a.Cmid; g.rows_per_sample = S_out;
            PROF(DWN_FAM_PWL_DGRAD, launch_gemm_nn(g, dt, s));
        }
        {
            LoadDesc u = ld_plain(a.z3, a.Cmid);
            u.gate = a.se_gate; u.gate_ld = a.Cmid; u.rows_per_sample = S_out;
            GemmTN g = tn_base(ld_plain(a.dy4, a.Cout), LD_PLAIN, u, LD_GATE, (int)Mout, a.Cout, a.Cmid, a.dw_pwl, a.Cmid, 1);
            PROF(DWN_FAM_PWL_WGRAD, launch_gemm_tn(g, dt, s));
        }
        TRY(k_se_mlp_bwd(dg, a.se_gate, a.se_hidpre, a.se_pmean, a.se_wr, a.se_we, a.B, a.Cmid, a.se_r,
                         1.0f / (float)S_out, w.dgp, w.dhp, w.dps, a.dse_wr, a.dse_br, a.dse_we, a.dse_be, s, false));
        // bn3 backward sums over dh3 = (du*gate + dpS) * silu'(h3)
        LoadDesc d3; memset(&d3, 0, sizeof(d3));
        d3.p = du; d3.q = a.y3; d3.ld = a.Cmid; d3.v1 = w.ident3; d3.v2 = w.ident3 + a.Cmid; d3.v3 = w.ident3 + 2 * a.Cmid;
        d3.v4 = a.bn3.coef; d3.v5 = a.bn3.coef + a.Cmid; d3.gate = a.se_gate; d3.gate2 = w.dps; d3.gate_ld = a.Cmid;
        d3.rows_per_sample = S_out;
        // ... and dh3 replaces du in place, so the temporal kernel reads (dh3, y3) with the plain BN-backward affine
        PROF(DWN_FAM_BN3_REDUCE, k_bn3_bwd_reduce(d3, a.bn3.coef, Mout, a.Cmid, w.st3, du, dt, s));
    }
    TRY(k_bn_bwd_finalize(bwd_job(w.st3, (double)Mout, a.bn3, w.abc3, a.Cmid, p.frozen), BnBwdJob{}, s));
    {   // ---- temporal dw backward
        DwTemporalBwd d; memset(&d, 0, sizeof(d));
        d.dy = ld_affine2(du, a.y3, a.Cmid, w.abc3, a.Cmid);
        d.dy_kind = LD_PLAIN;                           // y3 is recomputed from y2 inside the kernel (one E-wide pass less)
        d.y2 = ld_ycoef(a.y2, a.Cmid, a.bn2.coef, a.Cmid);
        d.w = w.wdwt; d.dh2 = a.buf_b; d.dw = a.dw_dwt; d.B = a.B; d.T = a.T; d.HW = a.Hout * a.Wout; d.C = a.Cmid;
        d.kt = a.kt; d.stats = w.st2;
        PROF(DWN_FAM_DWT_BWD, launch_dw_temporal_bwd(d, dt, s));
    }
    TRY(k_bn_bwd_finalize(bwd_job(w.st2, (double)Mout, a.bn2, w.abc2, a.Cmid, p.frozen), BnBwdJob{}, s));
    // ---- spatial dw backward (du is dead: reuse buf_a for dh1)
    void* dh1 = a.buf_a;
    {
        DwSpatialBwd d = dws_desc<DwSpatialBwd>(a, y1_free);
        d.dy = ld_affine2(a.buf_b, a.y2, a.Cmid, w.abc2, a.Cmid);
        d.y1 = ld_ycoef(y1_free ? nullptr : a.y1, a.Cmid, a.bn1.coef, a.Cmid);
        if (y1_free) { d.a0 = xin.p; d.w1 = w.wpw; }                                      // y1 rebuilt from the block input
        d.w = w.wdws; d.dh1 = dh1; d.dw = a.dw_dws; d.stats = w.st1;
        PROF(DWN_FAM_DWS_BWD, launch_dw_spatial_bwd(d, dt, s));
    }
    TRY(k_bn_bwd_finalize(bwd_job(w.st1, (double)Min, a.bn1, w.abc1, a.Cmid, p.frozen), BnBwdJob{}, s));
    // ---- conv_pw backward WITHOUT y1.  dy1 = A1*dh1 + A2*y1 + A3 is linear and y1 = a0.W1^T, so the y1 terms fold into Cin x Cin
    // matrices on either side:  da0 = [dh1 | a0] . [diag(A1) W1 ; G] + r3  (Bp, r3: k_pw_bwd_prep) and
    // dW1 = diag(A1) (dh1^T a0) + diag(A2) W1 (a0^T a0) + A3 (1^T a0)  (raw products in tacc, folded by k_pw_wgrad_fold)
    // On a stride-1 block of 64 or 128 channels (identity shortcut map, output channels = input channels tiled once or twice) the shortcut branch's
    // gradient is folded into this GEMM and its result IS dx: no pass over (da0, x, dout) -> dx (BlockPlan::dx_folded).
    // (one-pass kernel only: as an epilogue of the two-GEMM path's data-gradient GEMM it cost 30-60 us where the pass it replaces
    // takes 20-35.)  On a strided block the epilogue gathers: only the rows the nearest map samples carry the shortcut's terms.
    TRY(pw_backward(dt, dh1, xin.p, a.w_pw, w.abc1, a.Cmid, a.Cin, Min, w.bp, w.gacc, w.r3, w.tacc, p.dx_folded ? a.dx : a.da0, a.dw_pw,
                    p.dx_folded ? a.dout : nullptr, w.abcsc, a.Cout, p.sc_gathered ? &gm : nullptr, s, false));
    if (!p.dx_folded) PROF(DWN_FAM_RESID_BWD, k_residual_bwd_dx(xin, a.da0, a.dout, w.abcsc, gm, a.dx, dt, s));
    // ---- the parameter-gradient tail, last launch of the block: the SE MLP's parameter gradients (from dgp / dhp, k_se_mlp_bwd above)
    // and dW1 folded from tacc.  Nothing in the block reads them, so they leave the chain between the SE kernel and the dh3 GEMM
    return k_block_param_tail(w.dgp, w.dhp, a.se_pmean, a.se_hidpre, a.B, a.Cmid, a.se_r, a.dse_wr, a.dse_br, a.dse_we, a.dse_be,
                              w.tacc, w.abc1, a.w_pw, a.Cmid, a.Cin, a.dw_pw, dt, s);
}

// Which of the intermediates dwn_block_forward will write for these arguments: bit 0 = y1, bit 1 = y3 (BlockPlan::writes) — the
// caller need not allocate what is not written (and may pass NULL for it).
// Null arguments or a refused geometry: check_block's negative code, with the error set (both entries).
int dwn_block_forward_writes(const dwn_block_args* ap) {
    ARGS(ap, "block_forward_writes");
    TRY(check_block(ap));
    return plan_block(*ap).writes;
}
// How dwn_block_backward forms dx for these arguments: bit 0 = BlockPlan::dx_folded, bit 1 = BlockPlan::sc_gathered
int dwn_block_backward_route(const dwn_block_args* ap) {
    ARGS(ap, "block_backward_route");
    TRY(check_block(ap));
    const BlockPlan p = plan_block(*ap);
    return (p.dx_folded ? 1 : 0) | (p.sc_gathered ? 2 : 0);
}

// ------------------------------------------------------------------------------------------------ pool
// (BT and the rows BT * HW are 64-bit in the launchers and their grids are capped: no int product to bound)
static int pool_geometry(const dwn_pool_args* a) {
    if (a->C % 8) return dwn_set_error(-2, "pool: C must be a multiple of 8");      // (the kernels move whole 16-byte channel vectors)
    if (a->BT <= 0 || a->HW <= 0 || a->C <= 0) return dwn_set_error(-2, "pool: BT, HW, C must be positive");
    if (!dtype_ok(a->dtype)) return dwn_set_error(-2, "pool: dtype must be DWN_F32 or DWN_BF16");
    return 0;
}
int dwn_pool_forward(const dwn_pool_args* a, int device, void* stream) {
    ARGS(a, "pool_forward");
    TRY(pool_geometry(a));
    if (!a->x || !a->out) return dwn_set_error(-1, "pool_forward: null pointer (x, out)");
    ENTER(device);
    return k_pool_fwd(a->x, a->out, a->BT, a->HW, a->C, a->dtype, (hipStream_t)stream);
}
int dwn_pool_backward(const dwn_pool_args* a, int device, void* stream) {
    ARGS(a, "pool_backward");
    TRY(pool_geometry(a));
    if (!a->dout || !a->dx) return dwn_set_error(-1, "pool_backward: null pointer (dout, dx)");
    ENTER(device);
    return k_pool_bwd(a->dout, a->dx, a->BT, a->HW, a->C, a->dtype, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------------ cortex
namespace {
struct CortexWs { void* wp; double *st, *stsc; float *abc, *abcsc; void *dy, *dxmain; char *zb, *ze; size_t bytes; };
CortexWs carve_cortex(const dwn_cortex_args& a, int backward, void* base, size_t cap) {
    CortexWs w; memset(&w, 0, sizeof(w));
    Carver c(base, cap);
    const size_t ts = tsize(a.dtype);
    const i64 M = (i64)a.B * a.T;
    w.wp = c.take<char>((size_t)a.C * (a.Cin / a.groups) * ts);
    c.take<char>(0);
    size_t z0 = (c.off + 255) & ~(size_t)255;
    w.st = c.take<double>(nstat(a.C));
    w.stsc = c.take<double>(nstat(backward ? a.C : a.Cin));
    size_t z1 = c.off;
    if (backward) {
        w.abc = c.take<float>(3 * (size_t)a.C);
        w.abcsc = c.take<float>(3 * (size_t)a.C);
        w.dy = c.take<char>((size_t)M * a.C * ts);
        w.dxmain = c.take<char>((size_t)M * a.Cin * ts);
    }
    w.bytes = c.off + 256;
    if (base) { w.zb = (char*)base + z0; w.ze = (char*)base + z1; }
    return w;
}
// the size entry, forward and backward
int cortex_geometry(const dwn_cortex_args* a) {
    if (a->B <= 0 || a->T <= 0 || a->Cin <= 0 || a->C <= 0 || a->groups <= 0) return dwn_set_error(-2, "cortex: B, T, Cin, C, groups must be positive");
    if (a->Cin % (8ll * a->groups) || a->C % (8ll * a->groups)) return dwn_set_error(-2, "cortex: channels per group must be multiples of 8");
    if (!dtype_ok(a->dtype)) return dwn_set_error(-2, "cortex: dtype must be DWN_F32 or DWN_BF16");
    if (!bn_mode_ok(a->training)) return dwn_set_error(-2, "cortex: training must be DWN_BN_EVAL, DWN_BN_TRAIN or DWN_BN_FROZEN");
    // `M` = B * T rows is an int in both entries and in every launcher behind them
    if (!fits_int({a->B, a->T})) return dwn_set_error(-2, "cortex: B * T must stay below 2^31");
    // `grid` of k_cortex_residual_fwd / _bwd_dy / _bwd_dx: one workgroup per 256 of the M * C (M * Cin) elements, a grid dimension
    const i64 n = (i64)a->B * a->T * (a->C > a->Cin ? a->C : a->Cin);
    if ((n + 255) / 256 > INT_LIMIT) return dwn_set_error(-2, "cortex: B * T * max(C, Cin) / 256 workgroups must stay below 2^31");
    return 0;
}
}  // namespace

size_t dwn_cortex_workspace_bytes(const dwn_cortex_args* a, int backward) {
    WS_BYTES_OR_0(a, cortex_geometry, carve_cortex(*a, backward, nullptr, 0).bytes);
}
int dwn_cortex_forward(const dwn_cortex_args* ap, int device, void* stream) {
    ARGS(ap, "cortex_forward");
    const dwn_cortex_args& a = *ap;
    TRY(cortex_geometry(ap));
    if (!a.x || !a.out || !a.y || !a.w || !a.bn.coef || !a.bnsc.coef || !a.ws)
        return dwn_set_error(-1, "cortex_forward: null pointer (x, out, y, w, bn.coef, bnsc.coef, ws)");
    CortexWs w = carve_cortex(a, 0, a.ws, a.ws_bytes);
    if (w.bytes > a.ws_bytes) return dwn_set_error(-6, "cortex_forward: workspace too small");
    // tr: the training path's products (DWN_BN_TRAIN / _FROZEN); bs: batch statistics.  Frozen: coefficients in the prep launch
    const int M = a.B * a.T, Kg = a.Cin / a.groups, Ng = a.C / a.groups, dt = a.dtype, tr = a.training != DWN_BN_EVAL;
    const bool bs = a.training == DWN_BN_TRAIN;
    PrepArgs pa;
    {
        bool ok = pa.zero(w.zb, ((size_t)(w.ze - w.zb) + 15) & ~(size_t)15);
        ok = ok && pa.packw(a.w, w.wp, 1, a.C, Kg, 0, a.C, Kg);
        if (tr && !bs) ok = ok && pa.bneval(a.bn, a.C, a.eps) && pa.bneval(a.bnsc, a.C, a.eps);
        if (!ok) return dwn_set_error(-2, "cortex_forward: workspace arena must be 16-byte aligned");
    }
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    TRY(k_prep(pa, dt, s));
    GemmNN g = nn_base(ld_plain(a.x, a.Cin), LD_PLAIN, w.wp, Kg, a.y, a.C, M, Ng, Kg, a.groups);
    g.f32_split = f32_split_of(a.f32_products, !tr);
    // (no statistics epilogue: the batch statistics are summed in double by k_cortex_stats below, frozen statistics need none)
    PROF(DWN_FAM_CORTEX_FWD, launch_gemm_nn(g, dt, s));
    if (bs) {
        TRY(k_cortex_stats(a.y, a.x, M, a.Cin, a.C, w.st, w.stsc, dt, s));
        TRY(k_bn_finalize_train(fin_job(w.st, a.C, (double)M, a.bn, a.C), fin_job(w.stsc, a.Cin, (double)M, a.bnsc, a.C),
                                 a.momentum, a.eps, s));
    } else if (!tr) {
        TRY(bn_finalize(w.st, a.C, (double)M, a.bn, a.C, 0, a.momentum, a.eps, s));
        TRY(bn_finalize(w.stsc, a.Cin, (double)M, a.bnsc, a.C, 0, a.momentum, a.eps, s));
    }
    return k_cortex_residual_fwd(a.y, a.x, a.bn.coef, a.bnsc.coef, a.drop_scale, M, a.T, a.Cin, a.C, a.groups, a.out,
                                 dt, s);
}
int dwn_cortex_backward(const dwn_cortex_args* ap, int device, void* stream) {
    ARGS(ap, "cortex_backward");
    const dwn_cortex_args& a = *ap;
    if (a.training == DWN_BN_EVAL) return dwn_set_error(-7, "cortex_backward: only training-mode and frozen-statistics backward are built");
    TRY(cortex_geometry(ap));
    if (!a.x || !a.y || !a.w || !a.dout || !a.dx || !a.dw || !a.bn.coef || !a.bnsc.coef || !a.ws)
        return dwn_set_error(-1, "cortex_backward: null pointer (x, y, w, dout, dx, dw, bn.coef, bnsc.coef, ws)");
    const bool frozen = a.training == DWN_BN_FROZEN;
    CortexWs w = carve_cortex(a, 1, a.ws, a.ws_bytes);
    if (w.bytes > a.ws_bytes) return dwn_set_error(-6, "cortex_backward: workspace too small");
    const int M = a.B * a.T, Kg = a.Cin / a.groups, Ng = a.C / a.groups, dt = a.dtype;
    PrepArgs pa;
    {
        bool ok = pa.zero(w.zb, ((size_t)(w.ze - w.zb) + 15) & ~(size_t)15);
        ok = ok && pa.packw(a.w, w.wp, a.groups, Ng, Kg, 1, Kg, Ng);       // per group W^T [Kg][Ng]
        // dw is accumulated with atomics by the weight-gradient product: cleared here, in the same launch (as dwn_block_backward
        // clears its dw_*), not by the caller
        ok = ok && pa.zero(a.dw, (size_t)a.C * Kg * sizeof(float));
        if (!ok) return dwn_set_error(-2, "cortex_backward: workspace arena and dw must be 16-byte aligned (C * Cin / groups a multiple of 4)");
    }
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    TRY(k_prep(pa, dt, s));
    TRY(k_cortex_bwd_reduce(a.y, a.x, a.dout, a.dout_mask, a.dout_mask_ld, a.bn.coef, a.bnsc.coef, a.drop_scale, M, a.T,
                            a.Cin, a.C, a.groups, w.st, w.stsc, dt, s));
    TRY(k_bn_bwd_finalize(bwd_job(w.st, (double)M, a.bn, w.abc, a.C, frozen), bwd_job(w.stsc, (double)M, a.bnsc, w.abcsc, a.C, frozen), s));
    TRY(k_cortex_bwd_dy(a.y, a.dout, a.dout_mask, a.dout_mask_ld, a.bn.coef, w.abc, a.drop_scale, M, a.T, a.C, a.groups,
                        w.dy, dt, s));
    {
        GemmNN g = nn_base(ld_plain(w.dy, a.C), LD_PLAIN, w.wp, Ng, w.dxmain, a.Cin, M, Kg, Ng, a.groups);
        PROF(DWN_FAM_CORTEX_BWD, launch_gemm_nn(g, dt, s));
    }
    {
        GemmTN g = tn_base(ld_plain(w.dy, a.C), LD_PLAIN, ld_plain(a.x, a.Cin), LD_PLAIN, M, Ng, Kg, a.dw, Kg, a.groups);
        PROF(DWN_FAM_CORTEX_BWD, launch_gemm_tn(g, dt, s));
    }
    return k_cortex_bwd_dx(w.dxmain, a.x, a.dout, a.dout_mask, a.dout_mask_ld, w.abcsc, M, a.T, a.Cin, a.C, a.dx, dt, s);
}

// ------------------------------------------------------------------------------------------------ readout
namespace {
struct ReadoutWs { void* wp; void* dz; void* xd; double* dbp; size_t bytes; int Npad, Rg, Rp, ldp, ldt; };
ReadoutWs carve_readout(const dwn_readout_args& a, int backward, void* base, size_t cap) {
    ReadoutWs w; memset(&w, 0, sizeof(w));
    Carver c(base, cap);
    const size_t ts = tsize(a.dtype);
    const i64 M = (i64)a.B * a.T;
    w.Npad = (a.n_out + a.groups - 1) / a.groups * a.groups;
    w.Rg = w.Npad / a.groups;
    w.Rp = (w.Rg + 63) / 64 * 64;      // the data-gradient product contracts over Rp: whole k-tiles (LDS-DMA variant)
    const int Kg = a.Cin / a.groups;
    w.ldp = Kg; w.ldt = w.Rp;          // (row padding of 8 / 64 / 72 elements measured: no effect, so none)
    w.wp = c.take<char>(backward ? (a.wt ? 0 : (size_t)a.groups * Kg * w.ldt * ts) : (size_t)w.Npad * w.ldp * ts);
    if (backward) w.dz = c.take<char>((size_t)M * a.groups * w.Rp * ts);
    if (a.drop_mask) w.xd = c.take<char>((size_t)M * a.Cin * ts);      // x * dropout mask, materialised once
    if (backward && a.beta_dev) w.dbp = c.take<double>(k_readout_dbeta_parts(a.B, w.Rp, a.groups));   // dbeta: one partial per workgroup
    w.bytes = c.off + 256;
    return w;
}
// the two size entries, forward and backward
int readout_geometry(const dwn_readout_args* a) {
    if (a->B <= 0 || a->T <= 0 || a->Cin <= 0 || a->groups <= 0 || a->n_out <= 0) return dwn_set_error(-2, "readout: B, T, Cin, groups, n_out must be positive");
    if (a->Cin % (8ll * a->groups)) return dwn_set_error(-2, "readout: in-channels per group must be a multiple of 8");
    if (!dtype_ok(a->dtype)) return dwn_set_error(-2, "readout: dtype must be DWN_F32 or DWN_BF16");
    // `M` = B * T rows is an int in both entries and in the GEMMs behind them
    if (!fits_int({a->B, a->T})) return dwn_set_error(-2, "readout: B * T must stay below 2^31");
    // ReadoutWs::Npad, Rg, Rp and the `groups * Rp + 63` of k_readout_dbeta_parts are ints: the last one is the largest
    const i64 rg = ((i64)a->n_out + a->groups - 1) / a->groups, rp = (rg + 63) / 64 * 64;
    if (a->groups * rp + 63 > INT_LIMIT) return dwn_set_error(-2, "readout: groups * (neurons per group, padded to 64) must stay below 2^31 - 63");
    // `a.groups * w.Rg * Kg`, the weight gradient's element count (k_fill_f32's n), is an int
    if (a->groups * rg * (a->Cin / a->groups) > INT_LIMIT) return dwn_set_error(-2, "readout: the padded weight [Npad][Cin / groups] must stay below 2^31 elements");
    return 0;
}
}  // namespace

size_t dwn_readout_workspace_bytes(const dwn_readout_args* a, int backward) {
    WS_BYTES_OR_0(a, readout_geometry, carve_readout(*a, backward, nullptr, 0).bytes);
}
size_t dwn_readout_wt_bytes(const dwn_readout_args* a) {
    WS_BYTES_OR_0(a, readout_geometry, (size_t)a->Cin * carve_readout(*a, 0, nullptr, 0).ldt * tsize(a->dtype));
}
int dwn_readout_forward(const dwn_readout_args* ap, int device, void* stream) {
    ARGS(ap, "readout_forward");
    const dwn_readout_args& a = *ap;
    TRY(readout_geometry(ap));
    if (!a.x || !a.w || !a.out || !a.ws) return dwn_set_error(-1, "readout_forward: null pointer (x, w, out, ws)");
    ReadoutWs w = carve_readout(a, 0, a.ws, a.ws_bytes);
    if (w.bytes > a.ws_bytes) return dwn_set_error(-6, "readout_forward: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    const int M = a.B * a.T, Kg = a.Cin / a.groups, dt = a.dtype;
    TRY(k_pack_weight_dual(a.w, w.wp, a.wt, a.groups, w.Rg, Kg, w.Rp, w.ldp, w.ldt, dt, s));   // both operand layouts, one read of the weight
    LoadDesc x = ld_plain(a.x, a.Cin);
    const int kind = LD_PLAIN;
    if (a.drop_mask) {
        // Dropout1d (dwiseneuro.py:275): the masked input (8 MB) is materialised once — applying the per-(sample,
        // channel) mask inside the GEMM's operand loader put a dependent mask load in front of every A chunk
        LoadDesc xm = x;
        xm.gate = a.drop_mask; xm.gate_ld = a.Cin; xm.rows_per_sample = a.T;
        TRY(k_ew_apply(xm, LD_GATE, w.xd, a.Cin, M, a.Cin, dt, s));
        x = ld_plain(w.xd, a.Cin);
    }
    GemmNN g = nn_base(x, kind, w.wp, w.ldp, nullptr, 0, M, w.Rg, Kg, a.groups);
    g.epi = EPI_READOUT; g.bias = a.bias; g.sp_beta = a.softplus_beta; g.sp_beta_dev = a.beta_dev; g.out_nct = a.out; g.Tn = a.T; g.n_valid = a.n_out;
    g.f32_split = f32_split_of(a.f32_products, false);            // the caller says (it knows whether this is an inference forward)
    PROF(DWN_FAM_READOUT_FWD, launch_gemm_nn(g, dt, s));
    return 0;
}
int dwn_readout_backward(const dwn_readout_args* ap, int device, void* stream) {
    ARGS(ap, "readout_backward");
    const dwn_readout_args& a = *ap;
    if ((a.beta_dev != nullptr) != (a.dbeta != nullptr))
        return dwn_set_error(-2, "readout_backward: beta_dev and dbeta come together (both null: the fixed softplus_beta)");
    TRY(readout_geometry(ap));
    if (!a.x || !(a.wt || a.w) || !a.out || !a.dout || !a.dx || !a.dw || !a.ws)
        return dwn_set_error(-1, "readout_backward: null pointer (x, w or wt, out, dout, dx, dw, ws)");
    ReadoutWs w = carve_readout(a, 1, a.ws, a.ws_bytes);
    if (w.bytes > a.ws_bytes) return dwn_set_error(-6, "readout_backward: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    const int M = a.B * a.T, Kg = a.Cin / a.groups, dt = a.dtype;
    const void* wt = a.wt;                       // per group W^T [Kg][Rp], zero padded: kept from the forward, or packed now
    if (!wt) { TRY(k_pack_weight_dual(a.w, nullptr, w.wp, a.groups, w.Rg, Kg, w.Rp, w.ldp, w.ldt, dt, s)); wt = w.wp; }
    TRY(k_readout_dz(a.dout, a.out, a.softplus_beta, a.beta_dev, w.dbp, a.dbeta, a.B, a.T, a.n_out, w.Rg, w.Rp, a.groups, w.dz, a.dbias, dt, s));
    LoadDesc dz = ld_plain(w.dz, (i64)a.groups * w.Rp);
    {
        GemmNN g = nn_base(dz, LD_PLAIN, wt, w.ldt, a.dx, a.Cin, M, Kg, w.Rp, a.groups);
        PROF(DWN_FAM_READOUT_BWD, launch_gemm_nn(g, dt, s));
    }
    LoadDesc x = ld_plain(a.x, a.Cin);
    const int kind = LD_PLAIN;
    if (a.drop_mask) {
        LoadDesc xm = x;
        xm.gate = a.drop_mask; xm.gate_ld = a.Cin; xm.rows_per_sample = a.T;
        TRY(k_ew_apply(xm, LD_GATE, w.xd, a.Cin, M, a.Cin, dt, s));      // masked input for the weight gradient
        x = ld_plain(w.xd, a.Cin);
        // grad wrt the un-dropped input: dx *= mask (in place)
        LoadDesc dxm = ld_plain(a.dx, a.Cin);
        dxm.gate = a.drop_mask; dxm.gate_ld = a.Cin; dxm.rows_per_sample = a.T;
        TRY(k_ew_apply(dxm, LD_GATE, a.dx, a.Cin, M, a.Cin, dt, s));
    }
    GemmTN g = tn_base(dz, LD_PLAIN, x, kind, M, w.Rg, Kg, a.dw, Kg, a.groups);
    g.R_load = w.Rp;
    // every element of dw [Npad][Kg] is produced here: written with plain stores when the tiles alone fill the chip (the real
    // readouts: 1984 tiles), zeroed + accumulated otherwise — the caller does not clear dw
    g.overwrite = ((size_t)a.dw & 15) == 0 && ((size_t)a.groups * w.Rg * Kg) % 4 == 0;
    if (!g.overwrite) TRY(k_fill_f32(a.dw, 0.f, a.groups * w.Rg * Kg, s));
    PROF(DWN_FAM_READOUT_BWD, launch_gemm_tn(g, dt, s));
    return 0;
}

// ------------------------------------------------------------------------------------------------ loss / optimizer
int dwn_poisson_loss_forward(const float* pred, const float* target, const float* w, long long per_sample,
                             long long total, float eps, double* loss_acc, int device, void* stream) {
    NEEDS(pred && target && w && loss_acc, "poisson_loss_forward: null pointer (pred, target, w, loss_acc)");
    ENTER(device);
    return k_poisson_fwd(pred, target, w, per_sample, total, eps, loss_acc, (hipStream_t)stream);
}
int dwn_poisson_loss_backward(const float* pred, const float* target, const float* w, const float* gscale,
                              long long per_sample, long long total, float eps, float* dpred, int device,
                              void* stream) {
    NEEDS(pred && target && w && dpred, "poisson_loss_backward: null pointer (pred, target, w, dpred)");      // (gscale is optional)
    ENTER(device);
    return k_poisson_bwd(pred, target, w, gscale, per_sample, total, eps, dpred, (hipStream_t)stream);
}
int dwn_f64_to_f32(const double* src, float* dst, int n, int device, void* stream) {
    NEEDS(src && dst, "f64_to_f32: null pointer (src, dst)");
    ENTER(device);
    return k_f64_to_f32(src, dst, n, (hipStream_t)stream);
}
int dwn_adamw_ema_multi(const dwn_tensor_entry* list, int ntensors, int max_blocks, double lr, double beta1,
                        double beta2, double eps, double weight_decay, long long step, double ema_decay,
                        double grad_scale, int device, void* stream) {
    NEEDS(list || ntensors <= 0, "adamw: null table");
    if (step < 1) return dwn_set_error(-2, "adamw: step must be >= 1");
    ENTER(device);
    const double bc1 = 1.0 - pow(beta1, (double)step);
    const double bc2 = 1.0 - pow(beta2, (double)step);
    return k_adamw_ema(list, ntensors, max_blocks, (float)(1.0 - lr * weight_decay), (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)eps, (float)(lr / bc1), (float)sqrt(bc2), (float)ema_decay,
                       (float)(1.0 - ema_decay), (float)grad_scale, (hipStream_t)stream);
}
int dwn_ema_lerp_multi(const dwn_tensor_entry* list, int ntensors, int max_blocks, double decay, int device,
                       void* stream) {
    NEEDS(list || ntensors <= 0, "ema_lerp: null table");
    ENTER(device);
    return k_ema_lerp(list, ntensors, max_blocks, (float)decay, (float)(1.0 - decay), (hipStream_t)stream);
}

// ---- guarded step: the argument checks need no device
size_t dwn_grad_guard_workspace_bytes(int ntensors, int max_blocks) {
    if (ntensors < 0 || max_blocks < 1) return 0;
    const size_t nseg = ntensors == 0 ? 1 : ((size_t)ntensors + DWN_GS_SEG - 1) / DWN_GS_SEG;
    return nseg * (size_t)max_blocks * 16;
}
int dwn_grad_sumsq_multi(const dwn_guarded_entry* list, int ntensors, int max_blocks, double grad_scale, void* ws,
                         size_t ws_bytes, double* pair, int device, void* stream) {
    g_err[0] = 0;
    if (ntensors < 0) return dwn_set_error(-2, "grad_sumsq_multi: ntensors < 0");
    if (max_blocks < 1 || max_blocks > 65536) return dwn_set_error(-2, "grad_sumsq_multi: 1 <= max_blocks <= 65536");
    if (!list && ntensors > 0) return dwn_set_error(-1, "grad_sumsq_multi: null table");
    if (!ws || !pair) return dwn_set_error(-1, "grad_sumsq_multi: null pointer (ws, pair)");
    if (((size_t)ws & 15) || ((size_t)pair & 7)) return dwn_set_error(-2, "grad_sumsq_multi: ws 16-byte, pair 8-byte aligned");
    if (ws_bytes < dwn_grad_guard_workspace_bytes(ntensors, max_blocks)) return dwn_set_error(-6, "grad_sumsq_multi: workspace too small");
    ENTER(device);
    return k_grad_sumsq(list, ntensors, max_blocks, grad_scale, ws, pair, (hipStream_t)stream);
}
int dwn_step_guard_finalize(const double* pair_a, const double* pair_b, double max_norm, int skip_nonfinite,
                            const dwn_guarded_entry* list, int ntensors, dwn_step_guard* guard, int device, void* stream) {
    g_err[0] = 0;
    if (ntensors < 0) return dwn_set_error(-2, "step_guard_finalize: ntensors < 0");
    if (!guard) return dwn_set_error(-1, "step_guard_finalize: null guard");
    if (!pair_a) return dwn_set_error(-1, "step_guard_finalize: null pair_a");
    if (!list && ntensors > 0) return dwn_set_error(-1, "step_guard_finalize: null table");
    if (!(max_norm == max_norm)) return dwn_set_error(-2, "step_guard_finalize: max_norm is NaN");
    ENTER(device);
    return k_step_guard_finalize(pair_a, pair_b, max_norm, skip_nonfinite ? 1 : 0, list, ntensors, guard, (hipStream_t)stream);
}
int dwn_adamw_ema_multi_guarded(const dwn_guarded_entry* list, int ntensors, int max_blocks, double lr, double beta1,
                                double beta2, double eps, double weight_decay, double ema_decay, double grad_scale,
                                const dwn_step_guard* guard, int device, void* stream) {
    g_err[0] = 0;
    if (ntensors < 0) return dwn_set_error(-2, "adamw_ema_multi_guarded: ntensors < 0");
    if (max_blocks < 1 || max_blocks > 65535 || ntensors > 65535)
        return dwn_set_error(-2, "adamw_ema_multi_guarded: max_blocks and ntensors are grid dimensions (1 <= max_blocks, both <= 65535)");
    if (!list && ntensors > 0) return dwn_set_error(-1, "adamw_ema_multi_guarded: null table");
    if (!guard) return dwn_set_error(-1, "adamw_ema_multi_guarded: null guard");
    ENTER(device);
    return k_adamw_ema_guarded(list, ntensors, max_blocks, lr, beta1, beta2, eps, weight_decay, ema_decay, grad_scale, guard,
                               (hipStream_t)stream);
}

int dwn_pw_bwd_fused_supported(int dtype, long long M, int E, int Cin) {
    return pw_bwd_fused_supported(dtype, M, E, Cin) ? 1 : 0;
}
static size_t pw_ws_bytes(int E, int Cin, int dtype) {
    return (size_t)Cin * ((size_t)E + Cin) * tsize(dtype) + 256 + (pw_fold_floats(Cin) + pw_wgrad_tacc_floats(E, Cin)) * sizeof(float) + 256;
}
size_t dwn_pw_backward_workspace_bytes(int E, int Cin, int dtype) {      // 0 for widths or a dtype dwn_pw_backward refuses
    return E > 0 && Cin > 0 && E % 8 == 0 && Cin % 8 == 0 && dtype_ok(dtype) ? pw_ws_bytes(E, Cin, dtype) : 0;
}
int dwn_pw_backward(const dwn_pw_bwd_args* a, int dtype, int device, void* stream) {
    ARGS(a, "pw_backward");
    if (a->E <= 0 || a->Cin <= 0 || a->E % 8 || a->Cin % 8 || a->M <= 0 || a->M > 0x7fffffffLL)
        return dwn_set_error(-2, "pw_backward: E and Cin must be positive multiples of 8, 0 < M < 2^31");
    if (!dtype_ok(dtype)) return dwn_set_error(-2, "pw_backward: dtype must be DWN_F32 or DWN_BF16");
    if (a->res && (!a->res_abc || a->res_C % a->Cin || a->res_C / a->Cin < 1 || a->res_C / a->Cin > 2))
        return dwn_set_error(-2, "pw_backward: the shortcut term needs res_abc and res_C in {Cin, 2 Cin}");
    if (a->res && !pw_bwd_fused_supported(dtype, a->M, a->E, a->Cin))
        return dwn_set_error(-3, "pw_backward: the shortcut term is built into the one-pass kernel only (dwn_pw_bwd_fused_supported)");
    if (!a->dh1 || !a->a0 || !a->w_pw || !a->abc || !a->da0 || !a->dw || !a->ws)
        return dwn_set_error(-1, "pw_backward: null pointer (dh1, a0, w_pw, abc, da0, dw, ws)");
    if (a->ws_bytes < pw_ws_bytes(a->E, a->Cin, dtype)) return dwn_set_error(-6, "pw_backward: workspace too small");
    ENTER(device);
    hipStream_t s = (hipStream_t)stream;
    Carver c(a->ws, a->ws_bytes);
    void* bp = c.take<char>((size_t)a->Cin * (a->E + a->Cin) * tsize(dtype));
    const size_t nz = pw_fold_floats(a->Cin) + pw_wgrad_tacc_floats(a->E, a->Cin);
    float* gacc = c.take<float>(nz);
    float* r3 = gacc + (size_t)a->Cin * a->Cin;
    float* tacc = gacc + pw_fold_floats(a->Cin);
    TRY(k_zero(gacc, nz * sizeof(float), s));
    ResGeom rg; memset(&rg, 0, sizeof(rg));
    rg.hinv = a->res_hinv; rg.winv = a->res_winv; rg.Hin = a->res_Hin; rg.Win = a->res_Win; rg.Hout = a->res_Hout; rg.Wout = a->res_Wout;
    return pw_backward(dtype, a->dh1, a->a0, a->w_pw, a->abc, a->E, a->Cin, a->M, bp, gacc, r3, tacc, a->da0, a->dw, a->res,
                       a->res_abc, a->res_C, a->res_hinv ? &rg : nullptr, s);
}

int dwn_assemble_inputs(const dwn_clip_desc* descs, int B, int T, int H0, int W0, int H, int W, float pad_fill,
                        float* x, int device, void* stream) {
    NEEDS(descs && x, "assemble_inputs: null pointer (descs, x)");
    if (B <= 0 || T <= 0 || H0 <= 0 || W0 <= 0) return dwn_set_error(-2, "assemble_inputs: B, T, H0, W0 must be positive");
    if (H < H0 || W < W0) return dwn_set_error(-2, "assemble_inputs: output frame smaller than the video");
    ENTER(device);
    return k_assemble_inputs(descs, B, T, H0, W0, H, W, pad_fill, x, (hipStream_t)stream);
}

int dwn_assemble_targets(const dwn_clip_desc* descs, int B, int T, float* const* targets, const int* n_neurons,
                         int n_mice, int max_neurons, float* mice_weights, int device, void* stream) {
    NEEDS(descs && targets && n_neurons && mice_weights, "assemble_targets: null pointer (descs, targets, n_neurons, mice_weights)");
    if (B <= 0 || T <= 0 || n_mice <= 0 || max_neurons <= 0)
        return dwn_set_error(-2, "assemble_targets: B, T, n_mice, max_neurons must be positive");
    if (B > 65535 || n_mice > 65535) return dwn_set_error(-2, "assemble_targets: B and n_mice are grid dimensions (<= 65535)");
    ENTER(device);
    return k_assemble_targets(descs, B, T, targets, n_neurons, n_mice, max_neurons, mice_weights, (hipStream_t)stream);
}

// ---- the analysis entries below share one video-plane check
// One plane of a [B][Cin][T][H][W] video, the channels [c, c + nc) and a window in it.  `parts` picks what is checked, always in
// this order: the plane (sizes, channels, counts), the window, the cell, the per-clip element bounds of the MEI entries.
enum { PL_PLANE = 1, PL_WINDOW = 2, PL_EMPTY_OK = 4, PL_CELL = 8, PL_CLIP = 16 };      // PL_EMPTY_OK: wh == ww == 0 at 0, 0 is the whole plane
struct PlaneArgs { int B, Cin, T, H, W, c, nc; const char* chan; int y0, x0, wh, ww, cell; };
static int plane_check(const char* who, unsigned parts, const PlaneArgs& p) {
    const char* bad = nullptr;
    const long long HW = (long long)p.H * p.W;
    if (parts & PL_PLANE) {
        if (p.B <= 0 || p.Cin <= 0 || p.T <= 0 || p.H <= 0 || p.W <= 0) bad = "B, Cin, T, H, W must be positive";
        else if (p.nc <= 0 || p.c < 0 || p.c >= p.Cin || p.nc > p.Cin - p.c) bad = p.chan;
        else if (HW > (1ll << 30) || (long long)p.B * p.Cin * p.T >= (1ll << 31)) bad = "more than 2^30 pixels per plane or 2^31 planes";
    }
    if (!bad && (parts & PL_WINDOW)) {
        if ((parts & PL_EMPTY_OK) && p.wh == 0 && p.ww == 0) {
            if (p.y0 != 0 || p.x0 != 0) bad = "window not inside the plane (an empty window must start at 0, 0)";
        } else if (p.y0 < 0 || p.x0 < 0 || p.wh <= 0 || p.ww <= 0 || p.wh > p.H - p.y0 || p.ww > p.W - p.x0) {
            bad = "window not inside the plane";
        }
    }
    if (!bad && (parts & PL_CELL) && (p.cell < 1 || p.wh % p.cell || p.ww % p.cell)) bad = "cell must be positive and divide both window sides";
    // one clip's window elements are indexed by an int, and every grid stays below 2^31 workgroups
    if (!bad && (parts & PL_CLIP) && (p.T * HW > (1ll << 30) || (long long)p.B * p.T * HW / 64 >= (1ll << 31))) bad = "more than 2^30 elements per clip or 2^37 in all";
    if (!bad) return 0;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %s", who, bad);
    return dwn_set_error(-2, msg);
}

// ---- gaze shifter
static int gaze_geometry(const dwn_gaze_args* a) {
    return plane_check("gaze_shift", PL_PLANE, {a->B, a->Cin, a->T, a->H, a->W, a->video_channel, 1, "video_channel outside [0, Cin)"});
}
int dwn_gaze_shift_forward(const dwn_gaze_args* a, int device, void* stream) {
    ARGS(a, "gaze_shift_forward");
    TRY(gaze_geometry(a));
    if (!a->x || !a->shift || !a->out) return dwn_set_error(-1, "gaze_shift_forward: null pointer (x, shift, out)");
    ENTER(device);
    return k_gaze_forward(*a, (hipStream_t)stream);
}
int dwn_gaze_shift_backward(const dwn_gaze_args* a, int device, void* stream) {
    ARGS(a, "gaze_shift_backward");
    TRY(gaze_geometry(a));
    if (!a->dx && !a->dshift) return dwn_set_error(-1, "gaze_shift_backward: dx and dshift are both null");
    if (!a->shift || !a->dout) return dwn_set_error(-1, "gaze_shift_backward: null pointer (shift, dout)");
    if (a->dshift && !a->x) return dwn_set_error(-1, "gaze_shift_backward: dshift needs x");
    ENTER(device);
    return k_gaze_backward(*a, (hipStream_t)stream);
}
int dwn_plane_mean(const float* x, int B, int Cin, int T, int H, int W, int c0, int nc, float* mean, int device, void* stream) {
    g_err[0] = 0;
    if (!x || !mean) return dwn_set_error(-1, "plane_mean: null pointer (x, mean)");
    TRY(plane_check("plane_mean", PL_PLANE, {B, Cin, T, H, W, c0, nc, "channels [c0, c0 + nc) outside [0, Cin)"}));
    ENTER(device);
    return k_plane_mean(x, B, Cin, T, H, W, c0, nc, mean, (hipStream_t)stream);
}

// ---- correlation objective: the argument checks need no device
static int corr_geometry(const dwn_corr_args* a) {
    if (a->B <= 0 || a->N <= 0 || a->T <= 0) return dwn_set_error(-2, "corr: B, N, T must be positive");
    if ((long long)a->N * a->T > (1ll << 31) - 4096) return dwn_set_error(-2, "corr: N * T must stay below 2^31 - 4096");
    if (a->w_stride < 1) return dwn_set_error(-2, "corr: w_stride must be at least 1");
    if (!(a->eps > 0.0)) return dwn_set_error(-2, "corr: eps must be positive");
    if (a->reduction != DWN_CORR_MEAN && a->reduction != DWN_CORR_SUM) return dwn_set_error(-2, "corr: reduction must be DWN_CORR_MEAN or DWN_CORR_SUM");
    return 0;
}
size_t dwn_corr_ws_bytes(const dwn_corr_args* a) { return a && a->N > 0 ? k_corr_ws_bytes(a->N) : 0; }
int dwn_corr_moments(const dwn_corr_args* a, int device, void* stream) {
    ARGS(a, "corr_moments");
    TRY(corr_geometry(a));
    if (!a->pred || !a->target || !a->w || !a->stat || !a->count) return dwn_set_error(-1, "corr_moments: null pointer (pred, target, w, stat, count)");
    ENTER(device);
    return k_corr_moments(*a, (hipStream_t)stream);
}
int dwn_corr_loss_finalize(const dwn_corr_args* a, int device, void* stream) {
    ARGS(a, "corr_loss_finalize");
    TRY(corr_geometry(a));
    if (!a->stat || !a->count || !a->share || !a->loss_acc || !a->ws) return dwn_set_error(-1, "corr_loss_finalize: null pointer (stat, count, share, loss_acc, ws)");
    WS_CHECK(a, -3, "corr_loss_finalize", k_corr_ws_bytes(a->N), "dwn_corr_ws_bytes", 8);
    ENTER(device);
    return k_corr_finalize(*a, (hipStream_t)stream);
}
int dwn_corr_loss_backward(const dwn_corr_args* a, int device, void* stream) {
    ARGS(a, "corr_loss_backward");
    TRY(corr_geometry(a));
    if (!a->pred || !a->target || !a->w || !a->stat || !a->share || !a->dpred) return dwn_set_error(-1, "corr_loss_backward: null pointer (pred, target, w, stat, share, dpred)");
    ENTER(device);
    return k_corr_backward(*a, (hipStream_t)stream);
}

// ---- in-silico stimuli
static int gabor_geometry(const dwn_gabor_args* a) {
    const PlaneArgs p = {a->B, a->Cin, a->T, a->H, a->W, a->video_channel, 1, "video_channel outside [0, Cin)", a->y0, a->x0, a->wh, a->ww};
    TRY(plane_check("gabor", PL_PLANE, p));
    if (a->envelope != DWN_GABOR_GAUSSIAN && a->envelope != DWN_GABOR_NONE) return dwn_set_error(-2, "gabor: envelope must be DWN_GABOR_GAUSSIAN or DWN_GABOR_NONE");
    TRY(plane_check("gabor", PL_WINDOW | PL_EMPTY_OK, p));      // (the envelope answers before the window)
    if (a->clamp != 0 && a->clamp != 1) return dwn_set_error(-2, "gabor: clamp must be 0 or 1");
    if (a->clamp && !(a->lo <= a->hi)) return dwn_set_error(-2, "gabor: video range needs lo <= hi");
    const long long wpix = a->wh ? (long long)a->wh * a->ww : (long long)a->H * a->W;
    if ((long long)a->B * a->T * ((wpix + 1023) / 1024) >= (1ll << 31)) return dwn_set_error(-2, "gabor: more than 2^31 partial sums");
    return 0;
}
size_t dwn_gabor_workspace_bytes(const dwn_gabor_args* a) {
    WS_BYTES_OR_0(a, gabor_geometry, k_gabor_ws_bytes(*a));
}
int dwn_gabor_forward(const dwn_gabor_args* a, int device, void* stream) {
    ARGS(a, "gabor_forward");
    TRY(gabor_geometry(a));
    if (!a->x || !a->params || !a->out) return dwn_set_error(-1, "gabor_forward: null pointer (x, params, out)");
    ENTER(device);
    return k_gabor_forward(*a, (hipStream_t)stream);
}
int dwn_gabor_backward(const dwn_gabor_args* a, int device, void* stream) {
    ARGS(a, "gabor_backward");
    TRY(gabor_geometry(a));
    if (!a->params || !a->dout || !a->dparams || !a->ws) return dwn_set_error(-1, "gabor_backward: null pointer (params, dout, dparams, ws)");
    WS_CHECK(a, -3, "gabor_backward", k_gabor_ws_bytes(*a), "dwn_gabor_workspace_bytes", 8);
    ENTER(device);
    return k_gabor_backward(*a, (hipStream_t)stream);
}

// ---- behaviour modulator: the argument checks need no device
static int modulator_geometry(const dwn_modulator_args* a) {
    if (a->B <= 0 || a->N <= 0 || a->T <= 0) return dwn_set_error(-2, "modulator: B, N, T must be positive");
    if (a->K < 1 || a->K > 32) return dwn_set_error(-2, "modulator: K outside [1, 32]");
    if (!(a->max_log_gain > 0.f) || !(a->max_log_gain <= 3.402823466e38f)) return dwn_set_error(-2, "modulator: max_log_gain must be finite and positive");
    // the grids are one workgroup per (128 neurons, 64 frames, sample): keep them and the partial counts below 2^31
    const long long tiles = ((long long)a->N + 127) / 128 * (((long long)a->T + 63) / 64) * a->B;
    if (tiles >= (1ll << 31) || (long long)a->B * a->T * a->K >= (1ll << 31) || (long long)a->N * a->K >= (1ll << 31))
        return dwn_set_error(-2, "modulator: more than 2^31 tiles, behaviour features or weights");
    return 0;
}
size_t dwn_modulator_ws_bytes(const dwn_modulator_args* a) {
    WS_BYTES_OR_0(a, modulator_geometry, k_modulator_ws_bytes(*a));
}
int dwn_modulator_forward(const dwn_modulator_args* a, int device, void* stream) {
    ARGS(a, "modulator_forward");
    TRY(modulator_geometry(a));
    if (!a->y || !a->h || !a->u || !a->c || !a->out) return dwn_set_error(-1, "modulator_forward: null pointer (y, h, u, c, out)");
    if (a->out == a->y) return dwn_set_error(-2, "modulator_forward: out must not alias y");
    ENTER(device);
    return k_modulator_forward(*a, (hipStream_t)stream);
}
int dwn_modulator_backward(const dwn_modulator_args* a, int device, void* stream) {
    ARGS(a, "modulator_backward");
    TRY(modulator_geometry(a));
    if (!a->y || !a->h || !a->u || !a->c || !a->dout) return dwn_set_error(-1, "modulator_backward: null pointer (y, h, u, c, dout)");
    if (!a->dy && !a->dh && !a->du && !a->dc) return dwn_set_error(-1, "modulator_backward: dy, dh, du and dc are all null");
    if (!a->ws) return dwn_set_error(-1, "modulator_backward: null pointer (ws)");
    WS_CHECK(a, -2, "modulator_backward", k_modulator_ws_bytes(*a), "dwn_modulator_ws_bytes", 8);
    ENTER(device);
    return k_modulator_backward(*a, (hipStream_t)stream);
}

// ---- regularised MEI synthesis
static int mei_plane(const char* who, int B, int Cin, int T, int H, int W, int c, int y0, int x0, int wh, int ww) {
    return plane_check(who, PL_PLANE | PL_WINDOW | PL_EMPTY_OK | PL_CLIP, {B, Cin, T, H, W, c, 1, "channel outside [0, Cin)", y0, x0, wh, ww});
}
static int blur3d_geometry(const dwn_blur3d_args* a) {
    TRY(mei_plane("blur3d", a->B, a->Cin_src, a->T, a->H, a->W, a->c_src, a->y0, a->x0, a->wh, a->ww));
    TRY(mei_plane("blur3d", a->B, a->Cin_dst, a->T, a->H, a->W, a->c_dst, a->y0, a->x0, a->wh, a->ww));
    if (a->Rt < 0 || a->Rh < 0 || a->Rw < 0 || a->Rt > DWN_BLUR_MAX_RADIUS || a->Rh > DWN_BLUR_MAX_RADIUS || a->Rw > DWN_BLUR_MAX_RADIUS)
        return dwn_set_error(-2, "blur3d: radius outside [0, DWN_BLUR_MAX_RADIUS]");
    return 0;
}
static int moments_geometry(const dwn_clip_moments_args* a) {
    return mei_plane("clip_moments", a->B, a->Cin, a->T, a->H, a->W, a->c, a->y0, a->x0, a->wh, a->ww);
}
size_t dwn_blur3d_ws_bytes(const dwn_blur3d_args* a) {
    WS_BYTES_OR_0(a, blur3d_geometry, k_blur3d_ws_bytes(*a));
}
size_t dwn_clip_moments_ws_bytes(const dwn_clip_moments_args* a) {
    WS_BYTES_OR_0(a, moments_geometry, k_clip_moments_ws_bytes(*a));
}
int dwn_blur3d(const dwn_blur3d_args* a, int device, void* stream) {
    ARGS(a, "blur3d");
    TRY(blur3d_geometry(a));
    if (!a->src || !a->dst || !a->taps || !a->ws) return dwn_set_error(-1, "blur3d: null pointer (src, dst, taps, ws)");
    WS_CHECK(a, -3, "blur3d", k_blur3d_ws_bytes(*a), "dwn_blur3d_ws_bytes", 4);
    ENTER(device);
    return k_blur3d(*a, (hipStream_t)stream);
}
int dwn_clip_moments(const dwn_clip_moments_args* a, int device, void* stream) {
    ARGS(a, "clip_moments");
    TRY(moments_geometry(a));
    if (!a->x || !a->stat || !a->ws) return dwn_set_error(-1, "clip_moments: null pointer (x, stat, ws)");
    WS_CHECK(a, -3, "clip_moments", k_clip_moments_ws_bytes(*a), "dwn_clip_moments_ws_bytes", 8);
    ENTER(device);
    return k_clip_moments(*a, (hipStream_t)stream);
}
int dwn_mei_update(const dwn_mei_update_args* a, int device, void* stream) {
    ARGS(a, "mei_update");
    if (a->mode != DWN_MEI_STEP && a->mode != DWN_MEI_PROJECT) return dwn_set_error(-2, "mei_update: mode must be DWN_MEI_STEP or DWN_MEI_PROJECT");
    TRY(mei_plane("mei_update", a->B, a->Cin, a->T, a->H, a->W, a->c, a->y0, a->x0, a->wh, a->ww));
    if (a->mode == DWN_MEI_STEP) {
        TRY(mei_plane("mei_update", a->B, a->Cin_g, a->T, a->H, a->W, a->c_g, a->y0, a->x0, a->wh, a->ww));
        if (!a->x || !a->g || !a->stat || !a->lr) return dwn_set_error(-1, "mei_update: null pointer (x, g, stat, lr)");
    } else {
        if (!(a->lo <= a->hi)) return dwn_set_error(-2, "mei_update: video range needs lo <= hi");
        if (a->has_contrast && a->contrast_mode != DWN_MEI_CONTRAST_MAX && a->contrast_mode != DWN_MEI_CONTRAST_FIXED)
            return dwn_set_error(-2, "mei_update: contrast_mode must be DWN_MEI_CONTRAST_MAX or DWN_MEI_CONTRAST_FIXED");
        if (a->has_contrast && !(a->contrast >= 0.0 && a->contrast <= 1.7976931348623157e308)) return dwn_set_error(-2, "mei_update: contrast must be finite and not negative");
        if (a->has_mean && !(a->mean_target >= -1.7976931348623157e308 && a->mean_target <= 1.7976931348623157e308)) return dwn_set_error(-2, "mei_update: mean_target must be finite");
        if (!a->x || !a->stat) return dwn_set_error(-1, "mei_update: null pointer (x, stat)");
    }
    if ((size_t)a->stat & 7) return dwn_set_error(-2, "mei_update: stat must be 8-byte aligned");
    ENTER(device);
    return k_mei_update(*a, (hipStream_t)stream);
}

// ---- trial-level evaluation: the argument checks need no device
static int trial_counts(const dwn_trial_score_args* a) {
    if (a->N <= 0) return dwn_set_error(-2, "trial_score: N must be positive");
    if (a->n_all < 0 || a->n_repeat < 0 || a->n_group_frames < 0) return dwn_set_error(-2, "trial_score: negative count");
    if (a->n_all >= (1ll << 52)) return dwn_set_error(-2, "trial_score: n_all must stay below 2^52");
    // a repeat group adds R K to n_all and n_repeat and K to n_group_frames, R >= 2
    if (a->n_repeat > a->n_all || 2 * a->n_group_frames > a->n_repeat || (a->n_repeat > 0) != (a->n_group_frames > 0))
        return dwn_set_error(-2, "trial_score: counts contradict each other (n_repeat <= n_all, 2 n_group_frames <= n_repeat)");
    return 0;
}
size_t dwn_trial_score_ws_bytes(const dwn_trial_score_args* a) { return a && a->N > 0 ? k_trial_score_ws_bytes(a->N) : 0; }
int dwn_trial_moments(const dwn_trial_score_args* a, int device, void* stream) {
    ARGS(a, "trial_moments");
    TRY(trial_counts(a));
    if (a->n_trials <= 0 || a->n_groups <= 0 || a->n_groups > a->n_trials) return dwn_set_error(-2, "trial_moments: needs 1 <= n_groups <= n_trials");
    if (a->max_repeats < 1 || a->max_repeats > a->n_trials) return dwn_set_error(-2, "trial_moments: max_repeats must lie in [1, n_trials]");
    if (a->max_frames < 1) return dwn_set_error(-2, "trial_moments: max_frames must be positive");
    if ((long long)a->n_trials * a->max_frames >= (1ll << 52) - a->n_all) return dwn_set_error(-2, "trial_moments: the counts after the launch must stay below 2^52");
    if (!a->trials || !a->groups || !a->state) return dwn_set_error(-1, "trial_moments: null pointer (trials, groups, state)");
    if ((size_t)a->state & 7) return dwn_set_error(-2, "trial_moments: state must be 8-byte aligned");
    ENTER(device);
    return k_trial_moments(*a, (hipStream_t)stream);
}
int dwn_trial_score_finalize(const dwn_trial_score_args* a, int device, void* stream) {
    ARGS(a, "trial_score_finalize");
    TRY(trial_counts(a));
    if (!(a->eps > 0.0)) return dwn_set_error(-2, "trial_score_finalize: eps must be positive");
    if (a->fev_threshold != a->fev_threshold) return dwn_set_error(-2, "trial_score_finalize: fev_threshold is NaN");
    if (!a->state || !a->scores || !a->summary || !a->ws) return dwn_set_error(-1, "trial_score_finalize: null pointer (state, scores, summary, ws)");
    if (((size_t)a->state & 7) || ((size_t)a->scores & 7) || ((size_t)a->summary & 7)) return dwn_set_error(-2, "trial_score_finalize: state, scores and summary must be 8-byte aligned");
    WS_CHECK(a, -3, "trial_score_finalize", k_trial_score_ws_bytes(a->N), "dwn_trial_score_ws_bytes", 8);
    ENTER(device);
    return k_trial_score_finalize(*a, (hipStream_t)stream);
}

// ---- population structure: the argument checks need no device
static int pair_state(const dwn_pair_args* a, const char* who) {
    static char msg[96];
    const char* what = nullptr;
    if (a->N <= 0 || a->N > 65535) what = "N outside [1, 65535]";
    else if (a->n < 0 || a->n >= (1ll << 52)) what = "the sample count must lie in [0, 2^52)";
    if (!what) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return dwn_set_error(-2, msg);
}
static bool pair_cols_ok(const dwn_pair_args* a) { return a->cols > 0 && a->cols % DWN_PAIR_KSTEP == 0; }
long long dwn_pair_ldz(int N) { return N > 0 && N <= 65535 ? k_pair_ldz(N) : 0; }
size_t dwn_pair_state_bytes(const dwn_pair_args* a) {
    return a && a->N > 0 && a->N <= 65535 ? ((size_t)a->N * a->N + (size_t)a->N) * sizeof(double) : 0;
}
size_t dwn_pair_ws_bytes(const dwn_pair_args* a) {
    return a && a->N > 0 && a->N <= 65535 && pair_cols_ok(a) ? (size_t)a->cols * (size_t)k_pair_ldz(a->N) * sizeof(double) : 0;
}
size_t dwn_pair_compare_ws_bytes(const dwn_pair_compare_args* a) {
    if (!a || a->N <= 0 || a->N > 65535 || a->M < 1 || a->M > (1 << 20) || (!a->sel && a->M > a->N)) return 0;
    return k_pair_compare_ws_bytes(a->M);
}
int dwn_pair_stage(const dwn_pair_args* a, int device, void* stream) {
    ARGS(a, "pair_stage");
    TRY(pair_state(a, "pair_stage"));
    if (a->kind != DWN_PAIR_TOTAL && a->kind != DWN_PAIR_SIGNAL && a->kind != DWN_PAIR_NOISE) return dwn_set_error(-2, "pair_stage: unknown kind");
    if (a->n_segs <= 0 || a->n_groups <= 0 || a->n_groups > a->n_segs) return dwn_set_error(-2, "pair_stage: needs 1 <= n_groups <= n_segs");
    if (a->max_repeats < 1 || a->max_repeats > a->n_segs) return dwn_set_error(-2, "pair_stage: max_repeats must lie in [1, n_segs]");
    if (a->max_frames < 1) return dwn_set_error(-2, "pair_stage: max_frames must be positive");
    if ((long long)a->n_segs * a->max_frames >= (1ll << 52) - a->n) return dwn_set_error(-2, "pair_stage: the count after the launch must stay below 2^52");
    if (!pair_cols_ok(a)) return dwn_set_error(-2, "pair_stage: cols must be a positive multiple of DWN_PAIR_KSTEP");
    if (!a->segs || !a->groups || !a->state || !a->ws) return dwn_set_error(-1, "pair_stage: null pointer (segs, groups, state, ws)");
    if ((size_t)a->state & 7) return dwn_set_error(-2, "pair_stage: state must be 8-byte aligned");
    WS_CHECK(a, -3, "pair_stage", dwn_pair_ws_bytes(a), "dwn_pair_ws_bytes", 16);
    ENTER(device);
    return k_pair_stage(*a, (hipStream_t)stream);
}
int dwn_pair_syrk(const dwn_pair_args* a, int device, void* stream) {
    ARGS(a, "pair_syrk");
    TRY(pair_state(a, "pair_syrk"));
    if (!pair_cols_ok(a)) return dwn_set_error(-2, "pair_syrk: cols must be a positive multiple of DWN_PAIR_KSTEP");
    if (!a->state || !a->ws) return dwn_set_error(-1, "pair_syrk: null pointer (state, ws)");
    if ((size_t)a->state & 7) return dwn_set_error(-2, "pair_syrk: state must be 8-byte aligned");
    WS_CHECK(a, -3, "pair_syrk", dwn_pair_ws_bytes(a), "dwn_pair_ws_bytes", 16);
    ENTER(device);
    return k_pair_syrk(*a, (hipStream_t)stream);
}
int dwn_pair_corr_finalize(const dwn_pair_args* a, int device, void* stream) {
    ARGS(a, "pair_corr_finalize");
    TRY(pair_state(a, "pair_corr_finalize"));
    if (!(a->eps > 0.0)) return dwn_set_error(-2, "pair_corr_finalize: eps must be positive");
    if (!a->state || !a->out) return dwn_set_error(-1, "pair_corr_finalize: null pointer (state, out)");
    if (((size_t)a->state & 7) || ((size_t)a->out & (a->out_f32 ? 3 : 7))) return dwn_set_error(-2, "pair_corr_finalize: state or out misaligned");
    ENTER(device);
    return k_pair_corr_finalize(*a, (hipStream_t)stream);
}
int dwn_pair_compare(const dwn_pair_compare_args* a, int device, void* stream) {
    ARGS(a, "pair_compare");
    if (a->N <= 0 || a->N > 65535) return dwn_set_error(-2, "pair_compare: N outside [1, 65535]");
    if (a->M < 1 || a->M > (1 << 20)) return dwn_set_error(-2, "pair_compare: M outside [1, 2^20]");
    if (!a->sel && a->M > a->N) return dwn_set_error(-2, "pair_compare: without sel M must not exceed N");
    if (a->lda < a->N || a->ldb < a->N) return dwn_set_error(-2, "pair_compare: a leading dimension below N");
    if (!(a->eps > 0.0)) return dwn_set_error(-2, "pair_compare: eps must be positive");
    if (!a->A || !a->B || !a->per_neuron || !a->summary || !a->ws) return dwn_set_error(-1, "pair_compare: null pointer (A, B, per_neuron, summary, ws)");
    if (((size_t)a->A & 7) || ((size_t)a->B & 7) || ((size_t)a->per_neuron & 7) || ((size_t)a->summary & 7) || ((size_t)a->sel & 3))
        return dwn_set_error(-2, "pair_compare: A, B, per_neuron, summary or sel misaligned");
    WS_CHECK(a, -3, "pair_compare", k_pair_compare_ws_bytes(a->M), "dwn_pair_compare_ws_bytes", 8);
    ENTER(device);
    return k_pair_compare(*a, (hipStream_t)stream);
}

// ---- population modes: the argument checks need no device
enum { MO_A = 1, MO_Q = 2, MO_Y = 4, MO_V = 8, MO_K = 16 };
static int pad16i(int p) { return (p + 15) / 16 * 16; }
static const char* modes_geometry(const dwn_modes_args* a, int parts) {
    if (a->N <= 0 || a->N > 65535) return "N outside [1, 65535]";
    if (a->p < 1 || a->p > DWN_MODES_MAXP || a->p > a->N) return "p outside [1, min(N, DWN_MODES_MAXP)]";
    if ((parts & MO_K) && (a->k < 1 || a->k > a->p)) return "k outside [1, p]";
    if ((parts & MO_A) && a->lda < a->N) return "lda below N";
    if ((parts & MO_A) && !(fabs(a->scale) <= 1.7976931348623157e308)) return "scale is not finite";
    if ((parts & MO_Q) && a->ldq < pad16i(a->p)) return "ldq below p rounded up to 16";
    if ((parts & MO_Y) && a->ldy < pad16i(a->p)) return "ldy below p rounded up to 16";
    if ((parts & MO_V) && a->ldv < pad16i(a->p)) return "ldv below p rounded up to 16";
    return nullptr;
}
static int modes_check(const dwn_modes_args* a, int parts, const char* who) {
    static char msg[128];
    const char* what = modes_geometry(a, parts);
    if (!what) return 0;
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return dwn_set_error(-2, msg);
}
static bool modes_aligned(const dwn_modes_args* a) {
    return !(((size_t)a->A | (size_t)a->Q | (size_t)a->Y | (size_t)a->V | (size_t)a->H | (size_t)a->W | (size_t)a->values |
              (size_t)a->residuals | (size_t)a->moments) & 7) && !((size_t)a->status & 3);
}
size_t dwn_modes_moments_ws_bytes(const dwn_modes_args* a) { return a && a->N > 0 && a->N <= 65535 ? k_modes_moments_ws_bytes(a->N) : 0; }
size_t dwn_modes_ritz_ws_bytes(const dwn_modes_args* a) { return a && a->N > 0 && a->N <= 65535 ? k_modes_ritz_ws_bytes(a->N) : 0; }
size_t dwn_modes_solve_ws_bytes(const dwn_modes_args* a) { return a && !modes_geometry(a, 0) ? k_modes_solve_ws_bytes(a->N, a->p) : 0; }
size_t dwn_modes_overlap_ws_bytes(const dwn_modes_args* a) {
    if (!a || a->N <= 0 || a->N > 65535 || a->k < 1 || a->k > DWN_MODES_MAXP || a->k > a->N) return 0;
    return k_modes_overlap_ws_bytes(a->N, a->k, a->A != nullptr);
}
int dwn_modes_symm(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_symm");
    TRY(modes_check(a, MO_A | MO_Q | MO_Y, "modes_symm"));
    if (!a->A || !a->Q || !a->Y) return dwn_set_error(-1, "modes_symm: null pointer (A, Q, Y)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_symm: misaligned pointer");
    ENTER(device);
    return k_modes_symm(*a, (hipStream_t)stream);
}
int dwn_modes_moments(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_moments");
    if (a->N <= 0 || a->N > 65535) return dwn_set_error(-2, "modes_moments: N outside [1, 65535]");
    if (a->lda < a->N) return dwn_set_error(-2, "modes_moments: lda below N");
    if (!(fabs(a->scale) <= 1.7976931348623157e308)) return dwn_set_error(-2, "modes_moments: scale is not finite");
    if (!a->A || !a->moments || !a->ws) return dwn_set_error(-1, "modes_moments: null pointer (A, moments, ws)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_moments: misaligned pointer");
    WS_CHECK(a, -3, "modes_moments", k_modes_moments_ws_bytes(a->N), "dwn_modes_moments_ws_bytes", 16);
    ENTER(device);
    return k_modes_moments(*a, (hipStream_t)stream);
}
int dwn_modes_orth(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_orth");
    TRY(modes_check(a, MO_Q | MO_Y, "modes_orth"));
    if (!a->Q || !a->Y) return dwn_set_error(-1, "modes_orth: null pointer (Q, Y)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_orth: misaligned pointer");
    ENTER(device);
    return k_modes_orth(*a, (hipStream_t)stream);
}
int dwn_modes_small_eigh(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_small_eigh");
    if (a->p < 1 || a->p > DWN_MODES_MAXP) return dwn_set_error(-2, "modes_small_eigh: p outside [1, DWN_MODES_MAXP]");
    if (!a->H || !a->W || !a->values) return dwn_set_error(-1, "modes_small_eigh: null pointer (H, W, values)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_small_eigh: misaligned pointer");
    ENTER(device);
    return k_modes_small_eigh(*a, (hipStream_t)stream);
}
int dwn_modes_ritz(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_ritz");
    TRY(modes_check(a, MO_Q | MO_Y | MO_V | MO_K, "modes_ritz"));
    if (!(a->tol >= 0.0) || !(a->tol <= 1.7976931348623157e308)) return dwn_set_error(-2, "modes_ritz: tol must be finite and not negative");
    if (!a->Q || !a->Y || !a->V || !a->W || !a->values || !a->residuals || !a->status || !a->ws)
        return dwn_set_error(-1, "modes_ritz: null pointer (Q, Y, V, W, values, residuals, status, ws)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_ritz: misaligned pointer");
    WS_CHECK(a, -3, "modes_ritz", k_modes_ritz_ws_bytes(a->N), "dwn_modes_ritz_ws_bytes", 16);
    ENTER(device);
    return k_modes_ritz(*a, (hipStream_t)stream);
}
int dwn_modes_solve(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_solve");
    TRY(modes_check(a, MO_A | MO_V | MO_K, "modes_solve"));
    if (a->max_iters < 1 || a->max_iters > 4096) return dwn_set_error(-2, "modes_solve: max_iters outside [1, 4096]");
    if (!(a->tol >= 0.0) || !(a->tol <= 1.7976931348623157e308)) return dwn_set_error(-2, "modes_solve: tol must be finite and not negative");
    if (!a->A || !a->V || !a->values || !a->residuals || !a->moments || !a->status || !a->ws)
        return dwn_set_error(-1, "modes_solve: null pointer (A, V, values, residuals, moments, status, ws)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_solve: misaligned pointer");
    WS_CHECK(a, -3, "modes_solve", k_modes_solve_ws_bytes(a->N, a->p), "dwn_modes_solve_ws_bytes", 16);
    ENTER(device);
    return k_modes_solve(*a, (hipStream_t)stream);
}
int dwn_modes_overlap(const dwn_modes_args* a, int device, void* stream) {
    ARGS(a, "modes_overlap");
    if (a->N <= 0 || a->N > 65535) return dwn_set_error(-2, "modes_overlap: N outside [1, 65535]");
    if (a->k < 1 || a->k > DWN_MODES_MAXP || a->k > a->N) return dwn_set_error(-2, "modes_overlap: k outside [1, min(N, DWN_MODES_MAXP)]");
    if (a->ldq < pad16i(a->k) || a->ldy < pad16i(a->k)) return dwn_set_error(-2, "modes_overlap: a leading dimension below k rounded up to 16");
    if (a->A && a->lda < a->N) return dwn_set_error(-2, "modes_overlap: lda below N");
    if (a->A && !(fabs(a->scale) <= 1.7976931348623157e308)) return dwn_set_error(-2, "modes_overlap: scale is not finite");
    if (!a->Q || !a->Y || !a->values || !a->ws || (a->A && !a->moments))
        return dwn_set_error(-1, "modes_overlap: null pointer (Q, Y, values, ws; moments with A)");
    if (!modes_aligned(a)) return dwn_set_error(-2, "modes_overlap: misaligned pointer");
    WS_CHECK(a, -3, "modes_overlap", k_modes_overlap_ws_bytes(a->N, a->k, a->A != nullptr), "dwn_modes_overlap_ws_bytes", 16);
    ENTER(device);
    return k_modes_overlap(*a, (hipStream_t)stream);
}

// ---- retinotopic readout gain: the argument checks need no device
static int spatial_gain_geometry(const dwn_spatial_gain_args* a) {
    if (a->B <= 0 || a->N <= 0 || a->T <= 0 || a->Hf <= 0 || a->Wf <= 0) return dwn_set_error(-2, "spatial_gain: B, N, T, Hf, Wf must be positive");
    if (a->K < 1 || a->K > 64) return dwn_set_error(-2, "spatial_gain: K outside [1, 64]");
    if ((long long)a->Hf * a->Wf > 256) return dwn_set_error(-2, "spatial_gain: Hf * Wf above 256");
    if (a->g_dtype != DWN_F32 && a->g_dtype != DWN_BF16) return dwn_set_error(-2, "spatial_gain: g_dtype must be DWN_F32 or DWN_BF16");
    if (!(a->max_log_gain > 0.f) || !(a->max_log_gain <= 3.402823466e38f)) return dwn_set_error(-2, "spatial_gain: max_log_gain must be finite and positive");
    // one workgroup per (128 neurons, 32 frames, sample) and one wave per (sample, cell, 32 frames; bounded here as if 16): keep the grids below 2^31
    const long long tiles = ((long long)a->N + 127) / 128 * (((long long)a->T + 31) / 32) * a->B;
    const long long waves = (long long)a->B * a->Hf * a->Wf * (((long long)a->T + 15) / 16);
    if (tiles >= (1ll << 31) || waves >= (1ll << 31) || (long long)a->N * a->K >= (1ll << 31))
        return dwn_set_error(-2, "spatial_gain: more than 2^31 tiles or weights");
    return 0;
}
size_t dwn_spatial_gain_ws_bytes(const dwn_spatial_gain_args* a) {
    WS_BYTES_OR_0(a, spatial_gain_geometry, k_spatial_gain_ws_bytes(*a));
}
int dwn_spatial_gain_forward(const dwn_spatial_gain_args* a, int device, void* stream) {
    ARGS(a, "spatial_gain_forward");
    TRY(spatial_gain_geometry(a));
    if (!a->y || !a->g || !a->pos || !a->weight || !a->bias || !a->out) return dwn_set_error(-1, "spatial_gain_forward: null pointer (y, g, pos, weight, bias, out)");
    if (a->out == a->y) return dwn_set_error(-2, "spatial_gain_forward: out must not alias y");
    ENTER(device);
    return k_spatial_gain_forward(*a, (hipStream_t)stream);
}
int dwn_spatial_gain_backward(const dwn_spatial_gain_args* a, int device, void* stream) {
    ARGS(a, "spatial_gain_backward");
    TRY(spatial_gain_geometry(a));
    if (!a->y || !a->g || !a->pos || !a->weight || !a->bias || !a->dout) return dwn_set_error(-1, "spatial_gain_backward: null pointer (y, g, pos, weight, bias, dout)");
    if (!a->dy && !a->dg && !a->dpos && !a->dweight && !a->dbias) return dwn_set_error(-1, "spatial_gain_backward: dy, dg, dpos, dweight and dbias are all null");
    if (!a->ws) return dwn_set_error(-1, "spatial_gain_backward: null pointer (ws)");
    WS_CHECK(a, -2, "spatial_gain_backward", k_spatial_gain_ws_bytes(*a), "dwn_spatial_gain_ws_bytes", 16);
    ENTER(device);
    return k_spatial_gain_backward(*a, (hipStream_t)stream);
}

// ---- receptive-field mapping
static int rf_plane(const char* who, int B, int Cin, int T, int H, int W, int c, int y0, int x0, int wh, int ww, int cell) {
    return plane_check(who, PL_PLANE | PL_WINDOW | PL_CELL, {B, Cin, T, H, W, c, 1, "channel outside [0, Cin)", y0, x0, wh, ww, cell});
}
int dwn_noise_forward(const dwn_noise_args* a, int device, void* stream) {
    ARGS(a, "noise_forward");
    TRY(rf_plane("noise", a->B, a->Cin, a->T, a->H, a->W, a->video_channel, a->y0, a->x0, a->wh, a->ww, a->cell));
    if (a->kind != DWN_NOISE_BINARY && a->kind != DWN_NOISE_SPARSE) return dwn_set_error(-2, "noise: kind must be DWN_NOISE_BINARY or DWN_NOISE_SPARSE");
    if (a->hold < 1) return dwn_set_error(-2, "noise: hold must be positive");
    if (!(a->density >= 0.f && a->density <= 1.f)) return dwn_set_error(-2, "noise: density outside [0, 1]");
    if (a->first_clip < 0 || a->first_clip > (1ll << 32) - a->B) return dwn_set_error(-2, "noise: clip numbers must stay inside [0, 2^32): first_clip + B <= 2^32");
    if (!a->x || !a->out) return dwn_set_error(-1, "noise_forward: null pointer (x, out)");
    ENTER(device);
    return k_noise_forward(*a, (hipStream_t)stream);
}

// what the state's layout depends on: N, lags and the cell grid
static int sta_grid(const dwn_sta_args* a) {
    if (a->N <= 0) return dwn_set_error(-2, "sta: N must be positive");
    if (a->lags < 1 || a->lags > 65535) return dwn_set_error(-2, "sta: lags outside [1, 65535]");
    if (a->wh <= 0 || a->ww <= 0) return dwn_set_error(-2, "sta: the window sides must be positive");
    if (a->cell < 1 || a->wh % a->cell || a->ww % a->cell) return dwn_set_error(-2, "sta: cell must be positive and divide both window sides");
    const long long G = (long long)(a->wh / a->cell) * (a->ww / a->cell);
    if (G > (1ll << 22) || (long long)a->N * a->lags > (1ll << 40) / G) return dwn_set_error(-2, "sta: more than 2^22 cells or 2^40 state elements");
    return 0;
}
static int sta_accumulate_geometry(const dwn_sta_args* a) {
    TRY(sta_grid(a));
    TRY(rf_plane("sta", a->B, a->Cin, a->T, a->H, a->W, a->channel, a->y0, a->x0, a->wh, a->ww, a->cell));
    if (a->skip < 0) return dwn_set_error(-2, "sta: skip must not be negative");
    if ((a->skip > a->lags - 1 ? a->skip : a->lags - 1) >= a->T) return dwn_set_error(-2, "sta: no valid frame (max(skip, lags - 1) >= T)");
    if ((long long)a->B * a->T >= (1ll << 31)) return dwn_set_error(-2, "sta: more than 2^31 samples per call");
    return 0;
}
size_t dwn_sta_state_bytes(const dwn_sta_args* a) {
    WS_BYTES_OR_0(a, sta_grid, k_sta_state_bytes(*a));
}
size_t dwn_sta_ws_bytes(const dwn_sta_args* a) {
    WS_BYTES_OR_0(a, sta_grid, k_sta_ws_bytes(*a));
}
int dwn_sta_accumulate(const dwn_sta_args* a, int device, void* stream) {
    ARGS(a, "sta_accumulate");
    TRY(sta_accumulate_geometry(a));
    if (!a->x || !a->r || !a->state) return dwn_set_error(-1, "sta_accumulate: null pointer (x, r, state)");
    if ((size_t)a->state & 7) return dwn_set_error(-2, "sta_accumulate: state must be 8-byte aligned");
    ENTER(device);
    return k_sta_accumulate(*a, (hipStream_t)stream);
}
int dwn_sta_finalize(const dwn_sta_args* a, int device, void* stream) {
    ARGS(a, "sta_finalize");
    TRY(sta_grid(a));
    if (a->samples < 1 || a->samples >= (1ll << 52)) return dwn_set_error(-2, "sta_finalize: samples outside [1, 2^52)");
    if (!(a->rel_threshold >= 0.0 && a->rel_threshold <= 1.0)) return dwn_set_error(-2, "sta_finalize: rel_threshold outside [0, 1]");
    if (!a->state || !a->cov || !a->summary || !a->ws) return dwn_set_error(-1, "sta_finalize: null pointer (state, cov, summary, ws)");
    if (((size_t)a->state & 7) || ((size_t)a->summary & 7)) return dwn_set_error(-2, "sta_finalize: state and summary must be 8-byte aligned");
    WS_CHECK(a, -3, "sta_finalize", k_sta_ws_bytes(*a), "dwn_sta_ws_bytes", 8);
    ENTER(device);
    return k_sta_finalize(*a, (hipStream_t)stream);
}

// ---- parametric receptive-field fits: the argument checks need no device
static int gauss2d_grid(int gh, int gw) {
    if (gh < 3 || gw < 3) return dwn_set_error(-2, "gauss2d: gh and gw must be at least 3");
    if ((long long)gh * gw > 4096) return dwn_set_error(-2, "gauss2d: more than 4096 cells per map");
    return 0;
}
static int gauss2d_geometry(const dwn_gauss2d_args* a) {
    TRY(gauss2d_grid(a->gh, a->gw));
    if (a->M < 1 || a->R < 1) return dwn_set_error(-2, "gauss2d: M and R must be positive");
    if ((long long)a->M > (1ll << 31) / 4096 || (long long)a->R > (1ll << 40) / 4096) return dwn_set_error(-2, "gauss2d: more than 2^19 fits or 2^28 rows");
    return 0;
}
size_t dwn_gauss2d_ws_bytes(const dwn_gauss2d_args* a) {
    WS_BYTES_OR_0(a, gauss2d_geometry, k_gauss2d_ws_bytes(*a));
}
int dwn_gauss2d_fit(const dwn_gauss2d_args* a, int device, void* stream) {
    ARGS(a, "gauss2d_fit");
    TRY(gauss2d_geometry(a));
    if (!a->sel && a->M > a->R) return dwn_set_error(-2, "gauss2d_fit: M > R without a row table");
    if (a->max_iter < 0) return dwn_set_error(-2, "gauss2d_fit: max_iter must not be negative");
    if (!(a->rel_threshold >= 0.0 && a->rel_threshold <= 1.0)) return dwn_set_error(-2, "gauss2d_fit: rel_threshold outside [0, 1]");
    if (!(a->xtol >= 0.0) || !(a->ftol >= 0.0)) return dwn_set_error(-2, "gauss2d_fit: xtol and ftol must not be negative");
    if (!a->maps || !a->params || !a->table || !a->ws) return dwn_set_error(-1, "gauss2d_fit: null pointer (maps, params, table, ws)");
    if (((size_t)a->params & 7) || ((size_t)a->table & 7)) return dwn_set_error(-2, "gauss2d_fit: params and table must be 8-byte aligned");
    WS_CHECK(a, -3, "gauss2d_fit", k_gauss2d_ws_bytes(*a), "dwn_gauss2d_ws_bytes", 8);
    ENTER(device);
    return k_gauss2d_fit(*a, (hipStream_t)stream);
}
int dwn_gauss2d_profile(const dwn_gauss2d_profile_args* a, int device, void* stream) {
    ARGS(a, "gauss2d_profile");
    TRY(gauss2d_grid(a->gh, a->gw));
    if (a->N < 1 || a->L < 1 || a->L > 65535) return dwn_set_error(-2, "gauss2d_profile: N must be positive and L in [1, 65535]");
    if ((long long)a->N * a->L > (1ll << 40) / 4096) return dwn_set_error(-2, "gauss2d_profile: more than 2^28 maps");
    if (!a->params || !a->maps || !a->profile || !a->separability) return dwn_set_error(-1, "gauss2d_profile: null pointer (params, maps, profile, separability)");
    if (((size_t)a->params & 7) || ((size_t)a->profile & 7) || ((size_t)a->separability & 7)) return dwn_set_error(-2, "gauss2d_profile: params, profile and separability must be 8-byte aligned");
    ENTER(device);
    return k_gauss2d_profile(*a, (hipStream_t)stream);
}

}  // extern "C"

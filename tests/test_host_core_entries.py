"""CPU tests of the entry contract of the model's own C entries (DESIGN.md "The entry contract"): stem, block, pool, cortex, readout,
conv_pw backward, and the thin kernel-family, loss and optimizer entries above them.  One table row per entry.  Every refusal is
answered before a device is entered (``NO_DEVICE``: an entry that reached the device answers a HIP error, > 0), pointers are fake
(never dereferenced on the host), and nothing large is allocated.  No kernel runs here."""
import ctypes as C

import pytest

PTR = 256            # never dereferenced on the host
NO_DEVICE = 10 ** 6  # a device index no machine has
HUGE = 1 << 62       # a workspace size that never is the refusal
INT_MAX = 2 ** 31 - 1


def _lib():
    import sensorium_amd._lib as L
    return L


def _err():
    return _lib().lib.dwn_last_error()


def _point(struct, skip=()):
    """every pointer field of a ctypes struct (nested BatchNorm bundles included) set to the fake pointer"""
    for name, ctype in struct._fields_:
        if name in skip:
            continue
        if ctype is C.c_void_p:
            setattr(struct, name, PTR)
        elif isinstance(ctype, type) and issubclass(ctype, C.Structure):
            _point(getattr(struct, name))
    return struct


def _set(a, **kw):
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# ---- complete, valid arguments of each composite (the small shapes of tests/test_host_frozen.py)
def stem(**kw):
    L = _lib()
    a = _point(L.StemArgs(), skip=("pe_t", "pe_h", "pe_w", "y0"))
    return _set(a, **{**dict(dtype=L.DWN_BF16, training=L.BN_TRAIN, B=2, Cin=5, C0=64, S=128, ws_bytes=HUGE), **kw})


def stem_grad(**kw):
    L = _lib()
    return _set(_point(L.StemInputGradArgs()), **{**dict(dtype=L.DWN_BF16, training=L.BN_FROZEN, B=2, Cin=5, C0=64, S=128), **kw})


def block(**kw):
    L = _lib()
    a = _point(L.BlockArgs(), skip=("out_pe_t", "out_pe_h", "out_pe_w", "drop_scale"))
    return _set(a, **{**dict(dtype=L.DWN_BF16, training=L.BN_TRAIN, B=2, T=4, Hin=8, Win=16, Hout=8, Wout=16, Cin=64, Cmid=448, Cout=64,
                stride=1, ks=3, kt=5, se_r=14, x_has_pe=1, ws_bytes=HUGE), **kw})


def pool(**kw):
    L = _lib()
    return _set(_point(L.PoolArgs()), **{**dict(dtype=L.DWN_BF16, BT=8, HW=16, C=64), **kw})


def cortex(**kw):
    L = _lib()
    a = _point(L.CortexArgs(), skip=("drop_scale", "dout_mask"))
    return _set(a, **{**dict(dtype=L.DWN_BF16, training=L.BN_TRAIN, B=2, T=4, Cin=64, C=128, groups=2, ws_bytes=HUGE), **kw})


def readout(**kw):
    L = _lib()
    a = _point(L.ReadoutArgs(), skip=("drop_mask", "beta_dev", "dbeta"))
    return _set(a, **{**dict(dtype=L.DWN_BF16, B=2, T=4, Cin=128, groups=2, n_out=7, softplus_beta=1.0, ws_bytes=HUGE), **kw})


def pw(**kw):
    L = _lib()
    a = _point(L.PwBwdArgs(), skip=("res", "res_abc", "res_hinv", "res_winv"))
    return _set(a, **{**dict(M=1024, E=448, Cin=64, ws_bytes=HUGE), **kw})


def _call(name, *tail):
    """entry(a, *tail, device, stream) with a = a struct, or None for the null struct"""
    fn = getattr(_lib().lib, name)
    return lambda a, device=NO_DEVICE: fn(None if a is None else C.byref(a), *tail, device, None)


def _size(name, *tail):
    fn = getattr(_lib().lib, name)
    return lambda a: fn(None if a is None else C.byref(a), *tail)


# One row per composite entry: name, call, valid arguments, arguments with a refused geometry (field -> value; a row with `groups`
# has groups = 0 among them), a required pointer, the size entry behind its workspace check (or None), and the int bounds:
# (fields exactly at the bound, fields one step past it).
def composite_rows():
    L = _lib()
    block_bounds = [(dict(B=INT_MAX, T=1, Hin=1, Win=1, Hout=1, Wout=1), dict(B=2 ** 30, T=2, Hin=1, Win=1, Hout=1, Wout=1))]
    stem_bounds = [(dict(B=1, S=INT_MAX), dict(B=2, S=2 ** 30))]
    cortex_bounds = [(dict(B=INT_MAX, T=1, Cin=16, C=16), dict(B=2 ** 30, T=2, Cin=16, C=16)),      # M = B * T
                     (dict(B=INT_MAX // 4, T=1, Cin=64, C=1024), dict(B=INT_MAX // 4 + 1, T=1, Cin=64, C=1024))]   # elements / 256
    readout_bounds = [(dict(B=INT_MAX, T=1), dict(B=2 ** 30, T=2)),                                 # M = B * T
                      (dict(groups=2 ** 25 - 1, Cin=8 * (2 ** 25 - 1), n_out=1), dict(groups=2 ** 25, Cin=8 * 2 ** 25, n_out=1)),
                      (dict(groups=1, Cin=8, n_out=INT_MAX // 8), dict(groups=1, Cin=8, n_out=INT_MAX // 8 + 1))]
    pw_bounds = [(dict(M=INT_MAX), dict(M=2 ** 31))]
    bad_block = [dict(Cin=0), dict(stride=0), dict(se_r=0), dict(B=-2), dict(Cmid=452), dict(dtype=2), dict(training=3), dict(Hout=7)]
    bad_stem = [dict(C0=0), dict(C0=60), dict(B=0), dict(S=0), dict(Cin=-1), dict(dtype=5)]
    bad_cortex = [dict(groups=0), dict(groups=-1), dict(Cin=60), dict(C=0), dict(T=0), dict(dtype=2), dict(training=-1)]
    bad_readout = [dict(groups=0), dict(n_out=0), dict(Cin=100), dict(B=0), dict(dtype=-1)]
    bad_pool = [dict(C=12), dict(C=0), dict(BT=0), dict(HW=-1), dict(dtype=2)]
    bad_pw = [dict(E=0), dict(Cin=60), dict(M=0)]
    size_stem = _size("dwn_stem_workspace_bytes")
    return [
        ("dwn_stem_forward", _call("dwn_stem_forward"), stem, bad_stem + [dict(training=3)], "x", size_stem, -6, stem_bounds),
        ("dwn_stem_backward", _call("dwn_stem_backward"), stem, bad_stem + [dict(training=3)], "dout", size_stem, -6, stem_bounds),
        ("dwn_stem_backward_input", _call("dwn_stem_backward_input", PTR), stem, bad_stem, "xmom", size_stem, -6, stem_bounds),
        ("dwn_stem_input_grad", _call("dwn_stem_input_grad"), stem_grad, bad_stem, "dx", None, None, stem_bounds),
        ("dwn_block_forward", _call("dwn_block_forward"), block, bad_block, "z3", _size("dwn_block_workspace_bytes", 0), -6, block_bounds),
        ("dwn_block_backward", _call("dwn_block_backward"), block, bad_block[:-3] + bad_block[-1:], "dy4",
         _size("dwn_block_workspace_bytes", 1), -6, block_bounds),
        ("dwn_pool_forward", _call("dwn_pool_forward"), pool, bad_pool, "out", None, None, []),
        ("dwn_pool_backward", _call("dwn_pool_backward"), pool, bad_pool, "dout", None, None, []),
        ("dwn_cortex_forward", _call("dwn_cortex_forward"), cortex, bad_cortex, "y", _size("dwn_cortex_workspace_bytes", 0), -6, cortex_bounds),
        ("dwn_cortex_backward", _call("dwn_cortex_backward"), cortex, bad_cortex, "dw", _size("dwn_cortex_workspace_bytes", 1), -6,
         cortex_bounds),
        ("dwn_readout_forward", _call("dwn_readout_forward"), readout, bad_readout, "out", _size("dwn_readout_workspace_bytes", 0), -6,
         readout_bounds),
        ("dwn_readout_backward", _call("dwn_readout_backward"), readout, bad_readout, "dout", _size("dwn_readout_workspace_bytes", 1), -6,
         readout_bounds),
        ("dwn_pw_backward", _call("dwn_pw_backward", L.DWN_BF16), pw, bad_pw, "abc",
         lambda a: L.lib.dwn_pw_backward_workspace_bytes(a.E, a.Cin, L.DWN_BF16), -6, pw_bounds),
    ]


ROW_IDS = ["dwn_stem_forward", "dwn_stem_backward", "dwn_stem_backward_input", "dwn_stem_input_grad", "dwn_block_forward",
           "dwn_block_backward", "dwn_pool_forward", "dwn_pool_backward", "dwn_cortex_forward", "dwn_cortex_backward",
           "dwn_readout_forward", "dwn_readout_backward", "dwn_pw_backward"]


@pytest.fixture(scope="module")
def rows():
    got = {r[0]: r for r in composite_rows()}
    assert list(got) == ROW_IDS
    return got


@pytest.mark.parametrize("name", ROW_IDS)
def test_composite_entry_contract(rows, name):
    _, call, make, bad, pointer, size, ws_code, bounds = rows[name]
    # 1. a null struct
    assert call(None) == -1 and b"null" in _err(), name
    # 2. a zeroed struct, and each refused geometry with everything else valid: a negative code and a message
    rc = call(type(make())())
    assert rc < 0 and _err(), name
    for fields in bad:
        rc = call(make(**fields))
        assert rc in (-2, -4) and _err(), (name, fields, rc)
    # 3. valid geometry, a required pointer null (alone, and all of them): -1, and the message names a pointer
    assert call(make(**{pointer: None})) == -1 and pointer.encode() in _err(), (name, _err())
    bare = _set(type(make())(), **{f: getattr(make(), f) for f, t in make()._fields_ if t is not C.c_void_p and not issubclass(t, C.Structure)})
    assert call(bare) == -1 and b"null pointer" in _err(), name
    # 4. one byte short of what the size entry answers
    if size is not None:
        need = size(make())
        assert need > 0
        assert call(make(ws_bytes=need - 1)) == ws_code and b"workspace too small" in _err(), name
        assert call(make(ws_bytes=need)) > 0, name
    # 5. complete arguments: past every check, and nothing was touched in front of the device
    assert call(make()) > 0 and _err(), name
    # 6. each int bound: accepted exactly at it, -2 one step past it
    for at, past in bounds:
        assert call(make(**at)) > 0, (name, at, _err())
        assert call(make(**past)) == -2 and b"2^31" in _err(), (name, past)


def test_block_mode_and_route_entries():
    L = _lib()
    assert _call("dwn_block_backward")(block(training=L.BN_EVAL)) == -7 and b"frozen" in _err()
    assert _call("dwn_block_backward")(block(training=L.BN_EVAL, Cin=0)) == -7            # the mode answers before the geometry
    assert _call("dwn_cortex_backward")(cortex(training=L.BN_EVAL, groups=0)) == -7
    assert _call("dwn_block_forward")(block(x_has_pe=0, a0=None)) == -2 and b"a0 buffer" in _err()
    assert _call("dwn_block_forward")(block(x_has_pe=0)) > 0
    # y1 / y3 are required exactly where dwn_block_forward_writes names them; da0 unless the route folds dx
    writes, route = _size("dwn_block_forward_writes"), _size("dwn_block_backward_route")
    for y1_mode in (0, 1, 2):
        for training in (L.BN_EVAL, L.BN_TRAIN, L.BN_FROZEN):
            w = writes(block(training=training, y1_mode=y1_mode))
            assert w in (0, 1, 2, 3)
            for bit, field in ((1, "y1"), (2, "y3")):
                rc = _call("dwn_block_forward")(block(training=training, y1_mode=y1_mode, **{field: None}))
                assert (rc == -1) if w & bit else (rc > 0), (y1_mode, training, field, rc)
    assert route(block()) == 1 and _call("dwn_block_backward")(block(da0=None)) > 0
    assert route(block(dtype=L.DWN_F32)) == 0 and _call("dwn_block_backward")(block(dtype=L.DWN_F32, da0=None)) == -1
    # the two route entries answer the geometry's code with the error set
    for entry in (writes, route):
        assert entry(None) == -1 and b"null arguments" in _err()
        assert entry(L.BlockArgs()) == -2 and b"must be positive" in _err()
        assert entry(block(kt=4)) == -4 and b"temporal_kernel" in _err()
        assert entry(block(B=2 ** 30, T=2, Hin=1, Win=1, Hout=1, Wout=1)) == -2 and b"2^31" in _err()
        assert entry(block()) >= 0 and not _err()


def test_readout_pair_rule_and_stem_modes():
    L = _lib()
    assert _call("dwn_readout_backward")(readout(beta_dev=PTR)) == -2 and b"beta_dev and dbeta" in _err()
    assert _call("dwn_readout_backward")(readout(beta_dev=PTR, dbeta=PTR)) > 0
    assert _call("dwn_readout_backward")(readout(w=None)) > 0                   # the forward's wt stands in for w
    assert _call("dwn_readout_backward")(readout(w=None, wt=None)) == -1
    assert _call("dwn_stem_forward")(stem(training=L.BN_TRAIN, xmom=None)) == -1 and b"xmom" in _err()
    assert _call("dwn_stem_forward")(stem(training=L.BN_EVAL, xmom=None)) > 0
    assert _call("dwn_stem_backward")(stem(training=L.BN_FROZEN, xmom=None)) > 0
    assert _call("dwn_stem_forward")(stem(pe_t=PTR, T=2, H=8, W=7)) == -2 and b"T*H*W" in _err()
    assert _call("dwn_stem_forward")(stem(pe_t=PTR, T=2, H=8, W=8)) > 0
    for mode in (L.BN_EVAL, L.BN_FROZEN):
        assert _call("dwn_stem_backward_input", PTR)(stem(training=mode, C0=0)) == -7
    assert _call("dwn_stem_backward_input", None)(stem()) == -1
    assert _call("dwn_stem_backward_input", PTR)(stem(C0=256)) == -4
    for mode in (L.BN_EVAL, L.BN_TRAIN):
        assert _call("dwn_stem_input_grad")(stem_grad(training=mode, B=0)) == -7


def test_size_entries_answer_zero_and_leave_no_error():
    L = _lib()
    sizes = [(_size("dwn_stem_workspace_bytes"), stem, [dict(C0=0), dict(C0=60), dict(B=2, S=2 ** 30)], L.StemArgs),
             (_size("dwn_block_workspace_bytes", 0), block, [dict(Cin=0), dict(stride=0), dict(kt=4), dict(Hout=7)], L.BlockArgs),
             (_size("dwn_block_workspace_bytes", 1), block, [dict(Cin=0), dict(Cmid=452), dict(ks=4)], L.BlockArgs),
             (_size("dwn_cortex_workspace_bytes", 0), cortex, [dict(groups=0), dict(Cin=60)], L.CortexArgs),
             (_size("dwn_cortex_workspace_bytes", 1), cortex, [dict(groups=0), dict(B=2 ** 30, T=2)], L.CortexArgs),
             (_size("dwn_readout_workspace_bytes", 0), readout, [dict(groups=0), dict(n_out=0)], L.ReadoutArgs),
             (_size("dwn_readout_workspace_bytes", 1), readout, [dict(groups=0), dict(Cin=100)], L.ReadoutArgs),
             (_size("dwn_readout_wt_bytes"), readout, [dict(groups=0), dict(Cin=100)], L.ReadoutArgs)]
    for size, make, bad, struct in sizes:
        assert _call("dwn_block_backward")(block(kt=4)) == -4 and _err()        # an error is pending ...
        assert size(None) == 0 and not _err()                                   # ... and the size entry clears it
        assert size(struct()) == 0 and not _err()
        for fields in bad:
            assert size(make(**fields)) == 0 and not _err(), fields
        assert size(make()) > 0 and not _err()
        # pointers play no part in a size (but in the readout's: wt, drop_mask and beta_dev choose slices of its workspace)
        assert struct is L.ReadoutArgs or size(_set(struct(), **{f: getattr(make(), f) for f, t in struct._fields_
                                      if t is not C.c_void_p and not issubclass(t, C.Structure)})) == size(make())
    pws = L.lib.dwn_pw_backward_workspace_bytes
    for e, cin, dt in ((0, 64, 1), (448, 0, 1), (-8, 64, 1), (450, 64, 1), (448, 60, 0), (448, 64, 2)):
        assert pws(e, cin, dt) == 0 and not _err(), (e, cin, dt)
    assert pws(448, 64, L.DWN_BF16) > 0 and pws(448, 64, L.DWN_F32) > pws(448, 64, L.DWN_BF16)


# ---- the thin entries: the null refusals and their own checks in front of the device, no geometry of their own
def thin_rows():
    L = _lib()
    lib = L.lib
    bn = _point(L.BN())
    nd = NO_DEVICE

    def struct_entry(name, struct, **kw):
        return (name, lambda: getattr(lib, name)(None, L.DWN_BF16, nd, None), b"null arguments",
                lambda: getattr(lib, name)(C.byref(_set(struct(), **kw)), L.DWN_BF16, nd, None))
    return [
        struct_entry("dwn_gemm_nn", L.GemmNNArgs), struct_entry("dwn_gemm_tn", L.GemmTNArgs),
        struct_entry("dwn_dw_spatial_fwd", L.DwSpatialFwdArgs), struct_entry("dwn_dw_spatial_bwd", L.DwSpatialBwdArgs),
        struct_entry("dwn_dw_temporal_fwd", L.DwTemporalFwdArgs, kt=3, C=64),
        struct_entry("dwn_dw_temporal_bwd", L.DwTemporalBwdArgs, kt=5, C=64),
        struct_entry("dwn_dw_temporal_wide_fwd", L.DwTemporalFwdArgs, kt=7, C=64),
        struct_entry("dwn_dw_temporal_wide_bwd", L.DwTemporalBwdArgs, kt=9, C=64, dy_kind=L.LD_PLAIN),
        ("dwn_bn_finalize", lambda: lib.dwn_bn_finalize(PTR, 64, 8.0, None, 64, 1, 0.1, 1e-5, nd, None), b"bn",
         lambda: lib.dwn_bn_finalize(None, 64, 8.0, C.byref(bn), 64, 0, 0.1, 1e-5, nd, None)),
        ("dwn_bn_finalize", lambda: lib.dwn_bn_finalize(None, 64, 8.0, C.byref(bn), 64, 1, 0.1, 1e-5, nd, None), b"stats",
         lambda: lib.dwn_bn_finalize(PTR, 64, 8.0, C.byref(bn), 64, 1, 0.1, 1e-5, nd, None)),
        ("dwn_bn_bwd_finalize", lambda: lib.dwn_bn_bwd_finalize(PTR, 8.0, None, PTR, 64, nd, None), b"bn",
         lambda: lib.dwn_bn_bwd_finalize(PTR, 8.0, C.byref(bn), PTR, 64, nd, None)),
        ("dwn_pack_weight", lambda: lib.dwn_pack_weight(None, PTR, 1, 8, 8, 0, 8, 8, L.DWN_BF16, nd, None), b"src",
         lambda: lib.dwn_pack_weight(PTR, PTR, 1, 8, 8, 0, 8, 8, L.DWN_BF16, nd, None)),
        ("dwn_f64_to_f32", lambda: lib.dwn_f64_to_f32(PTR, None, 1, nd, None), b"dst", lambda: lib.dwn_f64_to_f32(PTR, PTR, 1, nd, None)),
        ("dwn_poisson_loss_forward", lambda: lib.dwn_poisson_loss_forward(PTR, PTR, PTR, 8, 16, 1e-8, None, nd, None), b"loss_acc",
         lambda: lib.dwn_poisson_loss_forward(PTR, PTR, PTR, 8, 16, 1e-8, PTR, nd, None)),
        ("dwn_poisson_loss_backward", lambda: lib.dwn_poisson_loss_backward(PTR, None, PTR, None, 8, 16, 1e-8, PTR, nd, None), b"target",
         lambda: lib.dwn_poisson_loss_backward(PTR, PTR, PTR, None, 8, 16, 1e-8, PTR, nd, None)),      # gscale is optional
        ("dwn_adamw_ema_multi", lambda: lib.dwn_adamw_ema_multi(None, 1, 16, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.999, 1.0, nd, None),
         b"null table", lambda: lib.dwn_adamw_ema_multi(PTR, 1, 16, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.999, 1.0, nd, None)),
        ("dwn_ema_lerp_multi", lambda: lib.dwn_ema_lerp_multi(None, 1, 16, 0.999, nd, None), b"null table",
         lambda: lib.dwn_ema_lerp_multi(PTR, 1, 16, 0.999, nd, None)),
        ("dwn_conv_pw_bn_stats", lambda: lib.dwn_conv_pw_bn_stats(PTR, 64, 128, PTR, 448, 64, None, 0.1, 1e-5, None, PTR, HUGE, 1, nd, None),
         b"null pointer", lambda: lib.dwn_conv_pw_bn_stats(PTR, 64, 128, PTR, 448, 64, C.byref(bn), 0.1, 1e-5, None, PTR, HUGE, 1, nd, None)),
        ("dwn_assemble_inputs", lambda: lib.dwn_assemble_inputs(None, 2, 4, 8, 8, 8, 8, 0.0, PTR, nd, None), b"null pointer",
         lambda: lib.dwn_assemble_inputs(PTR, 2, 4, 8, 8, 8, 8, 0.0, PTR, nd, None)),
        ("dwn_assemble_targets", lambda: lib.dwn_assemble_targets(PTR, 2, 4, PTR, None, 2, 10, PTR, nd, None), b"null pointer",
         lambda: lib.dwn_assemble_targets(PTR, 2, 4, PTR, PTR, 2, 10, PTR, nd, None)),
    ]


THIN_IDS = ["dwn_gemm_nn", "dwn_gemm_tn", "dwn_dw_spatial_fwd", "dwn_dw_spatial_bwd", "dwn_dw_temporal_fwd", "dwn_dw_temporal_bwd",
            "dwn_dw_temporal_wide_fwd", "dwn_dw_temporal_wide_bwd", "dwn_bn_finalize-bn", "dwn_bn_finalize-stats", "dwn_bn_bwd_finalize",
            "dwn_pack_weight", "dwn_f64_to_f32", "dwn_poisson_loss_forward", "dwn_poisson_loss_backward", "dwn_adamw_ema_multi",
            "dwn_ema_lerp_multi", "dwn_conv_pw_bn_stats", "dwn_assemble_inputs", "dwn_assemble_targets"]


@pytest.mark.parametrize("index", range(len(THIN_IDS)), ids=THIN_IDS)
def test_thin_entry_contract(index):
    name, null_call, names, complete_call = thin_rows()[index]
    assert THIN_IDS[index].startswith(name)
    assert null_call() == -1 and names in _err(), (name, _err())
    assert complete_call() > 0 and _err(), name            # the runtime's answer about the device: every check was passed before it


def test_thin_entries_keep_their_own_checks_in_front_of_the_device():
    L = _lib()
    lib, nd = L.lib, NO_DEVICE
    for entry, struct in ((lib.dwn_dw_temporal_fwd, L.DwTemporalFwdArgs), (lib.dwn_dw_temporal_bwd, L.DwTemporalBwdArgs)):
        for kt in (0, 7, 9):
            assert entry(C.byref(_set(struct(), kt=kt, C=64)), L.DWN_BF16, nd, None) == -4 and b"3 or 5" in _err()
    assert lib.dwn_adamw_ema_multi(PTR, 1, 16, 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 0.999, 1.0, nd, None) == -2 and b"step" in _err()
    assert lib.dwn_adamw_ema_multi(None, 0, 16, 1e-3, 0.9, 0.999, 1e-8, 0.01, 1, 0.999, 1.0, nd, None) > 0      # an empty table needs no pointer
    bn = _point(L.BN())
    stats = lambda *a: lib.dwn_conv_pw_bn_stats(*a, nd, None)
    assert stats(PTR, 64, 128, PTR, 448, 60, C.byref(bn), 0.1, 1e-5, None, PTR, HUGE, 1) == -2
    assert stats(PTR, 64, 2 ** 31, PTR, 448, 64, C.byref(bn), 0.1, 1e-5, None, PTR, HUGE, 1) == -2
    assert stats(PTR, 64, 2 ** 31 - 1, PTR, 448, 64, C.byref(bn), 0.1, 1e-5, None, PTR, HUGE, 1) > 0
    need = lib.dwn_conv_pw_bn_stats_workspace_bytes(64)
    assert stats(PTR, 64, 128, PTR, 448, 64, C.byref(bn), 0.1, 1e-5, None, PTR, need - 1, 1) == -6 and b"workspace too small" in _err()
    assert stats(PTR, 64, 128, None, 448, 64, C.byref(bn), 0.1, 1e-5, None, PTR, need, 1) == -1
    assert lib.dwn_assemble_inputs(PTR, 2, 4, 8, 8, 7, 8, 0.0, PTR, nd, None) == -2 and b"smaller than the video" in _err()
    assert lib.dwn_assemble_targets(PTR, 70000, 4, PTR, PTR, 2, 10, PTR, nd, None) == -2 and b"grid dimensions" in _err()
    # conv_pw backward: the shortcut term's two refusals are answered with the rest, before anything is queued
    assert _call("dwn_pw_backward", L.DWN_BF16)(pw(res=PTR, res_abc=PTR, res_C=96)) == -2 and b"res_C" in _err()
    assert _call("dwn_pw_backward", L.DWN_BF16)(pw(res=PTR, res_abc=None, res_C=64)) == -2
    assert _call("dwn_pw_backward", L.DWN_F32)(pw(res=PTR, res_abc=PTR, res_C=64)) == -3 and b"one-pass kernel" in _err()
    assert _call("dwn_pw_backward", L.DWN_BF16)(pw(res=PTR, res_abc=PTR, res_C=128)) > 0
    # the probes answer 0 for null arguments
    assert lib.dwn_dw_spatial_fwd_rc_supported(None, L.DWN_BF16) == 0 and lib.dwn_dw_spatial_bwd_rc_supported(None, L.DWN_BF16) == 0

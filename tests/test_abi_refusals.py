"""What the C ABI refuses, pinned: a table of (entry, one fault) -> (code, substring of `gta_strerror`).  Every request is refused by the
argument checks of gta_abi.cpp, in front of any HIP call, so the table needs no GPU; the operands are placeholder addresses that nothing reads.
Requests that break two rules at once are not pinned, beyond the one promise that a layout refusal is not masked by a stride complaint."""
import ctypes

import pytest
import torch

from gta_amd import native

X = ctypes.c_void_p(256)            # a non-null, 256-byte aligned placeholder operand
BIG = 1 << 60                       # a workspace size no check finds too small
BADARG, LAYOUT, UNSUPPORTED = -1, -2, -3
VT, EU, PRE, FUSED_KV, X3 = (native.FLAG_V_TRANSFORM, native.FLAG_EUCLID, native.FLAG_PRETRANSFORMED, native.FLAG_FUSED_KV,
                             native.FLAG_FP32_PRODUCTS)
B, H, TQ, TK, NQ, NK = 2, 2, 128, 192, 2, 3
CL = {"se3": 32, "so2": 32}                         # a fused layout (view and so2 tables)
T2 = {"se3": 32, "t2": 30, "triv": 2}               # a staged layout (view and coord tables)
SO2T2 = {"so2": 8, "t2": 24}                        # a staged layout with so2 and coord tables

FWD_ARGS = ("q", "k", "v", "vrep_q", "vrep_k", "cs_q", "cs_k", "trans_coeff", "tau", "out", "lse", "workspace", "workspace_bytes", "stream")
STAGED_ARGS = FWD_ARGS[:7] + ("coord_q", "coord_k") + FWD_ARGS[7:]
BWD_ARGS = ("q", "k", "v", "out", "dout", "lse", "vrep_q", "vrep_k", "cs_q", "cs_k", "trans_coeff", "tau", "kv_images", "dq", "dk", "dv",
            "dqkv_stride", "dout_stride", "dtrans_coeff", "dtau", "workspace", "workspace_bytes", "stream")


def _with(args, before, *names):
    i = args.index(before)
    return args[:i] + names + args[i:]


ENTRIES = {
    "gta_attn_fwd": FWD_ARGS,
    "gta_attn_fwd_varlen": _with(FWD_ARGS, "out", "key_lens"),
    "gta_attn_fwd_staged": STAGED_ARGS,
    "gta_attn_fwd_staged_varlen": _with(STAGED_ARGS, "out", "key_lens"),
    "gta_attn_bwd": BWD_ARGS,
    "gta_attn_bwd_varlen": _with(BWD_ARGS, "kv_images", "key_lens", "q_lens"),
    "gta_attn_fwd_plain": ("q", "k", "v", "key_bias", "bias_pitch", "tau", "out", "lse", "stream"),
}
FUSED = ("gta_attn_fwd", "gta_attn_fwd_varlen", "gta_attn_bwd", "gta_attn_bwd_varlen")
STAGED = ("gta_attn_fwd_staged", "gta_attn_fwd_staged_varlen")
VARLEN = ("gta_attn_fwd_varlen", "gta_attn_fwd_staged_varlen", "gta_attn_bwd_varlen")
BWD = ("gta_attn_bwd", "gta_attn_bwd_varlen")
SUPPORTED = ("gta_attn_fwd_supported", "gta_attn_fwd_varlen_supported", "gta_attn_bwd_varlen_supported", "gta_attn_fwd_staged_supported",
             "gta_attn_fwd_staged_varlen_supported")


def _desc(f_dims=CL, flags=VT, dtype=torch.bfloat16, so3_degree=0, dh=None, **fields):
    """a descriptor at contiguous strides; ``fields`` overwrite its members (a stride member: the token stride)"""
    dh = sum(f_dims.values()) if dh is None else dh
    qs, ks = (H * TQ * dh, TQ * dh, dh), (H * TK * dh, TK * dh, dh)
    d = native.make_desc_from(dtype, (B, H, TQ, dh), TK, (qs, ks, ks, qs), f_dims, so3_degree, NQ, NK, dh ** -0.5, flags)
    for name, val in fields.items():
        if name.endswith("_stride"):
            getattr(d, name)[2] = val
        else:
            setattr(d, name, val)
    return d


def _call(entry, desc, **args):
    """``entry`` on ``desc`` (None: a null descriptor) with every operand present and every size sufficient, but for ``args``"""
    if entry not in ENTRIES:                                            # a *_supported entry
        return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc))
    dh = 64 if desc is None else desc.dh
    full = {name: X for name in ENTRIES[entry]}
    full.update(workspace_bytes=BIG, bias_pitch=256, stream=None,
                dqkv_stride=(ctypes.c_int64 * 9)(*(H * TQ * dh, TQ * dh, dh) * 3), dout_stride=(ctypes.c_int64 * 3)(H * TQ * dh, TQ * dh, dh))
    full.update(args)
    return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc), *(full[name] for name in ENTRIES[entry]))


def _strides(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


ROWS = []


def row(entries, code, text, desc=None, **args):
    for e in ((entries,) if isinstance(entries, str) else entries):
        ROWS.append(pytest.param(e, desc or {}, args, code, text, id=f"{e}-{len(ROWS)}"))


# ---- every forward and backward entry: the descriptor's own faults
ALL = FUSED + STAGED
for e in ALL:
    lay = T2 if e in STAGED else CL
    row(e, BADARG, "null descriptor", desc=None, null_desc=True)
    row(e, BADARG, "abi_version mismatch", dict(f_dims=lay, abi_version=1))
    row(e, BADARG, "bad dtype", dict(f_dims=lay, dtype_=7))
    row(e, BADARG, "strides must keep every head row 16-byte aligned", dict(f_dims=lay, q_stride=68))
    row(e, BADARG, "strides must keep every head row 16-byte aligned", dict(f_dims=lay, o_stride=68))
    row(e, BADARG, "non-positive size", dict(f_dims=lay, H=0))
    row(e, BADARG, "tokens must split evenly into views", dict(f_dims=lay, Nk=5))
    row(e, UNSUPPORTED, "more than GTA_MAX_VIEWS views per side", dict(f_dims=lay, Nq=32))
    row(e, UNSUPPORTED, "more than 2^22 tokens per side", dict(f_dims=lay, Tk=3 << 21))
    row(e, LAYOUT, "f_dims do not sum to dh", dict(f_dims=lay, dh=72))
    row(e, LAYOUT, "negative slab size", dict(f_dims=lay, d_triv=-8, dh=56))
for e in SUPPORTED:
    lay = T2 if "staged" in e else CL
    row(e, BADARG, "null descriptor", desc=None, null_desc=True)
    row(e, BADARG, "abi_version mismatch", dict(f_dims=lay, abi_version=1))
    row(e, BADARG, "bad dtype", dict(f_dims=lay, dtype_=7))
    row(e, BADARG, "strides must keep every head row 16-byte aligned", dict(f_dims=lay, k_stride=68))
    row(e, LAYOUT, "f_dims do not sum to dh", dict(f_dims=lay, dh=72))
    row(e, LAYOUT, "negative slab size", dict(f_dims=lay, d_triv=-8, dh=56))

# ---- null operands, key_lens, workspace
for e in ("gta_attn_fwd", "gta_attn_fwd_varlen"):
    for name in ("q", "k", "v", "out"):
        row(e, BADARG, "null q/k/v/out", q_=name)
    row(e, BADARG, "workspace smaller than gta_attn_fwd_workspace_bytes()", workspace_bytes=4096)
for e in STAGED:
    for name in ("q", "k", "v", "out"):
        row(e, BADARG, "null q/k/v/out", dict(f_dims=T2), q_=name)
    row(e, BADARG, "workspace smaller than gta_attn_fwd_staged_workspace_bytes()", dict(f_dims=T2), workspace=None)
    row(e, BADARG, "workspace smaller than gta_attn_fwd_staged_workspace_bytes()", dict(f_dims=T2), workspace_bytes=4096)
    row(e, BADARG, "workspace must be 256-byte aligned", dict(f_dims=T2), workspace=ctypes.c_void_p(264))
for e in BWD:
    for name in ("q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "dqkv_stride", "dout_stride", "workspace"):
        row(e, BADARG, "null argument", q_=name)
    row(e, BADARG, "workspace smaller than gta_attn_bwd_workspace_bytes()", workspace_bytes=4096)
    row(e, BADARG, "gradient strides must keep rows 16-byte aligned", dqkv_stride=_strides(*(H * TQ * 64, TQ * 64, 64) * 2, H * TQ * 64, TQ * 64, 68))
    row(e, BADARG, "dout strides must keep rows 16-byte aligned", dout_stride=_strides(H * TQ * 64, TQ * 64, 68))
row("gta_attn_bwd", UNSUPPORTED, "backward of the pretransformed mode", dict(flags=VT | PRE))
row("gta_attn_fwd_varlen", BADARG, "per-scene key prefixes need the workspace of gta_attn_fwd_workspace_bytes()", workspace=None)
for e in VARLEN:
    row(e, BADARG, "null key_lens", dict(f_dims=T2 if e in STAGED else CL), key_lens=None)

# ---- the rep tables each layout needs
for e in FUSED:
    for name in ("vrep_q", "vrep_k"):
        row(e, BADARG, "se3/so3 slabs need vrep_q and vrep_k", q_=name)
    for name in ("cs_q", "cs_k"):
        row(e, BADARG, "so2 slab needs cs_q and cs_k", q_=name)
for e in STAGED:
    for name in ("vrep_q", "vrep_k"):
        row(e, BADARG, "se3/so3 slabs need vrep_q and vrep_k", dict(f_dims=T2), q_=name)
    for name in ("cs_q", "cs_k"):
        row(e, BADARG, "so2 slab needs cs_q and cs_k", dict(f_dims=SO2T2), q_=name)
    for name in ("coord_q", "coord_k"):
        row(e, BADARG, "t2 slab needs coord_q and coord_k", dict(f_dims=T2), q_=name)

# ---- layouts: mis-sized slabs (GTA_E_LAYOUT), and every reason a layout has no fused kernel (GTA_E_UNSUPPORTED)
for e in FUSED + ("gta_attn_fwd_supported", "gta_attn_fwd_varlen_supported", "gta_attn_bwd_varlen_supported"):
    row(e, LAYOUT, "se3 slab must be a multiple of 4 channels (gta.py:161)", dict(f_dims={"se3": 30, "triv": 2, "so2": 32}))
    row(e, LAYOUT, "so2 slab must be 4*nfreqs channels (gta.py:212-214)", dict(f_dims={"se3": 32, "so2": 30, "triv": 2}))
    row(e, LAYOUT, "t2 slab must be a multiple of 3 channels (gta.py:231)", dict(f_dims={"se3": 32, "t2": 32}))
    row(e, LAYOUT, "so3 slab must be r*sum(2l+1) channels (gta.py:182)", dict(f_dims={"se3": 32, "so3": 20, "so2": 12}, so3_degree=2))
    row(e, LAYOUT, "under euclid_sim the se3 slab holds 3-vectors (gta.py:147)", dict(flags=VT | EU))
    row(e, UNSUPPORTED, "euclid similarity has no fused kernel (gta_rep_apply + gta_attn_fwd_plain)",
        dict(f_dims={"triv": 2, "se3": 30, "so2": 32}, flags=VT | EU))
    row(e, UNSUPPORTED, "fused kernel needs dh % 8 == 0 and dh <= 128", dict(f_dims={"se3": 8, "so2": 4}, dtype=torch.float32))
    row(e, UNSUPPORTED, "fused kernel needs dh % 8 == 0 and dh <= 128", dict(f_dims={"triv": 136}))
    row(e, UNSUPPORTED, "t2 slab has no fused kernel (ablation; use the unfused path)", dict(f_dims=T2))
    row(e, UNSUPPORTED, "fused so3 needs degree 2 ([3|5] groups of 8 channels)", dict(f_dims={"se3": 48, "so3": 24, "so2": 24}, so3_degree=1))
    row(e, UNSUPPORTED, "fused kernel needs 4-aligned se3/so2 slabs and an 8-aligned so3 slab",
        dict(f_dims={"triv": 4, "se3": 32, "so3": 16, "so2": 12}, so3_degree=2))
for e in STAGED + ("gta_attn_fwd_staged_supported", "gta_attn_fwd_staged_varlen_supported"):
    row(e, LAYOUT, "se3 slab must be a multiple of 4 channels (gta.py:161)", dict(f_dims={"se3": 30, "triv": 2, "so2": 32}))
    row(e, LAYOUT, "under euclid_sim the se3 slab holds 3-vectors (gta.py:147)", dict(f_dims=CL, flags=VT | EU))
    row(e, LAYOUT, "so2 slab must be a whole number of 2-channel blocks", dict(f_dims={"se3": 32, "so2": 31, "triv": 1}))
    row(e, LAYOUT, "t2 slab must be a multiple of 3 channels (gta.py:231)", dict(f_dims={"se3": 32, "t2": 32}))
    row(e, LAYOUT, "so3 slab must be r*sum(2l+1) channels (gta.py:182)", dict(f_dims={"se3": 32, "so3": 20, "so2": 12}, so3_degree=2))
    row(e, UNSUPPORTED, "so3 of degree 1 or 2", dict(f_dims={"se3": 32, "so3": 15, "so2": 16, "triv": 1}, so3_degree=3))
    row(e, UNSUPPORTED, "staged generic forward needs dh % 8 == 0", dict(f_dims={"se3": 6, "so2": 6}, flags=VT | EU, dtype=torch.float32))
    row(e, UNSUPPORTED, "staged generic forward needs dh <= 128", dict(f_dims={"triv": 136}))
    row(e, UNSUPPORTED, "staged generic forward has no GTA_FLAG_FP32_PRODUCTS instances", dict(f_dims=T2, flags=VT | X3, dtype=torch.float32))
    row(e, UNSUPPORTED, "staged generic forward applies rho itself: no GTA_FLAG_PRETRANSFORMED", dict(f_dims=T2, flags=VT | PRE))

# ---- per-scene key prefixes: the flags they cannot be combined with
for e in ("gta_attn_fwd_varlen", "gta_attn_bwd_varlen", "gta_attn_fwd_varlen_supported", "gta_attn_bwd_varlen_supported"):
    row(e, UNSUPPORTED, "per-scene key prefixes run the two-stage plan: no GTA_FLAG_FUSED_KV", dict(flags=VT | FUSED_KV))
    row(e, UNSUPPORTED, "per-scene key prefixes have no GTA_FLAG_FP32_PRODUCTS instances", dict(flags=VT | X3, dtype=torch.float32))
    row(e, UNSUPPORTED, "per-scene key prefixes apply rho_k in the pre-pass: no GTA_FLAG_PRETRANSFORMED", dict(flags=VT | PRE))

# ---- the fp32-faithful mode is for fp32 inputs; grids
row("gta_attn_fwd", BADARG, "GTA_FLAG_FP32_PRODUCTS is for fp32 inputs (bf16 inputs ask for bf16 arithmetic)", dict(flags=VT | X3))
row("gta_attn_bwd", UNSUPPORTED, "GTA_FLAG_FP32_PRODUCTS backward: fp32 inputs at dh <= 64", dict(flags=VT | X3))
row("gta_attn_bwd", UNSUPPORTED, "GTA_FLAG_FP32_PRODUCTS backward: fp32 inputs at dh <= 64",
    dict(f_dims={"se3": 48, "so2": 48}, flags=VT | X3, dtype=torch.float32))
for e in FUSED:
    row(e, UNSUPPORTED, "B or H above 65535", dict(B=65536))
    row(e, UNSUPPORTED, "B or H above 65535", dict(H=65536))

# ---- plain attention
PLAIN = {"triv": 64}
row("gta_attn_fwd_plain", BADARG, "null argument", desc=None, null_desc=True)
for name in ("q", "k", "v", "out"):
    row("gta_attn_fwd_plain", BADARG, "null argument", dict(f_dims=PLAIN), q_=name)
row("gta_attn_fwd_plain", BADARG, "abi_version mismatch", dict(f_dims=PLAIN, abi_version=3))
row("gta_attn_fwd_plain", BADARG, "bad dtype", dict(f_dims=PLAIN, dtype_=-1))
row("gta_attn_fwd_plain", BADARG, "non-positive size", dict(f_dims=PLAIN, Tq=0))
row("gta_attn_fwd_plain", UNSUPPORTED, "plain attention needs dh % 8 == 0 and dh <= 128", dict(f_dims={"triv": 60}))
row("gta_attn_fwd_plain", UNSUPPORTED, "plain attention needs dh % 8 == 0 and dh <= 128", dict(f_dims={"triv": 136}))
row("gta_attn_fwd_plain", BADARG, "bias_pitch must be a multiple of 64 >= Tk", dict(f_dims=PLAIN), bias_pitch=128)
row("gta_attn_fwd_plain", BADARG, "bias_pitch must be a multiple of 64 >= Tk", dict(f_dims=PLAIN), bias_pitch=200)
row("gta_attn_fwd_plain", BADARG, "GTA_FLAG_FP32_PRODUCTS is for fp32 inputs", dict(f_dims=PLAIN, flags=X3))


@pytest.mark.parametrize("entry, desc, args, code, text", ROWS)
def test_refusal(entry, desc, args, code, text):
    args = dict(args)
    null = args.pop("null_desc", False)
    if "q_" in args:                                    # (the operand to pass as NULL)
        args[args.pop("q_")] = None
    if "dtype_" in desc:                                # (the raw dtype member; `dtype` is the torch dtype the descriptor is built for)
        desc = dict(desc, dtype=torch.bfloat16)
        raw = desc.pop("dtype_")
        d = _desc(**desc)
        d.dtype = raw
    else:
        d = None if null else _desc(**desc)
    rc = _call(entry, d, **args)
    assert rc == code, (rc, native.lib().gta_strerror(rc).decode())
    assert text in native.lib().gta_strerror(rc).decode()


def test_a_layout_refusal_is_not_masked_by_a_stride_complaint():
    for entry, f_dims, flags in (("gta_attn_fwd_supported", T2, VT), ("gta_attn_fwd_supported", {"triv": 2, "se3": 30, "so2": 32}, VT | EU),
                                 ("gta_attn_fwd_staged_supported", {"se3": 6, "so2": 8}, VT | EU)):
        assert _call(entry, _desc(f_dims, flags, q_stride=68)) == UNSUPPORTED, entry


def test_workspace_sizes_of_refused_requests_are_zero():
    L = native.lib()
    for name in ("gta_attn_fwd_workspace_bytes", "gta_attn_bwd_workspace_bytes"):
        assert getattr(native, name[4:])(_desc(T2)) == 0 and getattr(native, name[4:])(_desc(abi_version=1)) == 0
        assert getattr(L, name)(None) == 0
    assert native.attn_fwd_staged_workspace_bytes(_desc({"se3": 6, "so2": 8}, VT | EU)) == 0 and L.gta_attn_fwd_staged_workspace_bytes(None) == 0


# ---- gta_rep_grad_sums (and gta_rep_grad_workspace_bytes, which shares its geometry checks)
REPGRAD_ARGS = ("side", "n_pairs", "a0", "a0_stride", "b0", "b0_stride", "a1", "a1_stride", "b1", "b1_stride", "view_sums", "so2_sums", "t2_sums",
                "workspace", "workspace_bytes", "stream")


GEOMETRY = ("null descriptor", "abi_version mismatch", "non-positive size or tokens not a multiple of views",
            "rep-gradient sums serve at most 256 heads")


def _rep_grad(desc, **args):
    st = _strides(H * TQ * 64, TQ * 64, 64)
    full = dict(side=0, n_pairs=2, a0=X, b0=X, a1=X, b1=X, a0_stride=st, b0_stride=st, a1_stride=st, b1_stride=st, view_sums=X, so2_sums=X,
                t2_sums=None, workspace=X, workspace_bytes=BIG, stream=None)
    full.update(args)
    return native.lib().gta_rep_grad_sums(None if desc is None else ctypes.byref(desc), *(full[name] for name in REPGRAD_ARGS))


@pytest.mark.parametrize("desc, args, code, text", [
    (None, {}, BADARG, "null descriptor"),
    (dict(abi_version=1), {}, BADARG, "abi_version mismatch"),
    ({}, dict(side=2), BADARG, "side must be 0 (query) or 1 (key)"),
    (dict(Nq=3), {}, BADARG, "non-positive size or tokens not a multiple of views"),
    (dict(H=0), {}, BADARG, "non-positive size or tokens not a multiple of views"),
    (dict(H=257), {}, UNSUPPORTED, "rep-gradient sums serve at most 256 heads"),
    (dict(dtype_=7), {}, BADARG, "dtype must be GTA_DTYPE_F32 or GTA_DTYPE_BF16"),
    ({}, dict(n_pairs=3), BADARG, "n_pairs must be 1 or 2"),
    ({}, dict(view_sums=None, so2_sums=None), BADARG, "no output requested"),
    ({}, dict(a0=None), BADARG, "null, misaligned or negatively strided operand"),
    ({}, dict(b1_stride=None), BADARG, "null, misaligned or negatively strided operand"),
    ({}, dict(b0=ctypes.c_void_p(257)), BADARG, "null, misaligned or negatively strided operand"),
    ({}, dict(a1_stride=_strides(-64, 64, 64)), BADARG, "null, misaligned or negatively strided operand"),
    (dict(d_triv=-8, dh=56), {}, LAYOUT, "negative slab size"),
    (dict(dh=72), {}, LAYOUT, "f_dims do not sum to dh"),
    (dict(f_dims={"se3": 30, "triv": 2, "so2": 32}), {}, LAYOUT, "se3 / so2 / t2 slab not a whole number of groups"),
    (dict(flags=VT | EU), {}, LAYOUT, "se3 / so2 / t2 slab not a whole number of groups"),
    (dict(f_dims={"se3": 32, "so2": 31, "triv": 1}), {}, LAYOUT, "se3 / so2 / t2 slab not a whole number of groups"),
    (dict(f_dims={"se3": 32, "t2": 32}), dict(so2_sums=None), LAYOUT, "se3 / so2 / t2 slab not a whole number of groups"),
    ({}, dict(t2_sums=X), BADARG, "sums requested for an empty slab"),
    (dict(f_dims=T2), {}, BADARG, "sums requested for an empty slab"),
    (dict(f_dims={"so2": 64}), {}, BADARG, "sums requested for an empty slab"),
    ({}, dict(so2_sums=ctypes.c_void_p(258)), BADARG, "misaligned output"),
    ({}, dict(workspace=None), BADARG, "view sums need a workspace of gta_rep_grad_workspace_bytes"),
    ({}, dict(workspace_bytes=16), BADARG, "view sums need a workspace of gta_rep_grad_workspace_bytes"),
])
def test_rep_grad_sums_refusal(desc, args, code, text):
    if desc is not None:
        desc = dict(desc)
        raw = desc.pop("dtype_", None)
        desc = _desc(**desc)
        if raw is not None:
            desc.dtype = raw
    rc = _rep_grad(desc, **args)
    assert rc == code, (rc, native.lib().gta_strerror(rc).decode())
    assert text in native.lib().gta_strerror(rc).decode()
    if text in GEOMETRY:          # the size query shares these checks and refuses with the same code
        assert native.lib().gta_rep_grad_workspace_bytes(None if desc is None else ctypes.byref(desc), 0) == code

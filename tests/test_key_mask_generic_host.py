"""Host side of the key mask on the staged generic layouts (`gta_attention(..., key_mask=..., key_mask_generic=True)`,
`gta_attn_fwd_staged_gather`): the exported symbols and their ctypes signatures against include/gta_hip.h, the refusals of the new entry (the
rows tests/test_abi_refusals.py pins for `gta_attn_fwd_staged_varlen`, repeated, plus the null `key_idx`), the routes with and without the
opt-in (each refusal raises `GtaError` naming its reason before anything is launched -- these tests run without a GPU, on CPU tensors), the
cache contract, and the gather rule of tests/_staged_gather_images.py against a host emulation of the pre-pass with and without planted
defects."""
import ctypes
import functools

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from tests import _images as I
from tests import _staged_gather_images as SG
from tests import test_abi_refusals as R
from tests.test_key_views_host import _decl

CL = {"se3": 32, "so2": 32}
EUCLID = {"triv": 2, "se3": 30, "so2": 32}
T2 = {"se3": 32, "t2": 30, "triv": 2}
B, H, NK, PK, TQ = 4, 2, 5, 52, 150
TK = NK * PK

GATHER_ARGS = R._with(R.ENTRIES["gta_attn_fwd_staged_varlen"], "key_lens", "key_idx")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exist_and_signatures_match_the_header():
    L = native.lib()
    for s in ("gta_attn_fwd_staged_gather", "gta_attn_fwd_staged_gather_supported"):
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
    args, base = _decl("gta_attn_fwd_staged_gather"), _decl("gta_attn_fwd_staged_varlen")
    # the header: gta_attn_fwd_staged_varlen plus `const int32_t* key_idx` in front of key_lens
    i = [a.split()[-1] for a in args].index("key_idx")
    assert args[i] == "const int32_t* key_idx" and args[i + 1] == "const int32_t* key_lens"
    assert args[:i] + args[i + 1:] == base
    assert tuple(a.split()[-1].lstrip("*") for a in args[1:]) == GATHER_ARGS
    at = L.gta_attn_fwd_staged_gather.argtypes
    assert len(at) == len(args) == 19 and at[0] == ctypes.POINTER(native.GtaAttnDesc)
    for a, t in zip(args[1:], at[1:]):
        assert t == (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_void_p), (a, t)
    assert L.gta_attn_fwd_staged_varlen.argtypes == at[:i] + at[i + 1:]
    assert _decl("gta_attn_fwd_staged_gather_supported") == ["const GtaAttnDesc* desc"]
    assert L.gta_attn_fwd_staged_gather_supported.argtypes == [ctypes.POINTER(native.GtaAttnDesc)]
    assert L.gta_abi_version() == 2
    assert callable(native.attn_fwd_staged_gather) and callable(native.attn_fwd_staged_gather_supported)


def _call(entry, desc, **args):
    """tests/test_abi_refusals.py's `_call` for the two new entries"""
    if entry.endswith("_supported"):
        return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc))
    full = {name: R.X for name in GATHER_ARGS}
    full.update(workspace_bytes=R.BIG, stream=None)
    full.update(args)
    return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc), *(full[name] for name in GATHER_ARGS))


RENAME = {"gta_attn_fwd_staged_varlen": "gta_attn_fwd_staged_gather", "gta_attn_fwd_staged_varlen_supported": "gta_attn_fwd_staged_gather_supported"}
ROWS = [pytest.param(RENAME[p.values[0]], *p.values[1:], id=f"{RENAME[p.values[0]]}-{i}") for i, p in enumerate(R.ROWS) if p.values[0] in RENAME]
ROWS.append(pytest.param("gta_attn_fwd_staged_gather", dict(f_dims=T2), {"key_idx": None}, R.BADARG, "null key_idx",
                         id="gta_attn_fwd_staged_gather-null-key_idx"))


def test_the_staged_varlen_rows_are_all_there():
    """(the table above is built from another module's: it must not come out empty)"""
    n_call = sum(1 for p in ROWS if p.values[0] == "gta_attn_fwd_staged_gather")
    n_sup = sum(1 for p in ROWS if p.values[0] == "gta_attn_fwd_staged_gather_supported")
    assert n_call >= 20 and n_sup >= 8, (n_call, n_sup)
    texts = {p.values[4] for p in ROWS}
    for t in ("null key_lens", "null key_idx", "workspace smaller than gta_attn_fwd_staged_workspace_bytes()", "null q/k/v/out",
              "staged generic forward needs dh % 8 == 0", "staged generic forward needs dh <= 128"):
        assert t in texts, t


@pytest.mark.parametrize("entry, desc, args, code, text", ROWS)
def test_refusal(entry, desc, args, code, text):
    args = dict(args)
    null = args.pop("null_desc", False)
    if "q_" in args:
        args[args.pop("q_")] = None
    if "dtype_" in desc:
        desc = dict(desc, dtype=torch.bfloat16)
        raw = desc.pop("dtype_")
        d = R._desc(**desc)
        d.dtype = raw
    else:
        d = None if null else R._desc(**desc)
    rc = _call(entry, d, **args)
    assert rc == code, (rc, native.lib().gta_strerror(rc).decode())
    assert text in native.lib().gta_strerror(rc).decode()


def test_null_key_idx_is_not_read_under_kv_ready():
    """with GTA_FLAG_KV_READY a null key_idx passes the argument checks: the next refusal is the workspace's size"""
    d = R._desc(f_dims=T2, flags=R.VT | native.FLAG_KV_READY)
    rc = _call("gta_attn_fwd_staged_gather", d, key_idx=None, workspace_bytes=4096)
    assert rc == R.BADARG and "workspace smaller" in native.lib().gta_strerror(rc).decode()
    rc = _call("gta_attn_fwd_staged_gather", R._desc(f_dims=T2), key_idx=None, workspace_bytes=4096)
    assert rc == R.BADARG and "null key_idx" in native.lib().gta_strerror(rc).decode()


# ---- routes and refusals ----------------------------------------------------------------------------------------------------------------------
def _mask(b=B, t=TK):
    m = torch.ones(b, t, dtype=torch.bool)
    m[:, 1::3] = False
    return m


def _packed(f_dims, tq=TQ):
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
    if f_dims.get("so2"):
        packed.update(cs_q=torch.zeros(B, tq, f_dims["so2"] // 2, 2), cs_k=torch.zeros(B, TK, f_dims["so2"] // 2, 2))
    if f_dims.get("t2"):
        packed.update(coord_q=torch.zeros(B, tq, 2), coord_k=torch.zeros(B, TK, 2))
    return packed


def _cpu_call(f_dims=EUCLID, dh=64, euclid=True, grad=False, mask=None, generic=True, **kw):
    """gta_attention on CPU tensors: reaches a kernel only if nothing refuses first (and would then raise for the missing device)"""
    q = torch.zeros(B, H, TQ, dh, requires_grad=grad)
    k = torch.zeros(B, H, TK, dh)
    if generic:
        kw["key_mask_generic"] = True
    return gta_amd.gta_attention(q, k, k, f_dims, _packed(f_dims), key_mask=_mask() if mask is None else mask, euclid=euclid, **kw)


def _resolve(f_dims=EUCLID, dh=64, euclid=True, **kw):
    q = torch.zeros(B, H, TQ, dh)
    k = torch.zeros(B, H, TK, dh)
    args = dict(so3_degree=0, trans_coeff=None, tau=None, scale=None, v_transform=True, euclid=euclid, pretransformed=False, use_dma=True,
                kv_mode="auto", kv_cache=None, precise=None, key_views=None, key_lens=None, key_views_backward=False, query_views=None,
                return_lse=False, key_mask=_mask(), key_mask_backward=False, query_mask=None, key_mask_rep_grad=False)
    args.update(kw)
    with torch.no_grad():
        return G2._resolve(q, k, k, f_dims, _packed(f_dims), **args)


def test_without_the_keyword_everything_is_as_it_was():
    assert "key_mask_generic" in G2.MASK_OPT_INS and "key_mask_generic" in G2.MASK_KEYWORDS
    with torch.no_grad():
        with pytest.raises(native.GtaError, match="no gather pre-pass.*euclid"):
            _cpu_call(generic=False)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*t2"):
            _cpu_call(f_dims=T2, euclid=False, generic=False)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*dh % 8"):
            _cpu_call(f_dims={"se3": 8, "so2": 4}, dh=12, euclid=False, generic=False)
    shape = (B, H, TQ, 64)
    for dt in (torch.float32, torch.bfloat16):
        with pytest.raises(native.GtaError, match="no gather pre-pass"):
            G2.attention_route(shape, TK, dt, EUCLID, 0, 1, NK, euclid=True, key_mask=True)
        with pytest.raises(native.GtaError, match="no gather pre-pass"):
            G2.attention_route(shape, TK, dt, T2, 0, 1, NK, key_mask=True, key_mask_generic=False)
    with pytest.raises(native.GtaError, match="key_mask_generic=True comes with key_mask"):
        with torch.no_grad():
            gta_amd.gta_attention(torch.zeros(B, H, TQ, 64), torch.zeros(B, H, TK, 64), torch.zeros(B, H, TK, 64), EUCLID, _packed(EUCLID),
                                  euclid=True, key_mask_generic=True)


def test_routes_with_the_keyword():
    shape = (B, H, TQ, 64)
    for dt in (torch.float32, torch.bfloat16):
        for f, eu in ((EUCLID, True), (T2, False)):
            assert G2.attention_route(shape, TK, dt, f, 0, 1, NK, euclid=eu, key_mask=True, key_mask_generic=True) is None
            assert G2.generic_route(shape, TK, dt, f, 0, 1, NK, euclid=eu, key_mask_generic=True) == "staged"
        # so3 of degree 1 on unaligned slabs
        so3 = {"triv": 0, "se3": 48, "so3": 24, "so2": 24}
        assert G2.attention_route((B, H, TQ, 96), TK, dt, so3, 1, 1, NK, key_mask=True, key_mask_generic=True) is None
        assert G2.generic_route((B, H, TQ, 96), TK, dt, so3, 1, 1, NK, key_mask_generic=True) == "staged"
        # a fused layout: the keyword changes nothing
        assert (G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=True, key_mask_generic=True)
                == G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=True))
    for f, eu in ((EUCLID, True), (T2, False)):
        route, cfg, mask, *_ = _resolve(f, euclid=eu, key_mask_generic=True)
        assert route == "staged" and cfg[5] is None
        assert mask.kind == "gather" and mask.key_mask is not None and mask.key_idx is None and mask.q_live is None
    # ... and on a fused layout the record and the route are those of the call without it
    a, b = _resolve(CL, euclid=False, key_mask_generic=True), _resolve(CL, euclid=False)
    assert a[0] == b[0] == "forward" and a[1] == b[1] and a[2].kind == b[2].kind == "gather"
    # a mask_index companion: the record's own tensors stand in the mask record
    m = _mask()
    idx, lens = G2.key_index_tensors(m, "cpu")
    mi = G2.MaskIndex(m, None, idx, lens, m.clone())
    route, _cfg, mask, *_ = _resolve(key_mask=m, mask_index=mi, key_mask_generic=True)
    assert route == "staged" and mask.key_idx is idx and mask.key_lens is lens and mask.k_live is None


def test_refusals_with_the_keyword():
    with pytest.raises(native.GtaError, match="key_mask is forward-only"):
        _cpu_call(grad=True)
    with pytest.raises(native.GtaError, match="key_mask_generic is forward-only.*no masked backward.*key_mask_backward"):
        _cpu_call(grad=True, key_mask_backward=True)
    with pytest.raises(native.GtaError, match="key_mask_generic is forward-only"):
        _cpu_call(f_dims=T2, euclid=False, grad=True, key_mask_backward=True)
    shape = (B, H, TQ, 64)
    with pytest.raises(native.GtaError, match="key_mask_generic is forward-only"):
        G2.attention_route(shape, TK, torch.bfloat16, T2, 0, 1, NK, key_mask=True, key_mask_backward=True, needs_grad=True, key_mask_generic=True)
    with pytest.raises(native.GtaError, match="key_mask_generic is forward-only"):
        G2.generic_route(shape, TK, torch.bfloat16, T2, 0, 1, NK, needs_grad=True, key_mask_generic=True)
    with torch.no_grad():
        qm = torch.ones(B, TQ, dtype=torch.bool)
        with pytest.raises(native.GtaError, match="query_mask: the staged generic layouts .* have no query-side mask"):
            _cpu_call(query_mask=qm)
        with pytest.raises(native.GtaError, match="query_mask: the staged generic layouts .* have no query-side mask"):
            q = torch.zeros(B, H, TQ, 64)
            gta_amd.gta_attention(q, torch.zeros(B, H, TK, 64), torch.zeros(B, H, TK, 64), T2, _packed(T2), query_mask=qm, key_mask_generic=True)
        # layouts the staged entry refuses too: the old words
        with pytest.raises(native.GtaError, match="no gather pre-pass.*dh % 8"):
            _cpu_call(f_dims={"se3": 8, "so2": 4}, dh=12, euclid=False)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*dh <= 128"):
            _cpu_call(f_dims={"triv": 106, "t2": 30}, dh=136, euclid=False)
        with pytest.raises(native.GtaError, match="key_mask has no precise=True"):
            _cpu_call(precise=True)
        with pytest.raises(native.GtaError, match="key_mask with pretransformed=True"):
            _cpu_call(pretransformed=True)
        with pytest.raises(native.GtaError, match="key_mask runs the two-stage plan: kv_mode='fused'"):
            _cpu_call(kv_mode="fused")
        with pytest.raises(native.GtaError, match="key_mask with key_views"):
            _cpu_call(key_views=[1] * B)
        with pytest.raises(native.GtaError, match="gta_attention_by_view_groups takes no key_mask"):
            k = torch.zeros(B, H, TK, 64)
            gta_amd.gta_attention_by_view_groups(torch.zeros(B, H, TQ, 64), k, k, EUCLID, _packed(EUCLID), views_per_call=2, euclid=True,
                                                 key_mask=_mask(), key_mask_generic=True)
        # nothing refuses: the call gets as far as the checks in front of the kernels, which have no CPU path
        with pytest.raises(native.GtaError, match="cpu|CUDA"):
            _cpu_call()
        with pytest.raises(native.GtaError, match="cpu|CUDA"):
            _cpu_call(f_dims=T2, euclid=False, return_lse=True)


def test_kv_cache_keeps_indices_and_lengths_beside_the_images(monkeypatch):
    """the first call stores key_idx / key_lens and a plan key that says "key_mask"; the second runs on the stored lengths under KV_READY and
    is handed no indices; a call without the mask (or with key_views) on that cache is refused"""
    calls = []
    monkeypatch.setitem(native._OPT_IN_ENTRIES, "attn_fwd_staged_gather", lambda desc, q, k, v, *a: calls.append((desc.flags, a[8], a[9])))
    monkeypatch.setattr(native, "attn_fwd_staged_varlen", lambda *a, **k: None)
    monkeypatch.setattr(native, "attn_fwd_staged", lambda *a, **k: None)
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    cache = {}
    with torch.no_grad():
        _cpu_call(kv_cache=cache)
        assert cache["plan"][0] == "staged" and cache["plan"][-1] == "key_mask" and cache["images"] is not None
        assert cache["key_lens"].tolist() == [int(_mask()[0].sum())] * B and tuple(cache["key_idx"].shape) == (B, TK)
        _cpu_call(kv_cache=cache, mask=torch.ones(B, TK, dtype=torch.bool))        # (not looked at: the cache's lengths hold)
        (f0, i0, l0), (f1, i1, l1) = calls
        assert not f0 & native.FLAG_KV_READY and i0 is cache["key_idx"] and l0 is cache["key_lens"]
        assert f1 & native.FLAG_KV_READY and i1 is None and l1 is cache["key_lens"]
        q = torch.zeros(B, H, TQ, 64)
        k = torch.zeros(B, H, TK, 64)
        with pytest.raises(native.GtaError, match="another plan"):
            gta_amd.gta_attention(q, k, k, EUCLID, _packed(EUCLID), euclid=True, kv_cache=cache)
        with pytest.raises(native.GtaError, match="another plan"):
            gta_amd.gta_attention(q, k, k, EUCLID, _packed(EUCLID), euclid=True, kv_cache=cache, key_views=[5] * B)


def test_srt_sets_the_keyword_for_every_layer():
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    model.encoder = lambda images, cam, rays, extras: (None, extras)
    model.decode = lambda z, x, rays, extras=None: extras
    mine = {"input_coord": 1}
    m3 = torch.ones(2, 3, 4, dtype=torch.bool)
    seen = model(None, None, None, None, None, mine, input_mask=m3, input_mask_generic=True)
    assert seen["key_mask_generic"] is True and tuple(seen["key_mask"].shape) == (2, 12) and mine == {"input_coord": 1}
    assert "key_mask_generic" not in model(None, None, None, None, None, mine, input_mask=m3)
    with pytest.raises(native.GtaError, match="input_mask_generic=True comes with input_mask"):
        model(None, None, None, None, None, mine, input_mask_generic=True)
    with pytest.raises(native.GtaError, match="input_mask_generic=True comes with input_mask"):
        srt.render_image(model, None, torch.zeros(2, 3), torch.zeros(2, 4, 4, 3), {}, input_mask_generic=True)


# ---- the gather rule against a host emulation ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emu_case():
    """B = 3 scenes, H = 2, 3 views of 50 tokens (Tk = 150: three tiles), the euclid layout `triv 2 | se3 30 | so2 32`; masks: every third
    token dropped (100 keys: two tiles, 28 dead rows), one view and a half (75 keys), all keys"""
    c = I.key_side_case(EUCLID, 0, torch.bfloat16, B=3, H=2, Nk=3, Pk=50, seed=11)
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, c.so3, 0.37, True, True)
    mask = torch.ones(3, c.T, dtype=torch.bool)
    mask[0, 2::3] = False
    mask[1, :25] = False
    mask[1, 100:] = False
    idx, lens = (t.long() for t in G2.key_index_tensors(mask, "cpu"))               # (the emulation runs on what the operator would hand the kernel)
    assert lens.tolist() == [100, 75, 150] and torch.equal(idx, SG.index_tensors(mask)[0])
    return c, ref, idx, lens, I.staged_layout(c.B, c.H, c.T, c.dh).total + 512


def test_host_emulation_passes_the_rules():
    c, ref, idx, lens, total = _emu_case()
    ws = SG.emulate(c, ref, idx, lens, True, total)
    SG.check("emulation", ws, c, ref, idx, lens, True)
    # entries at or past key_lens are never looked at
    junk = idx.clone()
    for b, n in enumerate(lens.tolist()):
        junk[b, n:] = 10 ** 6
    SG.check("emulation", ws, c, ref, junk, lens, True)
    # the live indices reversed give the reversed rows, bias included
    rev = idx.clone()
    for b, n in enumerate(lens.tolist()):
        rev[b, :n] = idx[b, :n].flip(0)
    SG.check("reversed", SG.emulate(c, ref, rev, lens, True, total), c, ref, rev, lens, True)
    with pytest.raises(AssertionError):
        SG.check("reversed against ascending", ws, c, ref, rev, lens, True)
    # without euclid no bias is written, and a written one is caught
    ref_plain = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, c.so3, 0.37, True, True)
    SG.check("no bias", SG.emulate(c, ref_plain, idx, lens, False, total), c, ref_plain, idx, lens, False)
    with pytest.raises(AssertionError, match="without euclid"):
        SG.check("bias without euclid", ws, c, ref, idx, lens, False)


@pytest.mark.parametrize("defect", SG.DEFECTS)
def test_planted_defects_fail_the_rules(defect):
    c, ref, idx, lens, total = _emu_case()
    ws = SG.emulate(c, ref, idx, lens, True, total, defect=defect)
    assert not torch.equal(ws, SG.emulate(c, ref, idx, lens, True, total)), defect
    with pytest.raises(AssertionError):
        SG.check(defect, ws, c, ref, idx, lens, True)

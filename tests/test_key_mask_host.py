"""Host side of the key mask (`gta_attention(..., key_mask=...)`, `gta_attn_fwd_gather`): the exported symbols and their ctypes signatures
against include/gta_hip.h, the refusals of the new entry (the rows tests/test_abi_refusals.py pins for `gta_attn_fwd_varlen`, repeated, plus
the null `key_idx`), `key_index_tensors`, the refused combinations of the Python layer (each raises `GtaError` naming its reason before
anything is launched -- these tests run without a GPU, on CPU tensors), and the gather rule of tests/_gather_images.py against a host
emulation of the pre-pass with and without planted defects."""
import ctypes
import functools
import re

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from tests import _gather_images as GI
from tests import _images as I
from tests import test_abi_refusals as R
from tests.test_key_views_host import _decl

CL = {"se3": 32, "so2": 32}
EUCLID = {"triv": 2, "se3": 30, "so2": 32}
B, H, NK, PK, TQ = 4, 2, 5, 52, 150
TK = NK * PK

GATHER_ARGS = R._with(R.ENTRIES["gta_attn_fwd_varlen"], "key_lens", "key_idx")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exist_and_signatures_match_the_header():
    L = native.lib()
    for s in ("gta_attn_fwd_gather", "gta_attn_fwd_gather_supported"):
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
    args, base = _decl("gta_attn_fwd_gather"), _decl("gta_attn_fwd_varlen")
    # the header: gta_attn_fwd_varlen plus `const int32_t* key_idx` in front of key_lens
    i = [a.split()[-1] for a in args].index("key_idx")
    assert args[i] == "const int32_t* key_idx" and args[i + 1] == "const int32_t* key_lens"
    assert args[:i] + args[i + 1:] == base
    assert tuple(a.split()[-1].lstrip("*") for a in args[1:]) == GATHER_ARGS
    at = L.gta_attn_fwd_gather.argtypes
    assert len(at) == len(args) and at[0] == ctypes.POINTER(native.GtaAttnDesc)
    for a, t in zip(args[1:], at[1:]):
        assert t == (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_void_p), (a, t)
    assert L.gta_attn_fwd_varlen.argtypes == at[:i] + at[i + 1:]
    assert _decl("gta_attn_fwd_gather_supported") == ["const GtaAttnDesc* desc"]
    assert L.gta_attn_fwd_gather_supported.argtypes == [ctypes.POINTER(native.GtaAttnDesc)]
    assert L.gta_abi_version() == 2


def _call(entry, desc, **args):
    """tests/test_abi_refusals.py's `_call` for the two new entries"""
    if entry.endswith("_supported"):
        return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc))
    full = {name: R.X for name in GATHER_ARGS}
    full.update(workspace_bytes=R.BIG, stream=None)
    full.update(args)
    return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc), *(full[name] for name in GATHER_ARGS))


RENAME = {"gta_attn_fwd_varlen": "gta_attn_fwd_gather", "gta_attn_fwd_varlen_supported": "gta_attn_fwd_gather_supported"}
ROWS = [pytest.param(RENAME[p.values[0]], *p.values[1:], id=f"{RENAME[p.values[0]]}-{i}") for i, p in enumerate(R.ROWS) if p.values[0] in RENAME]
ROWS.append(pytest.param("gta_attn_fwd_gather", {}, {"key_idx": None}, R.BADARG, "null key_idx", id="gta_attn_fwd_gather-null-key_idx"))


def test_the_varlen_rows_are_all_there():
    """(the table above is built from another module's: it must not come out empty)"""
    assert all(hasattr(native.lib(), e) and e in native.ABI_SYMBOLS for e in RENAME.values())
    n_call = sum(1 for p in ROWS if p.values[0] == "gta_attn_fwd_gather")
    n_sup = sum(1 for p in ROWS if p.values[0] == "gta_attn_fwd_gather_supported")
    assert n_call >= 35 and n_sup >= 20, (n_call, n_sup)
    texts = {p.values[4] for p in ROWS}
    for t in ("null key_lens", "null key_idx", "per-scene key prefixes need the workspace of gta_attn_fwd_workspace_bytes()",
              "per-scene key prefixes run the two-stage plan: no GTA_FLAG_FUSED_KV", "null q/k/v/out"):
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
    d = R._desc(flags=R.VT | native.FLAG_KV_READY)
    rc = _call("gta_attn_fwd_gather", d, key_idx=None, workspace_bytes=4096)
    assert rc == R.BADARG and "workspace smaller" in native.lib().gta_strerror(rc).decode()
    rc = _call("gta_attn_fwd_gather", R._desc(), key_idx=None, workspace_bytes=4096)
    assert rc == R.BADARG and "null key_idx" in native.lib().gta_strerror(rc).decode()


# ---- key_index_tensors ------------------------------------------------------------------------------------------------------------------------
def test_key_index_tensors():
    T = 11
    all_true = torch.ones(2, T, dtype=torch.bool)
    idx, lens = G2.key_index_tensors(all_true, "cpu")
    assert idx.dtype == torch.int32 and lens.dtype == torch.int32 and idx.is_contiguous()
    assert idx.tolist() == [list(range(T))] * 2 and lens.tolist() == [T, T]
    one = torch.zeros(2, T, dtype=torch.bool)
    one[0, 7] = one[1, 0] = True
    idx, lens = G2.key_index_tensors(one, "cpu")
    assert lens.tolist() == [1, 1] and idx[0, 0] == 7 and idx[1, 0] == 0
    assert idx[0, 1:].tolist() == [t for t in range(T) if t != 7]                     # the masked tokens follow, in order (never read)
    inter = torch.arange(T)[None].expand(2, -1) % 2 == 1
    idx, lens = G2.key_index_tensors(inter, "cpu")
    assert lens.tolist() == [5, 5] and idx[0, :5].tolist() == [1, 3, 5, 7, 9] and idx[0, 5:].tolist() == [0, 2, 4, 6, 8, 10]
    assert torch.equal(idx.long(), GI.index_tensors(inter)[0])
    empty = inter.clone()
    empty[1] = False
    with pytest.raises(native.GtaError, match=r"scenes \[1\] have no valid key"):
        G2.key_index_tensors(empty, "cpu")
    for bad in (inter.int(), inter[0], [True, False]):
        with pytest.raises(native.GtaError, match="bool tensor"):
            G2.key_index_tensors(bad, "cpu")
    assert gta_amd.key_index_tensors is G2.key_index_tensors


# ---- Python refusals --------------------------------------------------------------------------------------------------------------------------
def _mask(b=B, t=TK):
    m = torch.ones(b, t, dtype=torch.bool)
    m[:, 1::3] = False
    return m


def _cpu_call(f_dims=CL, dh=64, euclid=False, grad=False, mask=None, **kw):
    """gta_attention on CPU tensors: reaches a kernel only if nothing refuses first (and would then raise for the missing device)"""
    q = torch.zeros(B, H, TQ, dh, requires_grad=grad)
    k = torch.zeros(B, H, TK, dh)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
    return gta_amd.gta_attention(q, k, k, f_dims, packed, key_mask=_mask() if mask is None else mask, euclid=euclid, **kw)


def test_refused_combinations_name_their_reason():
    with pytest.raises(native.GtaError, match="key_mask is forward-only"):
        _cpu_call(grad=True)
    with torch.no_grad():
        with pytest.raises(native.GtaError, match="key_mask has no precise=True"):
            _cpu_call(precise=True)
        with pytest.raises(native.GtaError, match="key_mask with pretransformed=True"):
            _cpu_call(pretransformed=True)
        with pytest.raises(native.GtaError, match="key_mask runs the two-stage plan: kv_mode='fused'"):
            _cpu_call(kv_mode="fused")
        with pytest.raises(native.GtaError, match="key_mask with key_views"):
            _cpu_call(key_views=[1] * B)
        with pytest.raises(native.GtaError, match="key_mask with key_views"):
            _cpu_call(key_lens=torch.zeros(B, dtype=torch.int32))
        # the staged layouts (euclid, t2) and the rho-apply ones (dh % 8 != 0)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*euclid"):
            _cpu_call(f_dims=EUCLID, euclid=True)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*t2"):
            _cpu_call(f_dims={"se3": 32, "t2": 30, "triv": 2})
        with pytest.raises(native.GtaError, match="no gather pre-pass.*dh % 8"):
            _cpu_call(f_dims={"se3": 8, "so2": 4}, dh=12)
        # the mask itself
        with pytest.raises(native.GtaError, match="bool tensor"):
            _cpu_call(mask=_mask().int())
        with pytest.raises(native.GtaError, match=re.escape(f"key_mask has shape ({B}, {TK - 1})")):
            _cpu_call(mask=_mask(t=TK - 1))
        empty = _mask()
        empty[2] = False
        with pytest.raises(native.GtaError, match=r"scenes \[2\] have no valid key"):
            _cpu_call(mask=empty)
        with pytest.raises(native.GtaError, match="gta_attention_by_view_groups takes no key_mask"):
            k = torch.zeros(B, H, TK, 64)
            gta_amd.gta_attention_by_view_groups(torch.zeros(B, H, TQ, 64), k, k, CL, {"vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)},
                                                 views_per_call=2, key_mask=_mask())
        # nothing refuses: the call gets as far as the checks in front of the kernels, which have no CPU path
        with pytest.raises(native.GtaError, match="cpu|CUDA"):
            _cpu_call()


def test_routes():
    shape = (B, H, TQ, 64)
    for dt in (torch.float32, torch.bfloat16):
        fl = G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=True)
        assert fl is not None and not fl & (native.FLAG_FUSED_KV | native.FLAG_FP32_PRODUCTS | native.FLAG_PRETRANSFORMED)
        assert G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=False) == G2.attention_route(shape, TK, dt, CL, 0, 1, NK)
        with pytest.raises(native.GtaError, match="no gather pre-pass"):
            G2.attention_route(shape, TK, dt, EUCLID, 0, 1, NK, euclid=True, key_mask=True)


def test_layers_refuse_return_attmap_and_elementwise_mul():
    from gta_amd import layers
    args = {"f_dims": CL, "so2": 8, "max_freq_h": 1, "max_freq_w": 1}
    att = layers.Attention(128, heads=2, dim_head=64, attn_args={"method": {"name": "gta", "args": args}})
    q = torch.zeros(2, 2, 8, 64)
    m = torch.ones(2, 8, dtype=torch.bool)
    with torch.no_grad(), pytest.raises(native.GtaError, match="key_mask with return_attmap"):
        att.core(q, q, q, {"key_mask": m}, return_attmap=True)
    att.elementwise_mul = True
    with torch.no_grad(), pytest.raises(native.GtaError, match="key_mask: the elementwise_mul ablation"):
        att.core(q, q, q, {"key_mask": m})


def test_srt_hands_the_mask_on_in_a_copy_of_extras():
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    model.encoder = lambda images, cam, rays, extras: (None, extras)
    model.decode = lambda z, x, rays, extras=None: extras
    mine = {"input_coord": 1}
    m3 = torch.ones(2, 3, 4, dtype=torch.bool)
    seen = model(None, None, None, None, None, mine, input_mask=m3)
    assert tuple(seen["key_mask"].shape) == (2, 12) and mine == {"input_coord": 1}
    assert tuple(model(None, None, None, None, None, mine, input_mask=m3.flatten(1))["key_mask"].shape) == (2, 12)
    assert "key_mask" not in model(None, None, None, None, None, mine)
    with pytest.raises(native.GtaError, match="input_mask with input_views"):
        model(None, None, None, None, None, mine, input_mask=m3, input_views=[1, 2])
    with pytest.raises(native.GtaError, match="bool tensor"):
        model(None, None, None, None, None, mine, input_mask=m3.float())


def test_kv_cache_keeps_indices_and_lengths_beside_the_images(monkeypatch):
    """the first call stores key_idx / key_lens and a plan key that says "key_mask"; the second runs on the stored lengths under KV_READY and
    is handed no indices; a call without the mask (or with key_views) on that cache is refused"""
    calls = []
    monkeypatch.setattr(native, "attn_fwd_gather", lambda desc, q, k, v, *a: calls.append((desc.flags, a[6], a[7])))
    monkeypatch.setattr(native, "attn_fwd_varlen", lambda *a, **k: None)
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    cache = {}
    with torch.no_grad():
        _cpu_call(kv_cache=cache)
        assert cache["plan"][-1] == "key_mask" and cache["images"] is not None
        assert cache["key_lens"].tolist() == [int(_mask()[0].sum())] * B and tuple(cache["key_idx"].shape) == (B, TK)
        _cpu_call(kv_cache=cache, mask=torch.ones(B, TK, dtype=torch.bool))        # (not looked at: the cache's lengths hold)
        (f0, i0, l0), (f1, i1, l1) = calls
        assert not f0 & native.FLAG_KV_READY and i0 is cache["key_idx"] and l0 is cache["key_lens"]
        assert f1 & native.FLAG_KV_READY and i1 is None and l1 is cache["key_lens"]
        q = torch.zeros(B, H, TQ, 64)
        k = torch.zeros(B, H, TK, 64)
        packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
        with pytest.raises(native.GtaError, match="another plan"):
            gta_amd.gta_attention(q, k, k, CL, packed, kv_cache=cache)
        with pytest.raises(native.GtaError, match="another plan"):
            gta_amd.gta_attention(q, k, k, CL, packed, kv_cache=cache, key_views=[5] * B)


# ---- the gather rule against a host emulation ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _emu_case():
    """B = 3 scenes, H = 2, 3 views of 50 tokens (Tk = 150: three tiles), se3 | so2 at dh 32; masks: every third token dropped (100 keys: two
    tiles, 28 dead rows), one view and a half (75 keys), all keys"""
    c = I.key_side_case({"se3": 16, "so2": 16}, 0, torch.bfloat16, B=3, H=2, Nk=3, Pk=50, seed=11)
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, c.so3, 0.37)
    mask = torch.ones(3, c.T, dtype=torch.bool)
    mask[0, 2::3] = False
    mask[1, :25] = False
    mask[1, 100:] = False
    idx, lens = (t.long() for t in G2.key_index_tensors(mask, "cpu"))               # (the emulation runs on what the operator would hand the kernel)
    assert lens.tolist() == [100, 75, 150] and torch.equal(idx, GI.index_tensors(mask)[0])
    return c, ref, idx, lens, I.fused_layout(c.B, c.H, c.T, c.dh).total + 512


def test_host_emulation_passes_the_rules():
    c, ref, idx, lens, total = _emu_case()
    ws = GI.emulate(c, ref, idx, lens, total)
    GI.check("emulation", ws, c, ref, idx, lens)
    # entries at or past key_lens are never looked at
    junk = idx.clone()
    for b, n in enumerate(lens.tolist()):
        junk[b, n:] = 10 ** 6
    GI.check("emulation", ws, c, ref, junk, lens)


@pytest.mark.parametrize("defect", GI.DEFECTS)
def test_planted_defects_fail_the_rules(defect):
    c, ref, idx, lens, total = _emu_case()
    ws = GI.emulate(c, ref, idx, lens, total, defect=defect)
    assert not torch.equal(ws, GI.emulate(c, ref, idx, lens, total)), defect
    with pytest.raises(AssertionError):
        GI.check(defect, ws, c, ref, idx, lens)

"""Host side of per-scene key prefixes (`key_views`): the exported symbols and their ctypes signatures against include/gta_hip.h, the
host validation of the view counts, the refused combinations (each raises `GtaError` naming its reason before anything is launched --
these tests run without a GPU, on CPU tensors), the routes, and the `kv_cache` plan key."""
import ctypes
import os
import re

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARLEN = ("gta_attn_fwd_varlen", "gta_attn_fwd_varlen_supported", "gta_attn_fwd_staged_varlen", "gta_attn_fwd_staged_varlen_supported")
CL = {"se3": 32, "so2": 32}
EUCLID = {"triv": 2, "se3": 30, "so2": 32}
B, H, NK, PK, TQ = 5, 2, 13, 20, 150
KV = [1, 3, 4, 7, 13]


def _decl(name):
    """the parameter list of `name` in include/gta_hip.h"""
    text = open(os.path.join(ROOT, "include", "gta_hip.h")).read()
    m = re.search(r"^\w[\w\s\*]*?\b" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_symbols_exist_and_signatures_match_the_header():
    L = native.lib()
    for s in VARLEN:
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
    for name, base in (("gta_attn_fwd_varlen", "gta_attn_fwd"), ("gta_attn_fwd_staged_varlen", "gta_attn_fwd_staged")):
        args, base_args = _decl(name), _decl(base)
        # the header: the entry without key_lens, plus `const int32_t* key_lens` in front of out
        i = [a.split()[-1] for a in args].index("key_lens")
        assert args[i] == "const int32_t* key_lens" and args[i + 1].split()[-1] == "out"
        assert args[:i] + args[i + 1:] == base_args
        at = getattr(L, name).argtypes
        assert len(at) == len(args) and at[0] == ctypes.POINTER(native.GtaAttnDesc)
        for a, t in zip(args[1:], at[1:]):
            assert t == (ctypes.c_int64 if a.startswith("int64_t") else ctypes.c_void_p), (name, a, t)
        assert getattr(L, base).argtypes == at[:i] + at[i + 1:]
    for name in ("gta_attn_fwd_varlen_supported", "gta_attn_fwd_staged_varlen_supported"):
        assert _decl(name) == ["const GtaAttnDesc* desc"] and getattr(L, name).argtypes == [ctypes.POINTER(native.GtaAttnDesc)]


def _desc(f_dims, flags, dh=64, dtype=torch.bfloat16):
    qs, ks = (H * TQ * dh, TQ * dh, dh), (H * NK * PK * dh, NK * PK * dh, dh)
    return native.make_desc_from(dtype, (B, H, TQ, dh), NK * PK, (qs, ks, ks, qs), f_dims, 0, 1, NK, 1.0, flags)


def test_supported_entries_answer_without_a_gpu():
    L = native.lib()
    assert native.attn_fwd_varlen_supported(_desc(CL, native.FLAG_V_TRANSFORM)) == 0
    for flag, word in ((native.FLAG_FUSED_KV, "FUSED_KV"), (native.FLAG_FP32_PRODUCTS, "FP32_PRODUCTS"), (native.FLAG_PRETRANSFORMED, "PRETRANSFORMED")):
        rc = native.attn_fwd_varlen_supported(_desc(CL, native.FLAG_V_TRANSFORM | flag, dtype=torch.float32))
        assert rc == -3 and word in L.gta_strerror(rc).decode(), (flag, L.gta_strerror(rc))
    # a generic layout: the fused varlen entry refuses like gta_attn_fwd_supported, the staged one serves it
    eu = _desc(EUCLID, native.FLAG_V_TRANSFORM | native.FLAG_EUCLID)
    assert native.attn_fwd_varlen_supported(eu) == -3 and native.attn_fwd_staged_varlen_supported(eu) == 0
    assert native.attn_fwd_staged_varlen_supported(_desc({"se3": 6, "so2": 8}, native.FLAG_EUCLID, dh=14)) == -3
    # NULL key_lens / NULL workspace: GTA_E_BADARG (checked before any launch)
    d = _desc(CL, native.FLAG_V_TRANSFORM)
    x = ctypes.c_void_p(256)
    assert L.gta_attn_fwd_varlen(ctypes.byref(d), x, x, x, x, x, x, x, None, None, None, x, x, x, 1 << 40, None) == -1
    assert "key_lens" in L.gta_strerror(-1).decode()
    assert L.gta_attn_fwd_varlen(ctypes.byref(d), x, x, x, x, x, x, x, None, None, x, x, x, None, 0, None) == -1
    assert L.gta_attn_fwd_staged_varlen(ctypes.byref(eu), x, x, x, x, x, x, x, None, None, None, None, None, x, x, x, 1 << 40, None) == -1
    assert L.gta_attn_fwd_staged_varlen(ctypes.byref(eu), x, x, x, x, x, x, x, None, None, None, None, x, x, x, None, 0, None) == -1


def test_check_key_views():
    assert G2.check_key_views(KV, B, NK) == tuple(KV)
    assert G2.check_key_views(torch.tensor(KV), B, NK) == tuple(KV)
    assert G2.check_key_views(torch.tensor(KV, dtype=torch.int32), B, NK) == tuple(KV)
    for bad, word in ((KV[:4], "entries"), (KV + [1], "entries"), ([0, 3, 4, 7, 13], "1..Nk"), ([1, 3, 4, 7, 14], "1..Nk"),
                      ([1.0, 3, 4, 7, 13], "integers"), (torch.tensor([1.0] * 5), "integer"), (7, "sequence")):
        with pytest.raises(native.GtaError, match=re.escape(word)):
            G2.check_key_views(bad, B, NK)
    with pytest.raises(native.GtaError, match="view"):
        G2.check_key_views(KV, B, None)
    assert G2.key_lens_tensor((1, 3), 20, "cpu").tolist() == [20, 60] and G2.key_lens_tensor((1, 3), 20, "cpu").dtype == torch.int32


def _cpu_call(f_dims=CL, key_views=KV, dh=64, euclid=False, grad=False, views=True, **kw):
    """gta_attention on CPU tensors: reaches a kernel only if nothing refuses first (and would then raise for the missing device)"""
    q = torch.zeros(B, H, TQ, dh, requires_grad=grad)
    k = torch.zeros(B, H, NK * PK, dh)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)} if views else {}
    return gta_amd.gta_attention(q, k, k, f_dims, packed, key_views=key_views, euclid=euclid, **kw)


@pytest.mark.parametrize("bad, word", [(KV[:4], "4 entries"), ([0, 3, 4, 7, 13], "1..Nk"), ([1, 3, 4, 7, 14], "1..Nk")])
def test_gta_attention_validates_on_the_host(bad, word):
    with torch.no_grad(), pytest.raises(native.GtaError, match=re.escape(word)):
        _cpu_call(key_views=bad)


def test_refused_combinations_name_their_reason():
    with pytest.raises(native.GtaError, match="forward-only"):
        _cpu_call(grad=True)
    with torch.no_grad():
        with pytest.raises(native.GtaError, match="precise"):
            _cpu_call(precise=True)
        with pytest.raises(native.GtaError, match="pretransformed"):
            _cpu_call(pretransformed=True)
        with pytest.raises(native.GtaError, match="kv_mode='fused'"):
            _cpu_call(kv_mode="fused")
        with pytest.raises(native.GtaError, match=r"_GenericAttn.*dh % 8"):
            _cpu_call(f_dims={"se3": 6, "so2": 8}, dh=14, euclid=True)
        with pytest.raises(native.GtaError, match="view structure"):
            _cpu_call(f_dims={"so2": 64}, views=False)
        with pytest.raises(native.GtaError, match="key_views"):
            gta_amd.gta_attention(torch.zeros(1, 1, 8, 64), torch.zeros(1, 1, 8, 64), torch.zeros(1, 1, 8, 64), CL, {}, key_lens=torch.zeros(1, dtype=torch.int32))
        # nothing refuses: the call gets as far as the checks in front of the kernels, which have no CPU path
        with pytest.raises(native.GtaError, match="cpu|CUDA"):
            _cpu_call()


def test_layers_refuse_return_attmap_and_the_drop_in_passes_key_views():
    from gta_amd import layers
    att = layers.Attention(128, heads=2, dim_head=64, attn_args={"method": {"name": "gta", "args": {"f_dims": CL, "so2": 8, "max_freq_h": 1, "max_freq_w": 1}}})
    q = torch.zeros(2, 2, 8, 64)
    with torch.no_grad(), pytest.raises(native.GtaError, match="return_attmap"):
        att.core(q, q, q, {"key_views": [1, 1]}, return_attmap=True)
    with torch.no_grad(), pytest.raises(native.GtaError, match="2 entries"):
        gta_amd.multihead_geometric_transform_attention(torch.zeros(B, H, TQ, 64), torch.zeros(B, H, NK * PK, 64), torch.zeros(B, H, NK * PK, 64),
                                                        f_dims=CL, reps={"gta_vrep_q": torch.zeros(B, 1, native.VREP_STRIDE),
                                                                         "gta_vrep_k": torch.zeros(B, NK, native.VREP_STRIDE),
                                                                         "gta_cs_q": torch.zeros(B, TQ, 16, 2), "gta_cs_k": torch.zeros(B, NK * PK, 16, 2)},
                                                        key_views=[1, 2])


def test_routes():
    shape = (B, H, TQ, 64)
    for dt in (torch.float32, torch.bfloat16):
        # without key_views the answers are the ones the routes gave before the keyword existed, pinned here flag by flag (150 query rows:
        # 'auto' is the single-kernel plan; a cache or kv_mode='prepass' the two-stage plan)
        V, FUSED_KV = native.FLAG_V_TRANSFORM, native.FLAG_FUSED_KV
        for kw, want in (({}, V | FUSED_KV), ({"kv_mode": "prepass"}, V), ({"kv_cache": True}, V), ({"needs_grad": True}, V | FUSED_KV),
                         ({"kv_mode": "fused"}, V | FUSED_KV), ({"kv_mode": "prepass_fwd2"}, V | native.FLAG_ROWS32 | native.FLAG_FWD2_GENERIC),
                         ({"v_transform": False, "use_dma": False}, native.FLAG_NO_DMA | FUSED_KV)):
            assert G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK, **kw) == want, kw
            assert G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK, key_views=False, **kw) == want, kw
        assert G2.attention_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True) is None
        assert G2.generic_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True) == G2.generic_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True, key_views=False) == "staged"
        # 150 query rows: 'auto' picks the single-kernel plan; with key_views the two-stage plan, whatever the shape
        assert G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK) & native.FLAG_FUSED_KV
        fl = G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK, key_views=True)
        assert fl is not None and not fl & (native.FLAG_FUSED_KV | native.FLAG_FP32_PRODUCTS | native.FLAG_PRETRANSFORMED)
        assert G2.attention_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True, key_views=True) is None
        assert G2.generic_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True, key_views=True) == "staged"
    for kw in ({"needs_grad": True}, {"precise": True}):
        with pytest.raises(native.GtaError):
            G2.generic_route(shape, NK * PK, torch.float32, EUCLID, 0, 1, NK, euclid=True, key_views=True, **kw)


def test_srt_forward_leaves_the_callers_extras_alone():
    """`TransformingSRT.forward(input_views=...)` hands the counts on in a copy of `extras`: a later call that reuses the caller's dict
    without `input_views` is not masked by them"""
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    model.encoder = lambda images, cam, rays, extras: (None, extras)
    model.decode = lambda z, x, rays, extras=None: extras
    mine = {"input_coord": 1}
    seen = model(None, None, None, None, None, mine, input_views=[2, 3])
    assert seen["key_views"] == [2, 3] and seen["input_coord"] == 1 and mine == {"input_coord": 1}
    assert "key_views" not in model(None, None, None, None, None, mine)


def test_kv_cache_plan_key_carries_the_view_counts(monkeypatch):
    """the plan key a cache is written under differs between two view-count vectors (and from the call without key_views), in both families"""
    for f_dims, euclid, entry in ((CL, False, "attn_fwd_varlen"), (EUCLID, True, "attn_fwd_staged_varlen")):
        monkeypatch.setattr(native, entry, lambda *a, **k: None)
        monkeypatch.setattr(native, "attn_fwd_staged", lambda *a, **k: None)
        monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
        keys = []
        for kv in (KV, [2, 3, 4, 7, 13]):
            cache = {}
            with torch.no_grad():
                _cpu_call(f_dims=f_dims, euclid=euclid, key_views=kv, kv_cache=cache)
            assert cache["plan"][-1] == tuple(kv) and cache["images"] is not None
            keys.append(cache["plan"])
        assert keys[0] != keys[1] and keys[0][:-1] == keys[1][:-1]
        # a cache written under other view counts is refused with the message of every other plan mismatch
        with torch.no_grad(), pytest.raises(native.GtaError, match="kv_cache holds images written under another plan"):
            _cpu_call(f_dims=f_dims, euclid=euclid, key_views=KV, kv_cache=cache)

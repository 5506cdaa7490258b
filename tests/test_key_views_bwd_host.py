"""Host side of the backward with per-scene prefixes (`key_views_backward`, `query_views`; `gta_attn_bwd_varlen`): the new symbols against
include/gta_hip.h, the opt-in (the default still says "forward-only"), the validation of `query_views`, the refusals that remain -- each a
`GtaError` naming its reason before anything is launched -- and the routes.  No GPU: CPU tensors throughout."""
import ctypes
import os
import re

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CL = {"se3": 32, "so2": 32}
EUCLID = {"triv": 2, "se3": 30, "so2": 32}
B, H, NK, PK, TQ = 5, 2, 13, 20, 150
KV = [1, 3, 4, 7, 13]


def _decl(name):
    text = open(os.path.join(ROOT, "include", "gta_hip.h")).read()
    m = re.search(r"^\w[\w\s\*]*?\b" + name + r"\(([^;]*?)\);", text, re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_symbols_are_declared_and_bound():
    L = native.lib()
    for s in ("gta_attn_bwd_varlen", "gta_attn_bwd_varlen_supported"):
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
    args, base = _decl("gta_attn_bwd_varlen"), _decl("gta_attn_bwd")
    # the header: gta_attn_bwd's arguments with key_lens, q_lens in front of kv_images
    i = [a.split()[-1] for a in args].index("key_lens")
    assert args[i:i + 2] == ["const int32_t* key_lens", "const int32_t* q_lens"] and args[i + 2].split()[-1] == "kv_images"
    assert args[:i] + args[i + 2:] == base
    at = L.gta_attn_bwd_varlen.argtypes
    assert len(at) == len(args) and at[0] == ctypes.POINTER(native.GtaAttnDesc)
    assert L.gta_attn_bwd.argtypes == at[:i] + at[i + 2:] and at[i] == at[i + 1] == ctypes.c_void_p
    assert _decl("gta_attn_bwd_varlen_supported") == ["const GtaAttnDesc* desc"]
    assert L.gta_attn_bwd_varlen_supported.argtypes == [ctypes.POINTER(native.GtaAttnDesc)]
    assert native.GTA_ABI_VERSION == 2 and L.gta_abi_version() == 2


def _desc(f_dims, flags, dh=64, dtype=torch.bfloat16):
    qs, ks = (H * TQ * dh, TQ * dh, dh), (H * NK * PK * dh, NK * PK * dh, dh)
    return native.make_desc_from(dtype, (B, H, TQ, dh), NK * PK, (qs, ks, ks, qs), f_dims, 0, 1, NK, 1.0, flags)


def test_supported_entry_answers_without_a_gpu():
    L = native.lib()
    assert native.attn_bwd_varlen_supported(_desc(CL, native.FLAG_V_TRANSFORM)) == 0
    assert native.attn_bwd_varlen_supported(_desc(CL, native.FLAG_V_TRANSFORM | native.FLAG_BWD_KEYS64)) == 0      # (ignored)
    for flag, word in ((native.FLAG_FUSED_KV, "FUSED_KV"), (native.FLAG_FP32_PRODUCTS, "FP32_PRODUCTS"), (native.FLAG_PRETRANSFORMED, "PRETRANSFORMED")):
        rc = native.attn_bwd_varlen_supported(_desc(CL, native.FLAG_V_TRANSFORM | flag, dtype=torch.float32))
        assert rc == -3 and word in L.gta_strerror(rc).decode(), (flag, L.gta_strerror(rc))
    eu = _desc(EUCLID, native.FLAG_V_TRANSFORM | native.FLAG_EUCLID)
    assert native.attn_bwd_varlen_supported(eu) == -3 and "fused kernel" in L.gta_strerror(-3).decode()


def _cpu_call(f_dims=CL, key_views=KV, dh=64, euclid=False, grad=True, nq=1, **kw):
    q = torch.zeros(B, H, TQ, dh, requires_grad=grad)
    k = torch.zeros(B, H, NK * PK, dh)
    packed = {"vrep_q": torch.zeros(B, nq, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
    packed.update(kw.pop("tables", {}))
    return gta_amd.gta_attention(q, k, k, f_dims, packed, key_views=key_views, euclid=euclid, **kw)


def test_opt_in_reaches_the_device_check_and_the_default_does_not():
    with pytest.raises(native.GtaError, match="forward-only"):
        _cpu_call()
    with pytest.raises(native.GtaError, match="forward-only"):
        _cpu_call(key_views_backward=False)
    # nothing refuses: the call gets as far as the checks in front of the kernels, which have no CPU path
    with pytest.raises(native.GtaError, match="cpu|CUDA"):
        _cpu_call(key_views_backward=True)
    with pytest.raises(native.GtaError, match="cpu|CUDA"):
        _cpu_call(key_views_backward=True, query_views=[1] * B)
    with pytest.raises(native.GtaError, match="comes with key_views"):
        _cpu_call(key_views=None, key_views_backward=True)


def test_query_views_validation():
    with pytest.raises(native.GtaError, match="needs key_views_backward"):
        _cpu_call(query_views=[1] * B)
    with torch.no_grad(), pytest.raises(native.GtaError, match="needs key_views_backward"):
        _cpu_call(query_views=[1] * B)
    for bad, word in (([1] * 4, "query_views has 4 entries"), ([0, 1, 1, 1, 1], "1..Nq = 1..5"), ([1, 1, 1, 1, 6], "1..Nq = 1..5"),
                      ([1.0] * B, "query_views must hold integers")):
        with pytest.raises(native.GtaError, match=re.escape(word)):
            _cpu_call(key_views_backward=True, query_views=bad, nq=5)
    assert G2.check_key_views([1, 2], 2, 3, name="query_views") == (1, 2)


def test_remaining_refusals_name_their_reason():
    kw = {"key_views_backward": True}
    with pytest.raises(native.GtaError, match="precise"):
        _cpu_call(precise=True, **kw)
    with pytest.raises(native.GtaError, match="pretransformed"):
        _cpu_call(pretransformed=True, **kw)
    with pytest.raises(native.GtaError, match="kv_mode='fused'"):
        _cpu_call(kv_mode="fused", **kw)
    with pytest.raises(native.GtaError, match="staged generic layouts"):
        _cpu_call(f_dims=EUCLID, euclid=True, **kw)
    with pytest.raises(native.GtaError, match="rep tables or poses"):
        _cpu_call(tables={"vrep_k": torch.zeros(B, NK, native.VREP_STRIDE, requires_grad=True)}, **kw)
    from gta_amd import layers
    att = layers.Attention(128, heads=2, dim_head=64, attn_args={"method": {"name": "gta", "args": {"f_dims": CL, "so2": 8, "max_freq_h": 1, "max_freq_w": 1}}})
    q = torch.zeros(2, 2, 8, 64)
    with pytest.raises(native.GtaError, match="return_attmap"):
        att.core(q, q, q, {"key_views": [1, 1], "key_views_backward": True}, return_attmap=True)


def test_routes():
    shape = (B, H, TQ, 64)
    bad = native.FLAG_FUSED_KV | native.FLAG_FP32_PRODUCTS | native.FLAG_PRETRANSFORMED
    for dt in (torch.float32, torch.bfloat16):
        fl = G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK, key_views=True, key_views_backward=True, needs_grad=True)
        assert fl is not None and not fl & bad
        assert fl == G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK, key_views=True)          # the flags of the forward-only call
        with pytest.raises(native.GtaError, match="forward-only"):
            G2.attention_route(shape, NK * PK, dt, CL, 0, 1, NK, key_views=True, needs_grad=True)
        assert G2.attention_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True, key_views=True, key_views_backward=True, needs_grad=True) is None
        with pytest.raises(native.GtaError, match="staged generic layouts"):
            G2.generic_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True, key_views=True, key_views_backward=True, needs_grad=True)
        assert G2.generic_route(shape, NK * PK, dt, EUCLID, 0, 1, NK, euclid=True, key_views=True, key_views_backward=True) == "staged"


def test_srt_forward_sets_the_keywords_per_stage():
    """input_views_backward: key_views_backward for every layer, query_views for the encoder alone; the caller's dict stays as it was"""
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    seen = {}
    model.encoder = lambda images, cam, rays, extras: (seen.update(enc=dict(extras)), (None, extras))[1]
    model.decode = lambda z, x, rays, extras=None: extras
    mine = {"input_coord": 1}
    dec = model(None, None, None, None, None, mine, input_views=[2, 3], input_views_backward=True)
    assert seen["enc"]["key_views"] == [2, 3] and seen["enc"]["key_views_backward"] is True and seen["enc"]["query_views"] == [2, 3]
    assert dec["key_views"] == [2, 3] and dec["key_views_backward"] is True and "query_views" not in dec and mine == {"input_coord": 1}
    dec = model(None, None, None, None, None, mine, input_views=[2, 3])
    assert "key_views_backward" not in dec and "query_views" not in dec

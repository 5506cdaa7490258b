"""Host path of `gta_attention` (no GPU): the `kv_cache` plan key of both families -- equal for equal calls, different across everything the
cached K'/V' images depend on -- and the messages of `check_key_views` under both argument names."""
import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native

CL = {"se3": 32, "so2": 32}                         # fused family
EUCLID = {"triv": 2, "se3": 30, "so2": 32}          # staged family (euclid=True)
T2 = {"se3": 32, "t2": 30, "triv": 2}               # staged family
B, H, NK, PK, TQ = 5, 2, 13, 20, 150
KV = [1, 3, 4, 7, 13]


def _plan(monkeypatch, f_dims=CL, dtype=torch.float32, key_views=None, **kw):
    """the plan key a first call leaves in its cache (CPU tensors; the launches and the table checks are stubbed out)"""
    for entry in ("attn_fwd", "attn_fwd_varlen", "attn_fwd_staged", "attn_fwd_staged_varlen"):
        monkeypatch.setattr(native, entry, lambda *a, **k: None)
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    q = torch.zeros(B, H, TQ, 64, dtype=dtype)
    k = torch.zeros(B, H, NK * PK, 64, dtype=dtype)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
    cache = {}
    with torch.no_grad():
        gta_amd.gta_attention(q, k, k, f_dims, packed, kv_cache=cache, key_views=key_views, **kw)
    assert cache["images"] is not None
    return cache["plan"]


FAMILIES = [("fused", dict(f_dims=CL)), ("staged", dict(f_dims=EUCLID, euclid=True)), ("staged-t2", dict(f_dims=T2))]


@pytest.mark.parametrize("key_views", [None, KV], ids=["all-views", "key_views"])
@pytest.mark.parametrize("family, kw", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_plan_key(monkeypatch, family, kw, key_views):
    base = _plan(monkeypatch, key_views=key_views, **kw)
    assert _plan(monkeypatch, key_views=key_views, **kw) == base                                   # equal calls
    assert base[-1] == (None if key_views is None else tuple(key_views))                           # the view counts come last
    assert _plan(monkeypatch, key_views=key_views, dtype=torch.bfloat16, **kw) != base
    assert _plan(monkeypatch, key_views=key_views, v_transform=False, **kw) != base
    other = _plan(monkeypatch, key_views=[2, 3, 4, 7, 13], **kw)
    assert other != base and (key_views is None or other[:-1] == base[:-1])
    # the scale enters under euclid alone (the cached key bias carries it)
    assert (_plan(monkeypatch, key_views=key_views, scale=0.25, **kw) != base) == bool(kw.get("euclid"))
    if family == "fused" and key_views is None:            # (precise: fp32 inputs on the fused family, not with key_views)
        assert _plan(monkeypatch, precise=True, **kw) != base


def test_plan_keys_differ_across_families(monkeypatch):
    keys = [_plan(monkeypatch, key_views=kv, **kw) for kv in (None, KV) for _, kw in FAMILIES]
    assert len(set(keys)) == len(keys)


def test_a_cache_of_another_plan_is_refused_in_both_families(monkeypatch):
    for _, kw in FAMILIES:
        for entry in ("attn_fwd", "attn_fwd_staged"):
            monkeypatch.setattr(native, entry, lambda *a, **k: None)
        monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
        q, k = torch.zeros(B, H, TQ, 64), torch.zeros(B, H, NK * PK, 64)
        packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
        cache = {}
        with torch.no_grad():
            gta_amd.gta_attention(q, k, k, packed=packed, kv_cache=cache, **kw)
            gta_amd.gta_attention(q[:, :, :20], k, k, packed=packed, kv_cache=cache, **kw)           # another query chunk: served
            with pytest.raises(native.GtaError, match="kv_cache holds images written under another plan"):
                gta_amd.gta_attention(q, k, k, packed=packed, kv_cache=cache, v_transform=False, **kw)
            cache["images"] = cache["images"][:16]
            with pytest.raises(native.GtaError, match="kv_cache holds images of a different key set"):
                gta_amd.gta_attention(q, k, k, packed=packed, kv_cache=cache, **kw)


VIEW_MESSAGES = [
    (torch.tensor([1.0, 2.0]), 3, "{name} must be a 1-D integer tensor"),
    (torch.tensor([[1, 2]]), 3, "{name} must be a 1-D integer tensor"),
    (torch.tensor([True, False]), 3, "{name} must be a 1-D integer tensor"),
    (7, 3, "{name} must be a sequence of B view counts"),
    ([1, 2.0], 3, "{name} must hold integers, got (1, 2.0)"),
    ([1, True], 3, "{name} must hold integers, got (1, True)"),
    ([1, 2, 3], 3, "{name} has 3 entries for a batch of 2 scenes"),
    ([0, 2], 3, "{name} entries must lie in 1..{bound} = 1..3, got (0, 2)"),
    ([1, 4], 3, "{name} entries must lie in 1..{bound} = 1..3, got (1, 4)"),
    ([1, 2], None, "{name} needs the number of {views} {bound}, which the view tables give ({table}): this layout has no se3 / so3 slab and so no "
                   "view structure"),
]


@pytest.mark.parametrize("name, bound, table, views", [("key_views", "Nk", "vrep_k", "key views"), ("query_views", "Nq", "vrep_q", "query views")])
def test_check_key_views_messages(name, bound, table, views):
    assert G2.check_key_views([1, 3], 2, 3, name=name) == (1, 3)
    assert G2.check_key_views(torch.tensor([1, 3]), 2, 3, name=name) == (1, 3)
    for bad, N, text in VIEW_MESSAGES:
        with pytest.raises(native.GtaError) as e:
            G2.check_key_views(bad, 2, N, name=name)
        assert str(e.value) == text.format(name=name, bound=bound, table=table, views=views)


def test_query_views_messages_as_literals():
    for bad, N, text in (
            ([1, 2, 3], 3, "query_views has 3 entries for a batch of 2 scenes"),
            ([1, 4], 3, "query_views entries must lie in 1..Nq = 1..3, got (1, 4)"),
            ([1, 2.0], 3, "query_views must hold integers, got (1, 2.0)"),
            (7, 3, "query_views must be a sequence of B view counts"),
            (torch.tensor([1.0, 2.0]), 3, "query_views must be a 1-D integer tensor"),
            ([1, 2], None, "query_views needs the number of query views Nq, which the view tables give (vrep_q): this layout has no se3 / so3 slab "
                           "and so no view structure")):
        with pytest.raises(native.GtaError) as e:
            G2.check_key_views(bad, 2, N, name="query_views")
        assert str(e.value) == text

"""Host side of the mask index (`gta_mask_index`, `gta_amd.mask_index`, `gta_attention(..., mask_index=)`, `TransformingSRT(input_mask_index=)`):
the symbol against include/gta_hip.h, the refusals of the C entry (dummy non-null pointers: each returns before anything touches a device),
the way of a record's tensors through `gta_attention` with the native entries and `repgrad.table_grads` replaced by spies and the torch index
functions replaced by ones that raise, the companion refusals, the unchanged messages of the masked call's own refusals, and the one build per
forward of the model.  No GPU: everything runs on CPU tensors."""
import ctypes

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from tests.test_key_views_host import _decl

CL = {"se3": 32, "so2": 32}
EUCLID = {"triv": 2, "se3": 30, "so2": 32}
B, H, N, P = 2, 2, 2, 40
T = N * P
X = ctypes.c_void_p(256)         # a non-null pointer that is never followed
BADARG = -1
COMPANION = "mask_index comes with the key_mask / query_mask it was built from"


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_listed_exported_and_bound():
    L = native.lib()
    assert "gta_mask_index" in native.ABI_SYMBOLS and hasattr(L, "gta_mask_index")
    args = _decl("gta_mask_index")
    assert args == ["const uint8_t* key_mask", "int32_t B", "int32_t Tk", "int32_t* key_idx", "int32_t* key_lens", "uint8_t* k_live",
                    "const uint8_t* query_mask", "int32_t Tq", "int32_t* q_lens", "void* stream"]
    at = L.gta_mask_index.argtypes
    assert len(at) == len(args)
    for a, t in zip(args, at):
        assert t == (ctypes.c_int32 if a.startswith("int32_t ") else ctypes.c_void_p), (a, t)
    assert L.gta_abi_version() == 2 and native.GTA_ABI_VERSION == 2
    assert callable(native.mask_index) and callable(gta_amd.mask_index) and gta_amd.MaskIndex is G2.MaskIndex


FULL = dict(key_mask=X, B=2, Tk=8, key_idx=X, key_lens=X, k_live=X, query_mask=X, Tq=8, q_lens=X, stream=None)
REFUSALS = [
    ("B-zero", dict(B=0), ["B"]),
    ("B-negative", dict(B=-3), ["B"]),
    ("both-masks-null", dict(key_mask=None, query_mask=None), ["key_mask", "query_mask"]),
    ("Tk-zero", dict(Tk=0), ["Tk"]),
    ("Tk-zero-key-side-alone", dict(Tk=0, query_mask=None, Tq=0, q_lens=None), ["Tk"]),
    ("Tq-zero", dict(Tq=0), ["Tq"]),
    ("Tq-negative-query-side-alone", dict(Tq=-1, key_mask=None, Tk=0, key_idx=None, key_lens=None, k_live=None), ["Tq"]),
    ("key-mask-without-key_idx", dict(key_idx=None), ["key_idx"]),
    ("key-mask-without-key_lens", dict(key_lens=None), ["key_lens"]),
    ("key-mask-without-both", dict(key_idx=None, key_lens=None, k_live=None, query_mask=None), ["key_idx"]),
    ("query-mask-without-q_lens", dict(q_lens=None), ["q_lens"]),
    ("query-mask-alone-without-q_lens", dict(key_mask=None, key_idx=None, key_lens=None, k_live=None, q_lens=None), ["q_lens"]),
]


@pytest.mark.parametrize("change, names", [pytest.param(c, n, id=i) for i, c, n in REFUSALS])
def test_refusal_of_the_c_entry(change, names):
    a = dict(FULL, **change)
    rc = native.lib().gta_mask_index(*(a[n] for n in ("key_mask", "B", "Tk", "key_idx", "key_lens", "k_live", "query_mask", "Tq", "q_lens", "stream")))
    text = native.lib().gta_strerror(rc).decode()
    assert rc == BADARG, (rc, text)
    assert text.startswith("bad argument: ")
    for name in names:
        assert name in text, (name, text)


def test_the_binding_holds_the_shapes_against_the_masks(monkeypatch):
    """(the kernel indexes every row from B, Tk and Tq alone: a buffer of another shape or type never reaches it)"""
    monkeypatch.setattr(native, "_require_cuda", lambda *a: pytest.fail("a device check: the shapes come first"))
    m = torch.ones(B, T, dtype=torch.bool)
    idx, lens, live = torch.zeros(B, T, dtype=torch.int32), torch.zeros(B, dtype=torch.int32), torch.zeros(B, T, dtype=torch.bool)
    for bad in (dict(key_idx=idx[:, :-1]), dict(key_idx=idx.long()), dict(key_lens=lens[:1]), dict(k_live=live.to(torch.uint8)),
                dict(k_live=live.t()), dict(q_lens=torch.zeros(B + 1, dtype=torch.int32)), dict(key_mask=m.to(torch.uint8)),
                dict(query_mask=torch.ones(B + 1, T, dtype=torch.bool)), dict(key_idx=None), dict(q_lens=None)):
        a = dict(key_mask=m, key_idx=idx, key_lens=lens, k_live=live, query_mask=m, q_lens=lens.clone())
        a.update(bad)
        with pytest.raises(native.GtaError, match="gta_mask_index: " + next(iter(bad))):
            native.mask_index(**a)
    with pytest.raises(native.GtaError, match="needs a key_mask or a query_mask"):
        native.mask_index(None, None, None, None, None, None)


# ---- the record ---------------------------------------------------------------------------------------------------------------------------------
def _key_mask():
    m = torch.ones(B, T, dtype=torch.bool)
    m[0, P:] = False                       # a whole view of scene 0
    m[1, 3::7] = False                     # scattered tokens of scene 1
    return m


def _query_mask():
    m = torch.ones(B, T, dtype=torch.bool)
    m[1, :P] = False                       # a dead scene-view
    m[0, T - 5:] = False
    return m


def _record(km, qm, all_keys=False):
    """a MaskIndex put together by hand from the torch functions, on the CPU; ``all_keys``: a record without a key side carrying the index of
    every key, so that the call builds nothing at all"""
    f = {}
    if km is not None:
        f["key_idx"], f["key_lens"] = G2.key_index_tensors(km, "cpu")
        f["k_live"] = G2.effective_key_mask(km, "cpu", unvalidated=True)
    elif all_keys:
        f["key_idx"], f["key_lens"] = G2._all_keys_tensors(B, T, torch.device("cpu"))
    if qm is not None:
        f["q_live"], f["q_lens"] = G2.query_mask_tensors(qm, "cpu")
    return G2.MaskIndex(key_mask=km, query_mask=qm, **f)


def test_fields_and_keys_only():
    km, qm = _key_mask(), _query_mask()
    assert G2.MaskIndex._fields == ("key_mask", "query_mask", "key_idx", "key_lens", "k_live", "q_live", "q_lens")
    mi = _record(km, qm)
    assert mi.key_mask is km and mi.query_mask is qm
    with pytest.raises(AttributeError):
        mi.key_idx = None
    ko = mi.keys_only()
    assert isinstance(ko, G2.MaskIndex) and ko.key_mask is km and ko.key_idx is mi.key_idx and ko.key_lens is mi.key_lens and ko.k_live is mi.k_live
    assert ko.query_mask is None and ko.q_live is None and ko.q_lens is None
    only_k = _record(km, None)
    assert only_k.query_mask is None and only_k.q_live is None and only_k.q_lens is None
    only_q = _record(None, qm)
    assert only_q.key_mask is None and only_q.key_idx is None and only_q.key_lens is None and only_q.k_live is None


def _no_torch_index_chain(monkeypatch):
    for name in ("key_index_tensors", "query_mask_tensors", "effective_key_mask", "_all_keys_tensors"):
        monkeypatch.setattr(G2, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called beside a mask_index"))


def _spies(monkeypatch, seen):
    def fwd_gather(desc, q, k, v, vq, vk, cq, ck, tc, ta, key_idx, key_lens, out, lse, ws):
        seen["fwd"] = dict(key_idx=key_idx, key_lens=key_lens, q_live=None)
        out.zero_()

    def fwd_qmask(desc, q, k, v, vq, vk, cq, ck, tc, ta, key_idx, key_lens, q_live, out, lse, ws):
        seen["fwd"] = dict(key_idx=key_idx, key_lens=key_lens, q_live=q_live)
        out.zero_()

    def bwd_gather(desc, q, k, v, out, dout, lse, vq, vk, cq, ck, tc, ta, key_idx, key_lens, kv_images, dq, dk, dv, dtc, ws, dta=None):
        seen["bwd"] = dict(key_idx=key_idx, key_lens=key_lens, q_live=None, q_lens=None)
        for t in (dq, dk, dv, dtc):
            t.fill_(1.0)

    def bwd_qmask(desc, q, k, v, out, dout, lse, vq, vk, cq, ck, tc, ta, key_idx, key_lens, q_live, q_lens, kv_images, dq, dk, dv, dtc, ws, dta=None):
        seen["bwd"] = dict(key_idx=key_idx, key_lens=key_lens, q_live=q_live, q_lens=q_lens)
        for t in (dq, dk, dv, dtc):
            t.fill_(1.0)

    def grads(desc, tables, meta, tc, q_pairs, k_pairs, direct, **kw):
        seen["tg"] = kw
        return [None if m is None else torch.zeros(m[0], dtype=m[1]) for m in meta]

    monkeypatch.setattr(native, "attn_fwd_gather", fwd_gather)
    monkeypatch.setattr(native, "attn_fwd_qmask", fwd_qmask)
    monkeypatch.setattr(native, "attn_bwd_gather", bwd_gather)
    monkeypatch.setattr(native, "attn_bwd_qmask", bwd_qmask)
    monkeypatch.setattr(native, "mask_index", lambda *a, **k: pytest.fail("a launch beside a ready record"))
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    monkeypatch.setattr(G2, "_refuse_cpu_carriers", lambda *a, **k: None)       # (the tables of this test live on the CPU)
    monkeypatch.setattr(G2._repgrad, "table_grads", grads)


def _operands(grad, table_grad=False):
    q, k, v = (torch.zeros(B, H, T, 64, requires_grad=grad) for _ in range(3))
    packed = {"vrep_q": torch.zeros(B, N, native.VREP_STRIDE, requires_grad=table_grad), "vrep_k": torch.zeros(B, N, native.VREP_STRIDE, requires_grad=table_grad),
              "cs_q": torch.zeros(B, T, 16), "cs_k": torch.zeros(B, T, 16, requires_grad=table_grad)}
    return q, k, v, packed


SIDES = [pytest.param(True, False, id="key-mask"), pytest.param(False, True, id="query-mask"), pytest.param(True, True, id="both")]


@pytest.mark.parametrize("with_key, with_query", SIDES)
def test_the_records_tensors_reach_forward_backward_and_table_grads(monkeypatch, with_key, with_query):
    """under grad with carriers (`key_mask_rep_grad`): both native entries and `table_grads` get the record's very objects, nothing is built"""
    km, qm = _key_mask() if with_key else None, _query_mask() if with_query else None
    mi = _record(km, qm, all_keys=True)
    seen = {}
    _spies(monkeypatch, seen)
    _no_torch_index_chain(monkeypatch)
    q, k, v, packed = _operands(True, table_grad=True)
    masks = {n: m for n, m in (("key_mask", km), ("query_mask", qm)) if m is not None}
    out = gta_amd.gta_attention(q, k, v, CL, packed, trans_coeff=0.5, key_mask_backward=True, key_mask_rep_grad=True, mask_index=mi, **masks)
    assert seen["fwd"]["key_idx"] is mi.key_idx and seen["fwd"]["key_lens"] is mi.key_lens and seen["fwd"]["q_live"] is mi.q_live
    out.sum().backward()
    assert seen["bwd"]["key_idx"] is mi.key_idx and seen["bwd"]["key_lens"] is mi.key_lens
    assert seen["bwd"]["q_live"] is mi.q_live and seen["bwd"]["q_lens"] is mi.q_lens
    assert set(seen["tg"]) == {"masks"} and seen["tg"]["masks"][0] is mi.q_live and seen["tg"]["masks"][1] is mi.k_live
    assert (mi.q_live is None) == (not with_query) and (mi.k_live is None) == (not with_key)
    assert q.grad is not None and k.grad is not None and packed  # (the five gradients and the carriers' came back)


@pytest.mark.parametrize("with_key, with_query", SIDES)
def test_a_record_without_a_key_side_leaves_the_arange_to_the_call(monkeypatch, with_key, with_query):
    """`mask_index(query_mask=...)` has no key fields: the call then builds the index of every key (`_all_keys_tensors`, no sort) as it always
    did, and nothing else; with a key side it builds nothing"""
    km, qm = _key_mask() if with_key else None, _query_mask() if with_query else None
    mi = _record(km, qm)
    seen, built = {}, []
    _spies(monkeypatch, seen)
    real = G2._all_keys_tensors
    for name in ("key_index_tensors", "query_mask_tensors", "effective_key_mask"):
        monkeypatch.setattr(G2, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called beside a mask_index"))
    monkeypatch.setattr(G2, "_all_keys_tensors", lambda *a: built.append(real(*a)) or built[-1])
    q, k, v, packed = _operands(True)
    masks = {n: m for n, m in (("key_mask", km), ("query_mask", qm)) if m is not None}
    gta_amd.gta_attention(q, k, v, CL, packed, trans_coeff=0.5, key_mask_backward=True, mask_index=mi, **masks).sum().backward()
    assert len(built) == (0 if with_key else 1)
    want = (mi.key_idx, mi.key_lens) if with_key else built[0]
    for leg in ("fwd", "bwd"):
        assert seen[leg]["key_idx"] is want[0] and seen[leg]["key_lens"] is want[1] and seen[leg]["q_live"] is mi.q_live
    assert seen["bwd"]["q_lens"] is mi.q_lens and "tg" not in seen


def test_forward_only_with_a_kv_cache_stores_the_records_tensors(monkeypatch):
    km = _key_mask()
    mi = _record(km, None)
    seen = {}
    _spies(monkeypatch, seen)
    _no_torch_index_chain(monkeypatch)
    q, k, v, packed = _operands(False)
    cache = {}
    with torch.no_grad():
        gta_amd.gta_attention(q, k, v, CL, packed, key_mask=km, mask_index=mi, kv_cache=cache)
        assert seen["fwd"]["key_idx"] is mi.key_idx and seen["fwd"]["key_lens"] is mi.key_lens
        assert cache["key_idx"] is mi.key_idx and cache["key_lens"] is mi.key_lens and cache["images"] is not None
        # the next query set: the cached images under the stored lengths, as without a record
        seen.clear()
        gta_amd.gta_attention(q, k, v, CL, packed, key_mask=km, mask_index=mi, kv_cache=cache)
        assert seen["fwd"]["key_idx"] is None and seen["fwd"]["key_lens"] is mi.key_lens
        # and without a cache, without a query mask
        seen.clear()
        gta_amd.gta_attention(q, k, v, CL, packed, key_mask=km, mask_index=mi)
        assert seen["fwd"]["key_idx"] is mi.key_idx and seen["fwd"]["key_lens"] is mi.key_lens and seen["fwd"]["q_live"] is None


def test_without_carriers_k_live_stays_out_as_before(monkeypatch):
    km, qm = _key_mask(), _query_mask()
    mi = _record(km, qm)
    got = []
    monkeypatch.setattr(G2._FusedAttn, "apply", staticmethod(lambda *a: got.append(a) or torch.zeros(1)))
    _no_torch_index_chain(monkeypatch)
    q, k, v, packed = _operands(True)
    gta_amd.gta_attention(q, k, v, CL, packed, key_mask=km, query_mask=qm, key_mask_backward=True, mask_index=mi)
    (cfg, kv_cache, mask), = [a for a in got[0] if isinstance(a, tuple)]
    assert mask.kind == "gather" and mask.key_idx is mi.key_idx and mask.q_live is mi.q_live and mask.q_lens is mi.q_lens and mask.k_live is None


# ---- companion refusals ---------------------------------------------------------------------------------------------------------------------------
def test_companion_refusals(monkeypatch):
    _spies(monkeypatch, {})
    km, qm = _key_mask(), _query_mask()
    mi = _record(km, qm)
    q, k, v, packed = _operands(False)

    def call(**kw):
        with torch.no_grad():
            return gta_amd.gta_attention(q, k, v, CL, packed, **kw)

    call(key_mask=km, query_mask=qm, mask_index=mi)                           # (the record beside its masks: served)
    with pytest.raises(native.GtaError, match=COMPANION):                     # without masks
        call(mask_index=mi)
    with pytest.raises(native.GtaError, match=COMPANION):                     # one of its masks missing
        call(key_mask=km, mask_index=mi)
    with pytest.raises(native.GtaError, match=COMPANION):
        call(query_mask=qm, mask_index=mi)
    with pytest.raises(native.GtaError, match=COMPANION):                     # equal masks, other objects
        call(key_mask=km.clone(), query_mask=qm, mask_index=mi)
    with pytest.raises(native.GtaError, match=COMPANION):
        call(key_mask=km, query_mask=qm.clone(), mask_index=mi)
    with pytest.raises(native.GtaError, match=COMPANION):                     # the keys-only record beside both masks
        call(key_mask=km, query_mask=qm, mask_index=mi.keys_only())
    call(key_mask=km, mask_index=mi.keys_only())
    with pytest.raises(native.GtaError, match=COMPANION):                     # key_views beside it
        call(key_views=[1] * B, mask_index=mi)
    with pytest.raises(native.GtaError, match=COMPANION):                     # not a MaskIndex
        call(key_mask=km, query_mask=qm, mask_index=tuple(mi))
    with pytest.raises(native.GtaError, match=COMPANION):
        call(key_mask=km, query_mask=qm, mask_index={"key_idx": mi.key_idx})
    with pytest.raises(native.GtaError, match=COMPANION):                     # tensors on another device
        call(key_mask=km, query_mask=qm, mask_index=mi._replace(key_idx=mi.key_idx.to("meta")))
    with pytest.raises(native.GtaError, match=COMPANION):
        call(key_mask=km, query_mask=qm, mask_index=mi._replace(q_lens=mi.q_lens.to("meta")))
    with pytest.raises(native.GtaError, match=COMPANION):                     # an incomplete side
        call(key_mask=km, query_mask=qm, mask_index=mi._replace(k_live=None))
    with pytest.raises(native.GtaError, match=COMPANION):                     # tensors of another shape
        call(key_mask=km, query_mask=qm, mask_index=mi._replace(key_idx=mi.key_idx[:, :-1].contiguous()))


def test_view_groups_refuse_it_by_name():
    q, k, v, packed = _operands(False)
    with pytest.raises(native.GtaError, match="gta_attention_by_view_groups takes no mask_index: every group is a call of its own"):
        gta_amd.gta_attention_by_view_groups(q, k, v, CL, packed, views_per_call=1, query_mask=_query_mask(), mask_index=_record(None, _query_mask()))


def _message(**kw):
    try:
        gta_amd.gta_attention(**kw)
    except native.GtaError as e:
        return str(e)
    pytest.fail("nothing was refused")


EXISTING = [
    ("precise", dict(precise=True), False, {}),
    ("pretransformed", dict(pretransformed=True), False, {}),
    ("kv_mode-fused", dict(kv_mode="fused"), False, {}),
    ("generic-layout", dict(f_dims=EUCLID, euclid=True), False, {}),
    ("return_lse-under-grad", dict(return_lse=True, key_mask_backward=True), True, {}),
    ("grad-without-key_mask_backward", dict(), True, {}),
    ("query_mask-with-kv_cache", dict(kv_cache={}), False, dict(query=True)),
]


@pytest.mark.parametrize("kw, grad, opts", [pytest.param(k, g, o, id=i) for i, k, g, o in EXISTING])
def test_the_masked_calls_own_refusals_say_what_they_said(kw, grad, opts):
    km, qm = _key_mask(), _query_mask() if opts.get("query") else None
    q, k, v, packed = _operands(grad)
    kw = dict(dict(q=q, k=k, v=v, f_dims=CL, packed=packed, key_mask=km), **kw)
    if qm is not None:
        kw["query_mask"] = qm
    with torch.set_grad_enabled(grad):
        without = _message(**kw)
        for mi in (_record(km, qm), "not a record", _record(km.clone(), qm)):          # (a fitting record or not: the masks' refusal comes first)
            assert _message(mask_index=mi, **kw) == without
    assert COMPANION not in without


# ---- gta_amd.mask_index ---------------------------------------------------------------------------------------------------------------------------
def test_mask_index_validates_on_the_host_and_launches_once(monkeypatch):
    calls = []
    monkeypatch.setattr(native, "mask_index", lambda *a: calls.append(a))
    km, qm = _key_mask(), _query_mask()
    mi = gta_amd.mask_index(km, qm, device="cpu")
    assert len(calls) == 1
    kmask, key_idx, key_lens, k_live, qmask, q_lens = calls[0]
    assert mi.key_mask is km and mi.query_mask is qm and mi.key_idx is key_idx and mi.key_lens is key_lens and mi.k_live is k_live
    assert mi.q_live is qmask and mi.q_lens is q_lens and torch.equal(qmask, qm) and torch.equal(kmask, km)
    assert key_idx.dtype == torch.int32 and tuple(key_idx.shape) == (B, T) and key_lens.dtype == torch.int32 and tuple(key_lens.shape) == (B,)
    assert k_live.dtype == torch.bool and tuple(k_live.shape) == (B, T) and q_lens.dtype == torch.int32 and tuple(q_lens.shape) == (B,)
    # one tensor for both sides: passed for both
    both = gta_amd.mask_index(km, km, device="cpu")
    assert calls[-1][0] is calls[-1][4] and both.q_live is calls[-1][0] and both.key_mask is km and both.query_mask is km
    # either side alone: the other side's fields are None
    only_k, only_q = gta_amd.mask_index(km, device="cpu"), gta_amd.mask_index(query_mask=qm, device="cpu")
    assert only_k.q_live is None and only_k.q_lens is None and calls[-2][4] is None and calls[-2][5] is None
    assert only_q.key_idx is None and only_q.key_lens is None and only_q.k_live is None and calls[-1][:4] == (None,) * 4
    n = len(calls)
    # what key_index_tensors / check_key_mask / check_query_mask refuse
    dead = km.clone()
    dead[1] = False
    with pytest.raises(native.GtaError, match=r"key_mask: scenes \[1\] have no valid key"):
        gta_amd.mask_index(dead, device="cpu")
    gta_amd.mask_index(query_mask=dead, device="cpu")                 # (a scene without a live query row is legal)
    with pytest.raises(native.GtaError, match="key_mask must be a bool tensor"):
        gta_amd.mask_index(km.to(torch.uint8), device="cpu")
    with pytest.raises(native.GtaError, match="query_mask must be a bool tensor"):
        gta_amd.mask_index(km, qm[0], device="cpu")
    with pytest.raises(native.GtaError, match="needs a key_mask or a query_mask"):
        gta_amd.mask_index(device="cpu")
    with pytest.raises(native.GtaError, match="key_mask has 2 scenes, query_mask 1"):
        gta_amd.mask_index(km, qm[:1], device="cpu")
    assert len(calls) == n + 1


def test_a_mask_on_another_device_is_refused_with_the_message_of_key_index_tensors(monkeypatch):
    monkeypatch.setattr(native, "mask_index", lambda *a: pytest.fail("a launch"))
    km = _key_mask()
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))       # (a CPU tensor that says it lives on a GPU: never read, never moved)
    monkeypatch.setattr(torch.Tensor, "any", lambda *a, **k: pytest.fail("a CUDA mask is not read on the host"))
    try:
        G2.key_index_tensors(km, "meta")
    except native.GtaError as e:
        want = str(e)
    with pytest.raises(native.GtaError) as e:
        gta_amd.mask_index(km, device="meta")
    assert str(e.value) == want == "key_mask lives on cpu, the call on meta"
    with pytest.raises(native.GtaError, match="query_mask lives on cpu, the call on meta"):
        gta_amd.mask_index(query_mask=km, device="meta")


# ---- the keyword's way down -------------------------------------------------------------------------------------------------------------------------
def test_layers_hand_the_record_on_and_the_maskless_paths_name_it(monkeypatch):
    from gta_amd import layers
    args = {"f_dims": CL, "so2": 8, "max_freq_h": 1, "max_freq_w": 1}
    att = layers.Attention(128, heads=2, dim_head=64, attn_args={"method": {"name": "gta", "args": args}})
    seen = []

    def fake(q, k, v, f_dims, packed, **kw):
        seen.append(kw)
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3]).permute(0, 2, 1, 3)

    monkeypatch.setattr(layers._gta, "gta_attention", fake)
    monkeypatch.setattr(layers._gta, "pack_reps", lambda extras, f_dims: {})
    monkeypatch.setattr(layers._gta, "_so3_degree", lambda *a: 0)
    q = torch.zeros(2, 2, 8, 64)
    m = torch.ones(2, 8, dtype=torch.bool)
    mi = G2.MaskIndex(key_mask=m)
    att.core(q, q, q, {"key_mask": m, "mask_index": mi})
    att.core(q, q, q, {"key_mask": m})
    assert seen[0]["key_mask"] is m and seen[0]["mask_index"] is mi and "mask_index" not in seen[1]
    with pytest.raises(native.GtaError, match="mask_index with return_attmap: the dense attention map has no mask index"):
        att.core(q, q, q, {"mask_index": mi}, return_attmap=True)
    att.elementwise_mul = True
    with pytest.raises(native.GtaError, match="mask_index: the elementwise_mul ablation has no mask index"):
        att.core(q, q, q, {"mask_index": mi})


def _bare_model():
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    return model


def test_srt_refuses_the_flag_without_a_mask():
    with pytest.raises(native.GtaError, match="input_mask_index=True comes with input_mask"):
        _bare_model()(None, None, None, None, None, {}, input_mask_index=True)


@pytest.mark.parametrize("queries", [False, True])
def test_srt_builds_one_record_per_forward(monkeypatch, queries):
    """the encoder's layers see the record (both sides from the one tensor under `input_mask_queries`), the decoder's its keys_only(); one launch"""
    launches = []
    monkeypatch.setattr(native, "mask_index", lambda *a: launches.append(a))
    model = _bare_model()
    at = {}
    model.encoder = lambda images, cam, rays, extras: (at.setdefault("encoder", extras) and None, extras)
    model.decode = lambda z, x, rays, extras=None: at.setdefault("decoder", extras)
    mine = {"input_coord": 1}
    m3 = torch.ones(2, 3, 4, dtype=torch.bool)
    images = torch.zeros(2, 3, 3, 8, 8)
    model(images, None, None, None, None, mine, input_mask=m3, input_mask_queries=queries, input_mask_index=True)
    assert len(launches) == 1 and mine == {"input_coord": 1}
    enc, dec = at["encoder"]["mask_index"], at["decoder"]["mask_index"]
    km = at["encoder"]["key_mask"]
    assert isinstance(enc, G2.MaskIndex) and enc.key_mask is km and at["decoder"]["key_mask"] is km
    assert enc.key_idx is launches[0][1] and enc.key_lens is launches[0][2] and enc.k_live is launches[0][3]
    if queries:
        assert at["encoder"]["query_mask"] is km and enc.query_mask is km and enc.q_live is launches[0][4] and enc.q_lens is launches[0][5]
        assert launches[0][0] is launches[0][4]                                  # (the one tensor for both sides)
        assert "query_mask" not in at["decoder"]
        assert dec is not enc and dec.query_mask is None and dec.q_live is None and dec.q_lens is None
    else:
        assert enc.query_mask is None and enc.q_live is None and launches[0][4] is None and dec is enc
    assert dec.key_mask is km and dec.key_idx is enc.key_idx and dec.key_lens is enc.key_lens and dec.k_live is enc.k_live
    # the default: no record, no launch, the extras of before
    at.clear()
    model(images, None, None, None, None, mine, input_mask=m3, input_mask_queries=queries)
    assert len(launches) == 1 and "mask_index" not in at["encoder"] and "mask_index" not in at["decoder"]

"""Host side of the query-side mask (`gta_attention(..., query_mask=m)`, `gta_attn_fwd_qmask` / `gta_attn_bwd_qmask`): the four exported symbols
and their ctypes signatures against include/gta_hip.h, the null `q_live`, the refused combinations of the Python layer (each raises `GtaError`
naming its reason before anything is launched -- these tests run without a GPU, on CPU tensors), `query_mask_tensors` on hand-made masks, the
autograd wiring of `_FusedAttn` under the masks with the native calls replaced, and the mask's way through `layers.Attention` and `TransformingSRT`."""
import ctypes

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from tests import test_abi_refusals as R
from tests.test_key_mask_bwd_host import B, CL, EUCLID, GATHER_ARGS, H, NK, TK, TQ, _cpu_call, _mask
from tests.test_key_views_host import _decl

FWD_Q = R._with(R._with(R.ENTRIES["gta_attn_fwd_varlen"], "key_lens", "key_idx"), "out", "q_live")
BWD_Q = R._with(GATHER_ARGS, "kv_images", "q_live", "q_lens")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exist_and_signatures_match_the_header():
    L = native.lib()
    for s in ("gta_attn_fwd_qmask", "gta_attn_fwd_qmask_supported", "gta_attn_bwd_qmask", "gta_attn_bwd_qmask_supported"):
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
    # the forward: gta_attn_fwd_gather plus `const uint8_t* q_live` in front of out
    args, base = _decl("gta_attn_fwd_qmask"), _decl("gta_attn_fwd_gather")
    names = [a.split()[-1].lstrip("*") for a in args]
    i = names.index("q_live")
    assert args[i] == "const uint8_t* q_live" and names[i - 1] == "key_lens" and names[i + 1] == "out"
    assert args[:i] + args[i + 1:] == base and tuple(names[1:]) == FWD_Q
    # the backward: gta_attn_bwd_gather plus q_live and q_lens in front of kv_images
    args, base = _decl("gta_attn_bwd_qmask"), _decl("gta_attn_bwd_gather")
    names = [a.split()[-1].lstrip("*") for a in args]
    i = names.index("q_live")
    assert args[i:i + 2] == ["const uint8_t* q_live", "const int32_t* q_lens"] and names[i - 1] == "key_lens" and names[i + 2] == "kv_images"
    assert args[:i] + args[i + 2:] == base and tuple(names[1:]) == BWD_Q
    for entry in ("gta_attn_fwd_qmask", "gta_attn_bwd_qmask"):
        at, args = getattr(L, entry).argtypes, _decl(entry)
        assert len(at) == len(args) and at[0] == ctypes.POINTER(native.GtaAttnDesc)
        for a, t in zip(args[1:], at[1:]):
            want = ctypes.c_int64 if a.startswith("int64_t") else ctypes.POINTER(ctypes.c_int64) if a.startswith("const int64_t*") else ctypes.c_void_p
            assert t == want, (entry, a, t)
        assert _decl(entry + "_supported") == ["const GtaAttnDesc* desc"]
        assert getattr(L, entry + "_supported").argtypes == [ctypes.POINTER(native.GtaAttnDesc)]
    assert L.gta_abi_version() == 2
    for f in (native.attn_fwd_qmask, native.attn_bwd_qmask, native.attn_fwd_qmask_supported, native.attn_bwd_qmask_supported):
        assert callable(f)


def _call(entry, desc, **args):
    names = FWD_Q if entry == "gta_attn_fwd_qmask" else BWD_Q
    full = {name: R.X for name in names}
    full.update(dqkv_stride=(ctypes.c_int64 * 9)(*([64] * 9)), dout_stride=(ctypes.c_int64 * 3)(64, 64, 64), workspace_bytes=R.BIG, stream=None)
    full.update(args)
    return getattr(native.lib(), entry)(ctypes.byref(desc), *(full[name] for name in names))


@pytest.mark.parametrize("entry", ["gta_attn_fwd_qmask", "gta_attn_bwd_qmask"])
def test_null_q_live_is_a_bad_argument(entry):
    L = native.lib()
    rc = _call(entry, R._desc(), q_live=None)
    assert rc == R.BADARG and "null q_live" in L.gta_strerror(rc).decode(), L.gta_strerror(rc)
    for other, text in (("key_lens", "null key_lens"), ("key_idx", "null key_idx")):      # (the gather's own refusals stand)
        rc = _call(entry, R._desc(), **{other: None})
        assert rc == R.BADARG and text in L.gta_strerror(rc).decode(), (other, L.gta_strerror(rc))
    d = R._desc(flags=R.VT | R.FUSED_KV)
    assert _call(entry, d) == R.UNSUPPORTED
    sup = getattr(L, entry + "_supported")
    assert sup(ctypes.byref(R._desc())) == 0 and sup(ctypes.byref(d)) == R.UNSUPPORTED
    assert sup(ctypes.byref(R._desc())) == L.gta_attn_fwd_gather_supported(ctypes.byref(R._desc()))


def test_the_forward_entry_runs_the_attention_step():
    rc = _call("gta_attn_fwd_qmask", R._desc(flags=R.VT | native.FLAG_PREP_ONLY))
    assert rc == R.BADARG and "GTA_FLAG_PREP_ONLY" in native.lib().gta_strerror(rc).decode()


# ---- query_mask_tensors -------------------------------------------------------------------------------------------------------------------------
def test_query_mask_tensors_on_hand_made_masks():
    m = torch.zeros(4, 6, dtype=torch.bool)
    m[0] = True                  # all live
    m[1, 2] = True               # one row
    m[3, 5] = True               # the last row only;  scene 2: none
    q_live, q_lens = G2.query_mask_tensors(m, "cpu")
    assert q_live.dtype == torch.bool and q_live.is_contiguous() and torch.equal(q_live, m)
    assert q_lens.dtype == torch.int32 and q_lens.tolist() == [6, 3, 0, 6]
    q_live, _ = G2.query_mask_tensors(m.t().contiguous().t(), "cpu")              # (a strided mask is made contiguous: the kernels index [B, Tq])
    assert q_live.is_contiguous() and torch.equal(q_live, m)
    for bad in (m.to(torch.uint8), m[0], m[None], [[True]]):
        with pytest.raises(native.GtaError, match="query_mask must be a bool tensor of shape \\[B, Tq\\]"):
            G2.check_query_mask(bad)
    with pytest.raises(native.GtaError, match="query_mask has shape \\(4, 6\\) for 4 scenes of 7 query tokens"):
        G2.check_query_mask(m, 4, 7)
    G2.check_query_mask(m, 4, 6)          # a scene without a live row is legal


# ---- Python refusals --------------------------------------------------------------------------------------------------------------------------
def _qm(t=TQ):
    m = torch.ones(B, t, dtype=torch.bool)
    m[:, ::4] = False
    m[1] = False
    return m


def test_refused_combinations_name_their_reason():
    qm = _qm()
    for kw in (dict(key_views=[1] * B), dict(key_views=[1] * B, key_views_backward=True, query_views=[1] * B), dict(key_lens=torch.zeros(B, dtype=torch.int32)),
               dict(key_views_backward=True)):
        for mask in (True, False):
            with pytest.raises(native.GtaError, match="query_mask with key_views / query_views / key_lens / key_views_backward"):
                _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, **kw)
    with pytest.raises(native.GtaError, match="query_mask with kv_cache"):
        _cpu_call(query_mask=qm, key_mask_backward=True, kv_cache={})
    with torch.no_grad(), pytest.raises(native.GtaError, match="query_mask with kv_cache"):
        _cpu_call(mask=False, query_mask=qm, kv_cache={})
    # under grad: the existing opt-in, with or without a key mask; the "forward-only" refusal stands otherwise
    for mask in (True, False):
        with pytest.raises(native.GtaError, match="key_mask is forward-only"):
            _cpu_call(mask=mask, query_mask=qm)
        # everything key_mask refuses
        with pytest.raises(native.GtaError, match="key_mask has no precise=True"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, precise=True)
        with pytest.raises(native.GtaError, match="key_mask with pretransformed=True"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, pretransformed=True)
        with pytest.raises(native.GtaError, match="key_mask runs the two-stage plan: kv_mode='fused'"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, kv_mode="fused")
        with pytest.raises(native.GtaError, match="return_lse under grad with key_mask_backward"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, return_lse=True)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*euclid"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, f_dims=EUCLID, euclid=True)
        with pytest.raises(native.GtaError, match="no gather pre-pass.*t2"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, f_dims={"se3": 32, "t2": 30, "triv": 2})
        with pytest.raises(native.GtaError, match="no gather pre-pass.*dh % 8"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, f_dims={"se3": 8, "so2": 4}, dh=12)
        with pytest.raises(native.GtaError, match="key_mask_backward: no pose / coordinate gradients under a key mask yet"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True, packed_grad=True)
        # the mask itself, by name
        with pytest.raises(native.GtaError, match="query_mask has shape"):
            _cpu_call(mask=mask, query_mask=_qm(TQ + 1), key_mask_backward=True)
        with pytest.raises(native.GtaError, match="query_mask must be a bool tensor"):
            _cpu_call(mask=mask, query_mask=qm.float(), key_mask_backward=True)
        # nothing refuses: the call gets as far as the checks in front of the kernels, which have no CPU path -- a scene without a live row,
        # return_lse without grad included
        with pytest.raises(native.GtaError, match="cpu|CUDA"):
            _cpu_call(mask=mask, query_mask=qm, key_mask_backward=True)
        with torch.no_grad(), pytest.raises(native.GtaError, match="cpu|CUDA"):
            _cpu_call(mask=mask, query_mask=qm, return_lse=True)
    # without a query mask the flag still comes with key_mask
    with pytest.raises(native.GtaError, match="key_mask_backward=True comes with key_mask"):
        _cpu_call(mask=False, key_mask_backward=True)


def test_attn_bwd_takes_q_live_with_the_gather():
    from gta_amd import backward as BW
    z = torch.zeros(1)
    with pytest.raises(native.GtaError, match="q_live comes with key_idx and key_lens"):
        BW.attn_bwd(None, *([z] * 12), q_live=z)
    with pytest.raises(native.GtaError, match="q_live comes with key_idx and key_lens"):
        BW.attn_bwd(None, *([z] * 12), q_live=z, key_lens=z, q_lens=z)


# ---- autograd wiring ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_key_mask", [True, False])
def test_autograd_wiring(monkeypatch, with_key_mask):
    """`_FusedAttn` under the masks with the native calls replaced: the same q_live / q_lens objects reach gta_attn_fwd_qmask and gta_attn_bwd_qmask, beside the
    key tensors (without key_mask: an arange and the full count) and the forward's workspace as kv_images; without query_mask neither appears"""
    seen = {}

    def fwd_q(desc, q, k, v, vq, vk, cq, ck, tc, ta, key_idx, key_lens, q_live, out, lse, ws):
        seen["fwd"] = (key_idx, key_lens, q_live, ws)
        out.zero_()

    def bwd_q(desc, q, k, v, out, dout, lse, vq, vk, cq, ck, tc, ta, key_idx, key_lens, q_live, q_lens, kv_images, dq, dk, dv, dtc, ws, dta=None):
        seen["bwd"] = (key_idx, key_lens, q_live, q_lens, kv_images)
        for t, val in ((dq, 1.0), (dk, 2.0), (dv, 3.0), (dtc, 4.0), (dta, 5.0)):
            t.fill_(val)

    def fwd_g(desc, q, k, v, vq, vk, cq, ck, tc, ta, key_idx, key_lens, out, lse, ws):
        seen["fwd_gather"] = (key_idx, key_lens)
        out.zero_()

    def bwd_g(desc, q, k, v, out, dout, lse, vq, vk, cq, ck, tc, ta, key_idx, key_lens, kv_images, dq, dk, dv, dtc, ws, dta=None):
        seen["bwd_gather"] = (key_idx, key_lens)
        for t in (dq, dk, dv, dtc, dta):
            t.zero_()

    monkeypatch.setattr(native, "attn_fwd_qmask", fwd_q)
    monkeypatch.setattr(native, "attn_bwd_qmask", bwd_q)
    monkeypatch.setattr(native, "attn_fwd_gather", fwd_g)
    monkeypatch.setattr(native, "attn_bwd_gather", bwd_g)
    monkeypatch.setattr(native, "attn_bwd_varlen", lambda *a, **k: pytest.fail("the varlen entry"))
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    made = {}
    real = G2.query_mask_tensors

    def spy(mask, device):
        made["q"] = real(mask, device)
        return made["q"]

    monkeypatch.setattr(G2, "query_mask_tensors", spy)
    q, k, v = (torch.zeros(B, H, T, 64, requires_grad=True) for T in (TQ, TK, TK))
    tc, ta = torch.tensor([0.5], requires_grad=True), torch.tensor([0.8], requires_grad=True)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE),
              "cs_q": torch.zeros(B, TQ, 16), "cs_k": torch.zeros(B, TK, 16)}
    km, qm = _mask(), _qm()
    kw = {"key_mask": km} if with_key_mask else {}
    out = gta_amd.gta_attention(q, k, v, CL, packed, trans_coeff=tc, tau=ta, key_mask_backward=True, query_mask=qm, **kw)
    q_live, q_lens = made["q"]
    assert torch.equal(q_live, qm) and q_lens.tolist() == [TQ, 0, TQ, TQ]
    if with_key_mask:
        idx, lens = G2.key_index_tensors(km, "cpu")
    else:
        idx, lens = torch.arange(TK, dtype=torch.int32).expand(B, TK), torch.full((B,), TK, dtype=torch.int32)
    assert torch.equal(seen["fwd"][0], idx) and torch.equal(seen["fwd"][1], lens) and seen["fwd"][0].is_contiguous()
    assert seen["fwd"][2] is q_live
    out.sum().backward()
    assert seen["bwd"][0] is seen["fwd"][0] and seen["bwd"][1] is seen["fwd"][1] and seen["bwd"][4] is seen["fwd"][3]
    assert seen["bwd"][2] is q_live and seen["bwd"][3] is q_lens
    for t, val in ((q, 1.0), (k, 2.0), (v, 3.0), (tc, 4.0), (ta, 5.0)):
        assert t.grad is not None and t.grad.shape == t.shape and bool((t.grad == val).all())
    assert "fwd_gather" not in seen and "bwd_gather" not in seen
    # without query_mask: the two gather entries, as before, and no query-mask tensor is built
    if with_key_mask:
        seen.clear()
        made.clear()
        gta_amd.gta_attention(q, k, v, CL, packed, trans_coeff=tc, tau=ta, key_mask=km, key_mask_backward=True).sum().backward()
        assert set(seen) == {"fwd_gather", "bwd_gather"} and not made
    # no grad: the forward entry alone, return_lse served
    seen.clear()
    with torch.no_grad():
        o, lse = gta_amd.gta_attention(q, k, v, CL, packed, trans_coeff=tc, tau=ta, query_mask=qm, return_lse=True, **kw)
    assert set(seen) == {"fwd"} and tuple(lse.shape) == (B, H, TQ) and seen["fwd"][2] is made["q"][0]


# ---- the mask's way down ------------------------------------------------------------------------------------------------------------------------
def test_layers_hand_the_mask_on(monkeypatch):
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
    att.core(q, q, q, {"key_mask": m, "key_mask_backward": True, "query_mask": m})
    att.core(q, q, q, {"query_mask": m})
    att.core(q, q, q, {"key_mask": m})
    att.core(q, q, q, {})
    assert seen[0]["key_mask"] is m and seen[0]["query_mask"] is m and seen[0]["key_mask_backward"] is True
    assert seen[1]["query_mask"] is m and "key_mask" not in seen[1]
    assert "query_mask" not in seen[2] and "query_mask" not in seen[3]
    with pytest.raises(native.GtaError, match="query_mask with return_attmap"):
        att.core(q, q, q, {"query_mask": m}, return_attmap=True)


def test_srt_sets_the_mask_in_its_copy_of_extras_and_takes_it_out_before_the_decoder():
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    at_encoder = []

    def encoder(images, cam, rays, extras):
        at_encoder.append(dict(extras))
        return None, extras

    model.encoder = encoder
    model.decode = lambda z, x, rays, extras=None: extras
    mine = {"input_coord": 1}
    m3 = torch.ones(2, 3, 4, dtype=torch.bool)
    seen = model(None, None, None, None, None, mine, input_mask=m3, input_mask_backward=True, input_mask_queries=True)
    enc = at_encoder[-1]
    assert enc["query_mask"] is enc["key_mask"] and tuple(enc["query_mask"].shape) == (2, 12) and enc["key_mask_backward"] is True
    assert "query_mask" not in seen and seen["key_mask"] is enc["key_mask"] and seen["key_mask_backward"] is True and mine == {"input_coord": 1}
    # the default: today's extras, at the encoder and at the decoder
    seen = model(None, None, None, None, None, mine, input_mask=m3, input_mask_backward=True)
    assert "query_mask" not in at_encoder[-1] and "query_mask" not in seen and set(seen) == {"input_coord", "key_mask", "key_mask_backward"}
    seen = model(None, None, None, None, None, mine, input_mask=m3, input_mask_queries=False)
    assert "query_mask" not in at_encoder[-1] and set(seen) == {"input_coord", "key_mask"}
    with pytest.raises(native.GtaError, match="input_mask_queries=True comes with input_mask"):
        model(None, None, None, None, None, mine, input_mask_queries=True)


def test_the_encoder_selects_masked_tokens_away():
    """with extras['query_mask'] the encoder's token-wise layers never see a masked token or the image of a view without a live token: NaN there
    reaches neither the transformer's input nor (through 0 * NaN) a weight gradient; without the mask nothing is touched"""
    from gta_amd import srt
    enc = srt.ImprovedSRTEncoder.__new__(srt.ImprovedSRTEncoder)
    torch.nn.Module.__init__(enc)
    enc.attn_args, enc.output_scaler = {}, False
    enc.conv_blocks = torch.nn.Conv2d(3, 4, 2, stride=2, bias=False)
    enc.per_patch_linear = torch.nn.Conv2d(4, 4, 1)
    enc.lin_out = torch.nn.Identity()
    got = {}

    def transformer(x, z, extras):
        got["x"] = x
        return x

    enc.transformer = transformer
    import gta_amd.srt as S
    real = S.pre_compute_reps_encoder
    S.pre_compute_reps_encoder = lambda *a: None
    try:
        images = torch.randn(2, 2, 3, 4, 4)
        images[0, 1] = float("nan")
        mask = torch.ones(2, 8, dtype=torch.bool)
        mask[0, 4:] = False                  # scene 0: view 1 wholly masked
        mask[1, 5] = False                   # scene 1: one token of view 1 (its pixels pass the convolution: finite)
        out, _ = enc(images, None, None, {"query_mask": mask})
        assert torch.isfinite(out).all() and torch.count_nonzero(out[~mask]) == 0 and bool((out[mask] != 0).any())
        out.sum().backward()
        assert all(torch.isfinite(p.grad).all() for p in enc.parameters())
        out2, _ = enc(images, None, None, {})
        assert not torch.isfinite(out2[0, 4:]).any() and torch.equal(out2[1], enc(images, None, None, {})[0][1])
        with pytest.raises(native.GtaError, match="query_mask has 10 tokens per scene, the encoder 8"):
            enc(images, None, None, {"query_mask": torch.ones(2, 10, dtype=torch.bool)})
        with pytest.raises(native.GtaError, match="query_mask has shape \\(2, 9\\) for 2 scenes of 2 views"):
            enc(images, None, None, {"query_mask": torch.ones(2, 9, dtype=torch.bool)})
    finally:
        S.pre_compute_reps_encoder = real


def test_view_groups_hand_the_query_mask_to_every_group(monkeypatch):
    """`gta_attention_by_view_groups` refuses the key-side masks (every group is a call of its own) but serves a query mask: it goes, with its
    opt-ins, to each group's `gta_attention` call as it was given"""
    seen = []

    def fake(q, k, v, f_dims, packed, **kw):
        seen.append(kw)
        return torch.zeros(q.shape), torch.zeros(q.shape[:3])

    monkeypatch.setattr(G2, "gta_attention", fake)
    monkeypatch.setattr(G2, "gta_attention_merge", lambda outs, lses: (outs[0], lses[0]))
    q, k = torch.zeros(B, H, TQ, 64), torch.zeros(B, H, TK, 64)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
    qm = _qm()
    out = G2.gta_attention_by_view_groups(q, k, k, CL, packed, views_per_call=2, query_mask=qm, key_mask_backward=True, key_mask_rep_grad=True)
    assert tuple(out.shape) == (B, H, TQ, 64) and len(seen) == -(-NK // 2)
    for kw in seen:
        assert kw["query_mask"] is qm and kw["key_mask_backward"] is True and kw["key_mask_rep_grad"] is True and kw["return_lse"] is True
    for name, val in (("key_mask", _mask()), ("key_views", [1] * B), ("kv_cache", {})):
        with pytest.raises(native.GtaError, match=f"gta_attention_by_view_groups takes no {name}"):
            G2.gta_attention_by_view_groups(q, k, k, CL, packed, views_per_call=2, query_mask=qm, **{name: val})

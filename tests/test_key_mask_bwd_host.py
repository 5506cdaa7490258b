"""Host side of the backward through a key mask (`gta_attention(..., key_mask=m, key_mask_backward=True)`, `gta_attn_bwd_gather`): the two
exported symbols and their ctypes signatures against include/gta_hip.h, the refusals of the new entry (the rows tests/test_abi_refusals.py pins
for `gta_attn_bwd_varlen`, repeated, plus the null `key_idx`), the refused combinations of the Python layer (each raises `GtaError` naming its
reason before anything is launched -- these tests run without a GPU, on CPU tensors), the autograd wiring of `_FusedAttn` under a key mask with the two native
calls replaced, and the flag's way through `layers.Attention` and `TransformingSRT`."""
import ctypes

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from tests import test_abi_refusals as R
from tests.test_key_views_host import _decl

CL = {"se3": 32, "so2": 32}
EUCLID = {"triv": 2, "se3": 30, "so2": 32}
B, H, NK, PK, TQ = 4, 2, 5, 52, 150
TK = NK * PK

# gta_attn_bwd_varlen's arguments with key_idx in front of key_lens and no q_lens
GATHER_ARGS = tuple(a for a in R._with(R.ENTRIES["gta_attn_bwd_varlen"], "key_lens", "key_idx") if a != "q_lens")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_exist_and_signatures_match_the_header():
    L = native.lib()
    for s in ("gta_attn_bwd_gather", "gta_attn_bwd_gather_supported"):
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
    args, base = _decl("gta_attn_bwd_gather"), _decl("gta_attn_bwd_varlen")
    names = [a.split()[-1].lstrip("*") for a in args]
    i = names.index("key_idx")
    assert args[i] == "const int32_t* key_idx" and args[i + 1] == "const int32_t* key_lens" and "q_lens" not in names
    assert args[:i] + args[i + 1:] == [a for a in base if a.split()[-1] != "q_lens"]
    assert tuple(names[1:]) == GATHER_ARGS
    at = L.gta_attn_bwd_gather.argtypes
    assert len(at) == len(args) and at[0] == ctypes.POINTER(native.GtaAttnDesc)
    for a, t in zip(args[1:], at[1:]):
        want = ctypes.c_int64 if a.startswith("int64_t") else ctypes.POINTER(ctypes.c_int64) if a.startswith("const int64_t*") else ctypes.c_void_p
        assert t == want, (a, t)
    assert L.gta_attn_bwd_varlen.argtypes == at          # (one pointer swapped for another: the same list of types)
    assert _decl("gta_attn_bwd_gather_supported") == ["const GtaAttnDesc* desc"]
    assert L.gta_attn_bwd_gather_supported.argtypes == [ctypes.POINTER(native.GtaAttnDesc)]
    assert L.gta_abi_version() == 2
    assert callable(native.attn_bwd_gather) and callable(native.attn_bwd_gather_supported)


def _call(entry, desc, **args):
    """tests/test_abi_refusals.py's `_call` for the two new entries"""
    if entry.endswith("_supported"):
        return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc))
    full = {name: R.X for name in GATHER_ARGS}
    full.update(dqkv_stride=(ctypes.c_int64 * 9)(*([64] * 9)), dout_stride=(ctypes.c_int64 * 3)(64, 64, 64), workspace_bytes=R.BIG, stream=None)
    full.update(args)
    return getattr(native.lib(), entry)(None if desc is None else ctypes.byref(desc), *(full[name] for name in GATHER_ARGS))


RENAME = {"gta_attn_bwd_varlen": "gta_attn_bwd_gather", "gta_attn_bwd_varlen_supported": "gta_attn_bwd_gather_supported"}
ROWS = [pytest.param(RENAME[p.values[0]], *p.values[1:], id=f"{RENAME[p.values[0]]}-{i}") for i, p in enumerate(R.ROWS) if p.values[0] in RENAME]
ROWS.append(pytest.param("gta_attn_bwd_gather", {}, {"key_idx": None}, R.BADARG, "null key_idx", id="gta_attn_bwd_gather-null-key_idx"))
ROWS.append(pytest.param("gta_attn_bwd_gather", {}, {"key_lens": None}, R.BADARG, "null key_lens", id="gta_attn_bwd_gather-null-key_lens"))
# key_idx is needed even when the images come with the call: the scatter reads it
ROWS.append(pytest.param("gta_attn_bwd_gather", {}, {"key_idx": None, "kv_images": R.X}, R.BADARG, "null key_idx",
                         id="gta_attn_bwd_gather-null-key_idx-with-images"))


def test_the_varlen_rows_are_all_there():
    """(the table above is built from another module's: it must not come out empty)"""
    n_call = sum(1 for p in ROWS if p.values[0] == "gta_attn_bwd_gather")
    n_sup = sum(1 for p in ROWS if p.values[0] == "gta_attn_bwd_gather_supported")
    assert n_call >= 20 and n_sup >= 10, (n_call, n_sup)
    texts = {p.values[4] for p in ROWS}
    for t in ("null key_lens", "null key_idx", "per-scene key prefixes run the two-stage plan: no GTA_FLAG_FUSED_KV",
              "per-scene key prefixes have no GTA_FLAG_FP32_PRODUCTS instances", "workspace smaller than gta_attn_bwd_workspace_bytes()"):
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


# ---- Python refusals --------------------------------------------------------------------------------------------------------------------------
def _mask(b=B, t=TK):
    m = torch.ones(b, t, dtype=torch.bool)
    m[:, 1::3] = False
    return m


def _cpu_call(f_dims=CL, dh=64, euclid=False, grad=True, mask=True, packed_grad=False, **kw):
    """gta_attention on CPU tensors: reaches a kernel only if nothing refuses first (and would then raise for the missing device)"""
    q = torch.zeros(B, H, TQ, dh, requires_grad=grad)
    k = torch.zeros(B, H, TK, dh)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE, requires_grad=packed_grad)}
    return gta_amd.gta_attention(q, k, k, f_dims, packed, euclid=euclid, **({"key_mask": _mask()} if mask else {}), **kw)


def test_without_the_flag_a_call_under_grad_is_still_forward_only():
    with pytest.raises(native.GtaError, match="key_mask is forward-only"):
        _cpu_call()
    with pytest.raises(native.GtaError, match="key_mask is forward-only"):
        _cpu_call(key_mask_backward=False)
    with pytest.raises(native.GtaError, match="key_mask is forward-only"):
        _cpu_call(grad=False, packed_grad=True)


def test_refused_combinations_name_their_reason():
    with pytest.raises(native.GtaError, match="key_mask_backward=True comes with key_mask"):
        _cpu_call(mask=False, key_mask_backward=True)
    with torch.no_grad(), pytest.raises(native.GtaError, match="key_mask_backward=True comes with key_mask"):
        _cpu_call(mask=False, key_mask_backward=True)
    with pytest.raises(native.GtaError, match="key_mask has no precise=True"):
        _cpu_call(key_mask_backward=True, precise=True)
    with pytest.raises(native.GtaError, match="key_mask with pretransformed=True"):
        _cpu_call(key_mask_backward=True, pretransformed=True)
    with pytest.raises(native.GtaError, match="key_mask runs the two-stage plan: kv_mode='fused'"):
        _cpu_call(key_mask_backward=True, kv_mode="fused")
    with pytest.raises(native.GtaError, match="return_lse under grad with key_mask_backward"):
        _cpu_call(key_mask_backward=True, return_lse=True)
    with pytest.raises(native.GtaError, match="kv_cache is an inference feature"):
        _cpu_call(key_mask_backward=True, kv_cache={})
    # the staged layouts (euclid, t2) and the rho-apply ones (dh % 8 != 0)
    with pytest.raises(native.GtaError, match="no gather pre-pass.*euclid"):
        _cpu_call(key_mask_backward=True, f_dims=EUCLID, euclid=True)
    with pytest.raises(native.GtaError, match="no gather pre-pass.*t2"):
        _cpu_call(key_mask_backward=True, f_dims={"se3": 32, "t2": 30, "triv": 2})
    with pytest.raises(native.GtaError, match="no gather pre-pass.*dh % 8"):
        _cpu_call(key_mask_backward=True, f_dims={"se3": 8, "so2": 4}, dh=12)
    # rep tables or poses that require grad
    with pytest.raises(native.GtaError, match="key_mask_backward: no pose / coordinate gradients under a key mask yet"):
        _cpu_call(key_mask_backward=True, packed_grad=True)
    with pytest.raises(native.GtaError, match="key_mask_backward: no pose / coordinate gradients under a key mask yet"):
        _cpu_call(key_mask_backward=True, grad=False, packed_grad=True)
    # one mask per call, as in the forward
    with pytest.raises(native.GtaError, match="key_mask with key_views"):
        _cpu_call(key_mask_backward=True, key_views=[1] * B, key_views_backward=True)
    # nothing refuses: the call gets as far as the checks in front of the kernels, which have no CPU path
    with pytest.raises(native.GtaError, match="cpu|CUDA"):
        _cpu_call(key_mask_backward=True)
    # without grad the flag changes nothing: return_lse and kv_cache are the forward's
    with torch.no_grad(), pytest.raises(native.GtaError, match="cpu|CUDA"):
        _cpu_call(key_mask_backward=True, return_lse=True, kv_cache={})


def test_routes():
    shape = (B, H, TQ, 64)
    for dt in (torch.float32, torch.bfloat16):
        fl = G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=True, needs_grad=True, key_mask_backward=True)
        assert fl == G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=True)
        with pytest.raises(native.GtaError, match="forward-only"):
            G2.attention_route(shape, TK, dt, CL, 0, 1, NK, key_mask=True, needs_grad=True)
        d = native.make_desc_from(dt, shape, TK, [(H * T * 64, T * 64, 64) for T in (TQ, TK, TK, TQ)], CL, 0, 1, NK, 0.125, fl)
        assert native.attn_bwd_gather_supported(d) == 0
        d.flags |= native.FLAG_FUSED_KV
        assert native.attn_bwd_gather_supported(d) == native.E_UNSUPPORTED


def test_autograd_wiring(monkeypatch):
    """`_FusedAttn` under a key mask with the two native calls replaced: the forward gets the tensors of key_index_tensors, the backward the same two, the
    forward's workspace as kv_images and no q_lens; five gradients come back"""
    seen = {}

    def fwd(desc, q, k, v, vq, vk, cq, ck, tc, ta, key_idx, key_lens, out, lse, ws):
        seen["fwd"] = (key_idx, key_lens, ws)
        out.zero_()

    def bwd(desc, q, k, v, out, dout, lse, vq, vk, cq, ck, tc, ta, key_idx, key_lens, kv_images, dq, dk, dv, dtc, ws, dta=None):
        seen["bwd"] = (key_idx, key_lens, kv_images)
        for t, val in ((dq, 1.0), (dk, 2.0), (dv, 3.0), (dtc, 4.0), (dta, 5.0)):
            t.fill_(val)

    monkeypatch.setattr(native, "attn_fwd_gather", fwd)
    monkeypatch.setattr(native, "attn_bwd_gather", bwd)
    monkeypatch.setattr(native, "attn_bwd_varlen", lambda *a, **k: pytest.fail("the varlen entry"))
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    q, k, v = (torch.zeros(B, H, T, 64, requires_grad=True) for T in (TQ, TK, TK))
    tc, ta = torch.tensor([0.5], requires_grad=True), torch.tensor([0.8], requires_grad=True)
    packed = {"vrep_q": torch.zeros(B, 1, native.VREP_STRIDE), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE),
              "cs_q": torch.zeros(B, TQ, 16), "cs_k": torch.zeros(B, TK, 16)}
    mask = _mask()
    out = gta_amd.gta_attention(q, k, v, CL, packed, trans_coeff=tc, tau=ta, key_mask=mask, key_mask_backward=True)
    idx, lens = G2.key_index_tensors(mask, "cpu")
    assert torch.equal(seen["fwd"][0], idx) and torch.equal(seen["fwd"][1], lens)
    out.sum().backward()
    assert seen["bwd"][0] is seen["fwd"][0] and seen["bwd"][1] is seen["fwd"][1] and seen["bwd"][2] is seen["fwd"][2]
    for t, val in ((q, 1.0), (k, 2.0), (v, 3.0), (tc, 4.0), (ta, 5.0)):
        assert t.grad is not None and t.grad.shape == t.shape and bool((t.grad == val).all())


def test_attn_bwd_takes_key_idx_with_key_lens_and_without_q_lens():
    from gta_amd import backward as BW
    z = torch.zeros(1)
    with pytest.raises(native.GtaError, match="key_idx comes with key_lens and without q_lens"):
        BW.attn_bwd(None, *([z] * 12), key_idx=z)
    with pytest.raises(native.GtaError, match="key_idx comes with key_lens and without q_lens"):
        BW.attn_bwd(None, *([z] * 12), key_idx=z, key_lens=z, q_lens=z)


# ---- the flag's way down ------------------------------------------------------------------------------------------------------------------------
def test_layers_hand_the_flag_on(monkeypatch):
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
    att.core(q, q, q, {"key_mask": m, "key_mask_backward": True})
    att.core(q, q, q, {"key_mask": m})
    att.core(q, q, q, {})
    assert seen[0]["key_mask"] is m and seen[0]["key_mask_backward"] is True
    assert seen[1]["key_mask"] is m and "key_mask_backward" not in seen[1]
    assert "key_mask" not in seen[2] and "key_mask_backward" not in seen[2]


def test_srt_sets_the_flag_in_its_copy_of_extras():
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    model.encoder = lambda images, cam, rays, extras: (None, extras)
    model.decode = lambda z, x, rays, extras=None: extras
    mine = {"input_coord": 1}
    m3 = torch.ones(2, 3, 4, dtype=torch.bool)
    seen = model(None, None, None, None, None, mine, input_mask=m3, input_mask_backward=True)
    assert tuple(seen["key_mask"].shape) == (2, 12) and seen["key_mask_backward"] is True and mine == {"input_coord": 1}
    assert "key_mask_backward" not in model(None, None, None, None, None, mine, input_mask=m3)
    with pytest.raises(native.GtaError, match="input_mask_backward=True comes with input_mask"):
        model(None, None, None, None, None, mine, input_mask_backward=True)
    with pytest.raises(native.GtaError, match="input_mask with input_views"):
        model(None, None, None, None, None, mine, input_mask=m3, input_views=[1, 2], input_mask_backward=True)

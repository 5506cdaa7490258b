"""GPU: attention over any per-scene subset of the key tokens (`gta_attention(..., key_mask=...)`; `gta_attn_fwd_gather`: the GATHER
instances of the K/V pre-pass compact the valid keys, the VARLEN `gta_fwd2_kernel` attends over them).

Shapes: B = 4 scenes, H = 2, 5 input views of 52 tokens (Tk = 260: five 64-key tiles with a tail of 4).  Query side: a decoder-like leg of
150 rows and a self-attention leg (Tq = Tk).  Layouts: CLEVR-TR `se3 32 | so2 32` (dh 64) and MSN `gta_so3` (dh 96); bf16 and fp32 inputs.

Mask sets, one mask per scene:
  edges    all 260 keys | token 137 alone (one tile: keeps the true row max) | the first 13 tokens of every view (65 keys: tile 0 holds rows of
           all five views, tile 1 one row) | exactly 64 keys spread over three views (one full tile, nothing behind it)
  random   Bernoulli at 0.9 / 0.5 / 0.25 / 0.05 from a fixed seed, at least one key each

Bars (none new): tests/test_gpu_forward.py's REL_MAX / REL_RMS for the output and its LSE bar (`test_lse_matches_logsumexp`: 2e-2 absolute,
trans_coeff 0.01), as tests/test_gpu_key_views.py uses them for the fused layouts; the workspace rules are those of tests/_gather_images.py."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _gather_images as GI
from tests import _hip_cases as C
from tests import _images as I
from tests.test_gpu_forward import REL_MAX, REL_RMS
from tests.test_gpu_run_configs import RUNS

pytestmark = pytest.mark.gpu

B, H, NK, PK, TQ_DEC = 4, 2, 5, 52, 150
TK = NK * PK
LAYOUTS = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
TC = 0.01
M13 = 13


@functools.lru_cache(maxsize=None)
def _masks(name):
    """bool [B, TK] on the CPU"""
    m = torch.zeros(B, TK, dtype=torch.bool)
    if name == "edges":
        m[0] = True
        m[1, 137] = True
        m[2] = (torch.arange(TK) % PK) < M13
        m[3, 0:20] = m[3, 2 * PK + 5:2 * PK + 25] = m[3, 4 * PK + 10:4 * PK + 34] = True
        assert m.sum(1).tolist() == [260, 1, 65, 64]
    elif name == "random":
        g = torch.Generator().manual_seed(20)
        m = torch.rand(B, TK, generator=g) < torch.tensor([0.9, 0.5, 0.25, 0.05])[:, None]
        assert bool(m.any(1).all()) and not bool(m.all(1).any())
    elif name == "first13":                                  # (every scene: the third scene of `edges`)
        m[:] = (torch.arange(TK) % PK) < M13
    else:                                                    # "views:1,3,4,5": whole leading views
        for b, n in enumerate(int(x) for x in name.split(":")[1].split(",")):
            m[b, :n * PK] = True
    return m


@functools.lru_cache(maxsize=None)
def _case(run, side, dtype):
    """masters on the CPU (rounded to the input type), device inputs and packed tables -- built once, never written to"""
    from gta_amd import synth
    dh, _mixed, enc, dec = RUNS[run]
    g = torch.Generator().manual_seed(sum(map(ord, run)) + 7 * (side == "dec"))
    ex = {"input_transforms": synth.random_extrinsics(B, NK, g), "input_coord": torch.rand(B, NK, PK, 2, generator=g)}
    Tq = TK
    if side == "dec":
        ex["target_transforms"] = synth.random_extrinsics(B, 1, g)
        ex["target_coord"] = torch.rand(B, 1, TQ_DEC, 2, generator=g)
        Tq = TQ_DEC
    q, k, v = (torch.randn(B, H, T, dh, generator=g) for T in (Tq, TK, TK))
    if dtype == torch.bfloat16:
        q, k, v = (t.bfloat16().float() for t in (q, k, v))
    exd = {kk: vv.cuda() for kk, vv in ex.items()}
    gta_amd.pre_compute_reps_encoder(enc, exd)
    args = enc
    if side == "dec":
        gta_amd.pre_compute_reps_decoder(dec, exd)
        args = dec
    f_dims = args["f_dims"]
    packed = {kk: vv.clone() for kk, vv in gta_amd.pack_reps(exd, f_dims).items()}
    dev = tuple(t.to(dtype).cuda() for t in (q, k, v))
    return SimpleNamespace(run=run, side=side, dtype=dtype, dh=dh, q=q, k=k, v=v, ex=ex, enc=enc, dec=dec, f_dims=f_dims, packed=packed,
                           so3=G2._so3_degree(f_dims, packed, exd), scale=dh ** -0.5, dev=dev, tc=torch.tensor([TC], device="cuda"),
                           Tq=Tq, Nq=1 if side == "dec" else NK, B=B, H=H, T=TK)


def _tensors(mask):
    return G2.key_index_tensors(mask, torch.device("cuda", torch.cuda.current_device()))


def _abi(c, key_idx, key_lens, packed=None, qkv=None, ws=None, flags_extra=0, entry="gather", Nk=NK):
    """one direct ctypes call of gta_attn_fwd_gather (or, entry='varlen', of gta_attn_fwd_varlen) on a 0xFF-filled workspace; returns out, lse,
    workspace"""
    q, k, v = qkv or c.dev
    pk = packed or c.packed
    out = torch.empty(B, c.Tq, H, c.dh, device="cuda", dtype=c.dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, c.Tq, device="cuda", dtype=torch.float32)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, Nk, c.scale, native.FLAG_V_TRANSFORM | flags_extra)
    p, L = native._ptr, native.lib()
    assert native.attn_fwd_gather_supported(desc) == 0
    if ws is None:
        ws = torch.full((native.attn_fwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    tables = (p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")), p(pk.get("cs_k")), p(c.tc), None)
    prep_only = bool(flags_extra & native.FLAG_PREP_ONLY)
    ends = (None if prep_only else p(out), None if prep_only else p(lse), p(ws), ws.numel(), native._stream())
    if entry == "gather":
        rc = L.gta_attn_fwd_gather(ctypes.byref(desc), None if prep_only else p(q), p(k), p(v), *tables, p(key_idx), p(key_lens), *ends)
    else:
        rc = L.gta_attn_fwd_varlen(ctypes.byref(desc), None if prep_only else p(q), p(k), p(v), *tables, p(key_lens), *ends)
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    return out, lse, ws


def _attention(c, mask=None, packed=None, qkv=None, **kw):
    q, k, v = qkv or c.dev
    with torch.no_grad():
        return gta_amd.gta_attention(q, k, v, c.f_dims, packed or c.packed, so3_degree=c.so3, trans_coeff=c.tc, scale=c.scale,
                                     **({"key_mask": mask} if mask is not None else {}), **kw)


# ---- 1. the workspace contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", ["edges", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_workspace_contract(run, dtype, masks):
    """a GTA_FLAG_PREP_ONLY call on a 0xFF-filled workspace, element by element against the gather rule, the zero rule, the skip rule and the
    key-norm bounds of tests/_gather_images.py; the entries of key_idx at or past key_lens point at other (in-range) tokens: never used"""
    c = _case(run, "dec", dtype)
    mask = _masks(masks)
    key_idx, key_lens = _tensors(mask)
    _, _, ws = _abi(c, key_idx, key_lens, flags_extra=native.FLAG_PREP_ONLY)
    cpu_tables = {n: t.cpu() for n, t in c.packed.items()}
    ref = I.ref_rows(c.k, c.v, cpu_tables, c.f_dims, NK, c.so3, TC)
    idx_ref, lens_ref = GI.index_tensors(mask)
    assert torch.equal(key_idx.cpu().long(), idx_ref) and torch.equal(key_lens.cpu().long(), lens_ref)
    assert ws.numel() == I.fused_layout(B, H, TK, c.dh, False, c.Nq, 2 if dtype == torch.bfloat16 else 4).total
    GI.check(f"{run} {dtype} {masks}", ws.cpu(), c, ref, idx_ref, lens_ref)
    # the index order is the caller's: the valid tokens reversed give the reversed rows
    rev = key_idx.clone()
    for b, n in enumerate(lens_ref.tolist()):
        rev[b, :n] = key_idx[b, :n].flip(0)
    _, _, ws2 = _abi(c, rev, key_lens, flags_extra=native.FLAG_PREP_ONLY)
    GI.check(f"{run} {dtype} {masks} reversed", ws2.cpu(), c, ref, rev.cpu().long(), lens_ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [16, 32, 40, 104, 128])
def test_workspace_contract_at_every_head_size(dh, dtype):
    """the GATHER instances the two layouts do not reach (dhp 32 and 128) and head sizes that leave chunks of a padded row unused, on
    token-major K and V ([B,T,H,dh] storage: the packed projection's strides); B = 3, H = 3, 3 views of 50 tokens (Tk = 150), masks: every
    third token dropped (100 keys), Bernoulli 0.3, all keys"""
    se3 = int(round(dh / 2 / 4)) * 4
    c = I.key_side_case({"se3": se3, "so2": dh - se3}, 0, dtype, B=3, H=3, Nk=3, Pk=50, seed=5)
    mask = torch.ones(c.B, c.T, dtype=torch.bool)
    mask[0, 2::3] = False
    mask[1] = torch.rand(c.T, generator=torch.Generator().manual_seed(dh)) < 0.3
    mask[1, 149] = True
    key_idx, key_lens = _tensors(mask)
    k, v = (t.to(dtype).cuda() for t in (c.k, c.v))
    assert k.stride() == (c.T * c.H * dh, dh, c.H * dh, 1)
    st = [tuple(k.stride()[:3])] * 4
    desc = native.make_desc_from(dtype, (c.B, c.H, c.T, dh), c.T, st, c.f_dims, 0, c.Nk, c.Nk, dh ** -0.5, native.FLAG_V_TRANSFORM | native.FLAG_PREP_ONLY)
    assert native.attn_fwd_gather_supported(desc) == 0
    ws = torch.full((native.attn_fwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    p, L = native._ptr, native.lib()
    vrep, cs, tc = c.packed["vrep_k"].cuda(), c.packed["cs_k"].cuda(), torch.tensor([TC], device="cuda")
    rc = L.gta_attn_fwd_gather(ctypes.byref(desc), None, p(k), p(v), p(vrep), p(vrep), p(cs), p(cs), p(tc), None, p(key_idx), p(key_lens), None, None,
                               p(ws), ws.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, 0, TC)
    GI.check(f"dh{dh} {dtype}", ws.cpu(), c, ref, *GI.index_tensors(mask))


# ---- 2. bit-for-bit equalities --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [(1, 3, 4, 5), (NK,) * B])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_a_mask_of_leading_views_is_key_views(run, side, dtype, views):
    """out, lse and every byte of the workspace (both calls start from 0xFF) equal those of gta_attn_fwd_varlen under the same prefixes: whole
    leading views, and the all-true mask against key_views = [Nk] * B; gta_attention(key_mask=) gives the same out"""
    c = _case(run, side, dtype)
    mask = _masks("views:" + ",".join(map(str, views)))
    key_idx, key_lens = _tensors(mask)
    assert key_lens.tolist() == [n * PK for n in views]
    out, lse, ws = _abi(c, key_idx, key_lens)
    out_v, lse_v, ws_v = _abi(c, None, G2.key_lens_tensor(views, PK, key_lens.device), entry="varlen")
    assert torch.equal(out, out_v) and torch.equal(lse, lse_v) and torch.equal(ws, ws_v)
    got, got_lse = _attention(c, mask.cuda(), return_lse=True)
    kv, kv_lse = _attention(c, key_views=list(views), return_lse=True)
    torch.cuda.synchronize()
    assert torch.equal(got, out) and torch.equal(got_lse, lse) and torch.equal(kv, out) and torch.equal(kv_lse, lse)
    assert torch.equal(_attention(c, mask), out)                    # (a CPU mask: validated and uploaded)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_first_tokens_of_every_view_is_the_call_on_sliced_keys(run, side, dtype):
    """the mask "first 13 tokens of every view" against gta_attn_fwd_varlen on k, v and cs_k physically cut to those tokens (five views of
    13 tokens, key_lens = 65): out and lse bit for bit; the sliced call's workspace has other strides, so its two tiles and norms are compared
    per (b, h, tile)"""
    c = _case(run, side, dtype)
    mask = _masks("first13")
    key_idx, key_lens = _tensors(mask)
    out, lse, ws = _abi(c, key_idx, key_lens)
    cols = mask[0].nonzero().flatten().cuda()
    q, k, v = c.dev
    pk = dict(c.packed)
    pk["cs_k"] = c.packed["cs_k"][:, cols].contiguous()
    ks, vs = k[:, :, cols].contiguous(), v[:, :, cols].contiguous()
    Tk1 = NK * M13
    out1 = torch.empty_like(out)
    lse1 = torch.empty_like(lse)
    desc = native.make_desc(q, ks, vs, out1, c.f_dims, c.so3, c.Nq, NK, c.scale, native.FLAG_V_TRANSFORM)
    ws1 = torch.full((native.attn_fwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    p, L = native._ptr, native.lib()
    lens1 = torch.full((B,), Tk1, device="cuda", dtype=torch.int32)
    rc = L.gta_attn_fwd_varlen(ctypes.byref(desc), p(q), p(ks), p(vs), p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")), p(pk["cs_k"]),
                               p(c.tc), None, p(lens1), p(out1), p(lse1), p(ws1), ws1.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    assert torch.equal(out, out1) and torch.equal(lse, lse1)
    d, d1 = I.decode(ws.cpu(), B, H, TK, c.dh), I.decode(ws1.cpu(), B, H, Tk1, c.dh)
    nt = d1.layout.n_tiles
    assert nt == 2 and torch.equal(d.bits[:, :, :nt], d1.bits) and torch.equal(d.aux_raw[:, :, :nt], d1.aux_raw)
    assert bool((d.bits[:, :, nt:] == -1).all()) and bool((d.aux_raw[:, :, nt:] == -1).all())


# ---- 3. oracle parity -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(run, side, dtype, masks):
    """fp64 per scene: O.transform_qkv on the whole key side, the valid key columns, O.softmax_attention, O.inverse_transform_out -> out, LSE"""
    c = _case(run, side, dtype)
    res = []
    for b in range(B):
        ex64 = {"input_transforms": c.ex["input_transforms"][b:b + 1].double(), "input_coord": c.ex["input_coord"][b:b + 1].double()}
        reps = O.encoder_reps(c.enc, ex64)
        if side == "dec":
            ex64["target_transforms"] = c.ex["target_transforms"][b:b + 1].double()
            ex64["target_coord"] = c.ex["target_coord"][b:b + 1].double()
            reps = O.decoder_reps(c.dec, ex64, reps)
        qt, kt, vt = O.transform_qkv(c.q[b:b + 1].double(), c.k[b:b + 1].double(), c.v[b:b + 1].double(), c.f_dims, reps, TC, True, False)
        cols = _masks(masks)[b].nonzero().flatten()
        o, _ = O.softmax_attention(qt, kt[:, :, cols], vt[:, :, cols], c.scale)
        out = O.inverse_transform_out(o, c.f_dims, reps, TC, False)
        res.append((out[0], torch.logsumexp(c.scale * qt @ kt[:, :, cols].transpose(-1, -2), -1)[0]))
    return res


@pytest.mark.parametrize("masks", ["edges", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_parity_with_the_oracle_on_the_valid_keys(run, side, dtype, masks):
    c = _case(run, side, dtype)
    mask = _masks(masks)
    out, lse = _attention(c, mask.cuda(), return_lse=True)
    torch.cuda.synchronize()
    for b, (ref, ref_lse) in enumerate(_oracle(run, side, dtype, masks)):
        st = C.err_stats(out[b].float().cpu(), ref.float())
        lse_err = (lse[b].double().cpu() - ref_lse).abs().max().item()
        print(f"KEY_MASK {run} {side} {dtype} {masks} scene {b} ({int(mask[b].sum())} keys): {st} | lse max_abs {lse_err:.3e}")
        assert torch.isfinite(lse[b]).all()
        assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] and st["rel_rms"] <= REL_RMS, (run, side, dtype, masks, b, st)
        assert lse_err < 2e-2, (run, side, dtype, masks, b, lse_err)


# ---- 4. masked content is never used -------------------------------------------------------------------------------------------------------
def _poisoned(c, mask, value):
    """k, v and cs_k with every masked row filled with `value` (a float or a callable giving a tensor)"""
    k, v = c.dev[1].clone(), c.dev[2].clone()
    pk = dict(c.packed)
    pk["cs_k"] = pk["cs_k"].clone()
    dead = (~mask).cuda()
    for t in (k, v):
        rows = t.permute(0, 2, 1, 3)[dead]                      # [n_dead, H, dh]
        t.permute(0, 2, 1, 3)[dead] = value(rows) if callable(value) else torch.full_like(rows, value)
    rows = pk["cs_k"][dead]
    pk["cs_k"][dead] = value(rows) if callable(value) else torch.full_like(rows, value)
    return (c.dev[0], k, v), pk


@pytest.mark.parametrize("masks", ["edges", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_masked_tokens_may_hold_nan_and_inf(run, dtype, masks):
    """NaN, then +-Inf, in every masked row of k, v and cs_k, with the entries of key_idx past key_lens pointing at exactly those rows (in
    range: the masked tokens, as key_index_tensors leaves them): out and lse are finite and bit-identical to the run with zeros there"""
    c = _case(run, "dec", dtype)
    mask = _masks(masks)
    key_idx, key_lens = _tensors(mask)
    for b, n in enumerate(key_lens.tolist()):                  # what lies past the count names masked tokens only
        assert not bool(mask[b][key_idx[b, n:].cpu().long()].any())
    qkv0, pk0 = _poisoned(c, mask, 0.0)
    out0, lse0, ws0 = _abi(c, key_idx, key_lens, pk0, qkv0)
    assert torch.isfinite(out0).all() and torch.isfinite(lse0).all()
    signs = lambda t: torch.where(torch.arange(t.numel(), device=t.device).reshape(t.shape) % 2 == 0, float("inf"), float("-inf")).to(t.dtype)
    for value in (float("nan"), signs):
        qkv, pk = _poisoned(c, mask, value)
        assert not torch.isfinite(qkv[1]).all() and not torch.isfinite(pk["cs_k"]).all()
        out, lse, ws = _abi(c, key_idx, key_lens, pk, qkv)
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), (run, dtype, masks)
        assert torch.equal(out, out0) and torch.equal(lse, lse0) and torch.equal(ws, ws0), (run, dtype, masks)
        assert torch.equal(_attention(c, mask.cuda(), packed=pk, qkv=qkv), out0)


# ---- 5. plumbing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", LAYOUTS)
def test_kv_cache_holds_the_compacted_images(run):
    """two calls with one cache dict, k and v overwritten in between: the second returns the same bits and runs no pre-pass (the workspace
    bytes do not change); the cache without the mask, or under key_views, is refused"""
    c = _case(run, "dec", torch.bfloat16)
    mask = _masks("random").cuda()
    q, k, v = c.dev[0], c.dev[1].clone(), c.dev[2].clone()
    cache = {}
    a = _attention(c, mask, qkv=(q, k, v), kv_cache=cache).clone()
    assert cache["plan"][-1] == "key_mask" and cache["images"].numel() > 0
    assert torch.equal(cache["key_lens"].cpu(), mask.sum(1).int().cpu()) and tuple(cache["key_idx"].shape) == (B, TK)
    assert torch.equal(a, _attention(c, mask))
    n_img = I.fused_layout(B, H, TK, c.dh).aux_end
    before = cache["images"][:n_img].clone()
    k.fill_(7.0)
    v.fill_(-3.0)
    b = _attention(c, mask, qkv=(q, k, v), kv_cache=cache)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(cache["images"][:n_img], before)
    with pytest.raises(native.GtaError, match="another plan"):
        _attention(c, None, qkv=(q, k, v), kv_cache=cache)
    with pytest.raises(native.GtaError, match="another plan"):
        _attention(c, None, qkv=(q, k, v), kv_cache=cache, key_views=[NK] * B)


@pytest.mark.parametrize("run", LAYOUTS)
def test_forward_plan_with_key_mask(run):
    from gta_amd import plan
    c = _case(run, "dec", torch.bfloat16)
    q, k, v = c.dev
    mask = _masks("edges")
    ref = _attention(c, mask)
    fp = plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, key_mask=mask)
    assert fp._entry == "gta_attn_fwd_gather" and fp.key_lens.tolist() == mask.sum(1).tolist() and tuple(fp.key_idx.shape) == (B, TK)
    pk = c.packed
    for _ in range(2):
        got = fp(q, k, v, pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"), c.tc)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    with pytest.raises(native.GtaError, match="key_mask with key_views"):
        plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, key_mask=mask, key_views=[NK] * B)
    for flag, word in ((native.FLAG_FUSED_KV, "FUSED_KV"), (native.FLAG_PRETRANSFORMED, "PRETRANSFORMED")):
        with pytest.raises(native.GtaError, match=word):
            plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, flags=flag, key_mask=mask)


def test_render_image_with_a_mask_of_leading_views_is_input_views():
    """a tiny TransformingSRT on a fused layout (se3 16 | so2 16 at dh 32), two scenes with 2 and 3 valid input views: encoder, render_image
    (chunked, with the K/V cache) and forward under input_mask = "the leading views" give the bits they give under input_views"""
    from gta_amd import srt
    method = {"method": {"name": "gta", "args": {"f_dims": {"se3": 16, "so2": 16}, "so2": 4, "max_freq_h": 1, "max_freq_w": 1}}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 64, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 64, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
                              "attn_args": method}}
    torch.manual_seed(0)
    model = srt.TransformingSRT(cfg).cuda().eval()
    nb, NV, h, w, views = 2, 3, 16, 20, [2, 3]
    data = srt.synthetic_batch(nb, n_in=NV, n_tgt=1, image=32, points_per_view=8, device="cuda", seed=1)
    P = data["input_coord"].shape[2]
    mask = torch.zeros(nb, NV, P, dtype=torch.bool, device="cuda")
    for b, n in enumerate(views):
        mask[b, :n] = True
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, h, w, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 3, generator=g).cuda()
    coord = torch.from_numpy(G2.make_2dcoord(h, w)).cuda().flatten(0, 1)[:40]

    def render(**how):
        extras = {"input_transforms": data["input_transforms"], "input_coord": data["input_coord"], "target_transforms": data["target_transforms"][:, :1]}
        enc_extra = {"key_views": how["input_views"]} if "input_views" in how else {"key_mask": how["input_mask"].flatten(1)}
        with torch.no_grad():
            z, ex = model.encoder(data["input_images"], data["input_camera_pos"], data["input_rays"], dict(extras, **enc_extra))
            ex = {k_: v_ for k_, v_ in ex.items() if k_ not in enc_extra}
            img, _ = srt.render_image(model, z, cam, rays, ex, max_num_rays=96, reuse_kv=True, **how)
            ex2 = dict(extras, target_coord=coord[None, None].expand(nb, 1, -1, -1))
            pix, _ = model(data["input_images"], data["input_camera_pos"], data["input_rays"], cam[:, None, None].expand(-1, 1, 40, -1),
                           rays.flatten(1, 2)[:, None, :40], ex2, **how)
            assert "key_mask" not in ex2 and "key_views" not in ex2
        return z, img, pix

    z_m, img_m, pix_m = render(input_mask=mask)
    z_v, img_v, pix_v = render(input_views=views)
    torch.cuda.synchronize()
    assert torch.isfinite(img_m).all() and torch.isfinite(pix_m).all()
    assert torch.equal(z_m, z_v) and torch.equal(img_m, img_v) and torch.equal(pix_m, pix_v)
    img_f, _pix = render(input_mask=mask.flatten(1))[1:]
    assert torch.equal(img_f, img_m)

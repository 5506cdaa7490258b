"""GPU: attention over any per-scene subset of the key tokens on the staged generic layouts (`gta_attention(..., key_mask=...,
key_mask_generic=True)`; `gta_attn_fwd_staged_gather`: the GATHER instances of `gta_gen_prep_kernel` compact the valid keys and their euclid
bias, the VARLEN `gta_gen_attn_kernel` attends over them).

Shapes and masks are those of tests/test_gpu_key_mask.py: B = 4 scenes, H = 2, 5 input views of 52 tokens (Tk = 260: five 64-key tiles with a
tail of 4), a decoder-like leg of 150 query rows and a self-attention leg; its `edges` and `random` masks (counts 260 / 1 / 65 / 64 and at least
one key per scene: asserted there).  Layouts: the four STAGED_RUNS of tests/test_gpu_staged.py and so3 of degree 1 on unaligned slabs
(`se3 48 | so3 24 | so2 24`); bf16 and fp32 inputs.

Bars (none new): the workspace rules and their element / bias bars are those of tests/_staged_gather_images.py (derived in
tests/test_gpu_prep_images.py); the output bar is tests/test_gpu_staged.py's `_bar`, the LSE bound its
1.01 * 2^-8 * scale / tau * max|q'| max|k'| + 1e-4 with the maxima over the VALID keys of the scene (trans_coeff 0.37, as there)."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests import _images as I
from tests import _staged_gather_images as SG
from tests.test_gpu_key_mask import B, H, M13, NK, PK, TK, TQ_DEC, _masks
from tests.test_gpu_run_configs import RUNS
from tests.test_gpu_staged import STAGED_RUNS, _bar

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
TC = 0.37
_SO3_1 = {"so2": 6, "so3": 1, "max_freq_h": 1, "max_freq_w": 1, "f_dims": {"triv": 0, "se3": 48, "so3": 24, "so2": 24}}
LAYOUT_ARGS = {run: RUNS[run] for run in STAGED_RUNS}
LAYOUT_ARGS["so3-1/unaligned"] = (96, True, _SO3_1, _SO3_1)
LAYOUTS = sorted(LAYOUT_ARGS)


@functools.lru_cache(maxsize=None)
def _case(run, side, dtype):
    """masters on the CPU (rounded to the input type), device inputs and packed tables -- built once, never written to"""
    from gta_amd import synth
    dh, _mixed, enc, dec = LAYOUT_ARGS[run]
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
                           euclid=bool(args.get("euclid_sim", False)), so3=G2._so3_degree(f_dims, packed, exd), scale=dh ** -0.5, dev=dev,
                           tc=torch.tensor([TC], device="cuda"), Tq=Tq, Nq=1 if side == "dec" else NK, B=B, H=H, T=TK)


def _tensors(mask):
    return G2.key_index_tensors(mask, torch.device("cuda", torch.cuda.current_device()))


def _flags(c, extra=0):
    return native.FLAG_V_TRANSFORM | (native.FLAG_EUCLID if c.euclid else 0) | extra


def _abi(c, key_idx, key_lens, packed=None, qkv=None, ws=None, flags_extra=0, entry="gather", tau=1.0):
    """one direct ctypes call of gta_attn_fwd_staged_gather (or, entry='varlen', of gta_attn_fwd_staged_varlen) on a 0xFF-filled workspace;
    returns out, lse, workspace"""
    q, k, v = qkv or c.dev
    pk = packed or c.packed
    Tk = k.shape[2]
    out = torch.empty(B, c.Tq, H, c.dh, device="cuda", dtype=c.dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, c.Tq, device="cuda", dtype=torch.float32)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, NK, c.scale, _flags(c, flags_extra))
    p, L = native._ptr, native.lib()
    assert native.attn_fwd_staged_gather_supported(desc) == 0
    need = native.attn_fwd_staged_workspace_bytes(desc)
    assert need == I.staged_layout(B, H, Tk, c.dh).total
    if ws is None:
        ws = torch.full((need,), 0xFF, device="cuda", dtype=torch.uint8)
    ta = torch.tensor([tau], device="cuda") if tau != 1.0 else None
    tables = (p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")), p(pk.get("cs_k")), p(pk.get("coord_q")), p(pk.get("coord_k")),
              p(c.tc), p(ta))
    prep_only = bool(flags_extra & native.FLAG_PREP_ONLY)
    ends = (None if prep_only else p(out), None if prep_only else p(lse), p(ws), ws.numel(), native._stream())
    if entry == "gather":
        rc = L.gta_attn_fwd_staged_gather(ctypes.byref(desc), None if prep_only else p(q), p(k), p(v), *tables, p(key_idx), p(key_lens), *ends)
    else:
        rc = L.gta_attn_fwd_staged_varlen(ctypes.byref(desc), None if prep_only else p(q), p(k), p(v), *tables, p(key_lens), *ends)
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    return out, lse, ws


def _attention(c, mask=None, packed=None, qkv=None, tau=1.0, generic=True, **kw):
    q, k, v = qkv or c.dev
    ta = torch.tensor([tau], device="cuda") if tau != 1.0 else None
    if mask is not None:
        kw["key_mask"] = mask
        if generic:
            kw["key_mask_generic"] = True
    with torch.no_grad():
        return gta_amd.gta_attention(q, k, v, c.f_dims, packed or c.packed, so3_degree=c.so3, trans_coeff=c.tc, tau=ta, scale=c.scale,
                                     euclid=c.euclid, **kw)


def _ref_rows(c):
    cpu_tables = {n: t.cpu() for n, t in c.packed.items()}
    return I.ref_rows(c.k, c.v, cpu_tables, c.f_dims, NK, c.so3, TC, True, c.euclid)


# ---- 1. the workspace contract -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", ["edges", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_workspace_contract(run, dtype, masks):
    """a GTA_FLAG_PREP_ONLY call on a 0xFF-filled workspace, element by element against the gather rule, the bias rule, the zero rule and the
    skip rule of tests/_staged_gather_images.py; the entries of key_idx at or past key_lens point at other (in-range) tokens: never used.
    Then the same with the live indices reversed."""
    c = _case(run, "dec", dtype)
    mask = _masks(masks)
    key_idx, key_lens = _tensors(mask)
    _, _, ws = _abi(c, key_idx, key_lens, flags_extra=native.FLAG_PREP_ONLY)
    ref = _ref_rows(c)
    idx_ref, lens_ref = SG.index_tensors(mask)
    assert torch.equal(key_idx.cpu().long(), idx_ref) and torch.equal(key_lens.cpu().long(), lens_ref)
    SG.check(f"{run} {dtype} {masks}", ws.cpu(), c, ref, idx_ref, lens_ref, c.euclid, c.scale)
    rev = key_idx.clone()
    for b, n in enumerate(lens_ref.tolist()):
        rev[b, :n] = key_idx[b, :n].flip(0)
    _, _, ws2 = _abi(c, rev, key_lens, flags_extra=native.FLAG_PREP_ONLY)
    SG.check(f"{run} {dtype} {masks} reversed", ws2.cpu(), c, ref, rev.cpu().long(), lens_ref, c.euclid, c.scale)


HEAD_SIZES = {16: {"se3": 4, "t2": 12}, 40: {"se3": 16, "t2": 24}, 104: {"se3": 32, "t2": 72}, 128: {"se3": 8, "t2": 120}}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", sorted(HEAD_SIZES))
def test_workspace_contract_at_every_head_size(dh, dtype):
    """the GATHER instances at dhp 32 / 64 / 128 on head sizes that leave chunks of a padded row unused (and the full 128), on token-major K
    and V ([B,T,H,dh] storage: the packed projection's strides); B = 3, H = 3, 3 views of 50 tokens (Tk = 150), masks: every third token
    dropped (100 keys), Bernoulli 0.3, all keys"""
    c = I.key_side_case(HEAD_SIZES[dh], 0, dtype, B=3, H=3, Nk=3, Pk=50, seed=5)
    assert c.dh == dh
    mask = torch.ones(c.B, c.T, dtype=torch.bool)
    mask[0, 2::3] = False
    mask[1] = torch.rand(c.T, generator=torch.Generator().manual_seed(dh)) < 0.3
    mask[1, 149] = True
    key_idx, key_lens = _tensors(mask)
    k, v = (t.to(dtype).cuda() for t in (c.k, c.v))
    assert k.stride() == (c.T * c.H * dh, dh, c.H * dh, 1)
    st = [tuple(k.stride()[:3])] * 4
    desc = native.make_desc_from(dtype, (c.B, c.H, c.T, dh), c.T, st, c.f_dims, 0, c.Nk, c.Nk, dh ** -0.5, native.FLAG_V_TRANSFORM | native.FLAG_PREP_ONLY)
    assert native.attn_fwd_staged_gather_supported(desc) == 0
    ws = torch.full((native.attn_fwd_staged_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    p, L = native._ptr, native.lib()
    vrep, coord, tc = c.packed["vrep_k"].cuda(), c.packed["coord_k"].cuda(), torch.tensor([TC], device="cuda")
    rc = L.gta_attn_fwd_staged_gather(ctypes.byref(desc), None, p(k), p(v), p(vrep), p(vrep), None, None, p(coord), p(coord), p(tc), None,
                                      p(key_idx), p(key_lens), None, None, p(ws), ws.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, 0, TC)
    SG.check(f"dh{dh} {dtype}", ws.cpu(), c, ref, *SG.index_tensors(mask), False)


# ---- 2. / 3. bit-for-bit equalities ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [(1, 3, 4, 5), (NK,) * B])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_a_mask_of_leading_views_is_key_views(run, side, dtype, views):
    """out, lse and every byte of the workspace -- written tiles and bias; both calls start from 0xFF -- equal those of
    gta_attn_fwd_staged_varlen under the same prefixes: whole leading views, and the all-true mask against key_views = [Nk] * B;
    gta_attention(key_mask=, key_mask_generic=True) gives the same out"""
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
    """the mask "first 13 tokens of every view" against gta_attn_fwd_staged_varlen on k, v, cs_k and coord_k physically cut to those tokens
    (five views of 13 tokens, key_lens = 65): out and lse bit for bit; the sliced call's workspace has other strides, so its two tiles and
    their bias are compared per (b, h, tile)"""
    c = _case(run, side, dtype)
    mask = _masks("first13")
    key_idx, key_lens = _tensors(mask)
    out, lse, ws = _abi(c, key_idx, key_lens)
    cols = mask[0].nonzero().flatten().cuda()
    q, k, v = c.dev
    pk = dict(c.packed)
    for name in ("cs_k", "coord_k"):
        if name in pk:
            pk[name] = c.packed[name][:, cols].contiguous()
    ks, vs = k[:, :, cols].contiguous(), v[:, :, cols].contiguous()
    Tk1 = NK * M13
    lens1 = torch.full((B,), Tk1, device="cuda", dtype=torch.int32)
    out1, lse1, ws1 = _abi(c, None, lens1, packed=pk, qkv=(q, ks, vs), entry="varlen")
    assert torch.equal(out, out1) and torch.equal(lse, lse1)
    d, d1 = I.decode(ws.cpu(), B, H, TK, c.dh, staged=True), I.decode(ws1.cpu(), B, H, Tk1, c.dh, staged=True)
    nt = d1.layout.n_tiles
    assert nt == 2 and torch.equal(d.bits[:, :, :nt], d1.bits) and torch.equal(d.aux_raw[:, :, :nt * 64], d1.aux_raw)
    assert bool((d.bits[:, :, nt:] == -1).all()) and bool((d.aux_raw[:, :, nt * 64:] == -1).all())
    assert bool((d.aux_raw[:, :, :nt * 64] != -1).all()) == c.euclid


# ---- 4. oracle parity -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle(run, side, dtype, masks):
    """fp64 per scene: O.transform_qkv on the whole key side, the valid key columns, softmax with the euclid bias (at tau 1.0 and 1.7),
    O.inverse_transform_out -> {tau: [(out, LSE, LSE bound on the valid keys)]}"""
    c = _case(run, side, dtype)
    res = {1.0: [], 1.7: []}
    for b in range(B):
        ex64 = {"input_transforms": c.ex["input_transforms"][b:b + 1].double(), "input_coord": c.ex["input_coord"][b:b + 1].double()}
        reps = O.encoder_reps(c.enc, ex64)
        if side == "dec":
            ex64["target_transforms"] = c.ex["target_transforms"][b:b + 1].double()
            ex64["target_coord"] = c.ex["target_coord"][b:b + 1].double()
            reps = O.decoder_reps(c.dec, ex64, reps)
        qt, kt, vt = O.transform_qkv(c.q[b:b + 1].double(), c.k[b:b + 1].double(), c.v[b:b + 1].double(), c.f_dims, reps, TC, True, c.euclid)
        cols = _masks(masks)[b].nonzero().flatten()
        kt, vt = kt[:, :, cols], vt[:, :, cols]
        # the LSE convention of the staged route (tests/test_gpu_staged.py): the key bias in, the row-constant -scale |q'|^2 / 2 out
        sim = c.scale * qt @ kt.transpose(-1, -2)
        if c.euclid:
            sim = sim - 0.5 * c.scale * kt.pow(2).sum(-1)[..., None, :]
        for tau in res:
            out = O.inverse_transform_out(torch.softmax(sim / tau, -1) @ vt, c.f_dims, reps, TC, c.euclid)
            lse_bar = 1.01 * 2.0 ** -8 * c.scale / tau * (qt.norm(dim=-1).max() * kt.norm(dim=-1).max()).item() + 1e-4
            res[tau].append((out[0], torch.logsumexp(sim / tau, -1)[0], lse_bar))
    return res


@pytest.mark.parametrize("tau", [1.0, 1.7])
@pytest.mark.parametrize("masks", ["edges", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_parity_with_the_oracle_on_the_valid_keys(run, side, dtype, masks, tau):
    c = _case(run, side, dtype)
    mask = _masks(masks)
    out, lse = _attention(c, mask.cuda(), tau=tau, return_lse=True)
    torch.cuda.synchronize()
    for b, (ref, ref_lse, lse_bar) in enumerate(_oracle(run, side, dtype, masks)[tau]):
        st = C.err_stats(out[b].float().cpu(), ref.float())
        lse_err = (lse[b].double().cpu() - ref_lse).abs().max().item()
        print(f"KEY_MASK_GENERIC {run} {side} {dtype} {masks} tau={tau} scene {b} ({int(mask[b].sum())} keys): {st} | lse max_abs {lse_err:.3e} "
              f"(bar {lse_bar:.3e})")
        assert torch.isfinite(lse[b]).all()
        assert _bar(st), (run, side, dtype, masks, tau, b, st)
        assert lse_err <= lse_bar, (run, side, dtype, masks, tau, b, lse_err, lse_bar)


# ---- 5. masked content is never used -------------------------------------------------------------------------------------------------------
def _poisoned(c, mask, value):
    """k, v, cs_k and coord_k with every masked row, and vrep_k with the record of every view without a live token, filled with `value` (a
    float or a callable giving a tensor)"""
    k, v = c.dev[1].clone(), c.dev[2].clone()
    pk = dict(c.packed)
    dead = (~mask).cuda()
    fill = lambda rows: value(rows) if callable(value) else torch.full_like(rows, value)
    for t in (k, v):
        t.permute(0, 2, 1, 3)[dead] = fill(t.permute(0, 2, 1, 3)[dead])                      # [n_dead, H, dh]
    for name in ("cs_k", "coord_k"):
        if name in pk:
            pk[name] = pk[name].clone()
            pk[name][dead] = fill(pk[name][dead])
    dead_views = (~mask.reshape(B, NK, PK).any(-1)).cuda()
    pk["vrep_k"] = pk["vrep_k"].clone()
    pk["vrep_k"][dead_views] = fill(pk["vrep_k"][dead_views])
    return (c.dev[0], k, v), pk, int(dead_views.sum())


@pytest.mark.parametrize("masks", ["edges", "random"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_masked_tokens_may_hold_nan_and_inf(run, dtype, masks):
    """NaN, then +-Inf, in every masked row of k, v, cs_k and coord_k and in the vrep_k record of every view without a live token, with the
    entries of key_idx past key_lens pointing at exactly those rows (in range: the masked tokens, as key_index_tensors leaves them): out, lse
    and the workspace are finite where written and bit-identical to the run with zeros there"""
    c = _case(run, "dec", dtype)
    mask = _masks(masks)
    key_idx, key_lens = _tensors(mask)
    for b, n in enumerate(key_lens.tolist()):                  # what lies past the count names masked tokens only
        assert not bool(mask[b][key_idx[b, n:].cpu().long()].any())
    qkv0, pk0, n_dead_views = _poisoned(c, mask, 0.0)
    if masks == "edges":
        assert n_dead_views == 4 + 2                           # scene 1: every view but token 137's; scene 3: views 1 and 3
    out0, lse0, ws0 = _abi(c, key_idx, key_lens, pk0, qkv0)
    assert torch.isfinite(out0).all() and torch.isfinite(lse0).all()
    signs = lambda t: torch.where(torch.arange(t.numel(), device=t.device).reshape(t.shape) % 2 == 0, float("inf"), float("-inf")).to(t.dtype)
    for value in (float("nan"), signs):
        qkv, pk, _ = _poisoned(c, mask, value)
        assert not torch.isfinite(qkv[1]).all() and (n_dead_views == 0 or not torch.isfinite(pk["vrep_k"]).all())
        out, lse, ws = _abi(c, key_idx, key_lens, pk, qkv)
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), (run, dtype, masks)
        assert torch.equal(out, out0) and torch.equal(lse, lse0) and torch.equal(ws, ws0), (run, dtype, masks)
        assert torch.equal(_attention(c, mask.cuda(), packed=pk, qkv=qkv), out0)


# ---- 6. plumbing -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", LAYOUTS)
def test_kv_cache_holds_the_compacted_images(run):
    """two calls with one cache dict, k and v overwritten in between: the second returns the same bits and runs no pre-pass (the workspace
    bytes do not change); the cache without the mask, or under key_views, is refused"""
    c = _case(run, "dec", torch.bfloat16)
    mask = _masks("random").cuda()
    q, k, v = c.dev[0], c.dev[1].clone(), c.dev[2].clone()
    cache = {}
    a = _attention(c, mask, qkv=(q, k, v), kv_cache=cache).clone()
    assert cache["plan"][0] == "staged" and cache["plan"][-1] == "key_mask" and cache["images"].numel() > 0
    assert torch.equal(cache["key_lens"].cpu(), mask.sum(1).int().cpu()) and tuple(cache["key_idx"].shape) == (B, TK)
    assert torch.equal(a, _attention(c, mask))
    before = cache["images"].clone()
    k.fill_(7.0)
    v.fill_(-3.0)
    b = _attention(c, mask, qkv=(q, k, v), kv_cache=cache)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(cache["images"], before)
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
    fp = plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, euclid=c.euclid, key_mask=mask)
    assert fp._staged and fp._entry == "gta_attn_fwd_staged_gather"
    assert fp.key_lens.tolist() == mask.sum(1).tolist() and tuple(fp.key_idx.shape) == (B, TK)
    pk = c.packed
    for _ in range(2):
        got = fp(q, k, v, pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"), c.tc, coord_q=pk.get("coord_q"),
                 coord_k=pk.get("coord_k"))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    with pytest.raises(native.GtaError, match="key_mask with key_views"):
        plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, euclid=c.euclid, key_mask=mask, key_views=[NK] * B)


@pytest.mark.parametrize("run", ["clevrtr/gta_euclid", "msn/gta_t2"])
def test_a_mask_index_companion_gives_the_same_bits(run):
    c = _case(run, "enc", torch.bfloat16)
    mask = _masks("random").cuda()
    out, lse = _attention(c, mask, return_lse=True)
    mi = G2.mask_index(mask, device=mask.device)
    got, got_lse = _attention(c, mask, return_lse=True, mask_index=mi)
    torch.cuda.synchronize()
    assert torch.equal(got, out) and torch.equal(got_lse, lse)


def test_render_image_with_a_mask_of_leading_views_is_input_views():
    """a tiny TransformingSRT with the gta_t2 attention settings (se3 12 | t2 12 at dh 24), two scenes with 2 and 3 valid input views:
    encoder, render_image (chunked, with the K/V cache) and forward under input_mask = "the leading views" with input_mask_generic=True give
    the bits they give under input_views; without the opt-in the mask is refused as before"""
    from gta_amd import srt
    args = {"f_dims": {"triv": 0, "se3": 12, "t2": 12}, "so2": False, "max_freq_h": 1, "max_freq_w": 1}
    method = {"method": {"name": "gta", "args": args}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 48, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 48, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
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
        if "input_views" in how:
            enc_extra = {"key_views": how["input_views"]}
        else:
            enc_extra = {"key_mask": how["input_mask"].flatten(1)}
            if how.get("input_mask_generic"):
                enc_extra["key_mask_generic"] = True
        with torch.no_grad():
            z, ex = model.encoder(data["input_images"], data["input_camera_pos"], data["input_rays"], dict(extras, **enc_extra))
            ex = {k_: v_ for k_, v_ in ex.items() if k_ not in enc_extra}
            caches = []
            real = G2._staged_forward

            def spy(*a, **kw):
                if a[11] is not None and not any(a[11] is s for s in caches):
                    caches.append(a[11])
                return real(*a, **kw)
            G2._staged_forward = spy
            try:
                img, _ = srt.render_image(model, z, cam, rays, ex, max_num_rays=96, reuse_kv=True, **how)
            finally:
                G2._staged_forward = real
            ex2 = dict(extras, target_coord=coord[None, None].expand(nb, 1, -1, -1))
            pix, _ = model(data["input_images"], data["input_camera_pos"], data["input_rays"], cam[:, None, None].expand(-1, 1, 40, -1),
                           rays.flatten(1, 2)[:, None, :40], ex2, **how)
            assert "key_mask" not in ex2 and "key_views" not in ex2 and "key_mask_generic" not in ex2
        return z, img, pix, caches

    z_m, img_m, pix_m, caches = render(input_mask=mask, input_mask_generic=True)
    assert len(caches) == 2 and all(c_["plan"][0] == "staged" and c_["plan"][-1] == "key_mask" and "key_idx" in c_ for c_ in caches)
    z_v, img_v, pix_v, _ = render(input_views=views)
    torch.cuda.synchronize()
    assert torch.isfinite(img_m).all() and torch.isfinite(pix_m).all()
    assert torch.equal(z_m, z_v) and torch.equal(img_m, img_v) and torch.equal(pix_m, pix_v)
    with pytest.raises(native.GtaError, match="no gather pre-pass"):
        render(input_mask=mask)


# ---- 7. without the keyword ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", LAYOUTS)
def test_without_the_keyword_the_call_still_raises(run):
    c = _case(run, "dec", torch.bfloat16)
    with pytest.raises(native.GtaError, match="no gather pre-pass"):
        _attention(c, _masks("edges").cuda(), generic=False)

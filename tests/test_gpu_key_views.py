"""GPU: per-scene key prefixes (`gta_attention(..., key_views=...)`; `gta_attn_fwd_varlen`, `gta_attn_fwd_staged_varlen`).

Shapes: B = 5 scenes, H = 2, 13 input views of 20 tokens (Tk = 260, five 64-key tiles), key_views = [1, 3, 4, 7, 13] -- prefixes of 20
(one tile: keeps the true row max), 60 (one ragged tile), 80 (64 + 16: a tail of whole 8-key groups, the lazy path), 140 (two tiles + 12:
shorter than the three-stage ring) and 260 keys (more tiles than ring stages, nothing padded).  Query side: a decoder-like leg of 150 rows
(two 128-row items, one ragged) and a self-attention leg (Tq = Tk).  Layouts: CLEVR-TR `se3 32 | so2 32` (dh 64) and MSN `gta_so3` (dh 96) on
the fused two-stage plan, `clevrtr/gta_euclid` and `msn/gta_t2` on the staged route; bf16 and fp32 inputs.

Bars (none new).  Fused layouts: tests/test_gpu_forward.py's REL_MAX / REL_RMS for the output and its LSE bar (`test_lse_matches_logsumexp`:
2e-2 absolute, trans_coeff 0.01).  Staged route: tests/test_gpu_staged.py's `_bar` for the output and its LSE bound (see that file's
docstring), evaluated per scene on the prefix."""
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
from tests.test_gpu_forward import REL_MAX, REL_RMS
from tests.test_gpu_run_configs import RUNS
from tests.test_gpu_staged import _bar as staged_bar

pytestmark = pytest.mark.gpu

B, H, NK, PK, TQ_DEC = 5, 2, 13, 20, 150
TK = NK * PK
KV = [1, 3, 4, 7, 13]
FUSED = ["clevrtr/gta", "msn/gta_so3"]
STAGED = ["clevrtr/gta_euclid", "msn/gta_t2"]
LAYOUTS = FUSED + STAGED
DTYPES = [torch.float32, torch.bfloat16]
K_TABLES = ("vrep_k", "cs_k", "coord_k")


def _tc(run):
    return 0.01 if run in FUSED else 0.37          # (the trans_coeff of the file each family's bars come from)


@functools.lru_cache(maxsize=None)
def _case(run, side, dtype):
    """masters on the CPU (rounded to the input type), device inputs and packed tables -- built once, never written to"""
    from gta_amd import synth
    dh, _mixed, enc, dec = RUNS[run]
    g = torch.Generator().manual_seed(sum(map(ord, run)) + (side == "dec"))
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
    tc = torch.tensor([_tc(run)], device="cuda") if f_dims.get("se3", 0) > 0 else None
    return SimpleNamespace(run=run, side=side, dtype=dtype, dh=dh, q=q, k=k, v=v, ex=ex, enc=enc, dec=dec, f_dims=f_dims, packed=packed,
                           euclid=args.get("euclid_sim", False), so3=G2._so3_degree(f_dims, packed, exd), scale=dh ** -0.5, dev=dev, tc=tc,
                           Tq=Tq, Nq=1 if side == "dec" else NK, fused=run in FUSED)


def _rows(c, b):
    """the query rows of scene b a test may look at: all of them, or (self-attention) those of its valid views"""
    return c.Tq if c.side == "dec" else KV[b] * PK


@functools.lru_cache(maxsize=None)
def _oracle(run, side, dtype):
    """fp64, scene by scene on the key prefix with the key-side tables cut to the valid views: out, LSE, LSE bar per scene"""
    c = _case(run, side, dtype)
    res = []
    for b, n in enumerate(KV):
        ex64 = {"input_transforms": c.ex["input_transforms"][b:b + 1, :n].double(), "input_coord": c.ex["input_coord"][b:b + 1, :n].double()}
        reps = O.encoder_reps(c.enc, ex64)
        q = c.q[b:b + 1].double()
        if side == "dec":
            ex64["target_transforms"] = c.ex["target_transforms"][b:b + 1].double()
            ex64["target_coord"] = c.ex["target_coord"][b:b + 1].double()
            reps = O.decoder_reps(c.dec, ex64, reps)
        else:
            q = q[:, :, :n * PK]
        k, v = c.k[b:b + 1, :, :n * PK].double(), c.v[b:b + 1, :, :n * PK].double()
        out, _ = O.gta_attention(q, k, v, c.f_dims, reps, _tc(run), True, c.euclid, scale=c.scale)
        qt, kt, _ = O.transform_qkv(q, k, v, c.f_dims, reps, _tc(run), True, c.euclid)
        sim = c.scale * qt @ kt.transpose(-1, -2)
        if c.euclid:
            sim = sim - 0.5 * c.scale * kt.pow(2).sum(-1)[..., None, :]
        lse_bar = 1.01 * 2.0 ** -8 * c.scale * (qt.norm(dim=-1).max() * kt.norm(dim=-1).max()).item() + 1e-4      # (tests/test_gpu_staged.py)
        res.append((out[0], torch.logsumexp(sim, -1)[0], lse_bar))
    return res


def _key_lens(kv=KV):
    return G2.key_lens_tensor(tuple(kv), PK, torch.device("cuda", torch.cuda.current_device()))


def _abi(c, key_lens, packed=None, qkv=None, ws=None, flags_extra=0):
    """one direct ctypes call of the varlen entry of the case's family; returns out, lse, workspace"""
    q, k, v = qkv or c.dev
    pk = packed or c.packed
    flags = native.FLAG_V_TRANSFORM | (native.FLAG_EUCLID if c.euclid else 0) | flags_extra
    out = torch.empty(B, c.Tq, H, c.dh, device="cuda", dtype=c.dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, c.Tq, device="cuda", dtype=torch.float32)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, NK, c.scale, flags)
    p, L = native._ptr, native.lib()
    if c.fused:
        assert native.attn_fwd_varlen_supported(desc) == 0
        need = native.attn_fwd_workspace_bytes(desc)
    else:
        assert native.attn_fwd_staged_varlen_supported(desc) == 0
        need = native.attn_fwd_staged_workspace_bytes(desc)
    if ws is None:
        ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    if c.fused:
        rc = L.gta_attn_fwd_varlen(ctypes.byref(desc), p(q), p(k), p(v), p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")), p(pk.get("cs_k")),
                                   p(c.tc), None, p(key_lens), p(out), p(lse), p(ws), ws.numel(), native._stream())
    else:
        rc = L.gta_attn_fwd_staged_varlen(ctypes.byref(desc), p(q), p(k), p(v), p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")),
                                          p(pk.get("cs_k")), p(pk.get("coord_q")), p(pk.get("coord_k")), p(c.tc), None, p(key_lens),
                                          p(out), p(lse), p(ws), ws.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    return out, lse, ws


def _attention(c, key_views=KV, packed=None, qkv=None, **kw):
    q, k, v = qkv or c.dev
    with torch.no_grad():
        return gta_amd.gta_attention(q, k, v, c.f_dims, packed or c.packed, so3_degree=c.so3, trans_coeff=c.tc, scale=c.scale, euclid=c.euclid,
                                     **({"key_views": key_views} if key_views is not None else {}), **kw)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_parity_with_the_oracle_on_the_prefix(run, side, dtype):
    """1. out and LSE of every valid query row against the fp64 oracle run scene by scene on the key prefix"""
    c = _case(run, side, dtype)
    out, lse, _ = _abi(c, _key_lens())
    got = _attention(c)
    torch.cuda.synchronize()
    assert torch.equal(got, out)                       # gta_attention took the varlen entry of the family
    for b, (ref, ref_lse, lse_bar) in enumerate(_oracle(run, side, dtype)):
        r = _rows(c, b)
        st = C.err_stats(out[b, :, :r].float().cpu(), ref.float())
        lse_err = (lse[b, :, :r].double().cpu() - ref_lse).abs().max().item()
        print(f"KEY_VIEWS {run} {side} {dtype} scene {b} ({KV[b]} views): {st} | lse max_abs {lse_err:.3e}")
        assert torch.isfinite(lse[b, :, :r]).all()
        if c.fused:                                    # tests/test_gpu_forward.py: _check, test_lse_matches_logsumexp
            assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] and st["rel_rms"] <= REL_RMS, (run, side, dtype, b, st)
            assert lse_err < 2e-2, (run, side, dtype, b, lse_err)
        else:                                          # tests/test_gpu_staged.py: _bar and its LSE bound
            assert staged_bar(st), (run, side, dtype, b, st)
            assert lse_err <= lse_bar, (run, side, dtype, b, lse_err, lse_bar)


def _poisoned(c, value):
    """q, k, v and the key-side tables with everything that belongs to a padded view filled with `value` (a float or a callable giving a tensor)"""
    k, v = c.dev[1].clone(), c.dev[2].clone()
    pk = dict(c.packed)
    for name in K_TABLES:
        if name in pk:
            pk[name] = pk[name].clone()
    for b, n in enumerate(KV):
        for t, cut in ((k[b, :, n * PK:], None), (v[b, :, n * PK:], None), (pk.get("vrep_k"), n), (pk.get("cs_k"), n * PK), (pk.get("coord_k"), n * PK)):
            if t is None:
                continue
            tgt = t if cut is None else t[b, cut:]
            if callable(value):
                tgt.copy_(value(tgt))
            else:
                tgt.fill_(value)
    return (c.dev[0], k, v), pk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_padded_views_may_hold_nan_and_inf(run, dtype):
    """2. K, V, cs_k, coord_k and the vrep_k records of every padded view filled with NaN, then with +-Inf: out and LSE of the cross-attention
    leg are finite and bit-identical to the run with zeros in the same places"""
    c = _case(run, "dec", dtype)
    kl = _key_lens()
    qkv0, pk0 = _poisoned(c, 0.0)
    out0, lse0, _ = _abi(c, kl, pk0, qkv0)
    assert torch.isfinite(out0).all() and torch.isfinite(lse0).all()
    signs = lambda t: torch.where(torch.arange(t.numel(), device=t.device).reshape(t.shape) % 2 == 0, float("inf"), float("-inf")).to(t.dtype)
    for value in (float("nan"), signs):
        qkv, pk = _poisoned(c, value)
        assert not torch.isfinite(qkv[1]).all() and not torch.isfinite(pk["vrep_k"]).all()
        out, lse, _ = _abi(c, kl, pk, qkv)
        assert torch.isfinite(out).all() and torch.isfinite(lse).all(), (run, dtype, value)
        assert torch.equal(out, out0) and torch.equal(lse, lse0), (run, dtype, value)
        assert torch.equal(_attention(c, packed=pk, qkv=qkv), out0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_bits_of_the_cut_down_call(run, side, dtype):
    """3. for each scene the batched varlen result equals, bit for bit, gta_attention on that scene alone with its key side cut to the prefix
    (on the same kernel family: kv_mode='prepass_fwd2' for the fused layouts, the staged route otherwise); the scene with every view equals
    the batched call without key_views as well"""
    c = _case(run, side, dtype)
    mode = {"kv_mode": "prepass_fwd2"} if c.fused else {}
    got = _attention(c)
    q, k, v = c.dev
    for b, n in enumerate(KV):
        pk = {}
        for name, t in c.packed.items():
            cut = {"vrep_k": n, "cs_k": n * PK, "coord_k": n * PK}.get(name)
            pk[name] = t[b:b + 1] if cut is None else t[b:b + 1, :cut].contiguous()
        alone = _attention(c, None, pk, (q[b:b + 1], k[b:b + 1, :, :n * PK], v[b:b + 1, :, :n * PK]), **mode)
        r = _rows(c, b)
        assert torch.equal(got[b, :, :r], alone[0, :, :r]), (run, side, dtype, b)
    full = _attention(c, None, **mode)
    torch.cuda.synchronize()
    assert KV[-1] == NK and torch.equal(got[-1], full[-1])


@pytest.mark.parametrize("run", ["clevrtr/gta", "msn/gta_so3", "clevrtr/gta_euclid"])
def test_kv_cache_holds_the_masked_images(run):
    """4. two calls with one cache dict, k and v overwritten in between: the second returns the same bits (no pre-pass ran); the same dict
    under other view counts is refused"""
    c = _case(run, "dec", torch.bfloat16)
    q, k, v = c.dev[0], c.dev[1].clone(), c.dev[2].clone()
    cache = {}
    a = _attention(c, qkv=(q, k, v), kv_cache=cache).clone()
    assert cache.get("images") is not None and cache["images"].numel() > 0 and cache["plan"][-1] == tuple(KV)
    assert torch.equal(a, _attention(c))
    k.fill_(7.0)
    v.fill_(-3.0)
    b = _attention(c, qkv=(q, k, v), kv_cache=cache)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    with pytest.raises(native.GtaError, match="another plan"):
        _attention(c, [2, 3, 4, 7, 13], qkv=(q, k, v), kv_cache=cache)
    with pytest.raises(native.GtaError, match="another plan"):
        _attention(c, None, qkv=(q, k, v), kv_cache=cache)


@pytest.mark.parametrize("run", ["msn/gta_so3", "msn/gta_t2"])
def test_forward_plan_with_key_views(run):
    """5a. a ForwardPlan built with key_views gives the bits of gta_attention"""
    from gta_amd import plan
    c = _case(run, "dec", torch.bfloat16)
    q, k, v = c.dev
    ref = _attention(c)
    fp = plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, euclid=c.euclid, key_views=KV)
    assert fp._staged == (not c.fused) and fp.key_lens.tolist() == [n * PK for n in KV]
    pk = c.packed
    for _ in range(2):
        got = fp(q, k, v, pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"), c.tc, coord_q=pk.get("coord_q"), coord_k=pk.get("coord_k"))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    with pytest.raises(native.GtaError):
        plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, euclid=c.euclid, key_views=[1, 3, 4, 7, 14])
    if c.fused:
        # a flag the varlen entry refuses on a fused layout raises with the library's reason: the plan does not go on to the staged entry
        for flag, word in ((native.FLAG_FUSED_KV, "FUSED_KV"), (native.FLAG_PRETRANSFORMED, "PRETRANSFORMED")):
            with pytest.raises(native.GtaError, match=word):
                plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=c.Nq, Nk=NK, scale=c.scale, euclid=c.euclid, flags=flag, key_views=KV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", ["clevrtr/gta", "msn/gta_t2"])
def test_abi_prep_only_then_kv_ready(run, dtype):
    """5b. both varlen entries through ctypes: GTA_FLAG_PREP_ONLY fills the workspace, GTA_FLAG_KV_READY on it with k and v overwritten gives
    the bits of the full call"""
    c = _case(run, "dec", dtype)
    kl = _key_lens()
    out, lse, _ = _abi(c, kl)
    _, _, ws = _abi(c, kl, flags_extra=native.FLAG_PREP_ONLY)
    junk = torch.full_like(c.dev[1], 3.0)
    out2, lse2, _ = _abi(c, kl, qkv=(c.dev[0], junk, junk), ws=ws, flags_extra=native.FLAG_KV_READY)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)


def test_srt_with_mixed_input_views():
    """6. a tiny TransformingSRT (the config of tests/test_gpu_staged.py's render test), two scenes with 2 and 3 valid input views in one batch
    against the same model run per scene on its valid views; rendered pixels within the bar of tests/test_gpu_modules.py's
    test_render_image_chunked_decode (max_abs < 1e-2, mse < 1e-5)"""
    from gta_amd import srt
    method = {"method": {"name": "gta", "args": {"f_dims": {"triv": 0, "se3": 12, "t2": 12}, "so2": False, "max_freq_h": 1, "max_freq_w": 1}}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 48, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 48, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
                              "attn_args": method}}
    torch.manual_seed(0)
    model = srt.TransformingSRT(cfg).cuda().eval()
    nb, NV, h, w, views = 2, 3, 16, 20, [2, 3]
    data = srt.synthetic_batch(nb, n_in=NV, n_tgt=1, image=32, points_per_view=8, device="cuda", seed=1)
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, h, w, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 3, generator=g).cuda()

    coord = torch.from_numpy(G2.make_2dcoord(h, w)).cuda().flatten(0, 1)[:40]

    def render(sl, n, input_views):
        """render_image of the whole view, and TransformingSRT.forward on its first 40 pixels"""
        nb_ = data["input_images"][sl].shape[0]
        extras = {"input_transforms": data["input_transforms"][sl, :n], "input_coord": data["input_coord"][sl, :n],
                  "target_transforms": data["target_transforms"][sl, :1]}
        images, cpos, irays = data["input_images"][sl, :n], data["input_camera_pos"][sl, :n], data["input_rays"][sl, :n]
        with torch.no_grad():
            z, ex = model.encoder(images, cpos, irays, dict(extras, **({"key_views": input_views} if input_views else {})))
            img, _ = srt.render_image(model, z, cam[sl], rays[sl], ex, max_num_rays=96, reuse_kv=True, input_views=input_views)
            ex2 = dict(extras, target_coord=coord[None, None].expand(nb_, 1, -1, -1))
            pix, _ = model(images, cpos, irays, cam[sl, None, None].expand(-1, 1, 40, -1), rays[sl].flatten(1, 2)[:, None, :40], ex2,
                           input_views=input_views)
            assert "key_views" not in ex2          # the counts of one call never stay behind in the caller's dict
        return img, pix

    img, pix = render(slice(0, nb), NV, views)
    torch.cuda.synchronize()
    for b, n in enumerate(views):
        ref_img, ref_pix = render(slice(b, b + 1), n, None)
        for name, a, r in (("render_image", img[b:b + 1], ref_img), ("forward", pix[b:b + 1], ref_pix)):
            st = C.err_stats(a.float().cpu(), r.float().cpu())
            mse = ((a.float() - r.float()) ** 2).mean().item()
            print(f"KEY_VIEWS srt {name} scene {b} ({n} views): {st} mse {mse:.3e}")
            assert st["finite"] and st["max_abs"] < 1e-2 and mse < 1e-5, (name, b, st, mse)

"""GPU: the staged generic forward (`gta_attn_fwd_staged`: one K/V pre-pass that writes tile images for ANY layout + one attention
kernel with row-wise rho_q / rho_q^-1 in LDS) at the layouts of the four run configs that have no fused kernel --
`clevrtr/gta_euclid`, `clevrtr/gta_t2`, `msn/gta_so3_euclid`, `msn/gta_t2` -- against the fp64 oracle, through the C ABI directly,
through `gta_attention` (route, `kv_cache`), `ForwardPlan` and `render_image`; and the route under grad, which stays `_GenericAttn`.

Bars.  Output: the project's bar for this route (tests/test_gpu_variants.py): finite, max_abs <= 3e-2 * ref_max, rel_rms <= 1.5e-2.
LSE: the kernel rounds q' (pre-scaled) and k' to bf16 once -- a relative error of at most 2^-9 each, so 2^-8 (+ 2^-18) on every product --
and accumulates in fp32; a logit therefore moves by at most 2^-8 * scale / tau * sum_i |q'_i k'_i| <= 2^-8 * scale / tau * |q'| |k'|
(Cauchy-Schwarz), the key bias is added in fp32, and log-sum-exp moves by at most the largest logit error.  The LSE bar is that bound
with the largest |q'| |k'| of the call, times 1.01 for the fp32 sums, plus 1e-4 absolute."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests.test_gpu_run_configs import RUNS, _inputs

pytestmark = pytest.mark.gpu

STAGED_RUNS = ["clevrtr/gta_euclid", "clevrtr/gta_t2", "msn/gta_so3_euclid", "msn/gta_t2"]
TC = 0.37


def _bar(st):
    return st["finite"] and st["max_abs"] <= 3e-2 * st["ref_max"] and st["rel_rms"] <= 1.5e-2


def _case(run, side, dtype, seed=0):
    """masters (rounded to the input type), extras with device reps, packed tables, the side's method args"""
    dh, _mixed, enc, dec = RUNS[run]
    q, k, v, w, ex = _inputs(dh, enc, dec, side, seed=sum(map(ord, run)) + (side == "dec") + seed)
    if dtype == torch.bfloat16:
        q, k, v = (t.bfloat16().float() for t in (q, k, v))
    exd = {kk: vv.cuda() for kk, vv in ex.items()}
    gta_amd.pre_compute_reps_encoder(enc, exd)
    args = enc
    if side == "dec":
        gta_amd.pre_compute_reps_decoder(dec, exd)
        args = dec
    packed = gta_amd.pack_reps(exd, args["f_dims"])
    return SimpleNamespace(dh=dh, q=q, k=k, v=v, w=w, ex=ex, exd=exd, enc=enc, dec=dec, args=args, side=side, packed=packed,
                           f_dims=args["f_dims"], euclid=args.get("euclid_sim", False), so3=G2._so3_degree(args["f_dims"], packed, exd),
                           scale=dh ** -0.5)


def _oracle(c, tau, v_transform=True):
    """fp64: out, and the LSE of the convention of the generic route (key bias in, the row-constant -scale |q'|^2 / 2 out)"""
    ex64 = {kk: (vv.double() if vv.is_floating_point() else vv) for kk, vv in c.ex.items()}
    reps = O.encoder_reps(c.enc, ex64)
    if c.side == "dec":
        reps = O.decoder_reps(c.dec, ex64, reps)
    q, k, v = c.q.double(), c.k.double(), c.v.double()
    out, _ = O.gta_attention(q, k, v, c.f_dims, reps, TC, v_transform, c.euclid, scale=c.scale, tau=tau)
    qt, kt, _ = O.transform_qkv(q, k, v, c.f_dims, reps, TC, v_transform, c.euclid)
    sim = c.scale * qt @ kt.transpose(-1, -2)
    if c.euclid:
        sim = sim - 0.5 * c.scale * kt.pow(2).sum(-1)[..., None, :]
    lse = torch.logsumexp(sim / tau, -1)
    lse_bar = 1.01 * 2.0 ** -8 * c.scale / tau * (qt.norm(dim=-1).max() * kt.norm(dim=-1).max()).item() + 1e-4
    return out, lse, lse_bar


def _dev(c, dtype):
    q, k, v = (t.to(dtype).cuda() for t in (c.q, c.k, c.v))
    tc = torch.tensor([TC], device="cuda") if c.f_dims.get("se3", 0) > 0 else None
    return q, k, v, tc


def _staged_abi(c, dtype, q, k, v, tc, tau, v_transform=True, ws=None, flags_extra=0):
    """one direct ctypes call of gta_attn_fwd_staged; returns out, lse, workspace"""
    B, H, Tq, dh = q.shape
    Nq, Nk = G2._views(c.f_dims, c.packed, q, k)
    flags = (native.FLAG_V_TRANSFORM if v_transform else 0) | (native.FLAG_EUCLID if c.euclid else 0) | flags_extra
    out = torch.empty(B, Tq, H, dh, device="cuda", dtype=dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, Tq, device="cuda", dtype=torch.float32)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, Nq, Nk, c.scale, flags)
    assert native.attn_fwd_staged_supported(desc) == 0
    need = native.attn_fwd_staged_workspace_bytes(desc)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, device="cuda", dtype=torch.uint8)
    ta = torch.tensor([tau], device="cuda") if tau != 1.0 else None
    p, pk = native._ptr, c.packed
    rc = native.lib().gta_attn_fwd_staged(ctypes.byref(desc), p(q), p(k), p(v), p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")),
                                          p(pk.get("cs_k")), p(pk.get("coord_q")), p(pk.get("coord_k")), p(tc), p(ta), p(out), p(lse),
                                          p(ws), ws.numel(), native._stream())
    assert rc == 0, native.lib().gta_strerror(rc)
    torch.cuda.synchronize()
    return out, lse, ws


def _attention(c, q, k, v, tc, tau, v_transform=True, kv_cache=None):
    ta = torch.tensor([tau], device="cuda") if tau != 1.0 else None
    return gta_amd.gta_attention(q, k, v, c.f_dims, c.packed, so3_degree=c.so3, trans_coeff=tc, tau=ta, scale=c.scale,
                                 v_transform=v_transform, euclid=c.euclid, kv_cache=kv_cache)


@pytest.mark.parametrize("tau", [1.0, 1.7])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("side", ["enc", "dec"])
@pytest.mark.parametrize("run", STAGED_RUNS)
def test_staged_forward_vs_oracle(run, side, dtype, tau):
    """out and LSE of the staged route against the fp64 oracle; today's route (`_GenericAttn`, forced by a requires_grad q) on the same
    inputs is printed beside it and held to the same output bar."""
    c = _case(run, side, dtype)
    ref, ref_lse, lse_bar = _oracle(c, tau)
    q, k, v, tc = _dev(c, dtype)
    route = G2.generic_route(tuple(q.shape), k.shape[2], dtype, c.f_dims, c.so3, *G2._views(c.f_dims, c.packed, q, k), euclid=c.euclid)
    assert route == "staged"
    with torch.no_grad():
        got = _attention(c, q, k, v, tc, tau)
    _, lse, _ = _staged_abi(c, dtype, q, k, v, tc, tau)
    with torch.enable_grad():
        old = _attention(c, q.clone().requires_grad_(), k, v, tc, tau).detach()
    torch.cuda.synchronize()
    st, st_old = C.err_stats(got.float().cpu(), ref.float()), C.err_stats(old.float().cpu(), ref.float())
    lse_err = (lse.double().cpu() - ref_lse).abs().max().item()
    print(f"STAGED {run} {side} {dtype} tau={tau}: staged {st} | apply {st_old} | lse max_abs {lse_err:.3e} (bar {lse_bar:.3e})")
    assert _bar(st), (run, side, dtype, tau, st)
    assert _bar(st_old), (run, side, dtype, tau, "apply route", st_old)
    assert torch.isfinite(lse).all() and lse_err <= lse_bar, (run, side, dtype, tau, lse_err, lse_bar)


@pytest.mark.parametrize("run", ["clevrtr/gta_euclid", "msn/gta_t2"])
def test_staged_forward_without_v_transform(run):
    c = _case(run, "dec", torch.float32, seed=3)
    ref, _, _ = _oracle(c, 1.0, v_transform=False)
    q, k, v, tc = _dev(c, torch.float32)
    with torch.no_grad():
        got = _attention(c, q, k, v, tc, 1.0, v_transform=False)
    st = C.err_stats(got.float().cpu(), ref.float())
    assert _bar(st), (run, st)


def test_staged_unaligned_slabs_and_so3_degree1():
    """slabs that start off the 8-channel chunks (`triv 2 | se3 32 | t2 30`, `triv 2 | se3 30 | so2 32` are in the run configs above) and so3 of
    degree 1 (`se3 48 | so3 24 | so2 24`, L = 1), ragged query and key tiles"""
    f_dims = {"triv": 0, "se3": 48, "so3": 24, "so2": 24}
    q, k, v, ex, ak, cross = C.synth_inputs(2, 2, 2, 75, 3, 50, f_dims, 6, 1, torch.float32, seed=5)
    ref = C.oracle_forward(q.double(), k.double(), v.double(), ex, ak, cross, TC, dtype=torch.float64)
    exd = {kk: vv.cuda() for kk, vv in ex.items()}
    gta_amd.pre_compute_reps_encoder(ak, exd)
    gta_amd.pre_compute_reps_decoder(ak, exd)
    packed = gta_amd.pack_reps(exd, f_dims)
    assert G2.attention_route(tuple(q.shape), k.shape[2], torch.float32, f_dims, 1, 2, 3) is None
    assert G2.generic_route(tuple(q.shape), k.shape[2], torch.float32, f_dims, 1, 2, 3) == "staged"
    with torch.no_grad():
        got = gta_amd.gta_attention(q.cuda(), k.cuda(), v.cuda(), f_dims, packed, so3_degree=1, trans_coeff=torch.tensor([TC], device="cuda"))
    st = C.err_stats(got.float().cpu(), ref.float())
    assert _bar(st), st


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("run", ["clevrtr/gta_euclid", "msn/gta_t2"])
def test_staged_abi_direct_and_kv_ready(run, dtype):
    """gta_attn_fwd_staged through ctypes: a full call, then GTA_FLAG_KV_READY on its workspace with k and v overwritten -- the same bits
    (the pre-pass did not run), and against the oracle; a short or missing workspace and a missing table are GTA_E_BADARG."""
    c = _case(run, "dec", dtype, seed=1)
    ref, _, _ = _oracle(c, 1.0)
    q, k, v, tc = _dev(c, dtype)
    out, lse, ws = _staged_abi(c, dtype, q, k, v, tc, 1.0)
    assert _bar(C.err_stats(out.float().cpu(), ref.float()))
    junk = torch.full_like(k, 3.0)
    out2, lse2, _ = _staged_abi(c, dtype, q, junk, junk, tc, 1.0, ws=ws, flags_extra=native.FLAG_KV_READY)
    assert torch.equal(out, out2) and torch.equal(lse, lse2)
    # argument checks
    B, H, Tq, dh = q.shape
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, *G2._views(c.f_dims, c.packed, q, k), c.scale,
                            native.FLAG_V_TRANSFORM | (native.FLAG_EUCLID if c.euclid else 0))
    p, pk, L = native._ptr, c.packed, native.lib()
    call = lambda ws_, n, vq: L.gta_attn_fwd_staged(ctypes.byref(desc), p(q), p(k), p(v), vq, p(pk.get("vrep_k")), p(pk.get("cs_q")),
                                                   p(pk.get("cs_k")), p(pk.get("coord_q")), p(pk.get("coord_k")), p(tc), None, p(out), p(lse),
                                                   ws_, n, native._stream())
    assert call(p(ws), ws.numel() - 1, p(pk.get("vrep_q"))) == -1
    assert call(None, 0, p(pk.get("vrep_q"))) == -1
    assert call(p(ws), ws.numel(), None) == -1
    torch.cuda.synchronize()


@pytest.mark.parametrize("run", STAGED_RUNS)
def test_kv_cache_reuses_images(run):
    """two calls with one cache dict, k and v overwritten in between: the second output is bit-identical (the pre-pass did not run) and
    the dict holds the images; another key shape with the same dict raises GtaError"""
    c = _case(run, "dec", torch.bfloat16, seed=2)
    q, k, v, tc = _dev(c, torch.bfloat16)
    cache = {}
    with torch.no_grad():
        a = _attention(c, q, k, v, tc, 1.0, kv_cache=cache).clone()
        assert cache.get("images") is not None and cache["images"].numel() > 0 and cache["plan"][0] == "staged", cache.keys()
        k.fill_(7.0)
        v.fill_(-3.0)
        b = _attention(c, q, k, v, tc, 1.0, kv_cache=cache)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        # a different key shape with the same dict
        k2 = torch.cat([k, k], 2)[:, :, :k.shape[2] * 2]
        ex2 = dict(c.packed)
        for name in ("cs_k", "coord_k"):
            if name in ex2:
                ex2[name] = torch.cat([ex2[name], ex2[name]], 1)
        with pytest.raises(native.GtaError):
            gta_amd.gta_attention(q, k2, k2, c.f_dims, ex2, so3_degree=c.so3, trans_coeff=tc, scale=c.scale, euclid=c.euclid, kv_cache=cache)


@pytest.mark.parametrize("run", ["clevrtr/gta_euclid", "msn/gta_so3_euclid", "clevrtr/gta_t2"])
def test_forward_plan_matches_gta_attention(run):
    from gta_amd import plan
    c = _case(run, "dec", torch.bfloat16, seed=4)
    q, k, v, tc = _dev(c, torch.bfloat16)
    Nq, Nk = G2._views(c.f_dims, c.packed, q, k)
    with torch.no_grad():
        ref = _attention(c, q, k, v, tc, 1.0)
    fp = plan.ForwardPlan(q, k, v, c.f_dims, so3_degree=c.so3, Nq=Nq, Nk=Nk, scale=c.scale, euclid=c.euclid)
    assert fp._staged
    pk = c.packed
    for _ in range(2):
        got = fp(q, k, v, pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"), tc, coord_q=pk.get("coord_q"), coord_k=pk.get("coord_k"))
    torch.cuda.synchronize()
    assert torch.equal(got, ref)
    got = fp(q, k, v, pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"), tc, coord_q=pk.get("coord_q"), coord_k=pk.get("coord_k"),
             flags_extra=native.FLAG_KV_READY)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


_SRT_ARGS = {
    "gta_euclid": {"f_dims": {"triv": 2, "se3": 6, "so2": 16}, "so2": 4, "max_freq_h": 1, "max_freq_w": 1, "euclid_sim": True},
    "gta_t2": {"f_dims": {"triv": 0, "se3": 12, "t2": 12}, "so2": False, "max_freq_h": 1, "max_freq_w": 1},
}


@pytest.mark.parametrize("name", sorted(_SRT_ARGS))
def test_render_image_reuses_staged_images(name, monkeypatch):
    """a tiny TransformingSRT with the gta_euclid / gta_t2 attention settings (dim_head 24): chunked full-image decode with the per-layer
    cache against the same without it, and every decoder layer's cache entry holds staged images"""
    from gta_amd import srt
    method = {"method": {"name": "gta", "args": _SRT_ARGS[name]}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 48, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 48, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
                              "attn_args": method}}
    torch.manual_seed(0)
    model = srt.TransformingSRT(cfg).cuda().eval()
    B, NV, h, w = 2, 2, 16, 20
    data = srt.synthetic_batch(B, n_in=NV, n_tgt=1, image=32, points_per_view=8, device="cuda", seed=1)
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(B, h, w, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(B, 3, generator=g).cuda()
    extras = {"input_transforms": data["input_transforms"], "input_coord": data["input_coord"], "target_transforms": data["target_transforms"][:, :1]}
    seen = []
    real = G2._staged_forward

    def spy(*a, **kw):
        cache = a[11] if len(a) > 11 else kw.get("kv_cache")
        if cache is not None and not any(cache is s for s in seen):
            seen.append(cache)
        return real(*a, **kw)
    monkeypatch.setattr(G2, "_staged_forward", spy)
    with torch.no_grad():
        z, extras = model.encoder(data["input_images"], data["input_camera_pos"], data["input_rays"], extras)
        img_c, _ = srt.render_image(model, z, cam, rays, extras, max_num_rays=96, reuse_kv=True)      # 320 rays: four chunks, the last ragged
        n_cached = len(seen)
        img_n, _ = srt.render_image(model, z, cam, rays, extras, max_num_rays=96, reuse_kv=False)
    torch.cuda.synchronize()
    assert n_cached == 2 and len(seen) == 2, (n_cached, len(seen))          # one entry per decoder layer; none without reuse_kv
    for cache in seen:
        assert cache.get("images") is not None and cache["plan"][0] == "staged"
    st = C.err_stats(img_c.cpu(), img_n.cpu())
    assert _bar(st), st


@pytest.mark.parametrize("run", ["clevrtr/gta_euclid", "msn/gta_t2"])
def test_route_under_grad_stays_generic_attn(run):
    """a layout the staged route serves without grad: under grad the call is `_GenericAttn`, and out, dq, dk, dv, d trans_coeff match the
    fp64 oracle's autograd within the bars tests/test_gpu_variants.py uses for the op_euclid (5e-2 * ref_max, rel_rms 2.5e-2) / op_t2
    (4e-2 * ref_max, rel_rms 2e-2) gradients; d trans_coeff within that file's one bar for it (the euclid fixture's)"""
    c = _case(run, "dec", torch.float32, seed=6)
    q, k, v, _ = _dev(c, torch.float32)
    assert G2.generic_route(tuple(q.shape), k.shape[2], torch.float32, c.f_dims, c.so3, *G2._views(c.f_dims, c.packed, q, k), euclid=c.euclid) == "staged"
    assert G2.generic_route(tuple(q.shape), k.shape[2], torch.float32, c.f_dims, c.so3, *G2._views(c.f_dims, c.packed, q, k), euclid=c.euclid,
                            needs_grad=True) == "apply"
    ex64 = {kk: (vv.double() if vv.is_floating_point() else vv) for kk, vv in c.ex.items()}
    reps = O.decoder_reps(c.dec, ex64, O.encoder_reps(c.enc, ex64))
    qo, ko, vo = (t.double().requires_grad_() for t in (c.q, c.k, c.v))
    tco = torch.tensor([TC], dtype=torch.float64, requires_grad=True)
    ref, _ = O.gta_attention(qo, ko, vo, c.f_dims, reps, tco, True, c.euclid, scale=c.scale)
    (ref * c.w.double()).sum().backward()
    qd, kd, vd = (t.requires_grad_() for t in (q, k, v))
    tcd = torch.tensor([TC], device="cuda", requires_grad=True)
    out = gta_amd.gta_attention(qd, kd, vd, c.f_dims, c.packed, so3_degree=c.so3, trans_coeff=tcd, scale=c.scale, euclid=c.euclid)
    assert type(out.grad_fn).__name__.startswith("_GenericAttn"), out.grad_fn
    (out.float() * c.w.cuda()).sum().backward()
    torch.cuda.synchronize()
    assert _bar(C.err_stats(out.detach().float().cpu(), ref.detach().float()))
    for nm, a, b in (("dq", qd.grad, qo.grad), ("dk", kd.grad, ko.grad), ("dv", vd.grad, vo.grad)):
        st = C.err_stats(a.float().cpu(), b.float())
        if c.euclid:          # the op_euclid bar of tests/test_gpu_variants.py
            assert st["finite"] and st["max_abs"] <= 5e-2 * st["ref_max"] + 1e-6 and st["rel_rms"] <= 2.5e-2, (nm, st)
        else:                 # its op_t2 bar
            assert st["finite"] and st["max_abs"] <= 4e-2 * st["ref_max"] and st["rel_rms"] <= 2e-2, (nm, st)
    r, g_ = float(tco.grad.item()), float(tcd.grad.item())
    assert abs(g_ - r) <= 5e-2 * max(1.0, abs(r)), (g_, r)


def test_kv_cache_refuses_another_scale_under_euclid():
    """the cached workspace of an euclid layout holds the key bias -0.5 scale |k'|^2: the same dict under another scale raises"""
    c = _case("clevrtr/gta_euclid", "dec", torch.bfloat16, seed=7)
    q, k, v, tc = _dev(c, torch.bfloat16)
    cache = {}
    with torch.no_grad():
        _attention(c, q, k, v, tc, 1.0, kv_cache=cache)
        c.scale = 0.5 * c.scale
        with pytest.raises(native.GtaError):
            _attention(c, q, k, v, tc, 1.0, kv_cache=cache)
    torch.cuda.synchronize()


def test_forward_plan_refusal_names_the_entry_that_spoke():
    """a layout neither entry serves (dh % 8 != 0): the error carries the staged entry's reason under the staged entry's name"""
    from gta_amd import plan
    f_dims = {"se3": 6, "so2": 8}
    x = torch.zeros(1, 2, 64, 16, device="cuda")[..., :14]
    with pytest.raises(native.GtaError, match=r"gta_attn_fwd_staged_supported.*dh % 8"):
        plan.ForwardPlan(x, x, x, f_dims, Nq=1, Nk=1, euclid=True)

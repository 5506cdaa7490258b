"""GPU: the backward with per-scene prefixes (`gta_attention(..., key_views=..., key_views_backward=True, query_views=...)`; `gta_attn_bwd_varlen`).

Shapes are those of tests/test_gpu_key_views.py (its cases are imported): B = 5, H = 2, 13 views x 20 tokens (Tk = 260, three 128-key blocks),
key_views = [1, 3, 4, 7, 13] -- prefixes of 20 (blocks 1 and 2 wholly padded, one tile), 60 (one ragged tile), 80 (the second tile of block 0
partial), 140 (block 1 with its first tile only, 12 keys; block 2 padded) and 260 keys (nothing padded, a ragged last block).  Decoder leg:
Tq = 150, no query_views.  Encoder leg: Tq = 260, query_views = key_views.  Layouts clevrtr/gta (dh 64) and msn/gta_so3 (dh 96), bf16 and fp32.

Bars (none new): tests/test_gpu_backward.py's REL_MAX / REL_RMS for dq, dk, dv (imported); d trans_coeff 2 % of max(1, |ref|) as its
test_golden_gradients; d tau 3 % of max(1, |ref|) as its test_tau_gradient_vs_oracle_autograd; the whole-model case the fp32 module bars of
tests/test_gpu_modules.py's `_srt_grad_check` (imported).

Whole-model case: the tiny config of tests/test_gpu_key_views.py's SRT test has a t2 slab -- a staged generic layout, whose backward under
key_views is refused -- so this file keeps that config's sizes and swaps the slabs for a fused layout (se3 16 | so2 8 at dh = 24)."""
import ctypes
import functools

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests.test_gpu_backward import REL_MAX, REL_RMS
from tests.test_gpu_key_views import B, H, NK, PK, TK, KV, _case, _key_lens, _tc
from tests.test_gpu_modules import _srt_grad_check

pytestmark = pytest.mark.gpu

LAYOUTS = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
SIDES = ["dec", "enc"]
TAU = 0.8


def _qv(side):
    return KV if side == "enc" else None


def _w(c):
    """random loss weights, one draw per (layout, leg)"""
    g = torch.Generator().manual_seed(101 + sum(map(ord, c.run)) + (c.side == "dec"))
    return torch.randn(B, H, c.Tq, c.dh, generator=g)


def _run(c, qkv=None, packed=None, w=None, backward=True, tau=True, **kw):
    """forward + backward through gta_attention; returns (dq, dk, dv, d trans_coeff or None, d tau or None)"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (qkv or c.dev))
    tc = c.tc.clone().requires_grad_() if c.tc is not None else None
    ta = torch.tensor([TAU], device="cuda", requires_grad=True) if tau else None
    w = _w(c).cuda() if w is None else w
    out = gta_amd.gta_attention(q, k, v, c.f_dims, packed or c.packed, so3_degree=c.so3, trans_coeff=tc, tau=ta, scale=c.scale,
                                key_views=KV, key_views_backward=backward, **({"query_views": _qv(c.side)} if c.side == "enc" else {}), **kw)
    out.backward(w.to(out.dtype))
    torch.cuda.synchronize()
    return q.grad, k.grad, v.grad, None if tc is None else tc.grad, None if ta is None else ta.grad


@functools.lru_cache(maxsize=None)
def _got(run, side, dtype):
    return _run(_case(run, side, dtype))


@functools.lru_cache(maxsize=None)
def _oracle_grads(run, side, dtype):
    """fp64 oracle autograd scene by scene on the key prefix (encoder leg: the query rows cut to the query prefix as well)"""
    c = _case(run, side, dtype)
    w = _w(c).to(dtype).double()
    res, dtc, dta = [], 0.0, 0.0
    for b, n in enumerate(KV):
        ex64 = {"input_transforms": c.ex["input_transforms"][b:b + 1, :n].double(), "input_coord": c.ex["input_coord"][b:b + 1, :n].double()}
        reps = O.encoder_reps(c.enc, ex64)
        rows = c.Tq
        if side == "dec":
            ex64["target_transforms"] = c.ex["target_transforms"][b:b + 1].double()
            ex64["target_coord"] = c.ex["target_coord"][b:b + 1].double()
            reps = O.decoder_reps(c.dec, ex64, reps)
        else:
            rows = n * PK
        q = c.q[b:b + 1, :, :rows].double().requires_grad_()
        k, v = (t[b:b + 1, :, :n * PK].double().requires_grad_() for t in (c.k, c.v))
        tc = torch.tensor([_tc(run)], dtype=torch.float64, requires_grad=True)
        ta = torch.tensor([TAU], dtype=torch.float64, requires_grad=True)
        out, _ = O.gta_attention(q, k, v, c.f_dims, reps, tc, True, c.euclid, scale=c.scale, tau=ta)
        (out * w[b:b + 1, :, :rows]).sum().backward()
        res.append((q.grad[0], k.grad[0], v.grad[0]))
        dtc += float(tc.grad.item()) if tc.grad is not None else 0.0
        dta += float(ta.grad.item())
    return res, dtc, dta


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_oracle_parity(run, side, dtype):
    """1. dq, dk, dv, d trans_coeff, d tau against fp64 oracle autograd per scene on the prefixes -- all five scenes"""
    c = _case(run, side, dtype)
    dq, dk, dv, dtc, dta = _got(run, side, dtype)
    ref, ref_dtc, ref_dta = _oracle_grads(run, side, dtype)
    for b, n in enumerate(KV):
        rows = c.Tq if side == "dec" else n * PK
        for name, got, r in (("dq", dq[b, :, :rows], ref[b][0]), ("dk", dk[b, :, :n * PK], ref[b][1]), ("dv", dv[b, :, :n * PK], ref[b][2])):
            st = C.err_stats(got.float().cpu(), r.float())
            print(f"KEY_VIEWS_BWD {run} {side} {dtype} scene {b} ({n} views) {name}: {st}")
            assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS, (run, side, dtype, b, name, st)
    print(f"KEY_VIEWS_BWD {run} {side} {dtype} dtc {None if dtc is None else dtc.item()} ref {ref_dtc} | dtau {dta.item()} ref {ref_dta}")
    if dtc is not None:
        assert abs(dtc.item() - ref_dtc) <= 2e-2 * max(1.0, abs(ref_dtc)), (dtc.item(), ref_dtc)
    assert abs(dta.item() - ref_dta) <= 3e-2 * max(1.0, abs(ref_dta)), (dta.item(), ref_dta)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_padded_outputs_are_exactly_zero(run, side, dtype):
    """2. dk / dv rows at or past the prefix, and (encoder leg) dq rows at or past the query prefix: exactly zero"""
    dq, dk, dv, _, _ = _got(run, side, dtype)
    for b, n in enumerate(KV):
        assert torch.count_nonzero(dk[b, :, n * PK:]) == 0 and torch.count_nonzero(dv[b, :, n * PK:]) == 0, (run, side, dtype, b)
        if side == "enc":
            assert torch.count_nonzero(dq[b, :, n * PK:]) == 0, (run, side, dtype, b)
        assert torch.isfinite(dq[b]).all() and torch.isfinite(dk[b]).all() and torch.isfinite(dv[b]).all()


def _poisoned(c, value):
    """inputs, tables and loss weights with everything that belongs to a padded view filled with `value`"""
    q, k, v = (t.clone() for t in c.dev)
    w = _w(c).cuda()
    pk = {name: t.clone() for name, t in c.packed.items()}
    for b, n in enumerate(KV):
        k[b, :, n * PK:] = value
        v[b, :, n * PK:] = value
        pk["vrep_k"][b, n:] = value
        if "cs_k" in pk:
            pk["cs_k"][b, n * PK:] = value
        if c.side == "enc":
            q[b, :, n * PK:] = value
            w[b, :, n * PK:] = value
            if "cs_q" in pk:
                pk["cs_q"][b, n * PK:] = value
    return (q, k, v), pk, w


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_padding_is_never_read(run, side, dtype):
    """3. NaN in k, v, cs_k, vrep_k of the padded views (encoder leg: q, dout, cs_q rows of padded views too): every gradient, d trans_coeff
    and d tau bit-identical to the run with finite padding"""
    c = _case(run, side, dtype)
    qkv0, pk0, w0 = _poisoned(c, 0.5)
    ref = _run(c, qkv0, pk0, w0)
    qkv, pk, w = _poisoned(c, float("nan"))
    assert not torch.isfinite(qkv[1]).all() and not torch.isfinite(pk["vrep_k"]).all()
    got = _run(c, qkv, pk, w)
    for name, a, r in zip(("dq", "dk", "dv", "dtc", "dtau"), got, ref):
        if r is None:
            assert a is None
            continue
        if side == "enc" and name == "dq":            # (the NaN-filled leaf rows themselves get zero gradient)
            assert torch.isfinite(a).all()
        assert torch.isfinite(a).all() and torch.equal(a, r), (run, side, dtype, name)


def _cut_scene(c, b, n, rows):
    pk = {}
    for name, t in c.packed.items():
        cut = {"vrep_k": n, "cs_k": n * PK, "vrep_q": None if c.side == "dec" else n, "cs_q": None if c.side == "dec" else n * PK}.get(name)
        pk[name] = t[b:b + 1] if cut is None else t[b:b + 1, :cut].contiguous()
    q, k, v = c.dev
    return (q[b:b + 1, :, :rows], k[b:b + 1, :, :n * PK], v[b:b + 1, :, :n * PK]), pk


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_bits_of_the_scene_alone(run, side, dtype):
    """4. against gta_attn_bwd on the scene alone with its keys (encoder leg: and queries) cut, on the same kernels (forward kv_mode
    'prepass_fwd2', backward GTA_FLAG_BWD_KEYS32): dq, dk, dv bit-identical; d trans_coeff and d tau within 1e-5 relative (the partial sums
    are grouped differently)"""
    c = _case(run, side, dtype)
    dq, dk, dv, dtc, dta = _got(run, side, dtype)
    w = _w(c).cuda()
    sum_dtc, sum_dta = 0.0, 0.0
    flags = native.FLAG_V_TRANSFORM | native.FLAG_ROWS32 | native.FLAG_FWD2_GENERIC | native.FLAG_BWD_KEYS32
    for b, n in enumerate(KV):
        rows = c.Tq if side == "dec" else n * PK
        (q, k, v), pk = _cut_scene(c, b, n, rows)
        q, k, v = (t.detach().clone().requires_grad_() for t in (q, k, v))
        tc = c.tc.clone().requires_grad_() if c.tc is not None else None
        ta = torch.tensor([TAU], device="cuda", requires_grad=True)
        cfg = ({k_: int(v_) for k_, v_ in c.f_dims.items()}, int(c.so3), 1 if side == "dec" else n, n, float(c.scale), flags)
        out = G2._FusedAttn.apply(q, k, v, tc, ta, (cfg, None, G2._Mask()), pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"))
        out.backward(w[b:b + 1, :, :rows].to(out.dtype))
        torch.cuda.synchronize()
        assert torch.equal(q.grad[0], dq[b, :, :rows]), (run, side, dtype, b, "dq")
        assert torch.equal(k.grad[0], dk[b, :, :n * PK]), (run, side, dtype, b, "dk")
        assert torch.equal(v.grad[0], dv[b, :, :n * PK]), (run, side, dtype, b, "dv")
        sum_dtc += float(tc.grad.item()) if tc is not None else 0.0
        sum_dta += float(ta.grad.item())
    print(f"KEY_VIEWS_BWD alone {run} {side} {dtype}: dtc {None if dtc is None else dtc.item()} vs {sum_dtc} | dtau {dta.item()} vs {sum_dta}")
    if dtc is not None:
        assert abs(dtc.item() - sum_dtc) <= 1e-5 * max(1.0, abs(sum_dtc)), (dtc.item(), sum_dtc)
    assert abs(dta.item() - sum_dta) <= 1e-5 * max(1.0, abs(sum_dta)), (dta.item(), sum_dta)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_direct_ctypes_call(run, dtype):
    """5. gta_attn_bwd_varlen through ctypes (encoder leg, q_lens given): kv_images = NULL and the forward's workspace give the same bits; the
    _supported query refuses the three flags with a reason"""
    c = _case(run, "enc", dtype)
    q, k, v = c.dev
    pk, p, L = c.packed, native._ptr, native.lib()
    kl = _key_lens()
    flags = native.FLAG_V_TRANSFORM
    out = torch.empty(B, c.Tq, H, c.dh, device="cuda", dtype=dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, c.Tq, device="cuda", dtype=torch.float32)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, NK, c.scale, flags)
    assert native.attn_bwd_varlen_supported(desc) == 0
    for flag, word in ((native.FLAG_FUSED_KV, "FUSED_KV"), (native.FLAG_FP32_PRODUCTS, "FP32_PRODUCTS"), (native.FLAG_PRETRANSFORMED, "PRETRANSFORMED")):
        bad = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, NK, c.scale, flags | flag)
        rc = native.attn_bwd_varlen_supported(bad)
        assert rc == -3 and word in L.gta_strerror(rc).decode(), (flag, L.gta_strerror(rc))
    ws_f = torch.empty(native.attn_fwd_workspace_bytes(desc), device="cuda", dtype=torch.uint8)
    native.attn_fwd_varlen(desc, q, k, v, pk.get("vrep_q"), pk.get("vrep_k"), pk.get("cs_q"), pk.get("cs_k"), c.tc, None, kl, out, lse, ws_f)
    dout = _w(c).to(dtype).cuda()
    res = []
    for images in (None, ws_f):
        dq, dk, dv = (torch.empty(B, T, H, c.dh, device="cuda", dtype=dtype).permute(0, 2, 1, 3) for T in (c.Tq, TK, TK))
        dtc = torch.empty(1, device="cuda")
        ws = torch.empty(native.attn_bwd_workspace_bytes(desc), device="cuda", dtype=torch.uint8)
        gs = (ctypes.c_int64 * 9)(*(list(dq.stride()[:3]) + list(dk.stride()[:3]) + list(dv.stride()[:3])))
        ds = (ctypes.c_int64 * 3)(*dout.stride()[:3])
        rc = L.gta_attn_bwd_varlen(ctypes.byref(desc), p(q), p(k), p(v), p(out), p(dout), p(lse), p(pk.get("vrep_q")), p(pk.get("vrep_k")),
                                   p(pk.get("cs_q")), p(pk.get("cs_k")), p(c.tc), None, p(kl), p(kl), p(images), p(dq), p(dk), p(dv), gs, ds,
                                   p(dtc) if c.tc is not None else None, None, p(ws), ws.numel(), native._stream())
        assert rc == 0, L.gta_strerror(rc)
        torch.cuda.synchronize()
        res.append((dq, dk, dv, dtc))
    for a, r in zip(*res):
        assert torch.equal(a, r)
    got = _run(c, tau=False)
    assert all(torch.equal(a, r) for a, r in zip(res[0][:3], got[:3]))          # gta_attention took this entry
    # NULL key_lens: GTA_E_BADARG before any launch
    x = ctypes.c_void_p(256)
    assert L.gta_attn_bwd_varlen(ctypes.byref(desc), x, x, x, x, x, x, x, x, x, x, None, None, None, None, None, x, x, x, gs, ds, None, None, x, 1 << 40, None) == -1


def test_whole_model_step_with_mixed_input_views():
    """6. one TransformingSRT step (fp32) with input_views = [2, 3] and input_views_backward=True: parameter gradients against the same
    model run scene by scene on its valid views, at the fp32 module bars of tests/test_gpu_modules.py (`_srt_grad_check`)"""
    from gta_amd import srt
    method = {"method": {"name": "gta", "args": {"f_dims": {"triv": 0, "se3": 16, "so2": 8}, "so2": 2, "max_freq_h": 1, "max_freq_w": 1}}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 48, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 48, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
                              "attn_args": method}}
    torch.manual_seed(0)
    model = srt.TransformingSRT(cfg).cuda().eval()
    nb, NV, views, npix = 2, 3, [2, 3], 40
    data = srt.synthetic_batch(nb, n_in=NV, n_tgt=1, image=32, points_per_view=8, device="cuda", seed=1)
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, 1, npix, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 1, 1, 3, generator=g).cuda().expand(-1, 1, npix, -1)
    coord = torch.from_numpy(G2.make_2dcoord(16, 20)).cuda().flatten(0, 1)[:npix]
    w = torch.randn(nb, npix, 3, generator=g).cuda()

    def step(sl, n, input_views):
        nb_ = data["input_images"][sl].shape[0]
        extras = {"input_transforms": data["input_transforms"][sl, :n], "input_coord": data["input_coord"][sl, :n],
                  "target_transforms": data["target_transforms"][sl, :1], "target_coord": coord[None, None].expand(nb_, 1, -1, -1)}
        pix, _ = model(data["input_images"][sl, :n], data["input_camera_pos"][sl, :n], data["input_rays"][sl, :n], cam[sl], rays[sl], extras,
                       input_views=input_views, input_views_backward=input_views is not None)
        (pix.reshape(nb_, npix, 3).float() * w[sl]).sum().backward()

    model.zero_grad(set_to_none=True)
    for b, n in enumerate(views):
        step(slice(b, b + 1), n, None)
    torch.cuda.synchronize()
    ref = {"grad." + name: prm.grad.detach().cpu().numpy().copy() for name, prm in model.named_parameters()}
    model.zero_grad(set_to_none=True)
    step(slice(0, nb), NV, views)
    torch.cuda.synchronize()
    worst = _srt_grad_check(model, ref, False)
    print(f"KEY_VIEWS_BWD srt: worst relative rms {worst:.3e}")


def test_default_keyword_under_grad_is_still_forward_only():
    """7. without key_views_backward a call under grad raises as before"""
    c = _case("clevrtr/gta", "dec", torch.bfloat16)
    with pytest.raises(native.GtaError, match="forward-only"):
        _run(c, backward=False)

"""GPU: the query-side mask of masked attention (`gta_attention(..., query_mask=m)`; `gta_attn_fwd_qmask` / `gta_attn_bwd_qmask`: the QMASK
instances of the VARLEN `gta_fwd2_kernel`, of the backward's q-side pre-pass and of its dQ walk, the GATHER dK/dV walk under q_lens).

Shapes are those of tests/test_gpu_key_mask.py (its cases are imported): B = 4, H = 2, 5 views x 52 keys (Tk = 260).  Self leg: Tq = 260 -- three
128-row work items, the last one with 4 rows.  Decoder leg: Tq = 150.  Layouts clevrtr/gta (dh 64) and msn/gta_so3 (dh 96), fp32 and bf16.  The
smallest shapes with a dead item, a one-row item, a ragged last item and a hole inside a live item.

Query-mask sets, one mask per scene (the decoder leg takes the first 150 columns):
  qblocks  all rows | row 137 alone (self leg: items 0 and 2 dead; decoder leg: item 0 dead) | the even rows | rows 0..127 (exactly one whole item
           and nothing behind it; on the self leg views 3 and 4 have no live row)
  same     (self leg only) the key mask of the call -- `blocks` and `random` of tests/test_gpu_key_mask_bwd.py: the padded self-attention batch
  empty    qblocks with no live row in scene 1

Bars (none new): out and lse as tests/test_gpu_key_mask.py (REL_MAX / REL_RMS of tests/test_gpu_forward.py, lse 2e-2 absolute); dq, dk, dv
REL_MAX / REL_RMS of tests/test_gpu_backward.py against the fp64 `_oracle_scene` of tests/test_gpu_key_mask_bwd.py with the dead query rows
left out of the loss (and its derived rounding bound where the exact gradient is zero: one key).  d trans_coeff and d tau have no bar of their
own: they are tied bit for bit to a key_mask-only run on zeroed rows (rule 4), which the existing tests hold to the oracle."""
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
from tests.test_gpu_forward import REL_MAX as F_REL_MAX, REL_RMS as F_REL_RMS
from tests.test_gpu_key_mask import B, H, NK, PK, TC, TK, TQ_DEC, _case, _tensors
from tests.test_gpu_key_mask_bwd import TAU, _bits, _filled, _mask_set, _oracle_scene, _w
from tests.test_gpu_modules import _srt_grad_check

pytestmark = pytest.mark.gpu

LAYOUTS = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
# (leg, key-mask set, query-mask set)
COMBOS = [("dec", "blocks", "qblocks"), ("enc", "blocks", "qblocks"), ("enc", "blocks", "same"), ("enc", "random", "same"),
          ("dec", "random", "empty"), ("enc", "random", "empty")]
NAN = float("nan")
FILLS = [0.0, 0.5, NAN, float("inf")]


@functools.lru_cache(maxsize=None)
def _qmask(name, side, kset):
    """bool [B, Tq] on the CPU"""
    if name == "same":
        assert side == "enc"
        return _mask_set(kset)
    m = torch.zeros(B, TK, dtype=torch.bool)
    m[0] = True
    m[1, 137] = name != "empty"
    m[2] = torch.arange(TK) % 2 == 0
    m[3, :128] = True
    return m[:, :TQ_DEC].clone() if side == "dec" else m


def test_mask_counts():
    assert _qmask("qblocks", "enc", None).sum(1).tolist() == [260, 1, 130, 128]
    assert _qmask("qblocks", "dec", None).sum(1).tolist() == [150, 1, 75, 128]
    assert _qmask("empty", "enc", None).sum(1).tolist() == [260, 0, 130, 128] and _qmask("empty", "dec", None).sum(1).tolist() == [150, 0, 75, 128]
    for side, T in (("enc", TK), ("dec", TQ_DEC)):
        m = _qmask("qblocks", side, None)
        items = [[bool(m[b, i:i + 128].any()) for i in range(0, T, 128)] for b in range(B)]
        assert items[1] == ([False, True, False] if side == "enc" else [False, True]), items      # the dead items
        assert all(items[0]) and all(items[2]) and items[3] == [True] + [False] * (len(items[3]) - 1)
    v = _qmask("qblocks", "enc", None).view(B, NK, PK).any(-1)
    assert v[3].tolist() == [True, True, True, False, False]                       # views without a live row
    assert _qmask("same", "enc", "blocks") is _mask_set("blocks")
    assert TK == 260 and TK % 128 == 4


def _poison(c, kset, qm, fill, same):
    """device copies of q, k, v and the tables with `fill` wherever the contract says nothing is read: dead rows of q and cs_q, the vrep_q record
    of a view without a live row, and -- in the `same` set -- the masked rows of k, v and cs_k"""
    q, k, v = (t.clone() for t in c.dev)
    pk = {n: t.clone() for n, t in c.packed.items()}
    dead = (~qm).cuda()
    q.permute(0, 2, 1, 3)[dead] = fill
    if "cs_q" in pk:
        pk["cs_q"][dead] = fill
    if "vrep_q" in pk:
        pk["vrep_q"][(~qm.view(B, c.Nq, -1).any(-1)).cuda()] = fill
    if same:
        kdead = (~_mask_set(kset)).cuda()
        k.permute(0, 2, 1, 3)[kdead] = fill
        v.permute(0, 2, 1, 3)[kdead] = fill
        if "cs_k" in pk:
            pk["cs_k"][kdead] = fill
    return (q, k, v), pk


def _step(c, qkv, pk, w, **kw):
    """out, lse (a call under no_grad with return_lse) and the five gradients (a call under grad) through gta_attention"""
    with torch.no_grad():
        out, lse = gta_amd.gta_attention(*qkv, c.f_dims, pk, so3_degree=c.so3, trans_coeff=c.tc, tau=torch.tensor([TAU], device="cuda"),
                                         scale=c.scale, return_lse=True, **kw)
    q, k, v = (t.detach().clone().requires_grad_() for t in qkv)
    tc = c.tc.clone().requires_grad_()
    ta = torch.tensor([TAU], device="cuda", requires_grad=True)
    o2 = gta_amd.gta_attention(q, k, v, c.f_dims, pk, so3_degree=c.so3, trans_coeff=tc, tau=ta, scale=c.scale, key_mask_backward=True, **kw)
    o2.backward(w.to(o2.dtype))
    torch.cuda.synchronize()
    assert torch.equal(_bits(o2.detach()), _bits(out))
    return dict(out=out, lse=lse, dq=q.grad, dk=k.grad, dv=v.grad, dtc=tc.grad, dta=ta.grad)


@functools.lru_cache(maxsize=None)
def _got(run, side, dtype, kset, qset, fill):
    """the query_mask run with `fill` in everything a dead row owns, dout included"""
    c = _case(run, side, dtype)
    qm = _qmask(qset, side, kset)
    qkv, pk = _poison(c, kset, qm, fill, qset == "same")
    w = _w(c).cuda()
    w.permute(0, 2, 1, 3)[(~qm).cuda()] = fill
    return _step(c, qkv, pk, w, key_mask=_mask_set(kset).cuda(), query_mask=qm.cuda())


@functools.lru_cache(maxsize=None)
def _oracle(run, side, dtype, kset, qset):
    """fp64 per scene on the valid key columns, the dead query rows left out of the loss: (out, lse, dq, dk, dv, one-key bounds or None)"""
    c = _case(run, side, dtype)
    qm = _qmask(qset, side, kset)
    w = _w(c).to(dtype).double() * qm[:, None, :, None]
    res = []
    for b in range(B):
        ex64 = {"input_transforms": c.ex["input_transforms"][b:b + 1].double(), "input_coord": c.ex["input_coord"][b:b + 1].double()}
        reps = O.encoder_reps(c.enc, ex64)
        if side == "dec":
            ex64["target_transforms"] = c.ex["target_transforms"][b:b + 1].double()
            ex64["target_coord"] = c.ex["target_coord"][b:b + 1].double()
            reps = O.decoder_reps(c.dec, ex64, reps)
        cols = _mask_set(kset)[b].nonzero().flatten()
        dq, dk, dv, _, _, zero, _ = _oracle_scene(c.q[b:b + 1], c.k[b:b + 1], c.v[b:b + 1], c.f_dims, reps, cols, w[b:b + 1], c.scale)
        with torch.no_grad():
            ta = torch.tensor([TAU], dtype=torch.float64)
            qt, kt, vt = O.transform_qkv(c.q[b:b + 1].double(), c.k[b:b + 1].double(), c.v[b:b + 1].double(), c.f_dims, reps, TC, True, False)
            o, _ = O.softmax_attention(qt, kt[:, :, cols], vt[:, :, cols], c.scale, ta)
            out = O.inverse_transform_out(o, c.f_dims, reps, TC, False)[0]
            lse = torch.logsumexp(c.scale / TAU * qt @ kt[:, :, cols].transpose(-1, -2), -1)[0]
        res.append((out, lse, dq, dk, dv, zero))
    return res


def _params(f):
    for name, vals in (("dtype", DTYPES), ("combo", COMBOS), ("run", LAYOUTS)):
        f = pytest.mark.parametrize(name, vals, ids=[str(v).replace("torch.", "") if name != "combo" else "-".join(v) for v in vals])(f)
    return f


# ---- 1. oracle parity on live rows ---------------------------------------------------------------------------------------------------------
@_params
def test_oracle_parity_on_live_rows(run, combo, dtype):
    side, kset, qset = combo
    qm, km = _qmask(qset, side, kset), _mask_set(kset)
    got = _got(run, side, dtype, kset, qset, NAN)
    for b, (out, lse, dq, dk, dv, zero) in enumerate(_oracle(run, side, dtype, kset, qset)):
        rows, cols = qm[b].nonzero().flatten(), km[b].nonzero().flatten()
        if rows.numel() == 0:
            continue                                            # (the scene without a live row: rule 5)
        st = C.err_stats(got["out"][b][:, rows.cuda()].float().cpu(), out[:, rows].float())
        lse_err = (got["lse"][b][:, rows.cuda()].double().cpu() - lse[:, rows]).abs().max().item()
        print(f"QUERY_MASK {run} {combo} {dtype} scene {b} ({rows.numel()} rows, {cols.numel()} keys) out: {st} | lse max_abs {lse_err:.3e}")
        assert st["finite"] and st["max_abs"] <= F_REL_MAX * st["ref_max"] and st["rel_rms"] <= F_REL_RMS, (run, combo, dtype, b, st)
        assert lse_err < 2e-2, (run, combo, dtype, b, lse_err)
        for name, g, r in (("dq", got["dq"][b][:, rows.cuda()], dq[:, rows]), ("dk", got["dk"][b][:, cols.cuda()], dk[:, cols]),
                           ("dv", got["dv"][b][:, cols.cuda()], dv[:, cols])):
            st = C.err_stats(g.float().cpu(), r.float())
            print(f"QUERY_MASK {run} {combo} {dtype} scene {b} {name}: {st} {zero or ''}")
            if st["ref_max"] == 0.0:                            # (one valid key: the exact dq and dk are zero -- the derived rounding bound)
                assert cols.numel() == 1 and name in ("dq", "dk") and st["finite"] and st["max_abs"] <= zero[name], (run, combo, dtype, b, name, st)
                continue
            assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS, (run, combo, dtype, b, name, st)


# ---- 2. exact zeros (the C entries, every output buffer starting at 0xFF) -----------------------------------------------------------------------
@_params
def test_dead_rows_are_zero_bits_through_the_c_entries(run, combo, dtype):
    side, kset, qset = combo
    c = _case(run, side, dtype)
    qm = _qmask(qset, side, kset)
    key_idx, key_lens = _tensors(_mask_set(kset))
    q_live, q_lens = G2.query_mask_tensors(qm, key_idx.device)
    assert q_lens.tolist() == [int(r.nonzero().max()) + 1 if r.any() else 0 for r in qm]
    qkv, pk = _poison(c, kset, qm, NAN, qset == "same")
    q, k, v = qkv
    dout = _w(c).to(dtype).cuda()
    dout.permute(0, 2, 1, 3)[(~qm).cuda()] = NAN
    p, L = native._ptr, native.lib()
    out = _filled((B, H, c.Tq, c.dh), dtype)
    lse = torch.full((4 * B * H * c.Tq,), 0xFF, device="cuda", dtype=torch.uint8).view(torch.float32).view(B, H, c.Tq)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, NK, c.scale, native.FLAG_V_TRANSFORM)
    assert native.attn_fwd_qmask_supported(desc) == 0 and native.attn_bwd_qmask_supported(desc) == 0
    ta = torch.tensor([TAU], device="cuda")
    tables = (p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")), p(pk.get("cs_k")), p(c.tc), p(ta))
    ws_f = torch.full((native.attn_fwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    rc = L.gta_attn_fwd_qmask(ctypes.byref(desc), p(q), p(k), p(v), *tables, p(key_idx), p(key_lens), p(q_live), p(out), p(lse), p(ws_f), ws_f.numel(),
                              native._stream())
    assert rc == 0, L.gta_strerror(rc)
    dq, dk, dv = (_filled((B, H, T, c.dh), dtype) for T in (c.Tq, TK, TK))
    dtc, dta = torch.full((1,), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    ws = torch.full((native.attn_bwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    gs = (ctypes.c_int64 * 9)(*(list(dq.stride()[:3]) + list(dk.stride()[:3]) + list(dv.stride()[:3])))
    ds = (ctypes.c_int64 * 3)(*dout.stride()[:3])
    rc = L.gta_attn_bwd_qmask(ctypes.byref(desc), p(q), p(k), p(v), p(out), p(dout), p(lse), *tables, p(key_idx), p(key_lens), p(q_live), p(q_lens),
                              p(ws_f), p(dq), p(dk), p(dv), gs, ds, p(dtc), p(dta), p(ws), ws.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    dead = (~qm).cuda()
    for name, t in (("out", out), ("dq", dq)):
        assert torch.isfinite(t).all(), name                        # (every row was written)
        assert torch.count_nonzero(_bits(t.permute(0, 2, 1, 3)[dead])) == 0, name
    assert torch.isfinite(lse).all() and torch.count_nonzero(lse.permute(0, 2, 1)[dead].contiguous().view(torch.int32)) == 0
    got = _got(run, side, dtype, kset, qset, NAN)                   # gta_attention gives the same bits, the dead rows included
    for name, t in (("out", out), ("lse", lse), ("dq", dq), ("dk", dk), ("dv", dv), ("dtc", dtc), ("dta", dta)):
        assert torch.isfinite(t).all() and torch.equal(_bits(t), _bits(got[name])), name
    # q_lens = NULL is Tq: the dK/dV walk then visits every query tile, the dead ones adding exact zeros
    dq2, dk2, dv2 = (_filled((B, H, T, c.dh), dtype) for T in (c.Tq, TK, TK))
    rc = L.gta_attn_bwd_qmask(ctypes.byref(desc), p(q), p(k), p(v), p(out), p(dout), p(lse), *tables, p(key_idx), p(key_lens), p(q_live), None,
                              p(ws_f), p(dq2), p(dk2), p(dv2), gs, ds, p(dtc), p(dta), p(ws), ws.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    for a, b_ in ((dq, dq2), (dk, dk2), (dv, dv2)):
        assert torch.equal(_bits(a), _bits(b_))


# ---- 3. never used ---------------------------------------------------------------------------------------------------------------------------
@_params
def test_what_a_dead_row_holds_is_never_used(run, combo, dtype):
    """0.0, 0.5, NaN and Inf in q, cs_q, the vrep_q records of views without a live row and dout at dead rows (`same`: in the masked k, v and cs_k
    rows too): every output is finite and bit for bit the same across the fills"""
    side, kset, qset = combo
    runs = [_got(run, side, dtype, kset, qset, f) for f in FILLS]
    for name in ("out", "lse", "dq", "dk", "dv", "dtc", "dta"):
        for f, r in zip(FILLS, runs):
            assert torch.isfinite(r[name]).all(), (name, f)
            assert torch.equal(_bits(r[name]), _bits(runs[0][name])), (name, f)


# ---- 4. zero-row equivalence, 5. the empty scene ------------------------------------------------------------------------------------------------
@_params
def test_equals_key_mask_alone_on_zeroed_rows(run, combo, dtype):
    """key_mask alone on the same data with the dead rows of q and of dout set to zero: out, lse and dq at live rows, dk, dv, d trans_coeff and
    d tau in full are the bits of the query_mask run.  The scene without a live row (`empty`): out, dq, dk and dv all zero."""
    side, kset, qset = combo
    c = _case(run, side, dtype)
    qm = _qmask(qset, side, kset)
    dead, live = (~qm).cuda(), qm.cuda()
    q = c.dev[0].clone()
    q.permute(0, 2, 1, 3)[dead] = 0.0
    w = _w(c).cuda()
    w.permute(0, 2, 1, 3)[dead] = 0.0
    ref = _step(c, (q, c.dev[1], c.dev[2]), c.packed, w, key_mask=_mask_set(kset).cuda())
    got = _got(run, side, dtype, kset, qset, NAN)
    for name in ("out", "dq"):
        assert torch.equal(_bits(got[name].permute(0, 2, 1, 3)[live]), _bits(ref[name].permute(0, 2, 1, 3)[live])), name
    assert torch.equal(got["lse"].permute(0, 2, 1)[live], ref["lse"].permute(0, 2, 1)[live])
    for name in ("dk", "dv", "dtc", "dta"):
        assert torch.equal(_bits(got[name]), _bits(ref[name])), (name, got[name].flatten()[:4], ref[name].flatten()[:4])
    for b in range(B):
        if not qm[b].any():
            for name in ("out", "dq", "dk", "dv"):
                assert torch.count_nonzero(got[name][b]) == 0, (b, name)
            assert torch.count_nonzero(got["lse"][b]) == 0
    assert (qset == "empty") == (not bool(qm.any(1).all()))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float32", "bfloat16"])
@pytest.mark.parametrize("run", LAYOUTS)
def test_without_a_key_mask_it_runs_under_an_all_true_one(run, dtype):
    c = _case(run, "dec", dtype)
    qm = _qmask("qblocks", "dec", None)
    w = _w(c).cuda()
    a = _step(c, c.dev, c.packed, w, query_mask=qm.cuda())
    b_ = _step(c, c.dev, c.packed, w, query_mask=qm.cuda(), key_mask=torch.ones(B, TK, dtype=torch.bool, device="cuda"))
    for name in a:
        assert torch.isfinite(a[name]).all() and torch.equal(_bits(a[name]), _bits(b_[name])), name
    with torch.no_grad():                                        # a CPU mask is uploaded
        o = gta_amd.gta_attention(*c.dev, c.f_dims, c.packed, so3_degree=c.so3, trans_coeff=c.tc, tau=torch.tensor([TAU], device="cuda"),
                                  scale=c.scale, query_mask=qm)
    assert torch.equal(_bits(o), _bits(a["out"]))


# ---- 6. whole model ------------------------------------------------------------------------------------------------------------------------------
def test_whole_model_step_with_nan_padding():
    """the whole-model case of tests/test_gpu_key_mask_bwd.py (fp32; se3 16 | so2 8 at dh = 24; a mask of leading views) with the padded inputs
    NaN instead of zero and input_mask_queries=True: held to the fp32 module bars of `_srt_grad_check` against the run under input_views on
    zero-filled padding.  (The same call without input_mask_queries is not asserted on.)  NaN goes into the images, camera positions and rays
    of the padded views; extras['input_transforms'] and ['input_coord'] stay finite, so the view records and (cos, sin) rows of masked views
    are finite here -- "the record of a view without a live row may hold anything" is exercised by the operator tests above (rule 3)."""
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
    P = data["input_coord"].shape[2]
    mask = torch.zeros(nb, NV, P, dtype=torch.bool, device="cuda")
    names = ("input_images", "input_camera_pos", "input_rays")
    nan_data = {n: data[n].clone() for n in names}
    for b, n in enumerate(views):
        mask[b, :n] = True
        for name in names:
            data[name][b, n:] = 0.0
            nan_data[name][b, n:] = NAN
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, 1, npix, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 1, 1, 3, generator=g).cuda().expand(-1, 1, npix, -1)
    coord = torch.from_numpy(G2.make_2dcoord(16, 20)).cuda().flatten(0, 1)[:npix]
    w = torch.randn(nb, npix, 3, generator=g).cuda()

    def step(d, **how):
        extras = {"input_transforms": data["input_transforms"], "input_coord": data["input_coord"],
                  "target_transforms": data["target_transforms"][:, :1], "target_coord": coord[None, None].expand(nb, 1, -1, -1)}
        model.zero_grad(set_to_none=True)
        pix, _ = model(d["input_images"], d["input_camera_pos"], d["input_rays"], cam, rays, extras, **how)
        loss = (pix.reshape(nb, npix, 3).float() * w).sum()
        loss.backward()
        torch.cuda.synchronize()
        return pix.detach().clone(), loss.item()

    pix_v, loss_v = step(data, input_views=views, input_views_backward=True)
    ref = {"grad." + name: prm.grad.detach().cpu().numpy().copy() for name, prm in model.named_parameters()}
    pix_m, loss_m = step(nan_data, input_mask=mask, input_mask_backward=True, input_mask_queries=True)
    print(f"QUERY_MASK srt: loss {loss_m} vs {loss_v}, max pixel difference {(pix_m - pix_v).abs().max().item():.3e}")
    assert torch.isfinite(pix_m).all()
    worst = _srt_grad_check(model, ref, False)
    print(f"QUERY_MASK srt: worst relative rms {worst:.3e}")

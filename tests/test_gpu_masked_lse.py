"""GPU: the gradient of the pair (out, lse) under key_views, key_mask and query_mask (`masked_lse_backward=True`; `gta_attn_bwd_varlen_dlse`,
`gta_attn_bwd_gather_dlse`, `gta_attn_bwd_qmask_dlse`: the DLSE twins of the masked q-side pre-pass, every walk as it was).

Shapes are those of tests/test_gpu_key_views.py (imported): B = 5, H = 2, 13 views x 20 tokens (Tk = 260), `clevrtr/gta` (dh 64) and `msn/gta_so3`
(dh 96), fp32 and bf16.  Decoder leg: Tq = 150 (64-row tiles 64 | 64 | 22, 128-row items 128 | 22).  Self-attention leg: Tq = 260.
  key_views   [1, 3, 4, 7, 13] with query_views the same on the self-attention leg: q_lens = 20, 60 (inside tile 0; tiles 1 .. 4 wholly past the
              prefix), 80, 140 (inside tiles 1 and 2), 260
  key_mask    `KM`: every key | Bernoulli 0.5 | every third token masked | views 0, 4, 9 whole plus 7 tokens of view 5 | Bernoulli 0.15 -- at
              least one live key in each of the token slices [0, 80), [80, 100), [100, 260) of test 4
  query_mask  `QM` on the decoder leg: every row | NO live row | Bernoulli 0.6 (both 128-row items live with dead rows inside) | rows 0 .. 39
              (q_lens = 40 inside tile 0, tiles 1 and 2 wholly dead) | every third row dead up to row 98, nothing behind (q_lens = 98: inside
              tile 1, the ragged tile wholly dead)
Test 5 has the 20 views of 8 tokens of tests/test_gpu_lse_merge.py's `_case20`; test 6 the `cl-dec` shape of tests/test_gpu_key_views_rep_grad.py,
once through `gta_attention` under a key mask and once through `gta_attention_by_view_groups` under a query mask.

Bars (none new).  The pre-pass: bit equality, and tests/_bwd_images.py's bar of the D half against fp64, (dhp / 4 + 4) 2^-24 sum |dout out| +
2^-24 |dlse|.  Gradients against fp64 autograd through the oracle, scene by scene over the live keys and live rows (formed as
tests/test_gpu_key_mask_bwd.py's `_oracle_scene`, with sum(u lse) in the loss): REL_MAX / REL_RMS of tests/test_gpu_backward.py for dq, dk, dv,
2 % / 3 % of max(1, |ref|) for d trans_coeff / d tau (tau = 0.8), the loss weights (w, u) drawn by the acceptance rule of
tests/test_gpu_lse_merge.py's `_oracle_grads` (the first seed from 77 up at which six times the fp64 reference's own move under 2^-9 input
noise fits inside both scalar bars: the rule looks at the reference alone).  Forward of the merged slices: REL_MAX / REL_RMS and the 2e-2 LSE
bar of tests/test_gpu_forward.py.  Pose and coordinate gradients: REL_MAX / REL_RMS of tests/test_gpu_rep_grad.py with the no-cancellation
criterion of tests/test_gpu_mask_rep_grad.py (the oracle's own gradient moves by at most half the bar under bf16-size input noise)."""
import functools
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import backward as BW
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _bwd_images as W
from tests import _hip_cases as C
from tests.test_gpu_backward import REL_MAX as G_MAX, REL_RMS as G_RMS
from tests.test_gpu_forward import REL_MAX as F_MAX, REL_RMS as F_RMS
from tests.test_gpu_key_views import B, H, KV, NK, PK, TK, TQ_DEC, _case
from tests.test_gpu_key_views_rep_grad import _parity_inputs
from tests.test_gpu_lse_merge import TAU, _case20, _weights
from tests.test_gpu_mask_rep_grad import _parity_mask
from tests.test_gpu_rep_grad import REL_MAX as R_MAX, REL_RMS as R_RMS

pytestmark = pytest.mark.gpu

FUSED = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
KINDS = ["views", "kmask", "kqmask"]
SLICES = ((0, 4), (4, 5), (5, 13))                        # key views per slice of test 4: 80, 20 and 160 tokens
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def _km():
    g = torch.Generator().manual_seed(41)
    m = torch.zeros(B, TK, dtype=torch.bool)
    m[0] = True
    m[1] = torch.rand(TK, generator=g) < 0.5
    m[2] = torch.arange(TK) % 3 != 2
    for n in (0, 4, 9):
        m[3, n * PK:(n + 1) * PK] = True
    m[3, 5 * PK:5 * PK + 7] = True
    m[4] = torch.rand(TK, generator=g) < 0.15
    return m


@functools.lru_cache(maxsize=None)
def _qm(Tq=TQ_DEC):
    m = torch.zeros(B, Tq, dtype=torch.bool)
    m[0] = True
    m[2] = torch.rand(Tq, generator=torch.Generator().manual_seed(43)) < 0.6
    m[3, :40] = True
    m[4, :99] = torch.arange(99) % 3 != 2
    return m


def test_masks_hold_what_the_docstring_says():
    km, qm = _km(), _qm()
    for v0, v1 in SLICES:                                  # every scene keeps a live key in every slice
        assert bool(km[:, v0 * PK:v1 * PK].any(1).all()), (v0, v1)
    assert km.sum(1).min().item() >= 8 and bool(km[0].all()) and not bool(km[1:].all(1).any())
    q_lens = G2.query_mask_tensors(qm, "cpu")[1].tolist()
    assert q_lens[0] == TQ_DEC and q_lens[1] == 0 and q_lens[3] == 40 and q_lens[4] == 98 and not bool(qm[1].any())
    assert bool(qm[2, :128].any()) and not bool(qm[2, :128].all()) and bool(qm[2, 128:].any()) and not bool(qm[2, 128:].all())
    assert [n * PK for n in KV] == [20, 60, 80, 140, 260]


def _setup(kind, run, dtype):
    """-> the case, the live key tokens per scene, the live query rows [B, Tq] and the mask keywords of the call (built per call: device tensors)"""
    if kind == "views":
        c = _case(run, "enc", dtype)
        cols = [torch.arange(n * PK) for n in KV]
        live = torch.stack([torch.arange(c.Tq) < n * PK for n in KV])
        return c, cols, live, lambda: dict(key_views=KV, query_views=KV, key_views_backward=True)
    if kind == "groups":
        c = _case20(dtype)
        cols = [torch.arange(c.k.shape[2])] * B
        return c, cols, _qm(), lambda: dict(query_mask=_qm().cuda(), key_mask_backward=True)
    c = _case(run, "dec", dtype)
    cols = [_km()[b].nonzero().flatten() for b in range(B)]
    if kind == "kmask":
        return c, cols, torch.ones(B, c.Tq, dtype=torch.bool), lambda: dict(key_mask=_km().cuda(), key_mask_backward=True)

    def kw():
        km, qm = _km().cuda(), _qm().cuda()
        return dict(key_mask=km, query_mask=qm, key_mask_backward=True, mask_index=G2.mask_index(km, qm, device="cuda"))
    return c, cols, _qm(), kw


# ---- the fp64 reference --------------------------------------------------------------------------------------------------------------------------
def _reps(c):
    out = []
    for b in range(B):
        ex64 = {kk: vv[b:b + 1].double() for kk, vv in c.ex.items()}
        reps = O.encoder_reps(c.enc, {kk: vv for kk, vv in ex64.items() if kk.startswith("input")})
        out.append(O.decoder_reps(c.dec, ex64, reps) if c.side == "dec" else reps)
    return out


def _eval(c, reps, qkv, cols):
    """fp64, scene by scene over the scene's live keys: out [B,H,Tq,dh], lse [B,H,Tq] (graphs attached) and the leaves q, k, v, trans_coeff, tau"""
    q, k, v = (t.double().requires_grad_() for t in qkv)
    tc = torch.tensor([float(c.tc.item())], dtype=torch.float64, requires_grad=True)
    tau = torch.tensor([TAU], dtype=torch.float64, requires_grad=True)
    outs, lses = [], []
    for b in range(B):
        qt, kt, vt = O.transform_qkv(q[b:b + 1], k[b:b + 1], v[b:b + 1], c.f_dims, reps[b], tc, True, False)
        kc, vc = kt[:, :, cols[b]], vt[:, :, cols[b]]
        o, _ = O.softmax_attention(qt, kc, vc, c.scale, tau)
        outs.append(O.inverse_transform_out(o, c.f_dims, reps[b], tc, False))
        lses.append(torch.logsumexp(c.scale * qt @ kc.transpose(-1, -2) / tau, -1))
    return torch.cat(outs), torch.cat(lses), (q, k, v, tc, tau)


@functools.lru_cache(maxsize=None)
def _reference(kind, run, dtype):
    """out, lse and the gradients of sum(w out) + sum(u lse) over the LIVE rows, with the draw of (w, u): the acceptance rule of
    tests/test_gpu_lse_merge.py's `_oracle_grads`, on this reference"""
    c, cols, live, _ = _setup(kind, run, dtype)
    reps = _reps(c)
    base = _eval(c, reps, (c.q, c.k, c.v), cols)
    gp = torch.Generator().manual_seed(1)
    shaken = [_eval(c, reps, [t.double() * (1 + (torch.rand(t.shape, generator=gp, dtype=torch.float64) - 0.5) * 2.0 ** -8) for t in (c.q, c.k, c.v)], cols)
              for _ in range(3)]
    scalars = lambda ev, w, u: [float(x) for x in torch.autograd.grad((ev[0] * w).sum() + (ev[1] * u).sum(), ev[2][3:], retain_graph=True)]
    for seed in range(77, 141):
        w, u = _weights(c, seed)
        w, u = w.to(dtype).double() * live[:, None, :, None], u.double() * live[:, None, :]
        s0 = scalars(base, w, u)
        sens = [max(abs(scalars(sh, w, u)[i] - s0[i]) for sh in shaken) for i in range(2)]
        if 6 * sens[0] <= 2e-2 * max(1.0, abs(s0[0])) and 6 * sens[1] <= 3e-2 * max(1.0, abs(s0[1])):
            break
    else:
        raise AssertionError("no draw of (w, u) in 64 seeds at which the scalars' bars are above the reference's own sensitivity")
    dq, dk, dv, dtc, dtau = torch.autograd.grad((base[0] * w).sum() + (base[1] * u).sum(), base[2])
    return SimpleNamespace(out=base[0].detach(), lse=base[1].detach(), dq=dq, dk=dk, dv=dv, dtc=float(dtc.item()), dtau=float(dtau.item()),
                           seed=seed, w=w.float(), u=u.float())


def _leaves(c, live, poison):
    q = c.dev[0].clone()
    if poison:
        q.permute(0, 2, 1, 3)[~live.cuda()] = NAN
    q, k, v = q.requires_grad_(), c.dev[1].clone().requires_grad_(), c.dev[2].clone().requires_grad_()
    return q, k, v, c.tc.clone().requires_grad_(), torch.tensor([TAU], device="cuda", requires_grad=True)


def _backward(c, ref, live, out, lse, poison):
    """(dout, dlse) = (w, u) on the live rows; on the dead rows NaN (poison) or zero"""
    dead = ~live.cuda()
    dout, dlse = ref.w.to(c.dtype).cuda(), ref.u.cuda()
    dout.permute(0, 2, 1, 3)[dead] = NAN if poison else 0.0
    dlse.permute(0, 2, 1)[dead] = NAN if poison else 0.0
    torch.autograd.backward([out, lse], [dout, dlse])
    torch.cuda.synchronize()


def _check_grads(tag, c, ref, cols, live, q, k, v, tc, tau):
    """dq, dk, dv scene by scene on the live rows / live keys at the bars of tests/test_gpu_backward.py; exact zeros on the dead ones; the scalars"""
    for name, t in (("dq", q), ("dk", k), ("dv", v), ("dtc", tc), ("dtau", tau)):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()), (tag, name)
    for b in range(B):
        rows = live[b].nonzero().flatten()
        dead_rows, dead_cols = (~live[b]).nonzero().flatten(), torch.ones(c.k.shape[2], dtype=torch.bool).index_fill_(0, cols[b], False).nonzero().flatten()
        dqd = q.grad[b][:, dead_rows.cuda()]
        assert torch.count_nonzero(dqd) == 0 and not bool(torch.signbit(dqd).any()), (tag, b, "dq at dead rows is not +0.0")
        for g in (k.grad, v.grad):
            assert torch.count_nonzero(g[b][:, dead_cols.cuda()]) == 0, (tag, b, "dk / dv at masked keys")
        for name, got, r in (("dq", q.grad[b][:, rows.cuda()], ref.dq[b][:, rows]), ("dk", k.grad[b][:, cols[b].cuda()], ref.dk[b][:, cols[b]]),
                             ("dv", v.grad[b][:, cols[b].cuda()], ref.dv[b][:, cols[b]])):
            if rows.numel() == 0:                          # a scene without a live row: it adds exact zeros
                assert torch.count_nonzero(got) == 0 and torch.count_nonzero(r) == 0, (tag, b, name)
                continue
            st = C.err_stats(got.float().cpu(), r.float())
            print(f"MASKED_LSE {tag} scene {b} ({cols[b].numel()} keys, {rows.numel()} rows) {name}: max {st['max_abs'] / st['ref_max']:.4f} rms {st['rel_rms']:.4f}")
            assert st["finite"] and st["max_abs"] <= G_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= G_RMS, (tag, b, name, st)
    print(f"MASKED_LSE {tag} seed {ref.seed}: dtc {tc.grad.item():.5f} ref {ref.dtc:.5f} | dtau {tau.grad.item():.5f} ref {ref.dtau:.5f}")
    assert abs(tc.grad.item() - ref.dtc) <= 2e-2 * max(1.0, abs(ref.dtc)), (tag, tc.grad.item(), ref.dtc)
    assert abs(tau.grad.item() - ref.dtau) <= 3e-2 * max(1.0, abs(ref.dtau)), (tag, tau.grad.item(), ref.dtau)


def _check_forward(tag, ref, live, out, lse):
    """tests/test_gpu_forward.py: REL_MAX / REL_RMS for out, 2e-2 for the LSE, on the live rows"""
    m = live.cuda()
    st = C.err_stats(out.detach().float().permute(0, 2, 1, 3)[m], ref.out.permute(0, 2, 1, 3)[live])
    lse_err = (lse.detach().double().permute(0, 2, 1)[m].cpu() - ref.lse.permute(0, 2, 1)[live]).abs().max().item()
    print(f"MASKED_LSE {tag}: out max {st['max_abs'] / st['ref_max']:.4f} rms {st['rel_rms']:.4f} | lse max_abs {lse_err:.3e}")
    assert st["finite"] and st["max_abs"] <= F_MAX * st["ref_max"] and st["rel_rms"] <= F_RMS, (tag, st)
    assert lse_err < 2e-2, (tag, lse_err)


def _attention(c, q, k, v, tc, tau, packed=None, **kw):
    return gta_amd.gta_attention(q, k, v, c.f_dims, packed or c.packed, so3_degree=c.so3, trans_coeff=tc, tau=tau, scale=c.scale, **kw)


# ---- 1. the pre-pass, directly ------------------------------------------------------------------------------------------------------------------
def _entry_inputs(kind, run, dtype):
    """a masked forward (out and lse are the forward's own), then NaN in q, dout, out, lse and dlse at every dead row; -> what the backward
    entries of the kind take"""
    c, cols, live, kw = _setup(kind, run, dtype)
    kw = {n: x for n, x in kw().items() if n != "mask_index"}
    q, k, v = (t.clone() for t in c.dev)
    tau = torch.tensor([TAU], device="cuda")
    with torch.no_grad():
        out, lse = _attention(c, q, k, v, c.tc, tau, return_lse=True, **{n: x for n, x in kw.items() if not n.endswith("_backward") and n != "query_views"})
    g = torch.Generator().manual_seed(7)
    dout = torch.randn(c.q.shape, generator=g).to(dtype).cuda()
    dlse = torch.randn(c.q.shape[:3], generator=g).cuda()
    dead = ~live.cuda()
    out, lse = out.clone(), lse.clone()
    for x in (q, dout, out):
        x.permute(0, 2, 1, 3)[dead] = NAN
    for x in (lse, dlse):
        x.permute(0, 2, 1)[dead] = NAN
    lens = {}
    if kind == "views":
        lens = dict(key_lens=G2.key_lens_tensor(tuple(KV), PK, q.device), q_lens=G2.key_lens_tensor(tuple(KV), PK, q.device))
    else:
        lens["key_idx"], lens["key_lens"] = G2.key_index_tensors(_km(), q.device)
        if kind == "kqmask":
            lens["q_live"], lens["q_lens"] = G2.query_mask_tensors(_qm(), q.device)
    return SimpleNamespace(c=c, live=live, q=q, k=k, v=v, out=out, lse=lse, dout=dout, dlse=dlse, tau=tau, lens=lens)


def _workspace(e, with_dlse):
    """one call of the entry (or of its _dlse twin) on a 0xFF-filled workspace, kv_images rebuilt -> the decoded workspace"""
    c = e.c
    desc = native.make_desc(e.q, e.k, e.v, e.out, c.f_dims, c.so3, c.Nq, NK, c.scale, native.FLAG_V_TRANSFORM)
    L = W.bwd_layout(B, H, c.Tq, TK, c.dh)
    assert native.attn_bwd_workspace_bytes(desc) == L.total
    ws = torch.full((L.total,), W.FILL, device="cuda", dtype=torch.uint8)
    dq, dk, dv = torch.empty_like(e.q), torch.empty_like(e.k), torch.empty_like(e.v)
    dtc, dta = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    t = [c.packed.get(n) for n in ("vrep_q", "vrep_k", "cs_q", "cs_k")]
    l = e.lens
    name = "qmask" if "q_live" in l else "gather" if "key_idx" in l else "varlen"
    lens = {"varlen": ("key_lens", "q_lens"), "gather": ("key_idx", "key_lens"), "qmask": ("key_idx", "key_lens", "q_live", "q_lens")}[name]
    fn = getattr(native, f"attn_bwd_{name}" + ("_dlse" if with_dlse else ""))
    fn(desc, e.q, e.k, e.v, e.out, e.dout, e.lse, *([e.dlse] if with_dlse else []), *t, c.tc, e.tau, *[l[n] for n in lens], None, dq, dk, dv, dtc, ws, dta)
    torch.cuda.synchronize()
    return W.decode_bwd(ws.cpu(), L), (dq, dk, dv, dtc, dta)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED)
@pytest.mark.parametrize("kind", KINDS)
def test_prepass_twin_changes_the_D_half_of_live_rows_only(kind, run, dtype):
    e = _entry_inputs(kind, run, dtype)
    c = e.c
    (a, ga), (b_, gb) = _workspace(e, True), _workspace(e, False)
    L = a.layout
    assert torch.equal(a.bits, b_.bits), "the images differ"
    assert torch.equal(a.stats_raw[:, :, :, 0], b_.stats_raw[:, :, :, 0]), "the lse half differs"
    assert torch.equal(a.dc_raw[:L.n_prep], b_.dc_raw[:L.n_prep])
    live = torch.zeros(B, L.n_qt * 64, dtype=torch.bool)
    live[:, :c.Tq] = e.live
    liveh = live[:, None].expand(B, H, -1)
    # dead rows (the rows past Tq among them): exactly what the base entry writes, which is (-1e30f, 0.0)
    sa, sb = (d.stats_raw.permute(0, 1, 3, 2, 4).reshape(B, H, 2, -1) for d in (a, b_))
    assert torch.equal(sa[:, :, 1][~liveh], sb[:, :, 1][~liveh]) and bool((sa[:, :, 1][~liveh] == 0).all())
    assert bool((sa[:, :, 0][~liveh] == torch.tensor(W.NEG_BIG, dtype=torch.float32).view(torch.int32)).all())
    # nothing of a dead row's NaN (q, dout, out, lse, dlse) reached the workspace
    for d in (a, b_):
        assert bool(torch.isfinite(d.q2).all()) and bool(torch.isfinite(d.do).all()) and bool(torch.isfinite(d.neg_lse2).all())
        assert bool(torch.isfinite(d.neg_D).all()) and bool(torch.isfinite(d.dc_raw.view(torch.float32)).all()) and bool(torch.isfinite(d.dt).all())
    # live rows: -(D - dlse) against fp64 at tests/_bwd_images.py's bar for D, and against the base entry's -D plus dlse
    lv = e.live[:, None].expand(B, H, -1)
    prod = (e.dout.double() * e.out.double()).cpu()
    D, sumabs, dl = prod.sum(-1)[lv], prod.abs().sum(-1)[lv], e.dlse.double().cpu()[lv]
    bar = (L.dhp / 4 + 4) * W.U24 * sumabs + W.U24 * dl.abs()
    got, base = a.neg_D[:, :, :c.Tq].double()[lv], b_.neg_D[:, :, :c.Tq].double()[lv]
    err, rel = (got - (-(D - dl))).abs(), (got - (base + dl)).abs()
    print(f"MASKED_LSE prepass {kind} {run} {dtype}: {int(lv.sum())} live rows, D err/bar {float((err / bar).max()):.3f}, against base + dlse {float((rel / bar).max()):.3f}")
    assert bool((err <= bar).all()) and bool((rel <= bar).all()) and bool((dl.abs() > 0).any())
    assert not torch.equal(sa[:, :, 1][liveh], sb[:, :, 1][liveh])
    for x, y in zip(ga[1:3], gb[1:3]):                      # (and the walks ran on them: dk, dv are finite and moved by dlse through dS)
        assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())
    assert not torch.equal(ga[1], gb[1])


# ---- 2. dlse = 0 is the masked backward, bit for bit ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED)
@pytest.mark.parametrize("kind", KINDS)
def test_zero_dlse_is_the_masked_backward(kind, run, dtype):
    e = _entry_inputs(kind, run, dtype)
    c = e.c
    how = dict(key_views=True, key_views_backward=True) if kind == "views" else dict(key_mask=True, key_mask_backward=True)
    flags = G2.attention_route(tuple(e.q.shape), TK, dtype, c.f_dims, c.so3, c.Nq, NK, needs_grad=True, **how)
    cfg = ({n: int(x) for n, x in c.f_dims.items()}, c.so3, c.Nq, NK, c.scale, flags)
    tables = [c.packed.get(t) for t in ("vrep_q", "vrep_k", "cs_q", "cs_k")]
    dlse0 = torch.where(e.live.cuda()[:, None, :], torch.zeros((), device="cuda"), e.dlse)          # 0 on the live rows, NaN on the dead ones
    run_ = lambda dlse: BW.attn_bwd(cfg, e.q, e.k, e.v, e.out, e.dout, e.lse, c.tc, e.tau, *tables, want_dtau=True, dlse=dlse, **e.lens)
    a, b_, c_ = run_(None), run_(dlse0), run_(dlse0 + 1.0)
    torch.cuda.synchronize()
    for name, x, y in zip(("dq", "dk", "dv", "dtc", "dtau"), a, b_):
        assert bool(torch.isfinite(x).all()) and torch.equal(x, y), (kind, name)
    assert bool(torch.isfinite(c_[0]).all()) and not torch.equal(a[0], c_[0])


# ---- 3. gradients against fp64 autograd through the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED)
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_through_lse_under_masks(kind, run, dtype):
    """views: key_views + query_views; kmask: key_mask; kqmask: key_mask + query_mask (through a MaskIndex) with NaN in q, dout and dlse at
    the dead rows"""
    c, cols, live, kw = _setup(kind, run, dtype)
    ref = _reference(kind, run, dtype)
    poison = kind != "kmask"                                # (views: the rows past query_views get NaN in dout and dlse, q stays finite)
    q, k, v, tc, tau = _leaves(c, live, poison and kind == "kqmask")
    out, lse = _attention(c, q, k, v, tc, tau, return_lse=True, masked_lse_backward=True, **kw())
    _backward(c, ref, live, out, lse, poison)
    tag = f"{kind} {run} {dtype}"
    _check_forward(tag, ref, live, out, lse)
    _check_grads(tag, c, ref, cols, live, q, k, v, tc, tau)


# ---- 4. split = whole under a mask -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED)
def test_split_equals_whole_under_a_key_mask(run, dtype):
    """the key side in three token slices (80, 20, 160 tokens), each a masked call with the opt-in, merged: against the oracle of the whole"""
    c, cols, live, _ = _setup("kmask", run, dtype)
    ref = _reference("kmask", run, dtype)
    km = _km()
    q, k, v, tc, tau = _leaves(c, live, False)
    parts = []
    for v0, v1 in SLICES:
        t0, t1 = v0 * PK, v1 * PK
        assert bool(km[:, t0:t1].any(1).all())
        sub = dict(c.packed)
        for name in G2._KEY_SIDE_TABLES:
            if torch.is_tensor(c.packed.get(name)):
                sub[name] = (c.packed[name][:, v0:v1] if name == "vrep_k" else c.packed[name][:, t0:t1]).contiguous()
        parts.append(_attention(c, q, k[:, :, t0:t1], v[:, :, t0:t1], tc, tau, packed=sub, return_lse=True, key_mask=km[:, t0:t1].contiguous().cuda(),
                                key_mask_backward=True, masked_lse_backward=True))
    out, lse = gta_amd.gta_attention_merge([p[0] for p in parts], [p[1] for p in parts])
    _backward(c, ref, live, out, lse, False)
    tag = f"split {run} {dtype}"
    _check_forward(tag, ref, live, out, lse)
    _check_grads(tag, c, ref, cols, live, q, k, v, tc, tau)


# ---- 5. view groups under a query mask, under grad -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_view_groups_under_a_query_mask_train(dtype):
    """20 views in groups of 8, 8, 4 under `QM`, NaN in q and in the (dout, dlse) that reach the merged pair at the dead rows"""
    c, cols, live, kw = _setup("groups", "clevrtr/gta", dtype)
    ref = _reference("groups", "clevrtr/gta", dtype)
    q, k, v, tc, tau = _leaves(c, live, True)
    out, lse = gta_amd.gta_attention_by_view_groups(q, k, v, c.f_dims, c.packed, views_per_call=8, so3_degree=c.so3, trans_coeff=tc, tau=tau, scale=c.scale,
                                                    return_lse=True, masked_lse_backward=True, **kw())
    dead = ~live.cuda()
    assert torch.count_nonzero(out.detach().permute(0, 2, 1, 3)[dead]) == 0 and bool(torch.isfinite(lse).all())
    _backward(c, ref, live, out, lse, True)
    tag = f"groups {dtype}"
    _check_forward(tag, ref, live, out, lse)
    _check_grads(tag, c, ref, cols, live, q, k, v, tc, tau)


# ---- 6. pose and coordinate gradients with the lse in the loss -----------------------------------------------------------------------------------
def _oracle_rep_grads(ak, ex, qkv, w, u, mask, tc, jitter=None, rows=None):
    """tests/test_gpu_mask_rep_grad.py's `_oracle_masked` (cross-attention) with sum(u lse) in the loss; rows (bool [B, Tq]): the loss over the
    live query rows alone"""
    grads = {k_: [] for k_ in ex}
    for b in range(mask.shape[0]):
        ex_b = {k_: v_[b:b + 1].clone().requires_grad_() for k_, v_ in ex.items()}
        reps = O.decoder_reps(ak, ex_b, O.encoder_reps(ak, ex_b))
        q, k, v = (t[b:b + 1] for t in qkv)
        if jitter is not None:
            q, k, v = (t * (1 + 2.0 ** -9 * (2 * torch.rand(t.shape, generator=jitter, dtype=torch.float64) - 1)) for t in (q, k, v))
        cols = mask[b].nonzero().flatten()
        scale = q.shape[-1] ** -0.5
        qt, kt, vt = O.transform_qkv(q, k, v, ak["f_dims"], reps, tc, True, False)
        o, _ = O.softmax_attention(qt, kt[:, :, cols], vt[:, :, cols], scale)
        out = O.inverse_transform_out(o, ak["f_dims"], reps, tc, False)
        lse = torch.logsumexp(scale * qt @ kt[:, :, cols].transpose(-1, -2), -1)
        live = slice(None) if rows is None else rows[b].nonzero().flatten()
        ((out * w[b:b + 1])[:, :, live].sum() + (lse * u[b:b + 1])[:, :, live].sum()).backward()
        for k_, v_ in ex_b.items():
            grads[k_].append(v_.grad)
    return {k_: torch.cat(v_) for k_, v_ in grads.items()}


def test_pose_and_coordinate_gradients_with_the_lse_in_the_loss():
    name, kind, tc = "cl-dec", "bern", 0.3
    ak, ex, qkv, w, _, self_attn, Pk, _ = _parity_inputs(name, seed=0)
    assert not self_attn
    mask = _parity_mask(name, kind)
    for seed in range(8):                                   # the first draw of u at which the reference is not a cancellation (fp64 alone)
        u = torch.randn(qkv[0].shape[:3], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        ref = _oracle_rep_grads(ak, ex, qkv, w, u, mask, tc)
        moved = _oracle_rep_grads(ak, ex, qkv, w, u, mask, tc, jitter=torch.Generator().manual_seed(99))
        if all(r.abs().max().item() > 0 and (moved[key] - r).abs().max().item() <= 0.5 * R_MAX * r.abs().max().item() for key, r in ref.items()):
            break
    else:
        raise AssertionError("no draw of u in 8 seeds at which the oracle's own gradients hold still under bf16-size input noise")
    exd = {k_: v_.float().cuda().requires_grad_() for k_, v_ in ex.items()}
    leaves = dict(exd)
    q, k, v = (t.to(torch.bfloat16).cuda().requires_grad_() for t in qkv)
    gta_amd.pre_compute_reps_encoder(ak, exd)
    gta_amd.pre_compute_reps_decoder(ak, exd)
    packed = gta_amd.pack_reps(exd, ak["f_dims"])
    out, lse = gta_amd.gta_attention(q, k, v, ak["f_dims"], packed, so3_degree=exd.get("gta_so3_degree", 0), trans_coeff=torch.tensor([tc], device="cuda"),
                                     key_mask=mask.cuda(), key_mask_backward=True, key_mask_rep_grad=True, return_lse=True, masked_lse_backward=True)
    ((out.float() * w.float().cuda()).sum() + (lse * u.float().cuda()).sum()).backward()
    torch.cuda.synchronize()
    Nk = mask.shape[1] // Pk
    for key, r in ref.items():
        st = C.err_stats(leaves[key].grad.detach().double().cpu(), r.double())
        print(f"MASKED_LSE rep_grad {name} {kind} u-seed {seed} d {key}: max {st['max_abs'] / st['ref_max']:.4f} rms {st['rel_rms']:.4f}")
        assert st["finite"] and st["max_abs"] <= R_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= R_RMS, (key, st)
    lv = mask.view(3, Nk, Pk).any(-1)
    assert torch.count_nonzero(leaves["input_transforms"].grad.cpu()[~lv]) == 0
    assert torch.count_nonzero(leaves["input_coord"].grad.cpu().reshape(3, Nk * Pk, 2)[~mask]) == 0


def test_view_groups_pose_gradients_under_a_query_mask():
    """gta_attention_by_view_groups with key_mask_rep_grad=True: the `cl-dec` shape in groups of 2 + 1 views under a Bernoulli 0.6 query mask
    (scene 1 without a live row), NaN in q and in (dout, dlse) at the dead rows; the same bars and the same criterion as above"""
    name, tc = "cl-dec", 0.3
    ak, ex, qkv, w, _, self_attn, Pk, _ = _parity_inputs(name, seed=0)
    Tq, Tk = qkv[0].shape[2], qkv[1].shape[2]
    qm = torch.rand(3, Tq, generator=torch.Generator().manual_seed(11)) < 0.6
    qm[1] = False
    every = torch.ones(3, Tk, dtype=torch.bool)
    for seed in range(8):
        u = torch.randn(qkv[0].shape[:3], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        ref = _oracle_rep_grads(ak, ex, qkv, w, u, every, tc, rows=qm)
        moved = _oracle_rep_grads(ak, ex, qkv, w, u, every, tc, jitter=torch.Generator().manual_seed(99), rows=qm)
        if all(r.abs().max().item() > 0 and (moved[key] - r).abs().max().item() <= 0.5 * R_MAX * r.abs().max().item() for key, r in ref.items()):
            break
    else:
        raise AssertionError("no draw of u in 8 seeds at which the oracle's own gradients hold still under bf16-size input noise")
    exd = {k_: v_.float().cuda().requires_grad_() for k_, v_ in ex.items()}
    leaves = dict(exd)
    dead = ~qm.cuda()
    q = qkv[0].to(torch.bfloat16).cuda()
    q.permute(0, 2, 1, 3)[dead] = NAN
    q, k, v = q.requires_grad_(), qkv[1].to(torch.bfloat16).cuda().requires_grad_(), qkv[2].to(torch.bfloat16).cuda().requires_grad_()
    gta_amd.pre_compute_reps_encoder(ak, exd)
    gta_amd.pre_compute_reps_decoder(ak, exd)
    packed = gta_amd.pack_reps(exd, ak["f_dims"])
    out, lse = gta_amd.gta_attention_by_view_groups(q, k, v, ak["f_dims"], packed, views_per_call=2, so3_degree=exd.get("gta_so3_degree", 0),
                                                    trans_coeff=torch.tensor([tc], device="cuda"), query_mask=qm.cuda(), key_mask_backward=True,
                                                    key_mask_rep_grad=True, masked_lse_backward=True, return_lse=True)
    dout, dlse = w.to(torch.bfloat16).cuda(), u.float().cuda()
    dout.permute(0, 2, 1, 3)[dead] = NAN
    dlse.permute(0, 2, 1)[dead] = NAN
    torch.autograd.backward([out, lse], [dout, dlse])
    torch.cuda.synchronize()
    assert torch.count_nonzero(q.grad.permute(0, 2, 1, 3)[dead]) == 0
    for t in (q, k, v):
        assert bool(torch.isfinite(t.grad).all())
    for key, r in ref.items():
        st = C.err_stats(leaves[key].grad.detach().double().cpu(), r.double())
        print(f"MASKED_LSE groups rep_grad {name} u-seed {seed} d {key}: max {st['max_abs'] / st['ref_max']:.4f} rms {st['rel_rms']:.4f}")
        assert st["finite"] and st["max_abs"] <= R_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= R_RMS, (key, st)
    assert torch.count_nonzero(leaves["target_transforms"].grad[1]) == 0 and torch.count_nonzero(leaves["target_coord"].grad[1]) == 0


# ---- 7. the flag alone is inert ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_the_flag_alone_is_inert(kind, dtype):
    c, _, live, kw = _setup(kind, "msn/gta_so3", dtype)
    dout = torch.randn(c.q.shape, generator=torch.Generator().manual_seed(3)).to(dtype).cuda()
    got = []
    for flag in (False, True):
        q, k, v, tc, tau = _leaves(c, live, False)
        out = _attention(c, q, k, v, tc, tau, masked_lse_backward=flag, **kw())
        out.backward(dout)
        got.append((out.detach(), q.grad, k.grad, v.grad, tc.grad, tau.grad))
    torch.cuda.synchronize()
    for name, x, y in zip(("out", "dq", "dk", "dv", "dtc", "dtau"), *got):
        assert torch.equal(x, y), (kind, name)
    with torch.no_grad():                                   # ... and so it is without grad, return_lse or not
        a = _attention(c, *c.dev, c.tc, None, return_lse=True, **{n: x for n, x in kw().items() if n != "query_views"})
        b_ = _attention(c, *c.dev, c.tc, None, return_lse=True, masked_lse_backward=True, **{n: x for n, x in kw().items() if n != "query_views"})
    assert torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1])

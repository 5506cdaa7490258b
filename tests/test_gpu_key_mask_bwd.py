"""GPU: the backward through a key mask (`gta_attention(..., key_mask=m, key_mask_backward=True)`; `gta_attn_bwd_gather`: the VARLEN q-side
pre-pass and dQ walk as they are, the GATHER instances of the dK/dV walk, which scatter dk / dv back through `key_idx`).

Shapes are those of tests/test_gpu_key_mask.py (its cases are imported): B = 4, H = 2, 5 views x 52 tokens (Tk = 260: three 128-key blocks, the
last one with 4 rows).  Decoder leg: Tq = 150.  Self-attention leg: Tq = 260 (no query-side mask: every query row is live).  Layouts clevrtr/gta
(dh 64) and msn/gta_so3 (dh 96), fp32 and bf16.

Mask sets, one mask per scene:
  blocks   all 260 keys | token 137 alone (one live row; blocks 1 and 2 wholly dead) | every second token (130 keys: block 0 full, block 1 with
           two live rows in its first tile, block 2 dead) | views 0 and 2 whole plus the first 24 tokens of view 3 (128 keys: exactly one full
           block and nothing behind it, view 1 wholly masked in the middle)
  random   tests/test_gpu_key_mask.py's Bernoulli set (0.9 / 0.5 / 0.25 / 0.05, fixed seed, at least one key each)

Bars (none new): tests/test_gpu_backward.py's REL_MAX / REL_RMS for dq, dk, dv (imported); d trans_coeff 2 % of max(1, |ref|) and d tau 3 % of
max(1, |ref|), as tests/test_gpu_key_views_bwd.py; the whole-model case the fp32 module bars of tests/test_gpu_modules.py's `_srt_grad_check`
(imported)."""
import ctypes
import functools

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests import _images as I
from tests.test_gpu_backward import REL_MAX, REL_RMS
from tests.test_gpu_key_mask import B, H, M13, NK, PK, TC, TK, _case, _masks, _poisoned, _tensors
from tests.test_gpu_modules import _srt_grad_check

pytestmark = pytest.mark.gpu

LAYOUTS = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
SIDES = ["dec", "enc"]
MASKS = ["blocks", "random"]
TAU = 0.8


@functools.lru_cache(maxsize=None)
def _mask_set(name):
    """bool [B, TK] on the CPU: `blocks` (above), or a set of tests/test_gpu_key_mask.py"""
    if name != "blocks":
        return _masks(name)
    m = torch.zeros(B, TK, dtype=torch.bool)
    m[0] = True
    m[1, 137] = True
    m[2] = torch.arange(TK) % 2 == 0
    m[3, 0:PK] = m[3, 2 * PK:3 * PK] = m[3, 3 * PK:3 * PK + 24] = True
    assert m.sum(1).tolist() == [260, 1, 130, 128] and not bool(m[3, PK:2 * PK].any())
    return m


def test_mask_counts():
    assert _mask_set("blocks").sum(1).tolist() == [260, 1, 130, 128]
    r = _mask_set("random")
    assert tuple(r.shape) == (B, TK) and bool(r.any(1).all()) and not bool(r.all(1).any())
    n = r.sum(1).tolist()
    assert n[0] > n[1] > n[2] > n[3] >= 1, n


# d trans_coeff and d tau are each ONE number summed over every token with both signs, and what bf16 operands leave of such a sum does not
# shrink with its value.  A bar of 2 % / 3 % of max(1, |ref|) says something only where the value is not itself a cancellation, and with random
# loss weights some of the sixteen (layout, leg, mask set) scalars always are (d tau = -3.2, d trans_coeff = 1.1 under the seed of
# tests/test_gpu_key_views_bwd.py).  Two criteria, both from the fp64 oracle and the number format alone, say when a reference is usable:
#   d trans_coeff: under bf16-size relative perturbations of q, k, v (2^-9, two draws) the oracle's own value moves by 0.1 .. 0.6 at these
#       shapes, whatever the value: |ref| >= 30 puts the 2 % bar at that or above.
#   d tau: `_dtau_sigma` -- the first-order standard deviation of d tau under the bf16 roundings of the forward's and the backward's operands
#       (0.40 .. 0.84 here; a Monte-Carlo of the same rounding sites, both q roundings and the rounding of dS included, gives 0.35 .. 1.4 from
#       eight draws).  The 3 % bar has to be at least FIVE of these sigmas.
# The draw of tests/test_gpu_key_views_bwd.py's `_w` gets one seed per (layout, leg): the first of 101, 211, 307, 401, 503, 601, 701, 809, 907,
# 1009, 1103, 1201, 1301, 1409, 1511, 1601, 1709, 1801, 1901, 2003, 2111 that meets both criteria under BOTH mask sets (bf16 inputs):
#                          d trans_coeff (blocks / random)      d tau (blocks / random)      3 % bar / sigma (blocks / random)
#   clevrtr/gta dec 1901        71.6 /   55.7                     -84.0 / -146.4                 5.3 / 11.0
#   clevrtr/gta enc 2111        85.1 /  -50.2                    -157.2 / -271.8                 6.9 / 14.9
#   msn/gta_so3 dec 2003        70.9 /   41.3                     182.9 /  111.4                 9.5 /  6.2
#   msn/gta_so3 enc  101       -46.9 /  135.9                     194.4 / -244.2                 7.0 / 10.6
# `test_oracle_parity_of_the_scalars` asserts both criteria on the references it uses.
W_SEEDS = {("clevrtr/gta", "dec"): 1901, ("clevrtr/gta", "enc"): 2111, ("msn/gta_so3", "dec"): 2003, ("msn/gta_so3", "enc"): 101}
DTC_MIN, DTAU_SIGMAS = 30.0, 5.0
RHO_BF16 = 2.0 ** -9 / 3 ** 0.5          # rms of a relative error uniform in the bf16 rounding interval +-2^-9


def _dtau_sigma2(qt, kt, vt, dO, out, w, scale, bf16):
    """Variance of one scene's d tau = -(1/tau) sum_ij dS_ij z_ij under independent relative roundings (rms RHO_BF16) of the operands the
    kernels round to bf16, to first order; qt [H,Tq,dh], kt / vt [H,n,dh] (the valid keys), dO = d loss / d o~, out and w (= dout) [H,Tq,dh]:
      dO~ image   dP_ij moves, D_i = <dout_i, out_i> (fp32, unrounded dout) does not:      sum_ic (dO_ic [(P z) V']_ic)^2
      V' image    shared by dP and, through out, by D, so the row mean drops out:          sum_jc (V'_jc [(P (z - m))^T dO~]_jc)^2,  m_i = sum_j P_ij z_ij
      K' image    dq' = c1 dS K':                                                          sum_jc (K'_jc c1 [dS^T q']_jc)^2
      P           rounded for the forward's P V' product: out, so D, carries it:           sum_ij (m_i P_ij dP_ij)^2
      out         rounded to bf16 where the inputs are:                                    sum_ic (m_i dout_ic out_ic)^2
    (the two roundings of q' and the rounding of dS are left to the Monte-Carlo named above; they do not change the picture)"""
    c1 = scale / TAU
    z = c1 * qt @ kt.transpose(-1, -2)
    P = torch.softmax(z, -1)
    m = (P * z).sum(-1, keepdim=True)
    dP = dO @ vt.transpose(-1, -2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    var = (dO * ((P * z) @ vt)).pow(2).sum() + (vt * ((P * (z - m)).transpose(-1, -2) @ dO)).pow(2).sum()
    var = var + (kt * (dS.transpose(-1, -2) @ qt) * c1).pow(2).sum() + (m * P * dP).pow(2).sum()
    if bf16:
        var = var + (m * w * out).pow(2).sum()
    return (RHO_BF16 / TAU) ** 2 * var.item()


def _w(c):
    """random loss weights, one draw per (layout, leg): the rule of tests/test_gpu_key_views_bwd.py's `_w` with the seeds of W_SEEDS"""
    g = torch.Generator().manual_seed(W_SEEDS[(c.run, c.side)] + sum(map(ord, c.run)) + (c.side == "dec"))
    return torch.randn(B, H, c.Tq, c.dh, generator=g)


def _run(c, mask, qkv=None, packed=None, w=None, how="mask", views=None):
    """forward + backward through gta_attention under the mask (how='views': under key_views = views with key_views_backward); returns
    (dq, dk, dv, d trans_coeff, d tau)"""
    q, k, v = (t.detach().clone().requires_grad_() for t in (qkv or c.dev))
    tc = c.tc.clone().requires_grad_()
    ta = torch.tensor([TAU], device="cuda", requires_grad=True)
    w = _w(c).cuda() if w is None else w
    kw = {"key_mask": mask.cuda(), "key_mask_backward": True} if how == "mask" else {"key_views": list(views), "key_views_backward": True}
    out = gta_amd.gta_attention(q, k, v, c.f_dims, packed or c.packed, so3_degree=c.so3, trans_coeff=tc, tau=ta, scale=c.scale, **kw)
    out.backward(w.to(out.dtype))
    torch.cuda.synchronize()
    return q.grad, k.grad, v.grad, tc.grad, ta.grad


@functools.lru_cache(maxsize=None)
def _got(run, side, dtype, masks):
    return _run(_case(run, side, dtype), _mask_set(masks))


def _one_key_bounds(qt, kt, vt, dO, reps, scale):
    """A scene with ONE valid key j: softmax over one key is constant, so the exact dq and dk are identically zero and a bar relative to the
    gradient's own magnitude says nothing.  What the kernels leave there is rounding: dS_ij = P_ij (dP_ij - D_i) with P_ij = 1 and
    dP_ij = <dO~_i, v'_j> = D_i exactly, where the walks form dP from operands rounded to bf16 (relative error 2^-9 each) and the pre-pass
    forms D_i = <dout_i, out_i> from the output as the forward stored it (from the bf16 V' image, rounded to bf16 for bf16 inputs: 2^-9 more),
    and P_ij is 1 to within the same roundings of the logit.  To first order |dS_ij| <= 4 * 2^-9 * |dO~_i| |v'_j| =: e_i (Cauchy-Schwarz), so with
    c1 = scale / tau, dq_i = A_q^T (c1 dS_ij k'_j) and dk_j = B_k^T (c1 sum_i dS_ij q'_i):
        max |dq| <= |A_q| c1 max_i e_i |k'_j|          max |dk| <= |B_k| c1 sum_i e_i |q'_i|
    with |.| the 2-norm (the so2 / so3 blocks of rho are orthogonal; the se3 blocks' norm is taken from the oracle's matrices).  Worst-case
    bounds from the number format alone -- nothing here is taken from the kernels' results."""
    msk = O.scale_mask(TC, None, torch.float64)
    nA = max(1.0, torch.linalg.matrix_norm(reps["inv_se3rep_q"] * msk, ord=2).max().item())
    nB = max(1.0, torch.linalg.matrix_norm(reps["se3rep_k"] * msk, ord=2).max().item())
    c1 = scale / TAU
    e = 2.0 ** -7 * dO.norm(dim=-1) * vt.norm(dim=-1)[:, None]                    # [H, Tq]
    return {"dq": (nA * c1 * e * kt.norm(dim=-1)[:, None]).max().item(), "dk": (nB * c1 * (e * qt.norm(dim=-1)).sum(1)).max().item()}


def _oracle_scene(q, k, v, f_dims, reps, cols, w, scale, bf16=False):
    """fp64 autograd of one scene: rho on the whole key side, the valid columns, softmax attention, rho^-1 -> (dq, dk, dv, d trans_coeff, d tau,
    the bounds of `_one_key_bounds` for a scene with one valid key or None, `_dtau_sigma2`)"""
    q, k, v = (t.double().requires_grad_() for t in (q, k, v))
    tc = torch.tensor([TC], dtype=torch.float64, requires_grad=True)
    ta = torch.tensor([TAU], dtype=torch.float64, requires_grad=True)
    qt, kt, vt = O.transform_qkv(q, k, v, f_dims, reps, tc, True, False)
    o, _ = O.softmax_attention(qt, kt[:, :, cols], vt[:, :, cols], scale, ta)
    o.retain_grad()
    out = O.inverse_transform_out(o, f_dims, reps, tc, False)
    (out * w).sum().backward()
    sig2 = _dtau_sigma2(qt[0].detach(), kt[0][:, cols].detach(), vt[0][:, cols].detach(), o.grad[0], out[0].detach(), w[0], scale, bf16)
    zero = None
    if cols.numel() == 1:
        j = int(cols[0])
        zero = _one_key_bounds(qt[0].detach(), kt[0, :, j].detach(), vt[0, :, j].detach(), o.grad[0], reps, scale)
    return q.grad[0], k.grad[0], v.grad[0], float(tc.grad.item()) if tc.grad is not None else 0.0, float(ta.grad.item()), zero, sig2


@functools.lru_cache(maxsize=None)
def _oracle_grads(run, side, dtype, masks):
    c = _case(run, side, dtype)
    w = _w(c).to(dtype).double()
    res, dtc, dta, sig2 = [], 0.0, 0.0, 0.0
    for b in range(B):
        ex64 = {"input_transforms": c.ex["input_transforms"][b:b + 1].double(), "input_coord": c.ex["input_coord"][b:b + 1].double()}
        reps = O.encoder_reps(c.enc, ex64)
        if side == "dec":
            ex64["target_transforms"] = c.ex["target_transforms"][b:b + 1].double()
            ex64["target_coord"] = c.ex["target_coord"][b:b + 1].double()
            reps = O.decoder_reps(c.dec, ex64, reps)
        cols = _mask_set(masks)[b].nonzero().flatten()
        dq, dk, dv, t, a, zero, s2 = _oracle_scene(c.q[b:b + 1], c.k[b:b + 1], c.v[b:b + 1], c.f_dims, reps, cols, w[b:b + 1], c.scale,
                                                   dtype == torch.bfloat16)
        res.append((dq, dk, dv, zero))
        dtc += t
        dta += a
        sig2 += s2
    return res, dtc, (dta, sig2 ** 0.5)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ---- 1. oracle parity -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_oracle_parity(run, side, dtype, masks):
    """dq, dk and dv at the valid rows against fp64 oracle autograd per scene on the valid key columns.  The scene with one
    valid key has dq = dk = 0 exactly: those two are held to the absolute rounding bounds of `_one_key_bounds` instead of a relative bar.
    Measured there (MI355X): max |dq| 1.8e-2 (float32, clevrtr/gta, decoder leg) against a bound of order 0.5"""
    mask = _mask_set(masks)
    dq, dk, dv, _, _ = _got(run, side, dtype, masks)
    ref, _, _ = _oracle_grads(run, side, dtype, masks)
    for b in range(B):
        cols = mask[b].nonzero().flatten()
        for name, got, r in (("dq", dq[b], ref[b][0]), ("dk", dk[b][:, cols.cuda()], ref[b][1][:, cols]), ("dv", dv[b][:, cols.cuda()], ref[b][2][:, cols])):
            st = C.err_stats(got.float().cpu(), r.float())
            print(f"KEY_MASK_BWD {run} {side} {dtype} {masks} scene {b} ({cols.numel()} keys) {name}: {st} {ref[b][3] or ''}")
            if st["ref_max"] == 0.0:                          # (the one-key scene's dq and dk, nothing else)
                assert cols.numel() == 1 and name in ("dq", "dk") and st["finite"] and st["max_abs"] <= ref[b][3][name], (run, side, dtype, masks, b, name, st)
                continue
            assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS, (run, side, dtype, masks, b, name, st)


@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_oracle_parity_of_the_scalars(run, side, dtype, masks):
    """d trans_coeff (2 % of max(1, |ref|)) and d tau (3 %) of the same runs against the sums of the same per-scene oracle gradients.  Both
    references are first held to the two criteria W_SEEDS was chosen by (above): a reference that is itself a cancellation proves nothing"""
    _, _, _, dtc, dta = _got(run, side, dtype, masks)
    _, ref_dtc, (ref_dta, sigma) = _oracle_grads(run, side, dtype, masks)
    print(f"KEY_MASK_BWD {run} {side} {dtype} {masks} dtc {dtc.item()} ref {ref_dtc} | dtau {dta.item()} ref {ref_dta} sigma {sigma:.3f}")
    assert abs(ref_dtc) >= DTC_MIN and 3e-2 * abs(ref_dta) >= DTAU_SIGMAS * sigma, (ref_dtc, ref_dta, sigma)
    assert abs(dtc.item() - ref_dtc) <= 2e-2 * max(1.0, abs(ref_dtc)), (dtc.item(), ref_dtc)
    assert abs(dta.item() - ref_dta) <= 3e-2 * max(1.0, abs(ref_dta)), (dta.item(), ref_dta)


# ---- direct calls -----------------------------------------------------------------------------------------------------------------------------
def _filled(shape, dtype):
    """a [B,H,T,dh] view of token-major storage with every byte 0xFF (a NaN in both types)"""
    Bq, Hq, T, dh = shape
    n = Bq * T * Hq * dh * (2 if dtype == torch.bfloat16 else 4)
    return torch.full((n,), 0xFF, device="cuda", dtype=torch.uint8).view(dtype).view(Bq, T, Hq, dh).permute(0, 2, 1, 3)


def _abi(c, entry, key_idx, key_lens, qkv=None, packed=None, images="forward", tau=True, dout=None, Nk=NK, bwd_ws_bytes=None, null=()):
    """gta_attn_fwd_gather + gta_attn_bwd_gather (entry='varlen': the varlen pair, q_lens NULL) through ctypes, the gradients pre-filled with
    0xFF; images: 'forward' (the forward's workspace) or None (rebuilt).  Returns (dq, dk, dv, d trans_coeff, d tau or None), out, lse -- or, with
    bwd_ws_bytes (the size the backward is told its workspace has) and null (names among key_idx, key_lens handed to the backward as NULL),
    the backward's return code"""
    q, k, v = qkv or c.dev
    pk = packed or c.packed
    Tk = k.shape[2]
    p, L = native._ptr, native.lib()
    out = torch.empty(B, c.Tq, H, c.dh, device="cuda", dtype=c.dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, c.Tq, device="cuda", dtype=torch.float32)
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, Nk, c.scale, native.FLAG_V_TRANSFORM)
    assert native.attn_bwd_gather_supported(desc) == 0
    ta = torch.tensor([TAU], device="cuda") if tau else None
    tables = (p(pk.get("vrep_q")), p(pk.get("vrep_k")), p(pk.get("cs_q")), p(pk.get("cs_k")), p(c.tc), p(ta))
    lens = (p(key_idx), p(key_lens)) if entry == "gather" else (p(key_lens),)
    ws_f = torch.full((native.attn_fwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    rc = getattr(L, "gta_attn_fwd_" + entry)(ctypes.byref(desc), p(q), p(k), p(v), *tables, *lens, p(out), p(lse), p(ws_f), ws_f.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    dout = _w(c).to(c.dtype).cuda() if dout is None else dout
    dq, dk, dv = (_filled((B, H, T, c.dh), c.dtype) for T in (c.Tq, Tk, Tk))
    dtc = torch.full((1,), float("nan"), device="cuda")
    dta = torch.full((1,), float("nan"), device="cuda") if tau else None
    ws = torch.full((native.attn_bwd_workspace_bytes(desc),), 0xFF, device="cuda", dtype=torch.uint8)
    gs = (ctypes.c_int64 * 9)(*(list(dq.stride()[:3]) + list(dk.stride()[:3]) + list(dv.stride()[:3])))
    ds = (ctypes.c_int64 * 3)(*dout.stride()[:3])
    lens = ((None if "key_idx" in null else p(key_idx), None if "key_lens" in null else p(key_lens)) if entry == "gather" else (p(key_lens), None))
    rc = getattr(L, "gta_attn_bwd_" + entry)(ctypes.byref(desc), p(q), p(k), p(v), p(out), p(dout), p(lse), *tables, *lens,
                                             p(ws_f) if images == "forward" else None, p(dq), p(dk), p(dv), gs, ds, p(dtc), p(dta), p(ws),
                                             ws.numel() if bwd_ws_bytes is None else bwd_ws_bytes, native._stream())
    if bwd_ws_bytes is not None:
        return rc
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    return (dq, dk, dv, dtc, dta), out, lse


# ---- 2. every row is written, the masked ones as zeros ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_every_row_is_written_and_masked_rows_are_zero_bits(run, side, dtype, masks):
    """dk / dv start as 0xFF bytes (NaN): after the call every one of the B H Tk rows is finite -- so each was written --, and the rows of masked
    tokens are all-bits-zero (the permutation tail of key_idx, the dead-block path, the 4-row last block); gta_attention gives the same bits"""
    c = _case(run, side, dtype)
    mask = _mask_set(masks)
    key_idx, key_lens = _tensors(mask)
    for b in range(B):                                        # the contract of this entry: every row a permutation, the valid tokens first
        assert sorted(key_idx[b].tolist()) == list(range(TK)) and bool(mask[b][key_idx[b, :int(key_lens[b])].cpu().long()].all())
    (dq, dk, dv, dtc, dta), _, _ = _abi(c, "gather", key_idx, key_lens)
    dead = (~mask).cuda()
    for name, g in (("dk", dk), ("dv", dv)):
        assert torch.isfinite(g).all(), (run, side, dtype, masks, name)
        rows = _bits(g.permute(0, 2, 1, 3)[dead])
        assert rows.numel() == int(dead.sum()) * H * c.dh and torch.count_nonzero(rows) == 0, (run, side, dtype, masks, name)
        live = g.permute(0, 2, 1, 3)[mask.cuda()]
        assert torch.count_nonzero(live) > 0.9 * live.numel()
    assert torch.isfinite(dq).all() and torch.isfinite(dtc).all() and torch.isfinite(dta).all()
    got = _got(run, side, dtype, masks)
    for a, r in zip((dq, dk, dv, dtc, dta), got):
        assert torch.equal(a, r.reshape(a.shape)), (run, side, dtype, masks)      # gta_attention took this entry
    dead_got = torch.cat([_bits(got[1].permute(0, 2, 1, 3)[dead]).flatten(), _bits(got[2].permute(0, 2, 1, 3)[dead]).flatten()])
    assert torch.count_nonzero(dead_got) == 0


# ---- 3. a mask of leading views is key_views_backward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("views", [(1, 3, 4, 5), (NK,) * B])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_a_mask_of_leading_views_is_key_views_backward(run, side, dtype, views):
    """whole leading views, and the all-true mask against key_views = [Nk] * B (no query_views): all five gradients bit for bit"""
    c = _case(run, side, dtype)
    mask = _mask_set("views:" + ",".join(map(str, views)))
    assert mask.sum(1).tolist() == [n * PK for n in views]
    got = _run(c, mask)
    ref = _run(c, None, how="views", views=views)
    for name, a, r in zip(("dq", "dk", "dv", "dtc", "dtau"), got, ref):
        assert torch.isfinite(a).all() and torch.equal(a, r), (run, side, dtype, views, name)


# ---- 4. the first 13 tokens of every view: the call on sliced keys ----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_first_tokens_of_every_view_is_the_call_on_sliced_keys(run, side, dtype):
    """gta_attn_bwd_gather under that mask against gta_attn_bwd_varlen on k, v, cs_k physically cut to those tokens (five views of 13 tokens,
    key_lens = 65): dq and d tau bit for bit, the dk / dv rows of the valid tokens bit for bit the sliced call's rows; d trans_coeff within the
    2 % bar only (the two calls sum a different number of per-block partials)"""
    c = _case(run, side, dtype)
    mask = _mask_set("first13")
    key_idx, key_lens = _tensors(mask)
    (dq, dk, dv, dtc, dta), out, lse = _abi(c, "gather", key_idx, key_lens)
    cols = mask[0].nonzero().flatten().cuda()
    q, k, v = c.dev
    pk = dict(c.packed)
    pk["cs_k"] = c.packed["cs_k"][:, cols].contiguous()
    ks, vs = k[:, :, cols].contiguous(), v[:, :, cols].contiguous()
    assert ks.shape[2] == NK * M13 == 65
    lens1 = torch.full((B,), NK * M13, device="cuda", dtype=torch.int32)
    (dq1, dk1, dv1, dtc1, dta1), out1, lse1 = _abi(c, "varlen", None, lens1, qkv=(q, ks, vs), packed=pk)
    assert torch.equal(out, out1) and torch.equal(lse, lse1)
    assert torch.equal(dq, dq1) and torch.equal(dta, dta1), (run, side, dtype)
    assert torch.equal(dk[:, :, cols], dk1) and torch.equal(dv[:, :, cols], dv1), (run, side, dtype)
    dead = torch.ones(TK, dtype=torch.bool, device="cuda")
    dead[cols] = False
    assert torch.count_nonzero(_bits(dk[:, :, dead])) == 0 and torch.count_nonzero(_bits(dv[:, :, dead])) == 0
    print(f"KEY_MASK_BWD sliced {run} {side} {dtype}: dtc {dtc.item()} vs {dtc1.item()}")
    assert abs(dtc.item() - dtc1.item()) <= 2e-2 * max(1.0, abs(dtc1.item())), (dtc.item(), dtc1.item())


# ---- 5. masked content is never used ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masks", MASKS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_masked_content_is_never_used(run, side, dtype, masks):
    """NaN, then +-Inf, in every masked row of k, v and cs_k, and NaN in the vrep_k record of every view no valid token belongs to (scene 3's
    view 1 in `blocks`); the query rows of masked tokens stay finite: all five gradients bit for bit those of the clean run"""
    c = _case(run, side, dtype)
    mask = _mask_set(masks)
    ref = _got(run, side, dtype, masks)
    n_views = 0
    signs = lambda t: torch.where(torch.arange(t.numel(), device=t.device).reshape(t.shape) % 2 == 0, float("inf"), float("-inf")).to(t.dtype)
    for value in (float("nan"), signs):
        qkv, pk = _poisoned(c, mask, value)
        pk["vrep_k"] = pk["vrep_k"].clone()
        for b in range(B):
            for n in range(NK):
                if not bool(mask[b, n * PK:(n + 1) * PK].any()):
                    pk["vrep_k"][b, n] = float("nan")
                    n_views += 1
        assert not torch.isfinite(qkv[1]).all() and not torch.isfinite(pk["cs_k"]).all() and torch.isfinite(qkv[0]).all()
        got = _run(c, mask, qkv, pk)
        for name, a, r in zip(("dq", "dk", "dv", "dtc", "dtau"), got, ref):
            assert torch.isfinite(a).all() and torch.equal(a, r), (run, side, dtype, masks, name)
    if masks == "blocks":
        assert n_views >= 2 and not bool(mask[3, PK:2 * PK].any())          # (scene 3's view 1 among them, in both rounds)


# ---- 6. ABI -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", LAYOUTS)
def test_direct_ctypes_call(run, dtype):
    """kv_images = NULL (the images rebuilt by the GATHER pre-pass) and the forward's workspace give the same bits; a NULL key_idx or key_lens
    is GTA_E_BADARG, with kv_images too; a too-small workspace is refused"""
    c = _case(run, "enc", dtype)
    mask = _mask_set("blocks")
    key_idx, key_lens = _tensors(mask)
    a, _, _ = _abi(c, "gather", key_idx, key_lens, images="forward")
    r, _, _ = _abi(c, "gather", key_idx, key_lens, images=None)
    for x, y in zip(a, r):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    L = native.lib()
    for images in ("forward", None):
        assert _abi(c, "gather", key_idx, key_lens, images=images, bwd_ws_bytes=1 << 40, null=("key_idx",)) == -1
        assert "null key_idx" in L.gta_strerror(-1).decode()
        assert _abi(c, "gather", key_idx, key_lens, images=images, bwd_ws_bytes=1 << 40, null=("key_lens",)) == -1
        assert "null key_lens" in L.gta_strerror(-1).decode()
    rc = _abi(c, "gather", key_idx, key_lens, bwd_ws_bytes=4096)
    assert rc == -1 and "workspace smaller" in L.gta_strerror(rc).decode()
    torch.cuda.synchronize()


# ---- 7. every head size --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [16, 40, 104, 128])
def test_every_head_size(dh, dtype):
    """the GATHER instances the two layouts do not reach (dhp 32 and 128) and head sizes that leave chunks of a padded row unused: B = 3, H = 3,
    3 views of 50 tokens (Tk = 150: two blocks, the second with 22 rows), a decoder-like query side of 100 rows, token-major storage; masks:
    every third token dropped (100 keys), Bernoulli 0.3, all keys.  dq, dk, dv against the oracle under the same bars"""
    se3 = int(round(dh / 2 / 4)) * 4
    c = I.key_side_case({"se3": se3, "so2": dh - se3}, 0, dtype, B=3, H=3, Nk=3, Pk=50, seed=5, Tq=100)
    mask = torch.ones(c.B, c.T, dtype=torch.bool)
    mask[0, 2::3] = False
    mask[1] = torch.rand(c.T, generator=torch.Generator().manual_seed(dh)) < 0.3
    mask[1, 149] = True
    assert mask[0].sum() == 100 and 20 < mask[1].sum() < 80 and mask[2].all()
    q, k, v = (t.to(dtype).cuda().requires_grad_() for t in (c.q, c.k, c.v))
    packed = {n: t.cuda() for n, t in c.packed.items()}
    w = torch.randn(c.B, c.H, c.Tq, dh, generator=torch.Generator().manual_seed(7 + dh)).to(dtype)
    tc = torch.tensor([TC], device="cuda")
    out = gta_amd.gta_attention(q, k, v, c.f_dims, packed, so3_degree=0, trans_coeff=tc, scale=dh ** -0.5, key_mask=mask.cuda(), key_mask_backward=True)
    out.backward(w.cuda())
    torch.cuda.synchronize()
    dead = (~mask).cuda()
    for g in (k.grad, v.grad):
        assert torch.isfinite(g).all() and torch.count_nonzero(_bits(g.permute(0, 2, 1, 3)[dead])) == 0
    for b in range(c.B):
        reps = {n: ([x[b:b + 1].double() for x in t] if isinstance(t, (list, tuple)) else t[b:b + 1].double()) for n, t in c.reps.items() if t is not None}
        cols = mask[b].nonzero().flatten()
        q64, k64, v64 = (t[b:b + 1].double().requires_grad_() for t in (c.q, c.k, c.v))
        qt, kt, vt = O.transform_qkv(q64, k64, v64, c.f_dims, reps, TC, True, False)
        o, _ = O.softmax_attention(qt, kt[:, :, cols], vt[:, :, cols], dh ** -0.5)
        (O.inverse_transform_out(o, c.f_dims, reps, TC, False) * w[b:b + 1].double()).sum().backward()
        for name, got, r in (("dq", q.grad[b], q64.grad[0]), ("dk", k.grad[b][:, cols.cuda()], k64.grad[0][:, cols]),
                             ("dv", v.grad[b][:, cols.cuda()], v64.grad[0][:, cols])):
            st = C.err_stats(got.float().cpu(), r.float())
            print(f"KEY_MASK_BWD dh{dh} {dtype} scene {b} ({cols.numel()} keys) {name}: {st}")
            assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS, (dh, dtype, b, name, st)


# ---- 8. whole model -----------------------------------------------------------------------------------------------------------------------------
def test_whole_model_step_under_a_mask_of_leading_views():
    """one TransformingSRT step (fp32; the tiny fused-layout config of tests/test_gpu_key_views_bwd.py: se3 16 | so2 8 at dh = 24) with
    input_mask = "the leading views" and input_mask_backward=True, the padded inputs zero-filled: the pixels are the bits of the run under
    input_views, the parameter gradients agree at the fp32 module bars (`_srt_grad_check`) -- not bit for bit: that route also masks the
    padded query rows"""
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
    for b, n in enumerate(views):
        mask[b, :n] = True
        for name in ("input_images", "input_camera_pos", "input_rays"):
            data[name][b, n:] = 0.0
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, 1, npix, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 1, 1, 3, generator=g).cuda().expand(-1, 1, npix, -1)
    coord = torch.from_numpy(G2.make_2dcoord(16, 20)).cuda().flatten(0, 1)[:npix]
    w = torch.randn(nb, npix, 3, generator=g).cuda()

    def step(**how):
        extras = {"input_transforms": data["input_transforms"], "input_coord": data["input_coord"],
                  "target_transforms": data["target_transforms"][:, :1], "target_coord": coord[None, None].expand(nb, 1, -1, -1)}
        model.zero_grad(set_to_none=True)
        pix, _ = model(data["input_images"], data["input_camera_pos"], data["input_rays"], cam, rays, extras, **how)
        loss = (pix.reshape(nb, npix, 3).float() * w).sum()
        loss.backward()
        torch.cuda.synchronize()
        return pix.detach().clone(), loss.item()

    pix_v, loss_v = step(input_views=views, input_views_backward=True)
    ref = {"grad." + name: prm.grad.detach().cpu().numpy().copy() for name, prm in model.named_parameters()}
    pix_m, loss_m = step(input_mask=mask, input_mask_backward=True)
    assert torch.isfinite(pix_m).all() and torch.equal(pix_m, pix_v) and loss_m == loss_v, (loss_m, loss_v)
    worst = _srt_grad_check(model, ref, False)
    print(f"KEY_MASK_BWD srt: loss {loss_m} vs {loss_v}, worst relative rms {worst:.3e}")


def test_default_keyword_under_grad_is_still_forward_only():
    c = _case("clevrtr/gta", "dec", torch.bfloat16)
    q = c.dev[0].detach().clone().requires_grad_()
    with pytest.raises(native.GtaError, match="forward-only"):
        gta_amd.gta_attention(q, c.dev[1], c.dev[2], c.f_dims, c.packed, so3_degree=c.so3, trans_coeff=c.tc, scale=c.scale,
                              key_mask=_mask_set("random").cuda())

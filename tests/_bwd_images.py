"""The backward's workspace as an executable statement (test infrastructure; plain numpy / torch on the CPU, no GPU, no kernel output).  It extends
tests/_images.py (the K/V pre-pass) to what `gta_bwd_prep_kernel`, the dQ and dK/dV kernels and `gta_reduce_kernel` (gta_amd/csrc/gta_bwd.hip)
leave in the caller's workspace, written from the kernel sources:

  regions       gta_abi.cpp: bwd_layout -- [Q''/dO~ images | statistics | d trans_coeff partials | d tau partials | K'/V' images], each 256-byte
                aligned.  A query tile (b, h, j) is `stage` = nimg * 64 * dhp * 2 bytes at ((b * H + h) * n_qt + j) * stage: the images
                [Q'' | dO~], or [Q''hi | dO~hi | Q''lo | dO~lo] under GTA_FLAG_FP32_PRODUCTS, each swizzled as the forward's (tests/_images.py)
  statistics    128 fp32 per tile: [-lse * log2e of its 64 rows | -D of its 64 rows], D = <dout, out> (the DLSE entry: D - dlse)
  partials      dc[0 : n_prep) one per 64-row tile (pre-pass: the C_q term), dc[n_prep : n_prep + n_dq) one per 128 query rows (dQ epilogue: the
                A_q term), then n_dkv, one per 128 keys (dK/dV epilogue: the B_k terms of K and V); dt[0 : n_dq) one per 128 query rows (<q, dq>),
                written only when tau and dtau are given.  gta_reduce_kernel sums dc[0 : n_prep + n_dq + n_dkv) and dt[0 : n_dq)

`ref_bwd_prep` and `ref_walk_partials` are the fp64 values of all of it computed from the very fp32 tables and inputs the kernels read;
`emulate_prep` is the pre-pass in fp32 on the host (with switchable defects) and `check_workspace` holds every rule and bar the GPU tests
assert (tests/test_gpu_bwd_prep.py), so that tests/test_bwd_images_host.py can prove on the CPU that the bars catch what they are meant to."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import _images as I
from tests._images import BN, _align256, _mask, bf16_bits, bits_to_f32, padded_dh, split_hi_lo, ulp_bf16, unit_positions

VREP_INV = 0                                         # include/gta_hip.h: the slot of a packed view record the query side reads (E itself)
LOG2E32 = float(np.float32(1.4426950408889634))      # gta_bwd.hip: LOG2E
NEG_BIG = float(np.float32(-1e30))                   # the -lse of a row past Tq / the prefix
U24 = 2.0 ** -24
FILL = 0xFF


def qscale32(scale, tau=None):
    """the pre-pass's `p.scale * LOG2E / tau` with every operation in fp32, in that order"""
    s = np.float32(np.float32(scale) * np.float32(LOG2E32))
    return float(s if tau is None else np.float32(s / np.float32(tau)))


def bwd_layout(B, H, Tq, Tk, dh, x3=False):
    """gta_abi.cpp: bwd_layout"""
    dhp = padded_dh(dh)
    n_qt, n_kt = (Tq + 63) // 64, (Tk + 63) // 64
    n_q128, n_k128 = (Tq + 127) // 128, (Tk + 127) // 128
    nimg = 4 if x3 else 2
    stage = nimg * 64 * dhp * 2
    n_prep, n_dq, n_dkv = B * H * n_qt, B * H * n_q128, B * H * n_k128
    off_qimg = 0
    qimg_end = B * H * n_qt * stage
    off_stats = _align256(qimg_end)
    stats_end = off_stats + B * H * n_qt * 128 * 4
    off_dc = _align256(stats_end)
    dc_end = off_dc + (n_prep + n_dq + n_dkv) * 4
    off_dt = _align256(dc_end)
    dt_end = off_dt + n_dq * 4
    off_kv = _align256(dt_end)
    total = _align256(off_kv + B * H * n_kt * stage)
    return SimpleNamespace(B=B, H=H, Tq=Tq, Tk=Tk, dh=dh, dhp=dhp, chp=dhp // 8, x3=x3, nimg=nimg, img=64 * dhp * 2, stage=stage, n_qt=n_qt,
                           n_kt=n_kt, n_q128=n_q128, n_k128=n_k128, n_prep=n_prep, n_dq=n_dq, n_dkv=n_dkv, dc_total=n_prep + n_dq + n_dkv,
                           off_qimg=off_qimg, qimg_end=qimg_end, off_stats=off_stats, stats_end=stats_end, off_dc=off_dc, dc_end=dc_end,
                           off_dt=off_dt, dt_end=dt_end, off_kv=off_kv, total=total,
                           gaps=((qimg_end, off_stats), (stats_end, off_dc), (dc_end, off_dt), (dt_end, off_kv)))


def decode_bwd(ws, L):
    """workspace bytes (CPU uint8 tensor or array) -> q2, do (q_lo, do_lo under x3): fp32 [B,H,n_qt*64,dhp]; bits: the bf16 bits of every image in
    logical order, int16 [B,H,n_qt,nimg,64,dhp]; neg_lse2, neg_D: fp32 [B,H,n_qt*64] with stats_raw int32 [B,H,n_qt,2,64]; dc_prep [B,H,n_qt],
    dc_dq [B,H,n_q128], dc_dkv [B,H,n_k128], dt [B,H,n_q128] as fp32 with dc_raw / dt_raw their int32 words (an untouched 0xFF fill reads -1);
    gaps_keep_fill: every byte of the alignment gaps is 0xFF"""
    raw = np.ascontiguousarray(ws.numpy() if torch.is_tensor(ws) else ws).view(np.uint8).reshape(-1)
    assert raw.size >= L.off_kv, (raw.size, L.off_kv)
    B, H = L.B, L.H
    phys = raw[:L.qimg_end].view(np.int16).reshape(B, H, L.n_qt, L.nimg, BN, L.chp, 8)
    logical = phys[:, :, :, :, np.arange(BN)[:, None], unit_positions(L.chp), :]
    bits = torch.from_numpy(np.ascontiguousarray(logical)).reshape(B, H, L.n_qt, L.nimg, BN, L.dhp)
    f = bits_to_f32(bits)
    rows = lambda i: f[:, :, :, i].reshape(B, H, L.n_qt * BN, L.dhp)
    words = lambda a, b: torch.from_numpy(raw[a:b].copy().view(np.int32))
    stats_raw = words(L.off_stats, L.stats_end).reshape(B, H, L.n_qt, 2, BN)
    st = stats_raw.view(torch.float32)
    dc_raw, dt_raw = words(L.off_dc, L.dc_end), words(L.off_dt, L.dt_end)
    dc = dc_raw.view(torch.float32)
    return SimpleNamespace(q2=rows(0), do=rows(1), q_lo=rows(2) if L.x3 else None, do_lo=rows(3) if L.x3 else None, bits=bits,
                           neg_lse2=st[:, :, :, 0].reshape(B, H, -1), neg_D=st[:, :, :, 1].reshape(B, H, -1), stats_raw=stats_raw,
                           dc_raw=dc_raw, dt_raw=dt_raw, dc_prep=dc[:L.n_prep].reshape(B, H, L.n_qt),
                           dc_dq=dc[L.n_prep:L.n_prep + L.n_dq].reshape(B, H, L.n_q128), dc_dkv=dc[L.n_prep + L.n_dq:].reshape(B, H, L.n_k128),
                           dt=dt_raw.view(torch.float32).reshape(B, H, L.n_q128),
                           gaps_keep_fill=all(bool((raw[a:b] == FILL).all()) for a, b in L.gaps), layout=L)


def encode_bwd(L, bits, neg_lse2, neg_D, dc_prep, dc_dq, dc_dkv, dt=None):
    """the inverse of decode_bwd: image bits int16 [B,H,n_qt,nimg,64,dhp], the statistics [B,H,n_qt*64], the partials -> workspace bytes; what
    is not given (dt, the gaps, the K'/V' images) holds the 0xFF fill"""
    B, H = L.B, L.H
    out = np.full(L.total, FILL, dtype=np.uint8)
    logical = bits.reshape(B, H, L.n_qt, L.nimg, BN, L.chp, 8).numpy()
    phys = np.empty_like(logical)
    phys[:, :, :, :, np.arange(BN)[:, None], unit_positions(L.chp), :] = logical
    out[:L.qimg_end] = phys.reshape(-1).view(np.uint8)
    st = torch.stack([neg_lse2.float().reshape(B, H, L.n_qt, BN), neg_D.float().reshape(B, H, L.n_qt, BN)], 3).contiguous()
    out[L.off_stats:L.stats_end] = st.numpy().reshape(-1).view(np.uint8)
    dc = torch.cat([t.float().reshape(-1) for t in (dc_prep, dc_dq, dc_dkv)]).contiguous()
    assert dc.numel() == L.dc_total, (dc.numel(), L.dc_total)
    out[L.off_dc:L.dc_end] = dc.numpy().view(np.uint8)
    if dt is not None:
        out[L.off_dt:L.dt_end] = dt.float().contiguous().reshape(-1).numpy().view(np.uint8)
    return torch.from_numpy(out)


def _se3_blocks(f_dims):
    """first channel of every se3 block"""
    c0 = int(f_dims.get("triv", 0))
    return [c0 + 4 * i for i in range(int(f_dims.get("se3", 0)) // 4)]


def t_col(vrep, slot, T, N):
    """the UNMASKED translation column [0:3,3] of a record's 4x4 at `slot`, per token: fp64 [B,T,3] (stage_brec: BREC_T)"""
    B = vrep.shape[0]
    view = torch.arange(T) // (T // N)
    return vrep.to(torch.float32)[..., slot:slot + 16].reshape(B, N, 4, 4)[:, view, :3, 3].double()


def rho_q(tables, f_dims, Tq, Nq, so3_degree=0, trans_coeff=None):
    """the query side's row transform x -> M x as fp64 [B,Tq,dh,dh] and ident (the channels it leaves alone) from the packed fp32 tables vrep_q
    [B,Nq,72] and cs_q [B,Tq,d_so2/2,2]: what stage_brec (side 0) and the pre-pass's chunk bodies compute.  so3 (D1 / D2 slots) and so2
    (rot2_apply<false>) are the key side's rules on the query side's tables; the se3 block is A_q = (vrep_q[INV slot] . mask)^T, product in fp32."""
    M, _off, ident = I.rho_k({"vrep_k": tables.get("vrep_q"), "cs_k": tables.get("cs_q")}, f_dims, Tq, Nq, so3_degree, trans_coeff)
    blocks = _se3_blocks(f_dims)
    if blocks:
        vrep = tables["vrep_q"].to(torch.float32)
        B = vrep.shape[0]
        view = torch.arange(Tq) // (Tq // Nq)
        A = (vrep[..., VREP_INV:VREP_INV + 16].reshape(B, Nq, 4, 4) * _mask(trans_coeff)).double().transpose(-1, -2)[:, view]
        for c0 in blocks:
            M[:, :, c0:c0 + 4, c0:c0 + 4] = A
    return M, ident


def _apply(M, x):
    return torch.einsum("btij,bhtj->bhti", M, x.double())


def _row_mask(B, T, lens):
    """[B,1,T] bool: row t of scene b is inside its prefix"""
    m = torch.ones(B, 1, T, dtype=torch.bool)
    if lens is not None:
        for b, n in enumerate(lens):
            m[b, :, int(n):] = False
    return m


def _tiles(x, n):
    """[B,H,T] -> [B,H,ceil(T/n)]: sums over groups of n rows"""
    B, H, T = x.shape
    g = (T + n - 1) // n
    p = torch.zeros(B, H, g * n, dtype=x.dtype)
    p[:, :, :T] = x
    return p.reshape(B, H, g, n).sum(-1)


def ref_bwd_prep(q, dout, out, lse, tables, f_dims, Nq, so3_degree, trans_coeff, scale, tau=None, v_transform=True, dlse=None, q_lens=None):
    """fp64 of what the pre-pass writes for q, dout, out [B,H,Tq,dh] (fp32 masters already rounded to the input type; out and lse as the forward
    wrote them): q2 = rho_q q * qscale, do = rho_q dout (dout itself without v_transform) with absprod_q / absprod_do (sum_j |M_ij| |x_j|, q's
    times qscale) and ident_q / ident_do; neg_lse2, neg_D, sumabs_D [B,H,Tq]; dc, dc_sumabs [B,H,n_qt].  Rows at or past q_lens[b]: zero rows,
    statistics (-1e30f, 0), no term."""
    B, H, Tq, dh = q.shape
    M, ident = rho_q(tables, f_dims, Tq, Nq, so3_degree, trans_coeff)
    if M.shape[0] != B:
        M = M.expand(B, -1, -1, -1)
    qs = qscale32(scale, tau)
    valid = _row_mask(B, Tq, q_lens)
    v4 = valid[..., None]
    absap = lambda x: torch.einsum("btij,bhtj->bhti", M.abs(), x.double().abs())
    r = SimpleNamespace(qscale=qs, valid=valid, M=M)
    r.q2, r.absprod_q, r.ident_q = _apply(M, q) * qs * v4, absap(q) * qs, ident
    if v_transform:
        r.do, r.absprod_do, r.ident_do = _apply(M, dout) * v4, absap(dout), ident
    else:
        r.do, r.absprod_do, r.ident_do = dout.double() * v4, dout.double().abs(), torch.ones(dh, dtype=torch.bool)
    r.neg_lse2 = torch.where(valid, -(lse.double() * LOG2E32), torch.full((), NEG_BIG, dtype=torch.float64))
    prod = dout.double() * out.double()
    D = prod.sum(-1)
    r.neg_D = torch.where(valid, -(D - dlse.double()) if dlse is not None else -D, torch.zeros((), dtype=torch.float64))
    r.sumabs_D = prod.abs().sum(-1)
    term, sumabs = torch.zeros(B, H, Tq, dtype=torch.float64), torch.zeros(B, H, Tq, dtype=torch.float64)
    blocks = _se3_blocks(f_dims)
    if v_transform and blocks:
        t = t_col(tables["vrep_q"], VREP_INV, Tq, Nq)[:, None]                       # [B,1,Tq,3]
        for c0 in blocks:
            p3 = dout[..., c0:c0 + 3].double() * t * out[..., c0 + 3:c0 + 4].double()
            term += p3.sum(-1)
            sumabs += p3.abs().sum(-1)
    r.dc, r.dc_sumabs = _tiles(term * valid, 64), _tiles(sumabs * valid, 64)
    r.has_dc = bool(v_transform and blocks)
    return r


def prep_chain(dhp):
    """addends of the longest chain behind one pre-pass partial: a thread adds its 2 * dhp / 32 block terms (dhp / 32 chunks per wave, two se3
    blocks each), wg_sum256 adds 6 shuffle levels and 3 wave sums"""
    return 2 * (dhp // 32) + 9


def ref_walk_partials(q, k, v, dout, tables, f_dims, Nq, Nk, so3_degree, trans_coeff, scale, tau=None, v_transform=True, dlse=None,
                      key_lens=None, q_lens=None, emulate=None, out_dtype=torch.float32, out=None, lse=None):
    """Dense fp64 backward of the transformed problem -> the dQ, dK/dV and d tau terms per token, summed over the 128-row / 128-key groups the
    slots stand for: dq [B,H,n_q128] (with dq_blocks / dk_blocks, one per se3 block), dk, dv, dkv = dk + dv [B,H,n_k128], dt [B,H,n_q128].
    emulate=None: q', k', v', do~ from rho_q / rho_k, P from the fp64 softmax, dq', dk', dv' from torch autograd on those leaves.
    emulate="bf16" / "x3": the same formulas with Q'', K', V', dO~ rounded to bf16 (x3: to a hi + lo pair), P and dS rounded before their
    products: the measure of what the matrix products leave of a slot.  With `out` and `lse` (the arrays the backward call was handed: the
    forward's own) the emulation takes what the kernels take from them -- P = exp2(S2 - lse * log2e) and D = <dout, out> -- so a row's dS carries
    the common-mode error the forward's rounding leaves in them (gta_bwd.hip, the X3 dQ epilogue's comment: "D_i comes from the forward's o,
    lse2_i from the forward's row sums"); without them P is normalised by its own row sum and D comes from P V' rounded to `out_dtype`."""
    B, H, Tq, dh = q.shape
    Tk = k.shape[2]
    Mq, _ = rho_q(tables, f_dims, Tq, Nq, so3_degree, trans_coeff)
    Mk, _off, _ = I.rho_k(tables, f_dims, Tk, Nk, so3_degree, trans_coeff)
    qp, kp = _apply(Mq, q), _apply(Mk, k)
    vp = _apply(Mk, v) if v_transform else v.double()
    dop = _apply(Mq, dout) if v_transform else dout.double()
    vq, vk = _row_mask(B, Tq, q_lens)[..., None], _row_mask(B, Tk, key_lens)[:, :, None]      # [B,1,Tq,1], [B,1,1,Tk]
    dop = dop * vq
    tau_f = 1.0 if tau is None else float(tau)
    c1 = float(scale) / tau_f
    dl = None if dlse is None else dlse.double() * vq[..., 0]
    neg_inf = torch.full((), float("-inf"), dtype=torch.float64)
    if emulate is None:
        qp_l, kp_l, vp_l = (t.clone().requires_grad_() for t in (qp, kp, vp))
        S = torch.where(vk, c1 * qp_l @ kp_l.transpose(-1, -2), neg_inf)
        lse = torch.logsumexp(S, -1)
        loss = ((torch.exp(S - lse[..., None]) @ vp_l) * dop).sum()
        if dl is not None:
            loss = loss + (lse * dl).sum()
        dqp, dkp, dvp = torch.autograd.grad(loss, (qp_l, kp_l, vp_l))
    else:
        if emulate == "x3":
            rnd = lambda x: (lambda hl: hl[0].double() + hl[1].double())(split_hi_lo(x.float()))
        else:
            rnd = lambda x: x.float().to(torch.bfloat16).double()
        q2, kb, vb, dob = rnd(qp * (c1 * math.log2(math.e))), rnd(kp), rnd(vp), rnd(dop)
        S2 = torch.where(vk, q2 @ kb.transpose(-1, -2), neg_inf)
        if lse is not None:
            P = torch.exp2(S2 - (lse.double() * LOG2E32)[..., None])
        else:
            P = torch.exp2(S2 - S2.max(-1, keepdim=True).values)
            P = P / P.sum(-1, keepdim=True)
        Pb = rnd(P)
        D = (dout.double() * out.double()).sum(-1) * vq[..., 0] if out is not None else (dop * (Pb @ vb).to(out_dtype).double()).sum(-1)
        D = D - (dl if dl is not None else 0.0)
        dSb = rnd(P * (dob @ vb.transpose(-1, -2) - D[..., None]) * vq)
        dqp, dkp, dvp = c1 * dSb @ kb, math.log(2.0) * dSb.transpose(-1, -2) @ q2, (Pb * vq).transpose(-1, -2) @ dob
    r = SimpleNamespace(dq_blocks=[], dk_blocks=[], dqp=dqp, dkp=dkp, dvp=dvp)
    zq, zk = torch.zeros(B, H, Tq, dtype=torch.float64), torch.zeros(B, H, Tk, dtype=torch.float64)
    dk_t, dv_t = zk.clone(), zk.clone()
    blocks = _se3_blocks(f_dims)
    if blocks:
        tE = t_col(tables["vrep_q"], VREP_INV, Tq, Nq)[:, None]
        tEi = t_col(tables["vrep_k"], I.VREP_REP, Tk, Nk)[:, None]
        for c0 in blocks:
            r.dq_blocks.append(_tiles(dqp[..., c0 + 3] * (tE * q[..., c0:c0 + 3].double()).sum(-1) * vq[..., 0], 128))
            kb = (dkp[..., c0:c0 + 3] * tEi).sum(-1) * k[..., c0 + 3].double()
            r.dk_blocks.append(_tiles(kb * vk[:, :, 0], 128))
            dk_t = dk_t + kb
            if v_transform:
                dv_t = dv_t + (dvp[..., c0:c0 + 3] * tEi).sum(-1) * v[..., c0 + 3].double()
    vk_rows = vk[:, :, 0]                                                                      # [B,1,Tk]
    r.dq = sum(r.dq_blocks) if blocks else _tiles(zq, 128)
    r.dk, r.dv = _tiles(dk_t * vk_rows, 128), _tiles(dv_t * vk_rows, 128)
    r.dkv = r.dk + r.dv
    dq_raw = torch.einsum("btji,bhtj->bhti", Mq.expand(B, -1, -1, -1) if Mq.shape[0] != B else Mq, dqp)
    r.dt = _tiles((q.double() * dq_raw).sum(-1) * vq[..., 0], 128)
    return r


def walk_sigma(ref, emu, pairs=False):
    """RMS over the case's slots of the emulation minus the fp64 value, per slot family"""
    f = (lambda x: _pair(x)) if pairs else (lambda x: x)
    return {n: float((f(getattr(emu, n)) - f(getattr(ref, n))).pow(2).mean().sqrt()) for n in ("dq", "dkv", "dt")}


def _pair(x):
    """[B,H,n] -> [B,H,ceil(n/2)]: sums of the slot pairs (2i, 2i+1) a generated stream's workgroup owns"""
    return _tiles(x, 2)


def emulate_prep(q, dout, out, lse, tables, f_dims, Nq, so3_degree, trans_coeff, scale, tau=None, v_transform=True, x3=False, defect=None):
    """The pre-pass in fp32 on the host -> (bits int16 [B,H,n_qt,nimg,64,dhp], neg_lse2, neg_D [B,H,n_qt*64], dc [B,H,n_qt]), in the kernel's
    roundings but not its order within a dot product.  defect: None, or one of "truncate" (images cut to bf16 instead of rounded), "share" (the
    fourth wave's share of D dropped), "lo_unscaled" (x3: the lo image taken before the qscale product), "pad_row" (the first row past Tq not
    zeroed), "hi_block" (the term of a chunk's second se3 block dropped from the partial)."""
    B, H, Tq, dh = q.shape
    dhp, n_qt = padded_dh(dh), (Tq + 63) // 64
    M64, _ = rho_q(tables, f_dims, Tq, Nq, so3_degree, trans_coeff)
    M = M64.float().expand(B, -1, -1, -1)
    ap = lambda x: torch.einsum("btij,bhtj->bhti", M, x.float())
    qs = torch.tensor(qscale32(scale, tau), dtype=torch.float32)
    qt = ap(q)
    dt_ = ap(dout) if v_transform else dout.float()

    def pad(x):
        p = torch.zeros(B, H, n_qt * 64, dhp, dtype=torch.float32)
        p[:, :, :Tq, :dh] = x
        if defect == "pad_row" and Tq < n_qt * 64:
            p[:, :, Tq, :dh] = x[:, :, Tq - 1]
        return p
    cut = (lambda x: (x.contiguous().view(torch.int32) >> 16).to(torch.int16)) if defect == "truncate" else bf16_bits
    imgs = []
    for x, unscaled in ((pad(qt * qs), pad(qt)), (pad(dt_), pad(dt_))):
        hi = cut(x)
        imgs.append((hi, bf16_bits((unscaled if defect == "lo_unscaled" else x) - bits_to_f32(hi))))
    order = [imgs[0][0], imgs[1][0]] + ([imgs[0][1], imgs[1][1]] if x3 else [])
    bits = torch.stack([t.reshape(B, H, n_qt, 64, dhp) for t in order], 3)
    prod = torch.zeros(B, H, Tq, dhp, dtype=torch.float32)
    prod[..., :dh] = dout.float() * out.float()
    shares = [prod.reshape(B, H, Tq, dhp // 8, 8)[:, :, :, w::4].sum((-1, -2)) for w in range(4)]
    if defect == "share":
        shares[3] = torch.zeros_like(shares[3])
    neg_D = torch.zeros(B, H, n_qt * 64, dtype=torch.float32)
    neg_D[:, :, :Tq] = -((shares[0] + shares[1]) + (shares[2] + shares[3]))
    neg_lse2 = torch.full((B, H, n_qt * 64), NEG_BIG, dtype=torch.float32)
    neg_lse2[:, :, :Tq] = -(lse.float() * torch.tensor(LOG2E32, dtype=torch.float32))
    term = torch.zeros(B, H, Tq, dtype=torch.float32)
    if v_transform:
        for c0 in _se3_blocks(f_dims):
            if defect == "hi_block" and c0 % 8 == 4:
                continue
            t = t_col(tables["vrep_q"], VREP_INV, Tq, Nq).float()[:, None]
            term = term + (dout[..., c0:c0 + 3].float() * t).sum(-1) * out[..., c0 + 3].float()
    return bits, neg_lse2, neg_D, _tiles(term, 64)


def bwd_case(f_dims, so3_degree=0, dtype=torch.bfloat16, B=3, H=3, Nk=3, Pk=50, seed=0, Nq=0, Pq=0):
    """`key_side_case` plus a query side: q and dout [B,H,Tq,dh] (fp32 masters rounded to `dtype`, token-major storage) and the q-side tables.
    Nq = 0: self-attention (the query side's tables are the key side's); else a decoder-like query side of Nq views of Pq rows."""
    import gta_amd
    from oracle import gta_oracle as O
    c = I.key_side_case(f_dims, so3_degree, dtype, B, H, Nk, Pk, seed)
    g = torch.Generator().manual_seed(5000 + seed)
    c.cross = Nq > 0
    c.Nq, c.Pq = (Nq, Pq) if c.cross else (Nk, Pk)
    c.Tq = c.Nq * c.Pq
    if c.cross:
        ex = {"target_transforms": O.random_extrinsics(B, c.Nq, g), "target_coord": torch.rand(B, c.Nq, c.Pq, 2, generator=g)}
        c.reps = O.decoder_reps(c.ak, ex, c.reps)
        c.packed = {name: t.clone() for name, t in gta_amd.pack_reps(dict(c.reps), c.f_dims).items()}
    rnd = lambda t: t.to(dtype).to(torch.float32)
    c.q, c.dout = (rnd(torch.randn(B, c.Tq, H, c.dh, generator=g)).permute(0, 2, 1, 3) for _ in range(2))
    return c


# ---- the rules -------------------------------------------------------------------------------------------------------------------------------
def _where(idx, shape):
    """flat index into a [B,H,T,dh] tensor -> scene, head, tile, row and chunk as text"""
    b, h, t, ch = np.unravel_index(int(idx), shape)
    return f"scene {b} head {h} tile {t // 64} row {t % 64} (token {t}) chunk {ch // 8} channel {ch}"


def _worst(err, bar, sel=None):
    """(index, err - bar there) of the worst selected element; NaN counts as +inf"""
    ex = err - bar
    ex = torch.where(torch.isnan(ex), torch.full_like(ex, float("inf")), ex)
    if sel is not None:
        ex = torch.where(sel.expand_as(ex), ex, torch.full_like(ex, float("-inf")))
    i = int(ex.argmax())
    return i, ex.flatten()[i].item()


def check_workspace(name, d, ref, *, dh, q=None, dout=None, walk=None, emu=None, want_dt=False, pairs=(), exact_q_ident=True, dlse_abs=None,
                    lens=None, log=print):
    """Every rule of tests/test_gpu_bwd_prep.py's docstring on one decoded workspace `d` against ref = ref_bwd_prep(...) (and walk / emu =
    ref_walk_partials(...) without / with emulation, when the case runs the dense backward).  Returns the list of (rule, message) that failed
    -- empty when the workspace is right -- and logs one line of margins (the worst err / bar per rule).
    pairs: slot families ("dq", "dkv") a generated stream wrote (pair sums compared, odd slots exactly 0.0); lens: q_lens or None."""
    L = d.layout
    B, H, Tq, dhp = L.B, L.H, L.Tq, L.dhp
    fails, margins = [], {}
    bad = lambda rule, msg: fails.append((rule, f"{name}: [{rule}] {msg}"))
    if not d.gaps_keep_fill:
        bad("gap", "a byte of an alignment gap was written")
    rows = d.bits.permute(0, 1, 3, 2, 4, 5).reshape(B, H, L.nimg, L.n_qt * 64, dhp)              # [B,H,image,token,channel]
    valid = ref.valid                                                                              # [B,1,Tq]
    # zero rules
    for b in range(B):
        n = Tq if lens is None else int(lens[b])
        if not bool((rows[b, :, :, n:] == 0).all()):
            bad("zero", f"scene {b}: rows {n}..{L.n_qt * 64 - 1} are not zero rows in every image")
        if not bool((rows[b, :, :, :, dh:] == 0).all()):
            bad("zero", f"scene {b}: padded channels are not zero")
    # images
    err32 = lambda ap: 16.0 * U24 * ap
    v4 = valid[..., None]
    for i, (what, r64, ap, ident, src) in enumerate((("Q''", ref.q2, ref.absprod_q, ref.ident_q, q), ("dO~", ref.do, ref.absprod_do, ref.ident_do, dout))):
        hi_bits = rows[:, :, i, :Tq, :dh]
        hi = bits_to_f32(hi_bits)
        if src is not None and bool(ident.any()):
            x32 = src.float() * torch.tensor(ref.qscale, dtype=torch.float32) if i == 0 else src.float()
            if i == 1 or exact_q_ident:
                same = (hi_bits == bf16_bits(x32)) | ~v4 | ~ident
                if not bool(same.all()):
                    bad("ident", f"{what}: an untransformed element is not RNE of its fp32 value: {_where(int((~same).flatten().int().argmax()), tuple(r64.shape))}")
            else:       # (tau cases, should the device quotient differ in its last place: see the GPU module's docstring)
                w, ex = _worst((hi.double() - r64).abs(), ulp_bf16(r64) / 2 + 4.0 * U24 * r64.abs(), v4 & ident)
                if ex > 0:
                    bad("ident", f"{what}: {_where(w, tuple(r64.shape))}: excess {ex:.3e}")
        sel = (v4 & ~ident).expand_as(r64)
        if bool(sel.any()):
            bar = ulp_bf16(r64) / 2 + err32(ap)
            w, ex = _worst((hi.double() - r64).abs(), bar, sel)
            margins[f"{what} err/bar"] = float(((hi.double() - r64).abs() / bar)[sel].nan_to_num(nan=float("inf")).max())
            if ex > 0:
                bad("image", f"{what}: {_where(w, tuple(r64.shape))}: ref64 {r64.flatten()[w].item()!r} img {hi.flatten()[w].item()!r} absprod {ap.flatten()[w].item()!r} excess {ex:.3e}")
        if L.x3:
            lo = bits_to_f32(rows[:, :, 2 + i, :Tq, :dh])
            s = hi.double() + lo.double()
            bar = 2.0 ** -16 * r64.abs() + err32(ap)
            w, ex = _worst((s - r64).abs(), bar, v4)
            margins[f"{what} hi+lo err/bar"] = float(((s - r64).abs() / bar.clamp_min(1e-300))[v4.expand_as(r64)].nan_to_num(nan=float("inf")).max())
            if ex > 0:
                bad("hilo", f"{what}: {_where(w, tuple(r64.shape))}: ref64 {r64.flatten()[w].item()!r} hi+lo {s.flatten()[w].item()!r} excess {ex:.3e}")
    # statistics
    got_l, got_D = d.neg_lse2[:, :, :Tq].double(), d.neg_D[:, :, :Tq].double()
    bar_l = 4.0 * U24 * ref.neg_lse2.abs()
    w, ex = _worst((got_l - ref.neg_lse2).abs(), bar_l, valid)
    if ex > 0:
        bad("lse", f"flat row {w}: -lse*log2e {got_l.flatten()[w].item()!r} ref {ref.neg_lse2.flatten()[w].item()!r} excess {ex:.3e}")
    bar_D = (dhp / 4 + 4) * U24 * ref.sumabs_D + (U24 * dlse_abs if dlse_abs is not None else 0.0)
    w, ex = _worst((got_D - ref.neg_D).abs(), bar_D, valid)
    margins["D err/bar"] = float(((got_D - ref.neg_D).abs() / bar_D.clamp_min(1e-300))[valid.expand_as(got_D)].nan_to_num(nan=float("inf")).max())
    if ex > 0:
        bad("D", f"flat row {w}: -D {got_D.flatten()[w].item()!r} ref {ref.neg_D.flatten()[w].item()!r} excess {ex:.3e} bar {bar_D.flatten()[w].item():.3e}")
    pad = torch.ones(B, H, L.n_qt * 64, dtype=torch.bool)
    pad[:, :, :Tq] = ~valid.expand(B, H, Tq)
    big = torch.tensor(NEG_BIG, dtype=torch.float32).view(torch.int32)
    sr = d.stats_raw.permute(0, 1, 3, 2, 4).reshape(B, H, 2, L.n_qt * 64)
    if not (bool((sr[:, :, 0][pad] == big).all()) and bool((sr[:, :, 1][pad] == 0).all())):
        bad("stat-pad", "the statistics of a row past Tq / the prefix are not exactly (-1e30f, 0.0)")
    # the partials and the fill
    if not bool(torch.isfinite(d.dc_raw.view(torch.float32)).all()):
        bad("fill", f"d trans_coeff slots {torch.nonzero(~torch.isfinite(d.dc_raw.view(torch.float32))).flatten().tolist()[:8]} are not finite (of {L.dc_total}: {L.n_prep} pre-pass, {L.n_dq} dQ, {L.n_dkv} dK/dV)")
    if want_dt and not bool(torch.isfinite(d.dt).all()):
        bad("fill", "a d tau slot is not finite")
    if not want_dt and not bool((d.dt_raw == -1).all()):
        bad("fill", "the d tau region was written without tau and dtau")
    if ref.has_dc:
        bar = (prep_chain(dhp) + 8) * U24 * ref.dc_sumabs
        w, ex = _worst((d.dc_prep.double() - ref.dc).abs(), bar)
        margins["prep err/bar"] = float(((d.dc_prep.double() - ref.dc).abs() / bar.clamp_min(1e-300)).nan_to_num(nan=float("inf")).max())
        if ex > 0:
            bad("prep-partial", f"flat tile {w}: {d.dc_prep.flatten()[w].item()!r} ref {ref.dc.flatten()[w].item()!r} excess {ex:.3e}")
    elif not bool((d.dc_raw[:L.n_prep] == 0).all()):
        bad("prep-partial", "a pre-pass partial is not exactly 0.0 without V_TRANSFORM / an se3 slab")
    if walk is not None:
        sig = walk_sigma(walk, emu)
        sig_p = walk_sigma(walk, emu, pairs=True)
        for fam, got in (("dq", d.dc_dq), ("dkv", d.dc_dkv)) + ((("dt", d.dt),) if want_dt else ()):
            g, r = got.double(), getattr(walk, fam)
            s = sig[fam]
            if fam in pairs:
                n = g.shape[-1]
                if not bool((got[..., 1::2].contiguous().view(torch.int32) == 0).all()):
                    bad("walk", f"{fam}: the second slot of a generated stream's pair is not exactly 0.0")
                g, r, s = _pair(g), _pair(r), sig_p[fam]
            e = (g - r).abs()
            worst = float(e.nan_to_num(nan=float("inf")).max())
            margins[f"{fam} sigma"] = s
            margins[f"{fam} worst/sigma"] = worst / s if s > 0 else (0.0 if worst == 0 else float("inf"))
            if not worst <= 6.0 * s:
                i = int(e.nan_to_num(nan=float("inf")).argmax())
                bad("walk", f"{fam} slot {i}: got {g.flatten()[i].item()!r} ref {r.flatten()[i].item()!r} |diff| {worst:.3e} > 6 sigma, sigma {s:.3e}")
    log(f"BWD_PREP {name}: " + ", ".join(f"{k} {v:.3g}" for k, v in margins.items()) + (f" | FAILED {sorted({r for r, _ in fails})}" if fails else " | ok"))
    return fails


def check_reduce(name, d, dtc=None, dtau=None, tau=None, log=print):
    """d trans_coeff / d tau against the fp64 sum of the partials read back: judges gta_reduce_kernel alone.  Returns the failures."""
    fails = []
    for what, got, words, div in (("dtrans_coeff", dtc, d.dc_raw, None), ("dtau", dtau, d.dt_raw, tau)):
        if got is None:
            continue
        part = words.view(torch.float32).double()
        ref = float(part.sum()) if div is None else -float(part.sum()) / float(div)
        bar = (math.ceil(part.numel() / 1024) + 14) * U24 * float(part.abs().sum()) / (1.0 if div is None else float(div))
        err = abs(float(got) - ref)
        log(f"BWD_PREP {name}: reduce {what} over {part.numel()} slots: got {float(got)!r} ref {ref!r} err/bar {err / bar if bar > 0 else 0.0:.3g}")
        if not err <= bar:
            fails.append(("reduce", f"{name}: [reduce] {what}: got {float(got)!r}, the fp64 sum of the partials gives {ref!r} (bar {bar:.3e})"))
    return fails


# ---- the cases of tests/test_gpu_bwd_prep.py (here so that the host tests can prove the walk bars on the same shapes) -------------------------
def half(dh):
    """se3 | so2 halves, slabs rounded to multiples of 4"""
    se3 = int(round(dh / 2 / 4)) * 4
    return {"se3": se3, "so2": dh - se3}


MS96 = {"se3": 48, "so3": 24, "so2": 24}
BF16, FP32 = torch.bfloat16, torch.float32
dt_name = lambda dt: "bf16" if dt == torch.bfloat16 else "fp32"


def _cs(name, f, dtype, **kw):
    d = dict(name=name, f=f, so3=2 if "so3" in f else 0, dtype=dtype, shape={}, vt=True, tau=None, tc=0.37, flags=(), entry="bwd", x3=False, pairs=(),
             walk=True, key_lens=None, q_lens=None, seed=0)
    d.update(kw)
    return SimpleNamespace(**d)


def _cases():
    out = []
    for dt in (BF16, FP32):
        n = dt_name(dt)
        out += [_cs(f"dh{dh}-{n}", half(dh), dt) for dh in (32, 40, 64, 72, 96, 104, 128)]
        out += [_cs(f"ms96-{n}", MS96, dt), _cs(f"triv-{n}", {"triv": 8, "se3": 16, "so2": 8}, dt),
                _cs(f"mixed-halves-{n}", {"triv": 4, "se3": 12, "so2": 16}, dt), _cs(f"tau-{n}", half(64), dt, tau=0.8),
                _cs(f"dlse-{n}", half(64), dt, entry="dlse"), _cs(f"cross-{n}", half(64), dt, shape=dict(Nq=2, Pq=70), seed=1),
                _cs(f"varlen-{n}", half(64), dt, entry="varlen", key_lens=(150, 100, 37), q_lens=(150, 100, 37), seed=2)]
    out += [_cs("no-vt-bf16", half(64), BF16, vt=False), _cs("tc001-bf16", half(64), BF16, tc=0.01),
            _cs("varlen-noq-bf16", half(64), BF16, entry="varlen", key_lens=(150, 100, 37), seed=2),
            _cs("ms96-split", MS96, BF16, flags=("FLAG_BWD_SPLIT",)), _cs("ms96-keys32", MS96, BF16, flags=("FLAG_BWD_KEYS32",)),
            _cs("ms96-joint", MS96, BF16, shape=dict(B=4, H=2))]           # (n_dkv = 16: the compiled pair in ONE launch; the default shape's 18 is two)
    for views in (3, 2):
        for fl in ((), ("FLAG_BWD_SPLIT",)):
            out.append(_cs(f"stream-{views}x128" + ("-split" if fl else ""), MS96, BF16, shape=dict(B=1, H=2, Nk=views, Pk=128),
                           flags=("FLAG_BWD_KEYS64",) + fl, pairs=("dq", "dkv"), seed=3))
    for dh in (32, 40, 64):
        for tau in (None, 0.8):
            for entry in ("bwd", "dlse"):
                out.append(_cs(f"x3-dh{dh}" + ("-tau" if tau else "") + ("-dlse" if entry == "dlse" else ""), half(dh), FP32, x3=True, tau=tau,
                               entry=entry, seed=4))
    # gta_reduce_kernel's four-wide loop: dc_total = 2560 * 3 = 7680 (every thread makes the trip once, threads below 512 twice, the rest end in
    # the tail loop).  Two views of 32 rows, not one of 64: view 0 is the canonical identity, whose translation is zero -- every partial of a
    # one-view batch is 0.0 and the sum would prove nothing
    out.append(_cs("reduce-7680", half(32), BF16, shape=dict(B=40, H=64, Nk=2, Pk=32), tau=0.8, walk=False, seed=5))
    return {c.name: c for c in out}


CASES = _cases()


def case_inputs(cs):
    """the seeded inputs of a case, its dlse (or None) and scale"""
    c = bwd_case(cs.f, cs.so3, cs.dtype, seed=cs.seed, **cs.shape)
    c.scale = c.dh ** -0.5
    c.dlse = torch.randn(c.B, c.H, c.Tq, generator=torch.Generator().manual_seed(77)) if cs.entry == "dlse" else None
    c.tc = cs.tc if c.f_dims.get("se3", 0) > 0 else None
    return c


def case_refs(cs, c, out, lse):
    """ref_bwd_prep and, for the cases that run the dense backward, ref_walk_partials without and with emulation"""
    ref = ref_bwd_prep(c.q, c.dout, out, lse, c.packed, c.f_dims, c.Nq, c.so3, c.tc, c.scale, cs.tau, cs.vt, c.dlse, cs.q_lens)
    walk = emu = None
    if cs.walk:
        args = (c.q, c.k, c.v, c.dout, c.packed, c.f_dims, c.Nq, c.Nk, c.so3, c.tc, c.scale, cs.tau, cs.vt, c.dlse, cs.key_lens, cs.q_lens)
        walk = ref_walk_partials(*args)
        emu = ref_walk_partials(*args, emulate="x3" if cs.x3 else "bf16", out_dtype=cs.dtype, out=out, lse=lse)
    return ref, walk, emu

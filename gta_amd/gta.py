"""Functional GTA operator on MI355X -- host-side mirror of ``source/utils/gta.py``.

``multihead_geometric_transform_attention`` keeps the reference's name, argument meaning and
``reps`` dict contract (gta.py:92-279) but runs the whole operator as one fused HIP kernel.
What differs, deliberately:
  * the dense attention matrix is never formed, so the second return value is ``None``
    (the reference only consumes it under ``return_attmap``, layers.py:441-442);
  * ``attn_fn`` is accepted for signature compatibility; its ``scale`` attribute is honoured,
    the softmax itself is the kernel's.
"""
from __future__ import annotations

import weakref
from collections import namedtuple
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import native
from . import repgrad as _repgrad

GROUP_ORDER = ("triv", "se3", "so3", "so2", "t2")   # gta.py:115


def make_2dcoord(H: int, W: int) -> np.ndarray:
    """[H, W, 2] with entry (i, j) = (i/H, j/W)   (gta.py:9-16)."""
    r = np.arange(H, dtype=np.float32) / H
    c = np.arange(W, dtype=np.float32) / W
    rr, cc = np.meshgrid(r, c, indexing="ij")
    return np.stack([rr, cc], -1)


def make_SO2mats(coord: torch.Tensor, nfreqs: int, max_freqs=(1, 1), shared_freqs: bool = False) -> torch.Tensor:
    """[..., F, 2, 2, 2] rotation blocks like gta.py:47-69, built from the device (cos,sin) table."""
    lead = coord.shape[:-1]
    cs = native.build_so2_table(coord.reshape(1, -1, 2), nfreqs, max_freqs[0], max_freqs[1], shared_freqs)
    c, s = cs[0, ..., 0], cs[0, ..., 1]                       # [T, 2F]
    m = torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)   # [T, 2F, 2, 2]
    return m.reshape(*lead, nfreqs, 2, 2, 2)


# --------------------------------------------------------------------------------------------
# reps: reference-style dict  ->  packed device tables the kernels read
# --------------------------------------------------------------------------------------------
def _pack_view(inv: Optional[torch.Tensor], rep: Optional[torch.Tensor], Ds) -> torch.Tensor:
    ref = inv if inv is not None else (rep if rep is not None else Ds[0])
    B, N = ref.shape[:2]
    if native.wants_grad(inv, rep):
        # built with torch ops so that the table's gradient (E / inv(E) slots) reaches the dense tensors; the D slots stay detached
        z = torch.zeros(B, N, 16, device=ref.device, dtype=torch.float32)
        tail = torch.zeros(B, N, native.VREP_STRIDE - 32, device=ref.device, dtype=torch.float32)
        if Ds:
            tail[..., native.VREP_D1 - 32:native.VREP_D1 - 23] = Ds[0].detach().reshape(B, N, 9)
            if len(Ds) > 1:
                tail[..., native.VREP_D2 - 32:native.VREP_D2 - 7] = Ds[1].detach().reshape(B, N, 25)
        return torch.cat([z if inv is None else inv.reshape(B, N, 16).float(), z if rep is None else rep.reshape(B, N, 16).float(), tail], -1)
    out = torch.zeros(B, N, native.VREP_STRIDE, device=ref.device, dtype=torch.float32)
    if inv is not None:
        out[..., native.VREP_INV:native.VREP_INV + 16] = inv.detach().reshape(B, N, 16)
    if rep is not None:
        out[..., native.VREP_REP:native.VREP_REP + 16] = rep.detach().reshape(B, N, 16)
    if Ds:
        out[..., native.VREP_D1:native.VREP_D1 + 9] = Ds[0].detach().reshape(B, N, 9)
        if len(Ds) > 1:
            out[..., native.VREP_D2:native.VREP_D2 + 25] = Ds[1].detach().reshape(B, N, 25)
    return out


def _pack_so2(rep: torch.Tensor) -> torch.Tensor:
    """[B,T,C,2,2] rotation blocks -> [B,T,C,2] (cos, sin) = (M[0,0], M[1,0])."""
    return torch.stack([rep[..., 0, 0], rep[..., 1, 0]], -1).detach().to(torch.float32).contiguous()


def _src_key(*tensors):
    """Identity of the tensors a packed table was built from: storage address, shape and in-place version counter
    (``id()`` can alias after garbage collection; a tensor replaced by the decoder changes at least the address)."""
    out = []
    for t in tensors:
        if torch.is_tensor(t):
            out.append((t.data_ptr(), tuple(t.shape), t._version))
        elif isinstance(t, (list, tuple)):
            out.append(tuple((u.data_ptr(), tuple(u.shape), u._version) for u in t))
        else:
            out.append(None)
    return tuple(out)


def _flat(sources):
    """the tensors among a table's sources (lists of tensors flattened, None dropped)"""
    out = []
    for t in sources:
        if torch.is_tensor(t):
            out.append(t)
        elif isinstance(t, (list, tuple)):
            out.extend(u for u in t if torch.is_tensor(u))
    return out


def pack_reps(reps: dict, f_dims: dict) -> dict:
    """Return (and cache in ``reps``) the packed tables for a reference-style ``reps`` dict.

    Accepts either the packed keys written by ``gta_amd.reps.pre_compute_reps_*``
    (``gta_vrep_q/k``, ``gta_cs_q/k``, ``gta_coord_q/k``) or the reference's own tensors (``se3rep_q/k``,
    ``inv_se3rep_q``, ``so3rep_q/k`` lists, ``so2rep_q/k``, ``t2rep_q/k``; encoder.py:197,208-215,235-236,259).
    A table packed from reference tensors is tied to them (``*_src``): when the decoder replaces the q side of the
    shared dict (decoder.py:283-311), the table is rebuilt -- for all three kinds.

    Reference tensors that require grad (poses, coordinates as autograd leaves): the view table is built with torch ops and never
    cached (a cached one would belong to an earlier graph); the dense so2 / t2 tensors the operator applies are handed on as
    ``grad_cs_*`` / ``grad_coord_*`` so that the backward returns their gradient in their own shape (gta_amd.repgrad).
    """
    need_view = f_dims.get("se3", 0) > 0 or f_dims.get("so3", 0) > 0
    need_so2 = f_dims.get("so2", 0) > 0
    out = {}

    def cached(key, sources, build):
        # tables written by gta_amd.reps carry no *_src: they are authoritative
        if key in reps and (key + "_src") not in reps:
            return reps[key]
        src = _src_key(*sources)
        # (address, shape, version) alone can alias: the caching allocator hands a freed block to the next tensor of the same
        # shape, at version 0.  The table therefore also holds WEAK references to its source tensors -- a dead one, or one that
        # is not the tensor now in the dict, forces a rebuild.
        alive = reps.get(key + "_ref")
        same = alive is not None and len(alive) == len(_flat(sources)) and all(r() is t for r, t in zip(alive, _flat(sources)))
        if key not in reps or reps.get(key + "_src") != src or not same:
            reps[key] = build()
            reps[key + "_src"] = src
            reps[key + "_ref"] = tuple(weakref.ref(t) for t in _flat(sources))
        return reps[key]

    if need_view:
        for side in ("q", "k"):
            inv = reps.get("inv_se3rep_q") if side == "q" else None
            rep, so3 = reps.get(f"se3rep_{side}"), reps.get(f"so3rep_{side}")
            Ds = list(so3 or []) if f_dims.get("so3", 0) > 0 else []
            if native.wants_grad(inv, rep):
                out[f"vrep_{side}"] = _pack_view(inv, rep, Ds)
            else:
                out[f"vrep_{side}"] = cached(f"gta_vrep_{side}", (rep, inv, so3), lambda: _pack_view(inv, rep, Ds))
    if f_dims.get("t2", 0) > 0:
        # make_T2mats (gta.py:72-89): T = [[1,0,0],[0,1,0],[cx,cy,1]] -> the kernel wants (cx, cy) per token
        for side in ("q", "k"):
            T = reps.get(f"t2rep_{side}")
            out[f"coord_{side}"] = cached(
                f"gta_coord_{side}", (T,),
                lambda: torch.stack([T[..., 2, 0], T[..., 2, 1]], -1).detach().float().contiguous())
            # the operator applies inv_t2rep_q on the q side and t2rep_k on the k side (gta.py:221-238,272-274)
            src = reps.get("inv_t2rep_q") if side == "q" else T
            if native.wants_grad(src):
                out[f"grad_coord_{side}"] = src
    if need_so2:
        for side in ("q", "k"):
            R = reps.get(f"so2rep_{side}")
            out[f"cs_{side}"] = cached(f"gta_cs_{side}", (R,), lambda: _pack_so2(R))
            if native.wants_grad(R):
                out[f"grad_cs_{side}"] = R
    return out


def _so3_degree(f_dims: dict, packed: dict, reps: dict) -> int:
    if f_dims.get("so3", 0) <= 0:
        return 0
    if "gta_so3_degree" in reps:
        return int(reps["gta_so3_degree"])
    return len(reps["so3rep_q"])


def _views(f_dims, packed, q, k) -> Tuple[int, int]:
    if "vrep_q" in packed:
        return packed["vrep_q"].shape[1], packed["vrep_k"].shape[1]
    return 1, 1


# --------------------------------------------------------------------------------------------
# autograd wrapper around the C ABI
# --------------------------------------------------------------------------------------------
def _as_kernel_layout(t: torch.Tensor) -> torch.Tensor:
    """[B,H,T,dh] view usable by the kernel as is (unit channel stride, 16-B aligned rows)."""
    return t if _kernel_layout_ok(t) else t.contiguous()


def _kernel_layout_ok(t: torch.Tensor) -> bool:
    """unit channel stride, 16-B aligned base and row strides: what the kernels read (and write) a [B,H,T,dh] view as"""
    esz = t.element_size()
    return t.stride(3) == 1 and t.data_ptr() % 16 == 0 and all((s * esz) % 16 == 0 for s in t.stride()[:3])


def _check_tables(q, k, f_dims, Nq, Nk, vrep_q, vrep_k, cs_q, cs_k, coord_q, coord_k, tc, ta, k_side=True):
    """Shape / dtype / device validation of everything that reaches the kernels as a raw pointer."""
    B, _, Tq, _ = q.shape
    Tk = k.shape[2]
    dev = q.device
    if f_dims.get("se3", 0) > 0 or f_dims.get("so3", 0) > 0:
        native.check_table("vrep_q", vrep_q, (B, Nq, native.VREP_STRIDE), dev)
        native.check_table("vrep_k", vrep_k, (B, Nk, native.VREP_STRIDE), dev, allow_none=not k_side)
    if f_dims.get("so2", 0) > 0:
        native.check_table("cs_q", cs_q, (B, Tq, f_dims["so2"] // 2, 2), dev)
        native.check_table("cs_k", cs_k, (B, Tk, f_dims["so2"] // 2, 2), dev, allow_none=not k_side)
    if f_dims.get("t2", 0) > 0:
        native.check_table("coord_q", coord_q, (B, Tq, 2), dev)
        native.check_table("coord_k", coord_k, (B, Tk, 2), dev, allow_none=not k_side)
    native.check_scalar("trans_coeff", tc, dev)
    native.check_scalar("tau", ta, dev)


# what a forward entry is called with: q, k, v as the kernels read them, out ([B,H,Tq,dh] view of [B,Tq,H,dh] memory, so the caller's
# 'b h n d -> b n (h d)' is a free view), the LSE, trans_coeff / tau as detached flat fp32 tensors (or None) and the descriptor
_Call = namedtuple("_Call", "q k v out lse tc ta desc")


def _setup_call(q, k, v, f_dims, so3_degree, Nq, Nk, scale, flags, tables, trans_coeff, tau, *, k_side=True, kernel_layout=True) -> _Call:
    """The host work in front of every forward entry: dtype check and coercion, kernel layout (skipped by ``_GenericAttn``, whose rho-apply
    kernels take any strides with unit channel stride), output buffers, descriptor, and the validation of everything that reaches the kernels
    as a raw pointer.  ``tables``: dict of the packed rep tables; ``k_side=False`` lets the key-side ones be absent (pretransformed)."""
    dt = q.dtype
    if dt not in (torch.float32, torch.bfloat16):
        raise native.GtaError(f"unsupported dtype {dt}: use float32 or bfloat16")
    k, v = k.to(dt), v.to(dt)
    if kernel_layout:
        q, k, v = _as_kernel_layout(q), _as_kernel_layout(k), _as_kernel_layout(v)
    B, H, Tq, dh = q.shape
    out = torch.empty(B, Tq, H, dh, device=q.device, dtype=dt).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, Tq, device=q.device, dtype=torch.float32)
    tc = trans_coeff.detach().to(torch.float32).reshape(-1) if torch.is_tensor(trans_coeff) else None
    ta = tau.detach().to(torch.float32).reshape(-1) if torch.is_tensor(tau) else None
    desc = native.make_desc(q, k, v, out, f_dims, so3_degree, Nq, Nk, scale, flags)
    _check_tables(q, k, f_dims, Nq, Nk, tables.get("vrep_q"), tables.get("vrep_k"), tables.get("cs_q"), tables.get("cs_k"),
                  tables.get("coord_q"), tables.get("coord_k"), tc, ta, k_side=k_side)
    return _Call(q, k, v, out, lse, tc, ta, desc)


def _scalar_meta(t):
    """(shape, dtype) of the trans_coeff / tau parameter a Function was given, None without one"""
    return (t.shape, t.dtype) if torch.is_tensor(t) else None


def _restore_scalar(grad, meta):
    """the kernels' flat fp32 d trans_coeff / d tau in the parameter's own shape and dtype"""
    return None if grad is None or meta is None else grad.reshape(meta[0]).to(meta[1])


def _layout_flags(v_transform: bool, euclid: bool) -> int:
    return (native.FLAG_V_TRANSFORM if v_transform else 0) | (native.FLAG_EUCLID if euclid else 0)


class _SplitPacked(torch.autograd.Function):
    """[B,T,n,H,dh] packed projection -> n strided [B,H,T,dh] views (layers.py:389,394-395), whose backward hands the
    attention backward's packed gradient buffer straight through (``backward._grad_buffers``) instead of letting autograd
    assemble it from three zero-filled scatters and two adds."""

    @staticmethod
    def forward(ctx, packed):
        ctx.pshape = packed.shape
        return tuple(packed[:, :, i].permute(0, 2, 1, 3) for i in range(packed.shape[2]))

    @staticmethod
    def backward(ctx, *grads):
        from .backward import packed_slices
        base = getattr(grads[0], "_base", None) if grads[0] is not None else None
        if (base is not None and all(g is not None and getattr(g, "_base", None) is base for g in grads)
                and tuple(base.shape) == tuple(ctx.pshape) and base.is_contiguous() and packed_slices(grads)):
            return base
        B, T, n, H, dh = ctx.pshape
        ref = next(g for g in grads if g is not None)
        out = torch.empty(ctx.pshape, device=ref.device, dtype=ref.dtype)
        for i, g in enumerate(grads):
            if g is None:
                out[:, :, i].zero_()
            else:
                out[:, :, i].copy_(g.permute(0, 2, 1, 3))
        return out


def split_packed(packed: torch.Tensor):
    """``packed`` [B,T,n,H,dh] -> n views [B,H,T,dh] (no copy in either direction when the consumer is ``gta_attention``)."""
    return _SplitPacked.apply(packed)


def _none_to_zero(dout, like):
    """the gradient of an output the loss did not use (``set_materialize_grads(False)``: None) as zeros of ``like``'s shape, dtype and memory"""
    return torch.zeros_like(like) if dout is None else dout


class _GenericAttn(torch.autograd.Function):
    """Ablation layouts the fused kernels refuse (t2 slab, so3 degree 1, unaligned slabs, euclid similarity):
    generic rho-apply kernels (gta_rep_apply) around the plain attention kernel, and for the backward their
    adjoints (gta_rep_apply_bwd) around the fused backward on an identity layout."""

    @staticmethod
    def forward(ctx, *args):
        return _GenericAttn._run(ctx, *args)[0]

    @staticmethod
    def backward(ctx, dout):
        return _GenericAttn._grads(ctx, dout)

    @staticmethod
    def _run(ctx, q, k, v, trans_coeff, tau, cfg, packed, *carriers):
        f_dims, so3_degree, scale, v_transform, euclid, precise = cfg
        flags = _layout_flags(v_transform, euclid)
        if q.dtype not in (torch.float32, torch.bfloat16):
            raise native.GtaError(f"unsupported dtype {q.dtype}")
        c = _setup_call(q, k, v, f_dims, so3_degree, *_views(f_dims, packed, q, k), scale, flags, packed, trans_coeff, tau, kernel_layout=False)
        k, v, out, lse, tc, ta, desc = c.k, c.v, c.out, c.lse, c.tc, c.ta, c.desc
        dt = q.dtype
        B, H, Tq, dh = q.shape
        Tk = k.shape[2]
        dhp = (dh + 7) // 8 * 8                                    # the attention kernel works on 8-channel chunks
        # (every kernel below writes all dh channels of every row: only PADDING channels need the zero fill -- 6 us + a launch boundary per buffer)
        alloc = torch.zeros if dhp != dh else torch.empty
        mk = lambda T: alloc(B, T, H, dhp, device=q.device, dtype=dt).permute(0, 2, 1, 3)
        qp, kp, vp, op = mk(Tq), mk(Tk), mk(Tk), mk(Tq)
        pitch = (Tk + 63) // 64 * 64
        kbias = torch.zeros(B, H, pitch, device=q.device, dtype=torch.float32) if euclid else None
        vq, vk = packed.get("vrep_q"), packed.get("vrep_k")
        native.rep_apply(desc, 0, q, vq, packed.get("cs_q"), packed.get("coord_q"), tc, qp[..., :dh])
        native.rep_apply(desc, 1, k, vk, packed.get("cs_k"), packed.get("coord_k"), tc, kp[..., :dh], kbias, scale)
        if v_transform:
            native.rep_apply(desc, 1, v, vk, packed.get("cs_k"), packed.get("coord_k"), tc, vp[..., :dh])
        else:
            vp[..., :dh] = v
        pdesc = native.make_desc(qp, kp, vp, op, {"triv": dhp}, 0, 1, 1, scale, native.FLAG_FP32_PRODUCTS if precise else 0)
        native.attn_fwd_plain(pdesc, qp, kp, vp, kbias, ta, op, lse)
        if v_transform:
            native.rep_apply(desc, 2, op[..., :dh], vq, packed.get("cs_q"), packed.get("coord_q"), tc, out)
        else:
            out.copy_(op[..., :dh])
        ctx.cfg, ctx.packed, ctx.flags = cfg, packed, flags
        ctx.tc_meta, ctx.tau_meta = _scalar_meta(trans_coeff), _scalar_meta(tau)
        ctx.carriers = _repgrad.carrier_meta(carriers)
        ctx.save_for_backward(q, k, v, qp, kp, vp, op, lse, tc, ta)
        return out, lse

    @staticmethod
    def _grads(ctx, dout, dlse=None):
        # dlse (``_GenericAttnLse``): the gradient of the plain attention's lse -- rho touches neither the logits nor lse, so it enters the plain
        # backward alone; under euclid the augmented channels carry the key bias, the logits and so lse are those of the forward
        from . import backward as _bw
        q, k, v, qp, kp, vp, op, lse, tc, ta = ctx.saved_tensors
        f_dims, so3_degree, scale, v_transform, euclid, _precise = ctx.cfg
        packed = ctx.packed
        want_dtau = ta is not None and ctx.needs_input_grad[4]
        dt = q.dtype
        B, H, Tq, dh = q.shape
        Tk = k.shape[2]
        dhp = qp.shape[-1]
        Nq, Nk = _views(f_dims, packed, q, k)
        desc = native.make_desc(q, k, v, q, f_dims, so3_degree, Nq, Nk, scale, ctx.flags)
        vq, vk = packed.get("vrep_q"), packed.get("vrep_k")
        # buffers the kernels write in full are not zero-filled (padding channels -- d > dh -- are); the per-row d trans_coeff terms of the four adjoints
        # share ONE buffer, summed once in fp64 (four separate reductions were 110 us of the fp32-faithful backward at the CLEVR shape)
        mk = lambda T, d=dhp: (torch.zeros if d != dh else torch.empty)(B, T, H, d, device=q.device, dtype=dt).permute(0, 2, 1, 3)
        need_tc = f_dims.get("se3", 0) > 0 and ctx.tc_meta is not None
        n_rq, n_rk = B * H * Tq, B * H * Tk
        n_rows = (n_rq + n_rk + (n_rk + n_rq if v_transform else 0)) if need_tc else 0
        row_buf = torch.empty(n_rows, device=q.device, dtype=torch.float32) if need_tc else None
        row_at = [0]

        def rows(T):
            a = row_at[0]
            row_at[0] = a + B * H * T
            return row_buf[a:row_at[0]].view(B, H, T)
        dout = dout.to(dt)
        # o = rho2(o~)  ->  do~ = rho2^T do
        dop = mk(Tq)
        r_o = rows(Tq) if (need_tc and v_transform) else None
        if v_transform:
            native.rep_apply_bwd(desc, 2, op[..., :dh], dout, vq, packed.get("cs_q"), packed.get("coord_q"), tc,
                                 dop[..., :dh], r_o)
        else:
            dop[..., :dh] = dout
        # plain attention backward on the padded identity layout.  euclid_sim: the key bias -s|k'|^2/2 of the forward
        # is carried by two spare channels, q' = (.., 1, 1), k' = (.., hi, lo) with hi + lo = -|k'|^2/2 split so that
        # bf16 keeps it to 2^-16 -- the same logits, no bias operand in the backward kernels; the gradient of the
        # bias comes back as dk'[hi channel] and is folded in by the adjoint below.
        dbias = None
        if euclid:
            dhp2 = (dh + 2 + 31) // 32 * 32
            grow = lambda x_, T: torch.cat([x_[..., :dh], torch.zeros(B, H, T, dhp2 - dh, device=q.device, dtype=dt)], -1)
            qp, kp, vp, op, dop = grow(qp, Tq), grow(kp, Tk), grow(vp, Tk), grow(op, Tq), grow(dop, Tq)
            bias = -0.5 * kp[..., :dh].float().pow(2).sum(-1)                         # [B,H,Tk]
            hi = bias.to(dt)
            qp[..., dh:dh + 2] = 1.0
            kp[..., dh] = hi
            kp[..., dh + 1] = (bias - hi.float()).to(dt)
            as_rows = lambda x_: x_.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)   # [B,T,H,d] memory like the kernels' outputs
            qp, kp, vp, op, dop = as_rows(qp), as_rows(kp), as_rows(vp), as_rows(op), as_rows(dop)
            dhp = dhp2
        pcfg = ({"triv": dhp}, 0, 1, 1, scale, 0)
        # (with the bias in the augmented channels, <q', dq'> also carries the bias part of d tau)
        if _precise and dt == torch.float32 and dlse is not None:
            raise native.GtaError("return_lse: the exact-fp32 backward (gta_attn_bwd_plain_f32) takes no gradient of the log-sum-exp")
        if _precise and dt == torch.float32:
            # fp32-faithful mode: exact-fp32 products and sums (gta_plain32.hip) -- the gradients of the reference's fp32 autograd
            dqp, dkp, dvp = mk(Tq, dhp), mk(Tk, dhp), mk(Tk, dhp)
            pdesc = native.make_desc(qp, kp, vp, op, {"triv": dhp}, 0, 1, 1, scale, 0)
            native.attn_bwd_plain_f32(pdesc, qp, kp, vp, op, dop, lse, ta, dqp, dkp, dvp)
            # dL/dtau = -(1/tau) sum_i <q'_i, dq'_i>  (the kernels of the default mode form it in their epilogue)
            dta = (-(qp.double() * dqp.double()).sum() / ta.double()).float().reshape(1) if (want_dtau and ta is not None) else None
        else:
            dqp, dkp, dvp, _, dta = _bw.attn_bwd(pcfg, qp, kp, vp, op, dop, lse, None, ta, None, None, None, None,
                                                 want_dtau=want_dtau, dlse=dlse)
        dta = _restore_scalar(dta, ctx.tau_meta)
        if euclid:
            pitch = (Tk + 63) // 64 * 64
            dbias = torch.zeros(B, H, pitch, device=q.device, dtype=torch.float32)
            dbias[..., :Tk] = dkp[..., dh].float()
        dq, dk, dv = mk(Tq, dh), mk(Tk, dh), mk(Tk, dh)
        r_q, r_k = (rows(Tq), rows(Tk)) if need_tc else (None, None)
        r_v = rows(Tk) if (need_tc and v_transform) else None
        native.rep_apply_bwd(desc, 0, q, dqp[..., :dh], vq, packed.get("cs_q"), packed.get("coord_q"), tc, dq, r_q)
        native.rep_apply_bwd(desc, 1, k, dkp[..., :dh], vk, packed.get("cs_k"), packed.get("coord_k"), tc, dk, r_k,
                             dkey_bias=dbias, bias_scale=1.0)
        if v_transform:
            native.rep_apply_bwd(desc, 1, v, dvp[..., :dh], vk, packed.get("cs_k"), packed.get("coord_k"), tc, dv, r_v)
        else:
            dv.copy_(dvp[..., :dh])
            r_v = None
        dtc = None
        if need_tc:
            assert row_at[0] == n_rows
            dtc = _restore_scalar(row_buf.sum(dtype=torch.float64), ctx.tc_meta)
        grads = ()
        if ctx.carriers:
            # gradients of the tables, in the transformed space: (q, dq'), (dout, o~) and (dk', k), (dv', v) (gta_amd/repgrad.py); under
            # euclid dk' is the total one, with the key bias -|k'|^2/2 folded in as the adjoint above does (dy - dbias y)
            meta = tuple(m if need else None for m, need in zip(ctx.carriers, ctx.needs_input_grad[7:]))
            dqt, opt, dvt = dqp[..., :dh], op[..., :dh], dvp[..., :dh]
            dkt = (dkp[..., :dh].float() - dbias[..., :Tk, None] * kp[..., :dh].float()).to(dt) if euclid else dkp[..., :dh]
            do = dout if dout.stride(3) == 1 else dout.contiguous()
            qpairs = ((q, dqt), (do, opt))[:1 + bool(v_transform)]
            kpairs = ((dkt, k), (dvt, v))[:1 + bool(v_transform)]
            qview = ((dqt, q), (do, opt))[:1 + bool(v_transform)] if euclid else None
            grads = tuple(_repgrad.table_grads(desc, packed, meta, tc, qpairs, kpairs, direct=True, euclid=euclid, q_view_pairs=qview))
        return (dq, dk, dv, dtc, dta, None, None) + grads


class _GenericAttnLse(torch.autograd.Function):
    """``_GenericAttn`` -> (out, lse), both differentiable (``return_lse``; default arithmetic): see ``_FusedAttnLse``"""

    @staticmethod
    def forward(ctx, *args):
        ctx.set_materialize_grads(False)
        return _GenericAttn._run(ctx, *args)

    @staticmethod
    def backward(ctx, dout, dlse):
        q = ctx.saved_tensors[0]
        if dout is None:
            dout = torch.zeros(q.shape, device=q.device, dtype=q.dtype)
        return _GenericAttn._grads(ctx, dout, dlse)


def _generic_forward(q, k, v, f_dims, packed, so3_degree, trans_coeff, tau, scale, v_transform, euclid, precise=False, carriers=(),
                     return_lse=False):
    """Generic path entry (forward + backward through _GenericAttn); ``return_lse``: -> (out, lse) through _GenericAttnLse."""
    tc = trans_coeff if torch.is_tensor(trans_coeff) else None
    ta = tau if torch.is_tensor(tau) else None
    fn = _GenericAttnLse if return_lse else _GenericAttn
    return fn.apply(q, k, v, tc, ta, (f_dims, so3_degree, scale, v_transform, euclid, precise), packed, *carriers)


_NO_GATHER_PREPASS = ("key_mask: the staged and rho-apply layouts (t2, euclid, so3 of degree 1, unaligned slabs) have no gather "
                      "pre-pass: ")


def _probe(dtype, q_shape, Tk: int, f_dims, so3_degree: int, Nq: int, Nk: int, flags: int):
    """the descriptor the routes ask the library about: the call's sizes at contiguous strides"""
    B, H, Tq, dh = q_shape
    qs, ks = (H * Tq * dh, Tq * dh, dh), (H * Tk * dh, Tk * dh, dh)
    return native.make_desc_from(dtype, q_shape, Tk, (qs, ks, ks, qs), f_dims, so3_degree, Nq, Nk, 1.0, flags)


def generic_route(q_shape, Tk: int, dtype, f_dims: Dict[str, int], so3_degree: int, Nq: int, Nk: int, *, v_transform: bool = True,
                  euclid: bool = False, precise: bool = False, needs_grad: bool = False, key_views: bool = False,
                  key_views_backward: bool = False, key_mask_generic: bool = False) -> str:
    """How ``gta_attention`` runs a call that ``attention_route`` hands to the generic path (it answered None):
    'staged' = the staged generic forward (``gta_attn_fwd_staged``: K/V pre-pass + one attention kernel, honours ``kv_cache``) when the
               library serves the descriptor, no gradient is needed and the arithmetic is the default one;
    'apply'  = ``_GenericAttn``: the rho-apply kernels around the plain attention kernel, with their adjoints for the backward.
    Sizes alone decide, as in ``attention_route`` (the descriptor is probed at contiguous strides); needs no GPU.
    key_views=True (the call comes with per-scene view counts): 'staged' means its varlen entry (``gta_attn_fwd_staged_varlen``), and a
    call that would be 'apply' raises ``GtaError`` instead -- ``_GenericAttn`` has no key mask; that holds under ``key_views_backward`` too (the
    backward with per-scene prefixes serves the fused layouts alone).
    key_mask_generic=True (the call comes with a key mask and its opt-in to these layouts): 'staged' means the gather entry
    (``gta_attn_fwd_staged_gather``), and everything else raises ``GtaError``: a call under grad (forward only, whatever ``key_mask_backward``
    says), precise=True, and the layouts the staged entry refuses too, which keep the words of the call without the opt-in."""
    if key_mask_generic:
        if key_views:
            raise native.GtaError("key_mask with key_views: a call takes one key mask")
        if needs_grad:
            raise native.GtaError("key_mask_generic is forward-only: the staged generic layouts (t2, euclid, so3 of degree 1, unaligned slabs) "
                                  "have no masked backward, and key_mask_backward serves the fused layouts alone: call under torch.no_grad()")
        _mask_refusals("key_mask", precise=precise)
        rc = native.E_UNSUPPORTED
        if dtype in (torch.float32, torch.bfloat16):
            rc = native.attn_fwd_staged_gather_supported(_probe(dtype, q_shape, Tk, f_dims, so3_degree, Nq, Nk, _layout_flags(v_transform, euclid)))
        if rc != 0:
            raise native.GtaError(_NO_GATHER_PREPASS + f"gta_attn_fwd_staged_gather_supported: {native.lib().gta_strerror(rc).decode()}")
        return "staged"
    if key_views:
        _mask_refusals("key_views", needs_grad=needs_grad, precise=precise, backward=key_views_backward)
        if needs_grad:
            raise native.GtaError("key_views_backward: the staged generic layouts (t2, euclid, so3 of degree 1, unaligned slabs) have no backward "
                                  "with a key mask")
    if needs_grad or precise or dtype not in (torch.float32, torch.bfloat16):
        if key_views:
            raise native.GtaError(f"key_views: unsupported dtype {dtype} (use float32 or bfloat16)")
        return "apply"
    probe = _probe(dtype, q_shape, Tk, f_dims, so3_degree, Nq, Nk, _layout_flags(v_transform, euclid))
    if key_views:
        rc = native.attn_fwd_staged_varlen_supported(probe)
        if rc != 0:
            raise native.GtaError("key_views: this layout is served by the rho-apply route (_GenericAttn) alone, which has no key mask: "
                                  f"gta_attn_fwd_staged_varlen_supported: {native.lib().gta_strerror(rc).decode()}")
        return "staged"
    return "staged" if native.attn_fwd_staged_supported(probe) == 0 else "apply"


# what the refusals of a masked call say per keyword: why it is forward-only without its opt-in, what of it lives in the K/V pre-pass, and what
# the single-kernel plan lacks
_MASK_WORDS = {"key_views": ("no backward with per-scene key prefixes yet", "key mask", "per-scene key mask"),
               "key_mask": ("no backward through the gathered keys yet", "gather", "gather")}


def _mask_refusals(name, *, needs_grad=False, precise=False, pretransformed=False, kv_mode="auto", backward=False):
    """what a call with ``name`` (``key_views`` or ``key_mask``) cannot be combined with: said here, before anything is launched, instead of
    running a route without the mask.  ``backward``: the keyword's opt-in to its backward (``key_views_backward``: ``gta_attn_bwd_varlen``,
    ``key_mask_backward``: ``gta_attn_bwd_gather``); without it a call under grad is refused as before."""
    forward_only, prepass, fused = _MASK_WORDS[name]
    if needs_grad and not backward:
        raise native.GtaError(f"{name} is forward-only ({forward_only}): call under torch.no_grad()")
    if precise:
        raise native.GtaError(f"{name} has no precise=True (fp32-faithful) instances")
    if pretransformed:
        raise native.GtaError(f"{name} with pretransformed=True: the {prepass} lives in the K/V pre-pass, which that mode skips")
    if kv_mode == "fused":
        raise native.GtaError(f"{name} runs the two-stage plan: kv_mode='fused' has no {fused}")


def _refuse_uneven(name, side, T, N):
    """the masked rep-gradient passes and the per-scene view counts work per view: the tokens of a side split evenly into its views"""
    if T % N:
        raise native.GtaError(f"{name}: {T} {side} tokens do not split evenly into {N} views")


def _refuse_cpu_carriers(name, gpu_pass, carriers):
    """said by name, before the forward is launched: the pass that serves the carriers under a mask has no CPU path"""
    if any(c is not None and not c.is_cuda for c in carriers):
        raise native.GtaError(f"{name}: the gradients of rep tables or poses come from a GPU pass ({gpu_pass}): "
                              "tables and poses that require grad must be CUDA tensors")


def check_key_views(key_views, B: int, Nk: Optional[int], name: str = "key_views") -> Tuple[int, ...]:
    """Host-side validation of per-scene view counts (a sequence or a CPU integer tensor of length B, each in 1..Nk) -> a tuple of ints.
    Nothing here touches the device, so there is no sync.  ``name``: what the messages call the argument (``query_views`` against Nq)."""
    bound, table, views = ("Nk", "vrep_k", "key views") if name == "key_views" else ("Nq", "vrep_q", "query views")
    if torch.is_tensor(key_views):
        if key_views.is_cuda:
            raise native.GtaError(f"{name} must be a host sequence or a CPU tensor (validating a device tensor would sync)")
        if key_views.is_floating_point() or key_views.is_complex() or key_views.dtype == torch.bool or key_views.dim() != 1:
            raise native.GtaError(f"{name} must be a 1-D integer tensor")
        key_views = key_views.tolist()
    try:
        vals = tuple(key_views)
    except TypeError:
        raise native.GtaError(f"{name} must be a sequence of B view counts") from None
    if any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in vals):
        raise native.GtaError(f"{name} must hold integers, got {vals}")
    vals = tuple(int(x) for x in vals)
    if len(vals) != B:
        raise native.GtaError(f"{name} has {len(vals)} entries for a batch of {B} scenes")
    if Nk is None:
        raise native.GtaError(f"{name} needs the number of {views} {bound}, which the view tables give ({table}): this layout has no "
                              "se3 / so3 slab and so no view structure")
    if any(x < 1 or x > Nk for x in vals):
        raise native.GtaError(f"{name} entries must lie in 1..{bound} = 1..{Nk}, got {vals}")
    return vals


def key_lens_tensor(key_views: Tuple[int, ...], Pk: int, device) -> torch.Tensor:
    """[B] int32 on ``device``: the valid key TOKENS per scene (view-major tokens: a prefix), what the varlen entries read"""
    return torch.tensor([n * Pk for n in key_views], dtype=torch.int32).to(device, non_blocking=True)


def check_key_mask(key_mask, B: Optional[int] = None, Tk: Optional[int] = None):
    """Validation of a key mask: a bool [B, Tk] tensor (the shape is held against B and Tk where given).  The values of a CPU mask are looked
    at -- every scene needs at least one valid key --, those of a device mask are not: that would sync."""
    if not torch.is_tensor(key_mask) or key_mask.dtype != torch.bool or key_mask.dim() != 2:
        raise native.GtaError("key_mask must be a bool tensor of shape [B, Tk] (True: the key is attended)")
    if B is not None and tuple(key_mask.shape) != (B, Tk):
        raise native.GtaError(f"key_mask has shape {tuple(key_mask.shape)} for {B} scenes of {Tk} key tokens")
    if not key_mask.is_cuda:
        empty = (~key_mask.any(1)).nonzero().flatten().tolist()
        if empty:
            raise native.GtaError(f"key_mask: scenes {empty} have no valid key (every scene attends at least one)")


def key_index_tensors(key_mask: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """key_mask (bool [B, Tk], True = attend) -> (key_idx [B, Tk] int32, key_lens [B] int32) on ``device``: what ``gta_attn_fwd_gather``
    reads.  key_idx[b, :key_lens[b]] are scene b's valid tokens in ascending order (a stable sort of ~mask), the rest of the row its
    masked tokens, which the kernel never reads.

    A CPU mask is validated here -- every scene needs at least one valid key, else ``GtaError`` -- and uploaded.  A CUDA mask is turned into
    indices on the device without a sync, so its values are not looked at: a scene with NO valid key then attends its token 0 alone (the
    kernels clamp the count to 1, and the first index of an all-false row is 0)."""
    check_key_mask(key_mask)
    if key_mask.is_cuda and key_mask.device != torch.device(device):
        raise native.GtaError(f"key_mask lives on {key_mask.device}, the call on {device}")
    idx = torch.sort((~key_mask).to(torch.uint8), dim=1, stable=True).indices.to(torch.int32)
    lens = key_mask.sum(1, dtype=torch.int32)
    return idx.contiguous().to(device, non_blocking=True), lens.to(device, non_blocking=True)


def effective_key_mask(key_mask: torch.Tensor, device, unvalidated: Optional[bool] = None) -> torch.Tensor:
    """The key mask the kernels act on, bool [B, Tk] on ``device``: what the rep-gradient pass (``gta_rep_grad_sums_masked``) must see.
    Under a CUDA mask a scene with NO valid key attends its token 0 (``key_index_tensors``: the count is clamped to 1 and the first index of
    an all-false row is 0), so token 0 of such a scene is live here too -- set on the device, without a sync.  A CPU mask was validated to
    have a valid key in every scene: it is uploaded as it is.  ``unvalidated``: whether the mask's values were not looked at (None: a CUDA
    mask)."""
    live = key_mask.to(device, non_blocking=True).clone()
    if key_mask.is_cuda if unvalidated is None else unvalidated:
        live[:, 0] |= ~live.any(1)
    return live.contiguous()


def check_query_mask(query_mask, B: Optional[int] = None, Tq: Optional[int] = None):
    """Validation of a query mask: a bool [B, Tq] tensor (the shape is held against B and Tq where given).  Its values are not looked at: a
    scene may have no live query row at all."""
    if not torch.is_tensor(query_mask) or query_mask.dtype != torch.bool or query_mask.dim() != 2:
        raise native.GtaError("query_mask must be a bool tensor of shape [B, Tq] (True: the query row is live)")
    if B is not None and tuple(query_mask.shape) != (B, Tq):
        raise native.GtaError(f"query_mask has shape {tuple(query_mask.shape)} for {B} scenes of {Tq} query tokens")


def query_mask_tensors(query_mask: torch.Tensor, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """query_mask (bool [B, Tq], True = the row is live) -> (q_live [B, Tq] bool, q_lens [B] int32) on ``device``: what ``gta_attn_fwd_qmask``
    and ``gta_attn_bwd_qmask`` read.  q_live is the mask itself (its storage: one byte per row); q_lens[b] is 1 + the index of scene b's last
    live row, 0 for a scene without one (legal: the kernels clamp it to 1 and find row 0 dead) -- the backward's dK/dV walk skips the query
    tiles behind it.  A CUDA mask is converted on the device without a sync, a CPU mask on the host and uploaded."""
    check_query_mask(query_mask)
    if query_mask.is_cuda and query_mask.device != torch.device(device):
        raise native.GtaError(f"query_mask lives on {query_mask.device}, the call on {device}")
    pos = torch.arange(1, query_mask.shape[1] + 1, dtype=torch.int32, device=query_mask.device)
    lens = (query_mask.to(torch.int32) * pos).amax(1) if query_mask.shape[1] else torch.zeros(query_mask.shape[0], dtype=torch.int32)
    return query_mask.contiguous().to(device, non_blocking=True), lens.to(torch.int32).to(device, non_blocking=True)


def _all_keys_tensors(B: int, Tk: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(key_idx, key_lens) of an all-True key mask -- a query mask without a key mask runs the key_mask route under it: the identity index
    (an arange, no sort) and the full count"""
    return (torch.arange(Tk, dtype=torch.int32, device=device).expand(B, Tk).contiguous(),
            torch.full((B,), Tk, dtype=torch.int32, device=device))


class MaskIndex(namedtuple("_MaskIndexFields", "key_mask query_mask key_idx key_lens k_live q_live q_lens", defaults=(None,) * 7)):
    """Everything the masked kernels read of a key mask and / or a query mask, built once (``mask_index``) and handed to every
    ``gta_attention`` call on those masks as its ``mask_index`` companion -- all layers of a step share one record.  Immutable.
      key_mask, query_mask   the very mask objects it was built from (``gta_attention`` compares by identity: no compare, no sync)
      key_idx [B, Tk] int32, key_lens [B] int32   ``key_index_tensors``
      k_live [B, Tk] bool    ``effective_key_mask``: the mask with token 0 of a scene without a live key set
      q_live [B, Tq] bool, q_lens [B] int32       ``query_mask_tensors``: the query mask, contiguous, on the device; its last live row + 1
    The fields of an absent side are None: that is every record ``mask_index`` returns.  One more shape is accepted by ``gta_attention`` and
    made by no constructor here: a record WITHOUT a key mask (``key_mask`` and ``k_live`` None) that still carries ``key_idx`` / ``key_lens``
    -- the index of every key (an arange per scene, the full count), which a call under a query mask alone otherwise builds itself on each
    call; a caller who keeps that pair puts it into the record with ``_replace`` and the call then builds nothing."""
    __slots__ = ()

    def keys_only(self) -> "MaskIndex":
        """the record of the same ``key_mask`` without a query side (a decoder behind an encoder with a query mask): the same key tensors,
        nothing launched"""
        return self._replace(query_mask=None, q_live=None, q_lens=None)


def _on_device(mask, device, name):
    if mask.is_cuda and mask.device != device:
        raise native.GtaError(f"{name} lives on {mask.device}, the call on {device}")
    return mask.contiguous().to(device, non_blocking=True)


def mask_index(key_mask: Optional[torch.Tensor] = None, query_mask: Optional[torch.Tensor] = None, *, device) -> MaskIndex:
    """The ``MaskIndex`` of ``key_mask`` (bool [B, Tk]) and / or ``query_mask`` (bool [B, Tq]) on ``device``: ONE launch
    (``gta_mask_index``, gta_maskidx.hip) on the current stream in place of ``key_index_tensors``, ``query_mask_tensors`` and
    ``effective_key_mask``, with their results bit for bit.  Validation as there: a CPU key mask has its values looked at (a scene without
    a valid key raises) and is uploaded; a CUDA mask is never read on the host -- a scene of it without a valid key attends its token 0.
    The same tensor may be both masks (self-attention over padded tokens): it is passed for both sides."""
    if key_mask is None and query_mask is None:
        raise native.GtaError("mask_index needs a key_mask or a query_mask")
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    km = qm = None
    if key_mask is not None:
        check_key_mask(key_mask)
        km = _on_device(key_mask, device, "key_mask")
    if query_mask is not None:
        check_query_mask(query_mask)
        qm = km if query_mask is key_mask else _on_device(query_mask, device, "query_mask")
    if km is not None and qm is not None and km.shape[0] != qm.shape[0]:
        raise native.GtaError(f"key_mask has {km.shape[0]} scenes, query_mask {qm.shape[0]}")
    B = (km if km is not None else qm).shape[0]
    key_idx = key_lens = k_live = q_lens = None
    if km is not None:
        key_idx = torch.empty(km.shape, dtype=torch.int32, device=device)
        key_lens = torch.empty(B, dtype=torch.int32, device=device)
        k_live = torch.empty(km.shape, dtype=torch.bool, device=device)
    if qm is not None:
        q_lens = torch.empty(B, dtype=torch.int32, device=device)
    native.mask_index(km, key_idx, key_lens, k_live, qm, q_lens)
    return MaskIndex(key_mask, query_mask, key_idx, key_lens, k_live, qm, q_lens)


def _check_mask_index(mi, key_mask, query_mask, B, Tq, Tk, device):
    """``gta_attention``'s ``mask_index`` is a companion of its masks, as ``key_lens`` is of ``key_views``: accepted only beside the very mask
    objects it was built from (identity: nothing is compared, nothing syncs), complete for each side it has, and on the call's device.
    (The masks' shapes were held against B, Tq, Tk before; a record without a key side may still carry the index of every key,
    ``_all_keys_tensors``, which the call builds itself otherwise.)"""
    def fits(t, shape, dtype):
        return torch.is_tensor(t) and t.device == device and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous()
    ok = isinstance(mi, MaskIndex) and (key_mask is not None or query_mask is not None) and mi.key_mask is key_mask and mi.query_mask is query_mask
    if ok and (key_mask is not None or mi.key_idx is not None):
        ok = fits(mi.key_idx, (B, Tk), torch.int32) and fits(mi.key_lens, (B,), torch.int32)
    if ok and key_mask is not None:
        ok = fits(mi.k_live, (B, Tk), torch.bool)
    if ok and query_mask is not None:
        ok = fits(mi.q_live, (B, Tq), torch.bool) and fits(mi.q_lens, (B,), torch.int32)
    if not ok:
        raise native.GtaError("mask_index comes with the key_mask / query_mask it was built from (gta_amd.mask_index(key_mask, query_mask, "
                              "device=q.device): the same mask objects, no key_views, tensors on the call's device)")


def _plan_key(family: str, flags, dt, B, H, Tk, dh, f_dims, so3_degree, Nk, scale, key_views):
    """what the images of a cache depend on besides the keys, reps and trans_coeff (the caller's contract, see gta_attention): the family
    ('fused' / 'staged': different tile images), the key side's shape and layout, the dtype (bf16 / fp32 inputs pick different instances), the
    arithmetic mode -- the fp32-faithful plan stores FOUR images per tile [K'hi | V'hi | K'lo | V'lo], the default plan two: a cache written
    under one plan must never be streamed under the other (the byte-size check alone let that through) --, under euclid the scale,
    which the cached key bias -0.5 scale |k'|^2 carries, and last the view counts of a call with key_views (else None; the word "key_mask"
    for a call with one: the cache then holds the indices and lengths its images were built under)."""
    euclid = bool(flags & native.FLAG_EUCLID)
    return (family, bool(flags & native.FLAG_FP32_PRODUCTS), bool(flags & native.FLAG_V_TRANSFORM), euclid, str(dt), B, H, int(Tk), dh,
            tuple(sorted((g, int(n)) for g, n in f_dims.items() if n)), int(so3_degree), int(Nk), float(scale) if euclid else None,
            None if key_views is None else key_views if isinstance(key_views, str) else tuple(key_views))


def _two_stage_workspace(desc, flags, plan_key, kv_cache, device, need, cache_bytes=0):
    """The K'/V' workspace of a two-stage call, ``need`` bytes, in both families: a fresh one -- stored in ``kv_cache`` with its plan key
    when there is a cache, and then of at least ``cache_bytes`` --, or the cache's images, with GTA_FLAG_KV_READY set in ``desc``; images
    written under another plan or for another key set raise ``GtaError``."""
    if kv_cache is None:
        return torch.empty(need, device=device, dtype=torch.uint8)
    ws = kv_cache.get("images")
    if ws is None:
        ws = torch.empty(max(need, cache_bytes), device=device, dtype=torch.uint8)
        kv_cache["images"], kv_cache["plan"] = ws, plan_key
        return ws
    # K'/V' tile images of an earlier call against the same keys (chunked decode): skip the pre-pass
    if kv_cache.get("plan") != plan_key:
        raise native.GtaError(f"kv_cache holds images written under another plan {kv_cache.get('plan')} (this call: {plan_key}): "
                              "use one cache dict per (key set, dtype, precise mode)")
    if ws.numel() < need or ws.device != device:
        raise native.GtaError("kv_cache holds images of a different key set")
    desc.flags = flags | native.FLAG_KV_READY
    return ws


def _fused_workspace(c: _Call, cfg, kv_cache, key_views=None):
    """``_two_stage_workspace`` for the fused family (``_fused_forward``, masked or not)"""
    f_dims, so3_degree, _, Nk, scale, flags = cfg
    need = native.attn_fwd_workspace_bytes(c.desc)
    if kv_cache is None:
        return _two_stage_workspace(c.desc, flags, None, None, c.q.device, need)
    # the workspace's tail (query-side operand tiles) grows with the number of QUERY views: a cache serves later query sets against the
    # same keys, so it is sized by asking the library for the most views a call can have (the size rule -- which instances carry a
    # tail, how large a tile is -- stays the library's)
    cache_bytes = 0
    if kv_cache.get("images") is None:
        widest = type(c.desc).from_buffer_copy(c.desc)
        widest.Nq = widest.Tq = native.MAX_VIEWS
        cache_bytes = native.attn_fwd_workspace_bytes(widest)
    B, H, Tk, dh = c.k.shape
    plan_key = _plan_key("fused", flags, c.q.dtype, B, H, Tk, dh, f_dims, so3_degree, Nk, scale, key_views)
    return _two_stage_workspace(c.desc, flags, plan_key, kv_cache, c.q.device, need, cache_bytes)


# How a call on the fused layouts is masked: what the forward launcher, ``_FusedAttn`` and its backward pass around.
#   kind     None (every key, every query row), "views" (per-scene prefixes of views: the varlen entries) or "gather" (key and / or query mask)
#   key_idx  gather: [B, Tk] int32, ``key_index_tensors`` (``_all_keys_tensors`` under a query mask alone)
#   key_lens views / gather: [B] int32, the valid key tokens per scene
#   q_live   gather under a query mask: the mask itself on the device (``query_mask_tensors``)
#   q_lens   with q_live, or views with ``query_views`` (backward only): [B] int32
#   k_live   gather with carriers: the effective key mask of the rep-gradient pass (None: every key is live)
#   views    views: the validated host tuples (query_views or None, key_views) the device tensors were built from
#   key_mask gather, forward only, no query mask: the caller's mask, from which the launcher builds key_idx / key_lens after its checks -- and a
#            later call on a ``kv_cache`` builds nothing
_Mask = namedtuple("_Mask", "kind key_idx key_lens q_live q_lens k_live views key_mask", defaults=(None,) * 8)
_NO_MASK = _Mask()


def _views_mask(key_views, key_lens, query_views, q, k, Nq, Nk) -> _Mask:
    """``key_views`` (validated; ``key_lens``: its ready-made device tensor or None) and ``query_views`` (validated, or None: no query side)"""
    if key_lens is None:
        key_lens = key_lens_tensor(key_views, k.shape[2] // Nk, q.device)
    q_lens = None if query_views is None else key_lens_tensor(query_views, q.shape[2] // Nq, q.device)
    return _Mask("views", key_lens=key_lens, q_lens=q_lens, views=(query_views, key_views))


def _gather_mask(key_mask, query_mask, q, k, needs_grad, carriers, mask_index=None) -> _Mask:
    """``key_mask`` and / or ``query_mask`` (both validated).  A query mask without a key mask runs under an all-True one; a forward-only call
    without a query mask leaves the key tensors to the launcher.  ``mask_index`` (checked: ``_check_mask_index``): the record's tensors
    stand where this would build them -- the very objects, on every path -- and nothing is built but the all-True index it does not carry."""
    if mask_index is not None:
        key_idx, key_lens = mask_index.key_idx, mask_index.key_lens
        if key_idx is None:
            key_idx, key_lens = _all_keys_tensors(q.shape[0], k.shape[2], q.device)
        k_live = mask_index.k_live if needs_grad and carriers and key_mask is not None else None
        return _Mask("gather", key_idx, key_lens, mask_index.q_live, mask_index.q_lens, k_live)
    if query_mask is None and not needs_grad:
        return _Mask("gather", key_mask=key_mask)
    q_live, q_lens = (None, None) if query_mask is None else query_mask_tensors(query_mask, q.device)
    key_idx, key_lens = _all_keys_tensors(q.shape[0], k.shape[2], q.device) if key_mask is None else key_index_tensors(key_mask, q.device)
    k_live = effective_key_mask(key_mask, q.device) if needs_grad and carriers and key_mask is not None else None
    return _Mask("gather", key_idx, key_lens, q_live, q_lens, k_live)


def _fused_forward(q, k, v, cfg, kv_cache, mask: _Mask, tables, trans_coeff, tau):
    """The forward of the fused layouts, one native entry by the mask's kind: ``gta_attn_fwd``; views: ``gta_attn_fwd_varlen`` (the two-stage
    plan's pre-pass and gta_fwd2_kernel in their VARLEN instances); gather: ``gta_attn_fwd_gather`` (the GATHER instances of the pre-pass
    compact the valid keys, the VARLEN gta_fwd2_kernel attends over them), under a query mask ``gta_attn_fwd_qmask`` (never with ``kv_cache``).
    The masked entries always run the two-stage plan; the plan key of their ``kv_cache`` carries the view counts, or the word "key_mask" --
    such a cache holds ``key_idx`` / ``key_lens`` beside the images, and later calls run on the stored lengths under GTA_FLAG_KV_READY.
    -> (the call, its workspace: the K'/V' tile images, or None on the single-kernel plan)"""
    flags = cfg[5]
    c = _setup_call(q, k, v, *cfg, tables, trans_coeff, tau, k_side=not (flags & native.FLAG_PRETRANSFORMED))
    kind = mask.kind
    operands = (c.desc, c.q, c.k, c.v, tables.get("vrep_q"), tables.get("vrep_k"), tables.get("cs_q"), tables.get("cs_k"), c.tc, c.ta)
    if kind is None:
        # (the single-kernel plan and a pretransformed call have no K/V pre-pass: no workspace)
        ws = None if flags & (native.FLAG_FUSED_KV | native.FLAG_PRETRANSFORMED) else _fused_workspace(c, cfg, kv_cache)
        native.attn_fwd(*operands, c.out, c.lse, ws)
    elif kind == "views":
        ws = _fused_workspace(c, cfg, kv_cache, mask.views[1])
        native.attn_fwd_varlen(*operands, mask.key_lens, c.out, c.lse, ws)
    else:
        ws = _fused_workspace(c, cfg, kv_cache, "key_mask")
        key_idx, key_lens = mask.key_idx, mask.key_lens
        if c.desc.flags & native.FLAG_KV_READY:
            key_idx, key_lens = None, kv_cache["key_lens"]
        else:
            if key_lens is None:
                key_idx, key_lens = key_index_tensors(mask.key_mask, c.q.device)
            if kv_cache is not None:
                kv_cache["key_idx"], kv_cache["key_lens"] = key_idx, key_lens
        if mask.q_live is not None:
            native.attn_fwd_qmask(*operands, key_idx, key_lens, mask.q_live, c.out, c.lse, ws)
        else:
            native.attn_fwd_gather(*operands, key_idx, key_lens, c.out, c.lse, ws)
    return c, ws


class _FusedAttn(torch.autograd.Function):
    """The fused layouts under autograd, masked or not: forward -> out through ``_fused_forward``, whose workspace (the K'/V' tile images, masked
    or compacted like the call) and LSE serve the backward entry of the same kind (``backward.attn_bwd``).  ``_FusedAttnLse`` below is the same
    call with the pair (out, lse) as differentiable outputs (``return_lse``); both share ``_run`` and ``_grads``.

    Arguments: (q, k, v, trans_coeff, tau, call, vrep_q, vrep_k, cs_q, cs_k, *carriers) -- ``call`` = (cfg, kv_cache, mask), the one non-tensor
    argument (kv_cache: the unmasked call's alone, None under a mask); carriers: () or six tensors / None (gta_amd.repgrad.split_tables) whose gradients the backward returns, from ``CARRIERS`` on.
    Gradients: q, k, v, trans_coeff, tau; dk / dv rows of padded views and masked tokens and dq rows of dead query rows are exact zeros.  With
    carriers the tables' too: the pass of gta_amd/repgrad.py over (q, dq), (dout, out) and (dk, k), (dv, v) -- views: over the prefixes alone
    (``gta_rep_grad_sums_varlen``), gather: over the live tokens alone (``gta_rep_grad_sums_masked``) under ``mask.q_live`` (None: every row)
    and ``mask.k_live`` --, exact zeros for padded or wholly masked views and for dead tokens.

    The mask's tensors (``_Mask``) are integer or bool tensors that take no gradient: they stay on ``ctx`` inside the record, as the objects
    themselves, never in ``save_for_backward`` -- the backward hands the native entries and ``table_grads`` the very objects the forward got."""

    CARRIERS = 10          # where the carriers start in the argument list

    @staticmethod
    def forward(ctx, *args):
        return _FusedAttn._run(ctx, *args).out

    @staticmethod
    def backward(ctx, dout):
        return _FusedAttn._grads(ctx, dout)

    @staticmethod
    def _run(ctx, q, k, v, trans_coeff, tau, call, vrep_q, vrep_k, cs_q, cs_k, *carriers):
        cfg, kv_cache, mask = call
        c, ws = _fused_forward(q, k, v, cfg, kv_cache, mask, dict(vrep_q=vrep_q, vrep_k=vrep_k, cs_q=cs_q, cs_k=cs_k), trans_coeff, tau)
        ctx.cfg, ctx.mask = cfg, mask
        # K'/V' tile images of the two-stage plan: reused by the backward (fp32-faithful plan: its hi / lo images by the X3 walks, r06)
        ctx.kv_images = ws
        ctx.save_for_backward(c.q, c.k, c.v, c.out, c.lse, c.tc, c.ta, vrep_q, vrep_k, cs_q, cs_k)
        ctx.tc_meta, ctx.tau_meta = _scalar_meta(trans_coeff), _scalar_meta(tau)
        ctx.carriers = _repgrad.carrier_meta(carriers)
        return c

    @staticmethod
    def _grads(ctx, dout, dlse=None):
        from . import backward as _bw
        q, k, v, out, lse, tc, ta, vrep_q, vrep_k, cs_q, cs_k = ctx.saved_tensors
        mask = ctx.mask
        want_dtau = ta is not None and ctx.needs_input_grad[4]
        dq, dk, dv, dtc, dta = _bw.attn_bwd(ctx.cfg, q, k, v, out, dout, lse, tc, ta, vrep_q, vrep_k, cs_q, cs_k, kv_images=ctx.kv_images,
                                            want_dtau=want_dtau, key_lens=mask.key_lens, q_lens=mask.q_lens, dlse=dlse, key_idx=mask.key_idx,
                                            q_live=mask.q_live)
        grads = ()
        if ctx.carriers:
            # gradients of the tables: a pass after the backward over (q, dq), (dout, out) and (dk, k), (dv, v) (gta_amd/repgrad.py) -- under
            # per-scene view counts over the prefixes, under masks over the live tokens
            meta = tuple(m if need else None for m, need in zip(ctx.carriers, ctx.needs_input_grad[_FusedAttn.CARRIERS:]))
            f_dims, so3_degree, Nq, Nk, scale, flags = ctx.cfg
            desc = native.make_desc(q, k, v, out, f_dims, so3_degree, Nq, Nk, scale, flags)
            do = _as_kernel_layout(dout.to(q.dtype))
            vt = bool(flags & native.FLAG_V_TRANSFORM)
            tables = dict(vrep_q=vrep_q, vrep_k=vrep_k, cs_q=cs_q, cs_k=cs_k)
            sides = {}
            if mask.kind == "views":
                sides = dict(views=mask.views, lens=(mask.q_lens, mask.key_lens))
            elif mask.kind == "gather":
                sides = dict(masks=(mask.q_live, mask.k_live))
            grads = tuple(_repgrad.table_grads(desc, tables, meta, tc, ((q, dq), (do, out))[:1 + vt], ((dk, k), (dv, v))[:1 + vt],
                                               direct=False, **sides))
        return (dq, dk, dv, _restore_scalar(dtc, ctx.tc_meta), _restore_scalar(dta, ctx.tau_meta)) + (None,) * (_FusedAttn.CARRIERS - 5) + grads


class _FusedAttnLse(torch.autograd.Function):
    """``_FusedAttn`` -> (out, lse), both differentiable: the backward takes (dout, dlse), either of which may be None, through
    ``gta_attn_bwd_dlse`` (dS = P (dP - D + dlse): the q-side pre-pass stores -(D - dlse), every walk is the one of ``gta_attn_bwd``); under a
    mask (``masked_lse_backward=True``) through the ``_dlse`` twin of the mask's backward entry."""

    @staticmethod
    def forward(ctx, *args):
        ctx.set_materialize_grads(False)
        c = _FusedAttn._run(ctx, *args)
        return c.out, c.lse

    @staticmethod
    def backward(ctx, dout, dlse):
        return _FusedAttn._grads(ctx, _none_to_zero(dout, ctx.saved_tensors[3]), dlse)


def _staged_forward(q, k, v, f_dims, packed, so3_degree, trans_coeff, tau, scale, v_transform, euclid, kv_cache=None, key_views=None,
                    key_lens=None, return_lse=False, mask=None):
    """The generic path without a gradient: one pre-pass launch + one attention launch (``gta_attn_fwd_staged``), and the attention
    launch alone on a call that finds its K'/V' images in ``kv_cache`` -- the contract of ``_fused_forward``: images and plan key are stored by
    the first call, later calls against another key set / plan raise ``GtaError``.  ``key_views`` (validated) with ``key_lens`` (device):
    the varlen entry, and the view counts join the plan key.  ``mask`` (a ``_Mask`` of kind "gather", no query side): the gather entry
    (``gta_attn_fwd_staged_gather``) -- the plan key ends in "key_mask", the cache holds ``key_idx`` / ``key_lens`` beside the compacted
    images and later calls run on the stored lengths, as in ``_fused_forward``."""
    flags = _layout_flags(v_transform, euclid)
    Nq, Nk = _views(f_dims, packed, q, k)
    c = _setup_call(q, k, v, f_dims, so3_degree, Nq, Nk, scale, flags, packed, trans_coeff, tau)
    B, H, Tk, dh = c.k.shape
    # (the workspace's size does not depend on the query side)
    plan_key = None if kv_cache is None else _plan_key("staged", flags, c.q.dtype, B, H, Tk, dh, f_dims, so3_degree, Nk, scale,
                                                       "key_mask" if mask is not None else key_views)
    ws = _two_stage_workspace(c.desc, flags, plan_key, kv_cache, c.q.device, native.attn_fwd_staged_workspace_bytes(c.desc))
    tables = [packed.get(t) for t in ("vrep_q", "vrep_k", "cs_q", "cs_k", "coord_q", "coord_k")]
    if mask is not None:
        key_idx, key_lens = mask.key_idx, mask.key_lens
        if c.desc.flags & native.FLAG_KV_READY:
            key_idx, key_lens = None, kv_cache["key_lens"]
        else:
            if key_lens is None:
                key_idx, key_lens = key_index_tensors(mask.key_mask, c.q.device)
            if kv_cache is not None:
                kv_cache["key_idx"], kv_cache["key_lens"] = key_idx, key_lens
        native.attn_fwd_staged_gather(c.desc, c.q, c.k, c.v, *tables, c.tc, c.ta, key_idx, key_lens, c.out, c.lse, ws)
    elif key_views is not None:
        native.attn_fwd_staged_varlen(c.desc, c.q, c.k, c.v, *tables, c.tc, c.ta, key_lens, c.out, c.lse, ws)
    else:
        native.attn_fwd_staged(c.desc, c.q, c.k, c.v, *tables, c.tc, c.ta, c.out, c.lse, ws)
    return (c.out, c.lse) if return_lse else c.out


def gta_attention(q, k, v, f_dims: Dict[str, int], packed: dict, *, so3_degree: int = 0,
                  trans_coeff=None, tau=None, scale: Optional[float] = None, v_transform: bool = True,
                  euclid: bool = False, pretransformed: bool = False, use_dma: bool = True,
                  kv_mode: str = "auto", kv_cache: Optional[dict] = None, precise: Optional[bool] = None,
                  key_views=None, key_lens: Optional[torch.Tensor] = None, key_views_backward: bool = False,
                  query_views=None, return_lse: bool = False, key_mask: Optional[torch.Tensor] = None, key_mask_backward: bool = False,
                  query_mask: Optional[torch.Tensor] = None, key_mask_rep_grad: bool = False,
                  mask_index: Optional[MaskIndex] = None, masked_lse_backward: bool = False, key_mask_generic: bool = False):
    """Fused GTA attention on packed reps.  q [B,H,Tq,dh], k/v [B,H,Tk,dh] -> out [B,H,Tq,dh].

    kv_mode: 'prepass' = K/V rep pre-pass + lean attention kernel (two launches; at dh = 96 in the MSN layout the attention kernel is
                         the 64-rows-per-wave one of gta_fwd64.hip, 'prepass_rows32' keeps gta_fwd2.hip's);
             'fused'   = one kernel, rho_k applied inside the attention loop;
             'auto'    = 'prepass' when several query tiles share each key tile, else 'fused'.
    precise: float32 inputs only.  False / None (default): operands are rounded to bf16 once, after
             rho, and the two contractions run on the bf16 MFMA (fp32 accumulation) -- the reference's bf16-autocast
             accuracy.  True: operands are kept as bf16 hi+lo pairs and every product is three MFMAs -- fp32-class results
             (max |error| ~1e-5 of max |out|) at 3x the matrix work; two-stage plan at dh <= 64 (r05), single-kernel plan otherwise.  When a gradient is wanted the call runs
             rho in fp32 (gta_rep_apply), the split-bf16 plain forward and an EXACT-fp32 backward (gta_plain32.hip: f32 matrix
             instructions, 1/16 of the bf16 rate) -- the arithmetic of the reference's ``mixed_prec: False`` training.
    kv_cache: a dict owned by the caller (inference only).  The first call stores the K'/V' tile images of the
             pre-pass in it; later calls with the same keys, reps and trans_coeff (e.g. the next query chunk of a
             full-image decode, trainer.py:137-181) stream them again without re-running the pre-pass.  The layouts of the generic
             path (t2, euclid, so3 of degree 1, unaligned slabs) honour it through the staged generic forward (``generic_route``).
    key_views: per-scene numbers of valid input views -- a host sequence or CPU integer tensor of length B, each in 1..Nk (None: every
             scene has all Nk).  Scene b attends over its first ``key_views[b]`` views (tokens are view-major, so over a prefix of its
             keys); whatever k, v and the key-side tables hold for the other views is never used.  out and LSE are those of the call on
             that scene alone with its key side cut to the prefix, and the padded key tiles are skipped, not computed.  Inference only,
             default arithmetic, two-stage plan (fused layouts) or staged route (generic layouts); anything else raises ``GtaError``.
             In self-attention the output rows of padded views are unspecified.  ``key_lens``: the ready-made device tensor of
             ``key_lens_tensor`` for these view counts (``ForwardPlan`` keeps one); built per call when None.
    key_views_backward: False (default): a call with ``key_views`` under grad raises "forward-only", as it always did.  True: the call is
             differentiable in q, k, v, trans_coeff and tau on the fused layouts (``gta_attn_fwd_varlen`` + ``gta_attn_bwd_varlen``): dk / dv rows
             of padded views are exactly zero and nothing of a padded view is read.  Rep tables and poses that require grad get their
             gradients too (gta_amd/repgrad.py over the prefixes, ``gta_rep_grad_sums_varlen``): exact zeros for the padded views' records
             and the padded tokens' entries -- with ``query_views`` on the query side as well --, whatever those hold (such tables must be
             CUDA tensors: the pass has no CPU path, and a CPU one is refused by name before anything is launched).  Still refused, by
             name: the staged generic layouts under grad, precise=True, pretransformed, kv_mode='fused', return_attmap, and return_lse
             under grad without ``masked_lse_backward=True`` (below).
    query_views: only with ``key_views_backward=True``; validated like ``key_views``, against Nq.  Backward only: the query rows of scene b's
             views past ``query_views[b]`` (self-attention over padded views, where they hold anything) send no gradient -- their ``dout`` is
             never read, their dq rows are zero.  The forward still computes (unspecified) output rows for them.
    return_lse: False (default): -> out, exactly as without the keyword.  True: -> (out, lse); lse [B,H,Tq] float32 is the natural log of
             sum_k exp((scale q'.k' + bias_k) / tau) per query row (bias_k: the euclid key bias, else 0) -- what every forward kernel writes
             beside out and ``gta_attention_merge`` combines partial attentions with.  Without grad on every route (fused, key_views, staged,
             rho-apply).  Under grad lse is a differentiable output like out -- the backward takes (dout, dlse), either may be missing -- in
             the default arithmetic (fused layouts and the rho-apply route) and with precise=True where the fused fp32-faithful backward runs
             (float32, dh <= 64); ``key_views_backward`` / ``key_mask_backward`` without ``masked_lse_backward=True`` and the exact-fp32
             route of precise=True (gta_plain32) raise ``GtaError``.
    key_mask: a bool [B, Tk] tensor (True: the key is attended; None: every key is) -- ANY per-scene subset of the key tokens: views of
             different size padded inside their slots, a missing view that is not the last, patches to ignore.  out (and lse, with
             ``return_lse``) are those of the attention over the valid keys alone; whatever k, v and cs_k hold at masked tokens is never
             used, NaN and Inf included.  The K/V pre-pass compacts the valid keys (``key_index_tensors``, ``gta_attn_fwd_gather``) and
             masked tiles are skipped, not computed.  A CPU mask is validated (every scene needs a valid key); a CUDA mask is used without
             a sync, and a scene of it with no valid key attends its token 0.  In self-attention the output rows of masked tokens are
             computed like any other.  With ``kv_cache`` later calls must pass ``key_mask`` again (it is not looked at: they run on the
             indices and lengths the first call stored).  Forward only unless ``key_mask_backward=True``; default arithmetic, two-stage plan,
             fused layouts; refused by name: a call under grad without ``key_mask_backward``, precise=True, pretransformed, kv_mode='fused',
             ``key_views`` beside it, and the staged and rho-apply layouts (t2, euclid, so3 of degree 1, unaligned slabs), which have no gather
             pre-pass.
    key_mask_backward: only with ``key_mask``.  False (default): a call with ``key_mask`` under grad raises "forward-only", as it always did.
             True: the call is differentiable in q, k, v, trans_coeff and tau (``gta_attn_fwd_gather`` + ``gta_attn_bwd_gather``; the forward's
             compacted images serve the backward).  dk / dv rows of masked tokens are exactly zero, and nothing of a masked KEY row -- k, v, cs_k,
             the vrep_k record of a wholly masked view -- is read: it may hold anything, NaN and Inf included.  Without ``query_mask`` (below) there is no query-side mask: in
             self-attention the masked tokens are query rows too, computed as in the forward, and they take part in the backward with whatever
             ``dout`` they get -- so masked QUERY rows (q, cs_q, and the dout that reaches them) must hold finite values; a zero ``dout`` row then
             adds exact zeros to dk / dv.  Still refused, by name: rep tables or poses that require grad without ``key_mask_rep_grad`` (below),
             return_lse under grad without ``masked_lse_backward=True`` (below), kv_cache under grad, precise=True, pretransformed,
             kv_mode='fused', and the staged and rho-apply layouts.
    key_mask_rep_grad: only with ``key_mask_backward=True``.  False (default): rep tables or poses that require grad are refused under a mask,
             as they always were.  True: they get their gradients (gta_amd/repgrad.py over the live tokens, ``gta_rep_grad_sums_masked``): the
             key side under the key mask, the query side under ``query_mask`` (without one every query row is live, in self-attention too).
             A view without a live token gets exact zeros in its record (its matrix is never inverted) and a masked token exact zeros in
             its so2 / coordinate entries, whatever those hold.  Under a CUDA key mask a scene without a valid key attends its token 0, and
             that token counts as live here too.  Such tables must be CUDA tensors (the pass has no CPU path; a CPU one is refused by name
             before anything is launched), and the masked sides' tokens must split evenly into views.
    masked_lse_backward: only with ``key_views_backward=True`` or ``key_mask_backward=True``.  False (default): ``return_lse`` under grad is
             refused under those, as it always was.  True: (out, lse) of the masked call is differentiable -- the backward takes (dout, dlse),
             either may be missing, through ``gta_attn_bwd_varlen_dlse`` (``key_views``, with or without ``query_views``),
             ``gta_attn_bwd_gather_dlse`` (``key_mask``) or ``gta_attn_bwd_qmask_dlse`` (with ``query_mask``); ``mask_index`` and
             ``key_mask_rep_grad`` go with it as with the backward without lse.  This is what lets masked partial attentions be merged
             (``gta_attention_merge``) and trained through.  ``dlse`` of dead rows (``query_mask``) and of rows at or past ``query_views``
             may hold anything, NaN and Inf included, as their ``dout`` may: it is never read.  Without ``return_lse`` or without grad the
             flag changes nothing.  Everything else the masked routes refuse stays refused (precise=True, pretransformed, kv_mode='fused',
             kv_cache under grad, the staged and rho-apply layouts).
    query_mask: a bool [B, Tq] tensor (True: the query row is live; None: every row is) -- the query side of ``key_mask``: padded tokens of
             a self-attention layer, scenes with different numbers of target rays.  A masked (dead) row is never used: its q row, its cs_q
             row and the vrep_q record of a view without a live row may hold anything, NaN and Inf included, and so may its ``dout`` row in
             the backward.  It receives exact zeros: out = +0.0 and lse = +0.0 (a later ``gta_attention_merge`` of such rows stays finite),
             dq = +0.0, and it adds nothing to dk, dv, d trans_coeff or d tau.  A scene may have no live row.  Work items (128 rows)
             without a live row cost a store of zeros; a dead row inside a live item is computed as a zero row.  The call runs the
             ``key_mask`` route (``gta_attn_fwd_qmask`` / ``gta_attn_bwd_qmask``) -- without ``key_mask`` under an all-True one, whose index is
             an arange (no sort) -- and with everything that route refuses: under grad it needs ``key_mask_backward=True``.  Refused by
             name: ``key_views`` / ``query_views`` / ``key_lens`` / ``key_views_backward`` beside it, ``kv_cache``, and what ``key_mask``
             refuses.  ``return_lse`` without grad is served.
    key_mask_generic: only with ``key_mask``.  False (default): a key mask on a layout without a fused kernel (t2 slab, euclid, so3 of degree
             1, unaligned slabs) raises "no gather pre-pass", as it always did.  True: such a call runs the staged generic forward over the
             masked keys (``gta_attn_fwd_staged_gather``: the GATHER instances of its pre-pass compact the valid keys and their euclid
             bias, its VARLEN attention kernel attends over them) -- forward only (under grad it raises, ``key_mask_backward`` or not),
             no ``query_mask``, with ``return_lse``, ``mask_index`` and ``kv_cache`` as on the fused layouts; layouts the staged entry
             refuses too (dh % 8 != 0, dh > 128) keep the old words.  On a fused layout it changes nothing.
    mask_index: the ``MaskIndex`` of this call's ``key_mask`` / ``query_mask`` (``gta_amd.mask_index``: one launch builds every tensor the
             masked kernels read) -- a companion of the masks, as ``key_lens`` is of ``key_views``.  The call then builds nothing from the
             masks: forward, ``kv_cache``, backward and the rep-gradient pass run on the record's tensors, so one record serves every layer of
             a step, with results bit for bit those of the call without it.  The masks are still passed and every refusal above runs on
             them as before; the record is accepted only beside the very mask objects it was built from (an identity check: no compare,
             no sync) and on the call's device, anything else raises ``GtaError``.
    """
    route, cfg, mask, packed, carriers, trans_coeff, tau = _resolve(
        q, k, v, f_dims, packed, so3_degree=so3_degree, trans_coeff=trans_coeff, tau=tau, scale=scale, v_transform=v_transform, euclid=euclid,
        pretransformed=pretransformed, use_dma=use_dma, kv_mode=kv_mode, kv_cache=kv_cache, precise=precise, key_views=key_views,
        key_lens=key_lens, key_views_backward=key_views_backward, query_views=query_views, return_lse=return_lse, key_mask=key_mask,
        key_mask_backward=key_mask_backward, query_mask=query_mask, key_mask_rep_grad=key_mask_rep_grad, mask_index=mask_index,
        masked_lse_backward=masked_lse_backward, key_mask_generic=key_mask_generic)
    scale = cfg[4]
    if route == "staged":
        return _staged_forward(q, k, v, f_dims, packed, so3_degree, trans_coeff, tau, scale, v_transform, euclid, kv_cache,
                               key_views=mask.views and mask.views[1], key_lens=mask.key_lens, return_lse=return_lse,
                               mask=mask if mask.kind == "gather" else None)
    if route == "apply":
        return _generic_forward(q, k, v, f_dims, packed, so3_degree, trans_coeff, tau, scale, v_transform, euclid, precise=bool(precise),
                                carriers=carriers, return_lse=return_lse)
    if route == "fused":
        # (a cache serves the unmasked call alone here: a masked call under grad never reads or fills one -- the kv_cache refusal does not
        # look at tau, so such a call can come with a dict)
        if mask.kind is not None:
            kv_cache = None
        return (_FusedAttnLse if return_lse else _FusedAttn).apply(q, k, v, trans_coeff, tau, (cfg, kv_cache, mask),
                                                                   packed.get("vrep_q"), packed.get("vrep_k"), packed.get("cs_q"),
                                                                   packed.get("cs_k"), *carriers)
    c = _fused_forward(q, k, v, cfg, kv_cache, mask, packed, trans_coeff, tau)[0]
    return (c.out, c.lse) if return_lse else c.out


def _resolve(q, k, v, f_dims, packed, *, so3_degree, trans_coeff, tau, scale, v_transform, euclid, pretransformed, use_dma, kv_mode, kv_cache,
             precise, key_views, key_lens, key_views_backward, query_views, return_lse, key_mask, key_mask_backward, query_mask,
             key_mask_rep_grad, mask_index=None, masked_lse_backward=False, key_mask_generic=False):
    """The host-only half of ``gta_attention`` (its arguments, the keyword-only ones by keyword): every refusal, in a fixed order, then how the call runs.
    -> (route, cfg, mask, packed, carriers, trans_coeff, tau): route 'fused' (through ``_FusedAttn``: every unmasked call, a masked one under
    grad), 'forward' (a masked call without grad: ``_fused_forward`` alone), 'staged' or 'apply' (``generic_route``; 'staged' with a mask
    record of kind "gather" for a key mask under ``key_mask_generic``);
    cfg = (f_dims, so3_degree, Nq, Nk, scale, flags), flags None off the fused routes; the ``_Mask`` record; the tables the kernels read
    (detached) and their carriers (``repgrad.split_tables``); trans_coeff and tau as tensors or None."""
    shape, Tk = tuple(q.shape), k.shape[2]
    B, Tq = shape[0], shape[2]
    views_given = key_views is not None or key_lens is not None or key_views_backward or query_views is not None
    if key_mask_backward and key_mask is None and query_mask is None:
        raise native.GtaError("key_mask_backward=True comes with key_mask")
    if key_mask_generic and key_mask is None and query_mask is None:
        raise native.GtaError("key_mask_generic=True comes with key_mask")
    if key_mask_rep_grad and not key_mask_backward:
        raise native.GtaError("key_mask_rep_grad=True comes with key_mask_backward=True (the pose / coordinate gradients are a pass after "
                              "the masked backward)")
    if masked_lse_backward and not (key_views_backward or key_mask_backward):
        raise native.GtaError("masked_lse_backward=True comes with key_views_backward=True or key_mask_backward=True (it lets the masked "
                              "backward take the gradient of the log-sum-exp)")
    if query_mask is not None and views_given:
        raise native.GtaError("query_mask with key_views / query_views / key_lens / key_views_backward: a query mask runs on the key_mask "
                              "route -- say the valid views as a key_mask (and the valid query rows as the query_mask)")
    if query_mask is not None and kv_cache is not None:
        raise native.GtaError("query_mask with kv_cache: a cache serves later query sets, a query mask belongs to one (no cached query-mask "
                              "calls yet)")
    if key_mask is not None and views_given:
        raise native.GtaError("key_mask with key_views (or its companions): a call takes one key mask -- a prefix of views is a mask too")
    if query_views is not None and not key_views_backward:
        raise native.GtaError("query_views masks padded query rows in the backward: it needs key_views_backward=True")
    if key_views_backward and key_views is None:
        raise native.GtaError("key_views_backward=True comes with key_views")
    if key_lens is not None and key_views is None:
        raise native.GtaError("key_lens comes with the key_views it was built from")
    if scale is None:
        scale = shape[-1] ** -0.5
    # tables that require grad (poses / coordinates as autograd leaves): the kernels read detached tables, the gradients go to the carriers
    packed, carriers = _repgrad.split_tables(packed)
    if kv_cache is not None and torch.is_grad_enabled() and (carriers or any(torch.is_tensor(t) and t.requires_grad for t in (q, k, v, trans_coeff))):
        raise native.GtaError("kv_cache is an inference feature: call under torch.no_grad()")
    if carriers and pretransformed:
        raise native.GtaError("pretransformed=True: q, k, v already carry rho, so the tables get no gradient here")
    if isinstance(trans_coeff, (int, float)):
        trans_coeff = torch.tensor([float(trans_coeff)], device=q.device, dtype=torch.float32)
    if isinstance(tau, (int, float)):
        tau = None if float(tau) == 1.0 else torch.tensor([float(tau)], device=q.device, dtype=torch.float32)
    needs_grad = torch.is_grad_enabled() and (bool(carriers) or any(torch.is_tensor(t) and t.requires_grad for t in (q, k, v, trans_coeff, tau)))
    if return_lse and needs_grad and key_views_backward and not masked_lse_backward:
        raise native.GtaError("return_lse under grad with key_views_backward: gta_attn_bwd_varlen takes no gradient of the log-sum-exp "
                              "(drop return_lse, or call under torch.no_grad())")
    Nq, Nk = _views(f_dims, packed, q, k)
    masked = key_mask is not None or query_mask is not None
    if key_views is not None:
        key_views = check_key_views(key_views, B, Nk if "vrep_k" in packed else None)
        _refuse_uneven("key_views", "key", Tk, Nk)
        if query_views is not None:
            query_views = check_key_views(query_views, B, Nq if "vrep_q" in packed else None, name="query_views")
            _refuse_uneven("query_views", "query", Tq, Nq)
        if key_views_backward:
            _refuse_cpu_carriers("key_views_backward", "gta_rep_grad_sums_varlen", carriers)
    if masked:
        if key_mask is not None:
            check_key_mask(key_mask, B, Tk)
        if query_mask is not None:
            check_query_mask(query_mask, B, Tq)
        if key_mask_backward and needs_grad:
            if carriers and key_mask_rep_grad:
                if key_mask is not None:
                    _refuse_uneven("key_mask_rep_grad", "key", Tk, Nk)
                if query_mask is not None:
                    _refuse_uneven("key_mask_rep_grad", "query", Tq, Nq)
                _refuse_cpu_carriers("key_mask_rep_grad", "gta_rep_grad_sums_masked", carriers)
            elif carriers:
                raise native.GtaError("key_mask_backward: no pose / coordinate gradients under a key mask yet (gta_rep_grad_sums_varlen knows "
                                      "prefixes only): detach the rep tables and poses")
            if return_lse and not masked_lse_backward:
                raise native.GtaError("return_lse under grad with key_mask_backward: gta_attn_bwd_gather takes no gradient of the log-sum-exp "
                                      "(drop return_lse, or call under torch.no_grad())")
    how = dict(v_transform=v_transform, euclid=euclid, precise=bool(precise), needs_grad=needs_grad)
    if masked:          # (key_views and its companions beside a mask were refused above)
        how.update(key_mask=True, key_mask_backward=bool(key_mask_backward), key_mask_generic=bool(key_mask_generic))
    else:
        how.update(key_views=key_views is not None, key_views_backward=bool(key_views_backward))
    flags = attention_route(shape, Tk, q.dtype, f_dims, so3_degree, Nq, Nk, pretransformed=pretransformed, use_dma=use_dma,
                            kv_mode=kv_mode, kv_cache=kv_cache is not None, **how)
    if mask_index is not None:          # (behind every refusal of the masks themselves: their messages are what they were)
        _check_mask_index(mask_index, key_mask, query_mask, B, Tq, Tk, q.device)
    cfg = ({k_: int(v_) for k_, v_ in f_dims.items()}, int(so3_degree), Nq, Nk, float(scale), flags)
    if masked and flags is None:
        # a staged generic layout under key_mask_generic (without it attention_route raised "no gather pre-pass"); never under grad
        if query_mask is not None:
            raise native.GtaError("query_mask: the staged generic layouts (t2, euclid, so3 of degree 1, unaligned slabs) have no query-side "
                                  "mask (key_mask_generic serves the key side alone)")
        return "staged", cfg, _gather_mask(key_mask, None, q, k, False, (), mask_index), packed, carriers, trans_coeff, tau
    if masked:
        mask = _gather_mask(key_mask, query_mask, q, k, needs_grad, carriers, mask_index)
        return "fused" if needs_grad else "forward", cfg, mask, packed, carriers, trans_coeff, tau
    # no fused kernel: 'staged' or 'apply' (under key_views: 'staged', or it raises)
    route = generic_route(shape, Tk, q.dtype, f_dims, so3_degree, Nq, Nk, **how) if flags is None else "fused"
    if route == "apply" and return_lse and needs_grad and precise and q.dtype == torch.float32:
        raise native.GtaError("return_lse under grad with precise=True at this layout: the exact-fp32 backward (gta_plain32) takes no "
                              "gradient of the log-sum-exp; the fused fp32-faithful backward (float32, dh <= 64, fused layouts) does")
    mask = _NO_MASK
    if key_views is not None:
        # (under grad: key_views_backward -- anything else was refused above, return_lse included; query_views masks the backward alone)
        mask = _views_mask(key_views, key_lens, query_views if needs_grad and route == "fused" else None, q, k, Nq, Nk)
        route = "forward" if route == "fused" and not needs_grad else route
    return route, cfg, mask, packed, carriers, trans_coeff, tau


class _MergeAttn(torch.autograd.Function):
    """``gta_attention_merge``: (out_1..n, lse_1..n) -> (out, lse) through gta_attn_merge, backward through gta_attn_merge_bwd"""

    @staticmethod
    def forward(ctx, n, *ts):
        ctx.set_materialize_grads(False)
        outs, lses = [_as_kernel_layout(t.detach()) for t in ts[:n]], [t.detach() for t in ts[n:]]
        B, H, Tq, dh = outs[0].shape
        out = torch.empty(B, Tq, H, dh, device=outs[0].device, dtype=outs[0].dtype).permute(0, 2, 1, 3)
        lse = torch.empty(B, H, Tq, device=outs[0].device, dtype=torch.float32)
        native.attn_merge(outs, lses, out, lse)
        ctx.n = n
        ctx.save_for_backward(*outs, *lses)
        return out, lse

    @staticmethod
    def backward(ctx, dout, dlse):
        n = ctx.n
        outs, lses = ctx.saved_tensors[:n], ctx.saved_tensors[n:]
        B, H, Tq, dh = outs[0].shape
        dev, dt = outs[0].device, outs[0].dtype
        dout = torch.zeros(B, Tq, H, dh, device=dev, dtype=dt).permute(0, 2, 1, 3) if dout is None else _as_kernel_layout(dout.to(dt))
        douts = [torch.empty(B, Tq, H, dh, device=dev, dtype=dt).permute(0, 2, 1, 3) for _ in range(n)]
        dlses = [torch.empty(B, H, Tq, device=dev, dtype=torch.float32) for _ in range(n)]
        native.attn_merge_bwd(outs, lses, dout, None if dlse is None else dlse.to(torch.float32), douts, dlses)
        return (None, *douts, *dlses)


def gta_attention_merge(outs, lses):
    """Combine n (1..8) partial attentions of the SAME queries over DISJOINT key sets -- each an ``(out_i, lse_i)`` of
    ``gta_attention(..., return_lse=True)`` -- into the attention over the union of the key sets: -> (out [B,H,Tq,dh], lse [B,H,Tq]).

    With a_i = softmax_i(lse_i) per query row: out = sum_i a_i out_i, lse = logsumexp_i(lse_i); differentiable in every out_i and lse_i
    (dout_i = a_i dout, dlse_i = a_i (dlse + <dout, out_i - out>)).  One HIP kernel each way (gta_merge.hip), fp32 arithmetic and one rounding
    to the dtype of ``outs``.  A partial whose lse_i is -inf on a row (it saw no key) is selected out, not multiplied: its out_i there may hold
    NaN; rows that are -inf in every partial give zeros and -inf.  dh % 8 == 0, dh <= 128."""
    outs, lses = list(outs), list(lses)
    if not 1 <= len(outs) <= native.MERGE_MAX or len(lses) != len(outs):
        raise native.GtaError(f"gta_attention_merge takes 1 to {native.MERGE_MAX} partial attentions, each an (out, lse) pair "
                              f"(got {len(outs)} outs, {len(lses)} lses)")
    return _MergeAttn.apply(len(outs), *outs, *lses)


_KEY_SIDE_TABLES = ("vrep_k", "cs_k", "coord_k", "grad_cs_k", "grad_coord_k")

# the keywords of ``gta_attention`` that mask a call, as the layers hand them on: masks and view counts first (absent when None), then the
# opt-in flags (absent unless set)
MASK_OPT_INS = ("key_views_backward", "key_mask_backward", "key_mask_rep_grad", "key_mask_generic")
MASK_KEYWORDS = ("key_views", "key_mask", "query_views", "query_mask", "mask_index") + MASK_OPT_INS
# what ``gta_attention_by_view_groups`` refuses: the key-side masks among them (a query mask and its opt-ins go to every group's call)
_NOT_PER_GROUP = ("kv_cache", "key_views", "key_lens", "key_views_backward", "query_views", "return_attmap", "key_mask", "mask_index")


def gta_attention_by_view_groups(q, k, v, f_dims: Dict[str, int], packed: dict, *, views_per_call: int, num_key_views: Optional[int] = None,
                                 **kw):
    """``gta_attention`` over a key side of ANY number of views: the key views are cut into groups of at most ``views_per_call``
    (<= GTA_MAX_VIEWS = 16, what one fused call takes; or a sequence of group sizes that add up to the number of key views), each group is one ``gta_attention(..., return_lse=True)`` call and the partial
    attentions are merged (``gta_attention_merge``, up to 8 at a time) -> out [B,H,Tq,dh], or (out, lse) with ``return_lse=True``.

    K and V of a group are token slices of k and v (tokens are view-major: no copy where the slice keeps 16-byte rows); the key-side tables'
    rows are copied per group (vrep_k per view, cs_k / coord_k per token).  The number of key views is that of ``packed['vrep_k']``;
    a layout without view tables says it with ``num_key_views``.  Differentiable wherever ``gta_attention(..., return_lse=True)`` is.  Every
    other keyword goes to ``gta_attention``; ``kv_cache``, ``key_views`` (with its companions), ``key_mask``, ``mask_index`` and ``return_attmap`` are refused.
    Under a ``query_mask`` (scenes with different numbers of target rays) the call is trainable with ``key_mask_backward=True,
    masked_lse_backward=True`` -- every group's call is a ``return_lse=True`` call under the query mask --, ``key_mask_rep_grad=True``
    included; dead rows get out = +0.0, dq = +0.0 and may hold NaN in q and in the ``dout`` that reaches the merged output."""
    for name in _NOT_PER_GROUP:
        if kw.get(name) is not None and kw.get(name) is not False:
            raise native.GtaError(f"gta_attention_by_view_groups takes no {name}: every group is a call of its own")
    return_lse = bool(kw.get("return_lse", False))
    kw = {n_: v_ for n_, v_ in kw.items() if n_ not in _NOT_PER_GROUP + ("return_lse",)}
    sizes = None if isinstance(views_per_call, (int, np.integer)) and not isinstance(views_per_call, bool) else views_per_call
    try:
        sizes = None if sizes is None else [int(x) for x in sizes if not isinstance(x, bool) and isinstance(x, (int, np.integer))]
        bad = sizes is not None and (len(sizes) != len(tuple(views_per_call)) or not sizes)
    except TypeError:
        bad = True
    if bad or any(not 1 <= x <= native.MAX_VIEWS for x in (sizes if sizes is not None else [views_per_call])):
        raise native.GtaError(f"views_per_call must be an integer (or a sequence of group sizes) in 1..GTA_MAX_VIEWS = 1..{native.MAX_VIEWS}, "
                              f"got {views_per_call!r}")
    Nk = packed["vrep_k"].shape[1] if "vrep_k" in packed else num_key_views
    if Nk is None:
        raise native.GtaError("gta_attention_by_view_groups: this layout has no view tables (vrep_k): pass num_key_views")
    Tk = k.shape[2]
    if Nk < 1 or Tk % Nk:
        raise native.GtaError(f"gta_attention_by_view_groups: {Tk} key tokens do not split evenly into {Nk} views")
    Pk = Tk // Nk
    if sizes is None:
        sizes = [min(int(views_per_call), Nk - g0) for g0 in range(0, Nk, int(views_per_call))]
    elif sum(sizes) != Nk:
        raise native.GtaError(f"views_per_call: the group sizes {sizes} do not add up to the {Nk} key views")
    partials, g1 = [], 0
    for n_views in sizes:
        g0, g1 = g1, g1 + n_views
        t0, t1 = g0 * Pk, g1 * Pk
        sub = dict(packed)
        for name in _KEY_SIDE_TABLES:
            if torch.is_tensor(packed.get(name)):
                sub[name] = (packed[name][:, g0:g1] if name == "vrep_k" else packed[name][:, t0:t1]).contiguous()
        partials.append(gta_attention(q, k[:, :, t0:t1], v[:, :, t0:t1], f_dims, sub, return_lse=True, **kw))
    # (more than 8 groups: merge in rounds of 8 -- a merge of merges is the merge)
    while len(partials) > 1:
        partials = [gta_attention_merge([p_[0] for p_ in partials[i:i + native.MERGE_MAX]], [p_[1] for p_ in partials[i:i + native.MERGE_MAX]])
                    for i in range(0, len(partials), native.MERGE_MAX)]
    return partials[0] if return_lse else partials[0][0]


# kv_mode name -> flags of its tuning knob; every name but 'auto' and 'fused' asks for the two-stage plan ('prepass')
KV_MODES = {
    "auto": 0, "fused": 0, "prepass": 0,
    "prepass_pg": native.FLAG_PERSIST,                                  # persistent grid instead of one workgroup per query tile
    "prepass_rows32": native.FLAG_ROWS32,                               # the 32-rows-per-wave attention kernel where the 64-rows one would run
    "prepass_fwd2": native.FLAG_ROWS32 | native.FLAG_FWD2_GENERIC,      # (r06) gta_fwd2_kernel where the dh = 64 bf16 instance gta_fwdc_kernel would run
    "prepass_item_cxx": native.FLAG_ITEM_CXX,                           # the 64-rows kernel with its compiler-scheduled item prologue / epilogue
    # the backward's: the 32-keys-per-wave dK/dV kernel / the generated 64-keys streams whatever the size / the dQ and dK/dV kernels (whichever
    # pair the size selects; keys64_split: the generated pair) as two launches instead of the joint one
    "prepass_bwd_keys32": native.FLAG_BWD_KEYS32,
    "prepass_bwd_keys64": native.FLAG_BWD_KEYS64,
    "prepass_bwd_split": native.FLAG_BWD_SPLIT,
    "prepass_bwd_keys64_split": native.FLAG_BWD_KEYS64 | native.FLAG_BWD_SPLIT,
}


def attention_route(q_shape, Tk: int, dtype, f_dims: Dict[str, int], so3_degree: int, Nq: int, Nk: int, *, v_transform: bool = True,
                    euclid: bool = False, pretransformed: bool = False, use_dma: bool = True, kv_mode: str = "auto",
                    kv_cache: bool = False, precise: bool = False, needs_grad: bool = False, key_views: bool = False,
                    key_views_backward: bool = False, key_mask: bool = False, key_mask_backward: bool = False,
                    key_mask_generic: bool = False) -> Optional[int]:
    """How ``gta_attention`` runs a call: the descriptor flags of the fused path, or None for the generic one (rho-apply kernels around the
    plain attention kernel).  q_shape = (B, H, Tq, dh); Tk keys; dtype of q.

    Sizes alone decide: the library is asked about a descriptor at contiguous strides, and its answers do not depend on strides that pass
    its row-alignment check -- those and the ones ``_as_kernel_layout`` hands the kernels both do.

    key_views=True (the call comes with per-scene view counts): the flags are those of ``gta_attn_fwd_varlen`` -- always the two-stage plan,
    whatever ``kv_mode`` 'auto' would pick for the shape -- or None for the generic layouts (``generic_route`` then answers for its varlen
    entry); the combinations that have no masked kernel raise ``GtaError``.  key_views_backward=True lets needs_grad through: the same flags
    serve ``gta_attn_bwd_varlen``.

    key_mask=True (the call comes with a key mask): the flags of ``gta_attn_fwd_gather`` -- the two-stage plan --, never None: the layouts
    without a fused kernel have no gather pre-pass and raise ``GtaError`` like every other combination without one.  key_mask_backward=True
    lets needs_grad through: the same flags serve ``gta_attn_bwd_gather``.  key_mask_generic=True (beside key_mask) changes nothing on a fused
    layout; on a layout without a fused kernel the answer is then None -- ``generic_route`` answers for the gather entry of the staged kernels
    (``gta_attn_fwd_staged_gather``) and says every refusal of it, a call under grad among them."""
    if kv_mode not in KV_MODES:
        raise ValueError(f"kv_mode {kv_mode!r}")
    flags = KV_MODES[kv_mode] | _layout_flags(v_transform, euclid) | (0 if use_dma else native.FLAG_NO_DMA)
    probe = lambda fl: _probe(dtype, q_shape, Tk, f_dims, so3_degree, Nq, Nk, fl)
    if key_mask:
        if key_views:
            raise native.GtaError("key_mask with key_views: a call takes one key mask")
        _mask_refusals("key_mask", needs_grad=needs_grad, precise=precise, pretransformed=pretransformed, kv_mode=kv_mode,
                       backward=key_mask_backward)
        rc = native.attn_fwd_supported(probe(flags))
        if rc == native.E_UNSUPPORTED and key_mask_generic:         # a generic layout under the opt-in: the staged gather entry, or its refusals
            generic_route(q_shape, Tk, dtype, f_dims, so3_degree, Nq, Nk, v_transform=v_transform, euclid=euclid, precise=precise,
                          needs_grad=needs_grad, key_mask_generic=True)
            return None
        if rc == native.E_UNSUPPORTED:
            raise native.GtaError(_NO_GATHER_PREPASS + f"gta_attn_fwd_supported: {native.lib().gta_strerror(rc).decode()}")
        native.check(native.attn_fwd_gather_supported(probe(flags)), "gta_attn_fwd_gather_supported")
        return flags
    if key_views:
        _mask_refusals("key_views", needs_grad=needs_grad, precise=precise, pretransformed=pretransformed, kv_mode=kv_mode,
                       backward=key_views_backward)
        if native.attn_fwd_supported(probe(flags)) == native.E_UNSUPPORTED:         # a generic layout
            return None
        # a fused layout: what the varlen entry refuses now is a flag (GTA_FLAG_FUSED_KV, ...), and that is said, not routed elsewhere
        native.check(native.attn_fwd_varlen_supported(probe(flags)), "gta_attn_fwd_varlen_supported")
        return flags
    if pretransformed:
        flags |= native.FLAG_PRETRANSFORMED
    if precise:
        if dtype != torch.float32:
            raise native.GtaError("precise=True is for float32 inputs (bf16 inputs ask for bf16 arithmetic)")
        flags |= native.FLAG_FP32_PRODUCTS
    Tq = q_shape[2]
    route = "prepass" if kv_cache or kv_mode.startswith("prepass") else kv_mode
    if route == "auto":
        route = "prepass" if Tq > 256 else "fused"
    if precise and route == "prepass" and not pretransformed and native.attn_fwd_workspace_bytes(probe(flags)) == 0:
        # r05: the mode has a two-stage plan of its own at dh <= 64 (CLEVR-TR, the reference's fp32 config) -- the pre-pass writes hi and lo
        # images, the 32-row kernel runs three MFMAs per product; other head sizes keep the single-kernel plan
        if kv_cache:
            raise native.GtaError("precise=True at this head size runs the single-kernel plan: no kv_cache")
        route = "fused"
    if route == "fused" or not use_dma:
        flags |= native.FLAG_FUSED_KV
    if precise and needs_grad and not pretransformed:
        # fp32-faithful TRAINING.  r06: where the fused kernels have split-bf16 instances on BOTH sides (fp32 inputs at dh <= 64: the two-stage forward
        # of r05 and the X3 walks of gta_bwd.hip) the call stays on the fused path -- hi / lo images, three MFMAs per product, rho and its adjoint in
        # fp32 inside the pre-passes and epilogues; the forward's images serve the backward -- on the two-stage plan whatever the number of query
        # rows.  Elsewhere, and when kv_mode='fused' asks for it by name: rho in fp32 (gta_rep_apply), split-bf16 plain forward, EXACT-fp32
        # backward (gta_plain32.hip) and the adjoint rho kernels -- the generic path serves every layout that way.
        flags &= ~native.FLAG_FUSED_KV        # (use_dma=False too ends on the two-stage plan here: kept as it was, changing it is a change of behaviour)
        return flags if kv_mode != "fused" and native.attn_fwd_workspace_bytes(probe(flags)) > 0 else None
    if not pretransformed and native.attn_fwd_supported(probe(flags)) == native.E_UNSUPPORTED:       # GTA_E_UNSUPPORTED: valid request, no fused kernel
        return None
    return flags


def _closure_has_tau(attn_fn) -> bool:
    """True when ``attn_fn`` is one of the reference's ``AttnFn`` / ``EuclidAttnFn`` instances (layers.py:202-224) --
    modules whose ``forward`` closes over the constructor's local ``tau`` -- and that ``tau`` is a tensor, i.e. the
    parameter of ``TemperatureAdjsutableSoftmax`` (layers.py:135-143,195-197) rather than the constant 1.0."""
    for fn in (getattr(attn_fn, "forward", None), attn_fn):
        fn = getattr(fn, "__func__", fn)
        code, cells = getattr(fn, "__code__", None), getattr(fn, "__closure__", None)
        if code is None or not cells:
            continue
        for name, cell in zip(code.co_freevars, cells):
            try:
                val = cell.cell_contents
            except ValueError:
                continue
            if name == "tau" and torch.is_tensor(val):
                return True
    return False


def multihead_geometric_transform_attention(q, k, v, attn_fn=None, f_dims=None, reps=None,
                                            trans_coeff=1.0, v_transform=True, euclid=False, key_views=None, key_views_backward=False,
                                            query_views=None, **kwargs):
    """Drop-in for gta.py:92-279.  Returns ``(out_t, None)``.

    Args mirror the reference: q [B,H,Nq*Tq,C]; k, v [B,H,Nk*Tk,C]; ``f_dims`` the slab sizes;
    ``reps`` the dict filled by ``pre_compute_reps`` (reference-style tensors or this package's
    packed tables); ``trans_coeff`` a scalar or the layer's 1-element parameter.

    Softmax temperature (``softmax: adjustable``, layers.py:135-143,195-200): the reference's ``AttnFn`` /
    ``EuclidAttnFn`` capture tau in a closure and expose only ``.scale``, so a reference-style ``attn_fn`` cannot
    hand it over -- pass ``tau=self.attend.tau`` (level 2).  An ``attn_fn`` that is one of the
    reference's closures over a module with a ``tau`` parameter and no ``tau=`` keyword raises instead of silently
    running with tau = 1.

    Arithmetic: products run on the bf16 MFMA with fp32 accumulation for fp32 inputs too (rho and the softmax are
    fp32); see DESIGN.md section 7 for the measured gap to the fp32 reference.

    ``key_views``: per-scene numbers of valid input views (``gta_attention``); inference only unless ``key_views_backward=True``, with which
    ``query_views`` masks padded query rows in the backward (``gta_attention``).
    """
    if f_dims is None or reps is None:
        raise TypeError("f_dims and reps are required")
    f_dims = {k_: v_ for k_, v_ in f_dims.items() if k_ in GROUP_ORDER}
    packed = pack_reps(reps, f_dims)
    scale = getattr(attn_fn, "scale", None)
    tau = kwargs.get("tau", getattr(attn_fn, "tau", None))
    if "tau" not in kwargs and not hasattr(attn_fn, "tau") and _closure_has_tau(attn_fn):
        raise native.GtaError("attn_fn closes over a softmax temperature (softmax: adjustable, layers.py:195-200) that "
                              "this drop-in cannot see: pass tau=self.attend.tau")
    if f_dims.get("se3", 0) <= 0:
        trans_coeff = None
    out = gta_attention(q, k, v, f_dims, packed, so3_degree=_so3_degree(f_dims, packed, reps),
                        trans_coeff=trans_coeff, tau=tau, scale=scale, v_transform=v_transform, euclid=euclid,
                        use_dma=kwargs.get("use_dma", True), kv_mode=kwargs.get("kv_mode", "auto"),
                        precise=kwargs.get("precise"), **({"key_views": key_views} if key_views is not None else {}),
                        **({"key_views_backward": True} if key_views_backward else {}),
                        **({"query_views": query_views} if query_views is not None else {}))
    return out, None


def multihead_vecrep_attention(q, k, v, attn_fn=None, extras=None, **kwargs):
    """Drop-in for gta.py:282-298 (the ``elementwise_mul`` ablation): elementwise per-token vectors
    around plain softmax attention.  The products are torch elementwise ops, the attention is the
    fused kernel on an identity layout; everything is differentiable.  Returns ``(out, None)``."""
    scale = getattr(attn_fn, "scale", None)
    dh = q.shape[-1]
    qq = extras["vecrep_q"][:, None].to(q.dtype) * q
    kk = extras["vecrep_k"][:, None].to(q.dtype) * k
    vv = extras["vecrep_k"][:, None].to(q.dtype) * v
    out = gta_attention(qq, kk, vv, {"triv": dh}, {}, scale=scale, tau=kwargs.get("tau"), v_transform=False)
    return extras["vecinvrep_q"][:, None].to(q.dtype) * out, None


def attention_map(q, k, f_dims, packed, *, so3_degree=0, trans_coeff=None, tau=None, scale=None, euclid=False):
    """Dense softmax matrix [B,H,Tq,Tk] (what the reference returns as ``attn``, layers.py:207-211,441-442).
    Materialising it is the point of the request, so after the HIP rho-apply kernels the matrix itself is
    one batched GEMM + softmax in PyTorch-ROCm.  No gradient."""
    with torch.no_grad():
        if scale is None:
            scale = q.shape[-1] ** -0.5
        dt = q.dtype
        B, H, Tq, dh = q.shape
        Tk = k.shape[2]
        Nq, Nk = _views(f_dims, packed, q, k)
        flags = native.FLAG_V_TRANSFORM | (native.FLAG_EUCLID if euclid else 0)
        qp = torch.empty(B, H, Tq, dh, device=q.device, dtype=dt)
        kp = torch.empty(B, H, Tk, dh, device=q.device, dtype=dt)
        desc = native.make_desc(q, k.to(dt), k.to(dt), qp, f_dims, so3_degree, Nq, Nk, scale, flags)
        tc = trans_coeff.detach().float().reshape(-1) if torch.is_tensor(trans_coeff) else (
            torch.tensor([float(trans_coeff)], device=q.device) if trans_coeff is not None else None)
        kb = torch.zeros(B, H, (Tk + 63) // 64 * 64, device=q.device) if euclid else None
        native.rep_apply(desc, 0, q, packed.get("vrep_q"), packed.get("cs_q"), packed.get("coord_q"), tc, qp)
        native.rep_apply(desc, 1, k.to(dt), packed.get("vrep_k"), packed.get("cs_k"), packed.get("coord_k"), tc, kp, kb, scale)
        sim = torch.matmul(qp.float(), kp.float().transpose(-1, -2)) * scale
        if euclid:
            sim = sim + kb[..., None, :Tk]
        t = float(tau.item()) if torch.is_tensor(tau) else (tau or 1.0)
        return torch.softmax(sim / t, dim=-1)

"""Backward of the fused GTA attention (binds ``gta_attn_bwd`` of the C ABI).

Replaces PyTorch autograd over gta.py:92-279 + layers.py:202-211: three HIP kernels (q-side
pre-pass, dQ, dK/dV) plus a deterministic reduction for ``d trans_coeff``.
"""
import torch

from . import native
from .gta import _kernel_layout_ok


def packed_slices(ts) -> bool:
    """True when the [B,H,T,dh] tensors ``ts`` are slices 0..n-1 of ONE [B,T,n,H,dh] buffer (the packed projections
    of layers.py:389,394: ``to_qkv(x).view(B,T,3,H,dh)[:, :, i].permute(0,2,1,3)``)."""
    t0 = ts[0]
    n = len(ts)
    B, H, T, dh = t0.shape
    want = (T * n * H * dh, dh, n * H * dh, 1)
    esz = t0.element_size()
    return all(t.shape == t0.shape and t.dtype == t0.dtype and tuple(t.stride()) == want
               and t.data_ptr() == t0.data_ptr() + i * H * dh * esz for i, t in enumerate(ts))


def _grad_buffers(q, k, v):
    """dq, dk, dv in the memory layout of the forward's q, k, v: slices of one packed buffer when those were (so the
    gradient of the packed projection is that buffer, no gather), else separate [B,T,H,dh] buffers viewed [B,H,T,dh]."""
    B, H, Tq, dh = q.shape
    Tk = k.shape[2]
    new = lambda T, n: torch.empty(B, T, n, H, dh, device=q.device, dtype=q.dtype)
    if Tq == Tk and packed_slices((q, k, v)):
        g = new(Tq, 3)
        return tuple(g[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    dq = new(Tq, 1)[:, :, 0].permute(0, 2, 1, 3)
    if packed_slices((k, v)):
        g = new(Tk, 2)
        return (dq,) + tuple(g[:, :, i].permute(0, 2, 1, 3) for i in range(2))
    return dq, new(Tk, 1)[:, :, 0].permute(0, 2, 1, 3), new(Tk, 1)[:, :, 0].permute(0, 2, 1, 3)


def attn_bwd(cfg, q, k, v, out, dout, lse, tc, ta, vrep_q, vrep_k, cs_q, cs_k, kv_images=None, want_dtau=False, key_lens=None, q_lens=None,
             dlse=None, key_idx=None, q_live=None):
    """Returns (dq, dk, dv, dtrans_coeff or None, dtau or None); dtau ([1] fp32) only with ``want_dtau``.
    key_lens (with q_lens or None): ``gta_attn_bwd_varlen`` -- per-scene prefixes, kv_images those of ``attn_fwd_varlen`` under the same key_lens.
    key_idx (with key_lens, without q_lens): ``gta_attn_bwd_gather`` -- the keys of ``attn_fwd_gather``, kv_images those of that call under the same
    key_idx / key_lens; dk / dv rows of masked tokens are zeros.
    q_live (with key_idx and key_lens; q_lens allowed): ``gta_attn_bwd_qmask`` -- the query-side mask of ``attn_fwd_qmask``; dq rows of dead rows
    are zeros and nothing of them (q, out, dout, lse) is used.
    dlse ([B,H,Tq], the gradient of the forward's lse): ``gta_attn_bwd_dlse`` -- the backward of the pair (out, lse); with key_lens, key_idx or
    q_live the ``_dlse`` twin of that entry (``gta_attn_bwd_varlen_dlse`` / ``_gather_dlse`` / ``_qmask_dlse``), where a dead row's dlse is never read."""
    if q_live is not None and (key_idx is None or key_lens is None):
        raise native.GtaError("q_live comes with key_idx and key_lens (gta_attn_bwd_qmask runs on the key_mask route)")
    if key_idx is not None and (key_lens is None or (q_lens is not None and q_live is None)):
        raise native.GtaError("key_idx comes with key_lens and without q_lens (gta_attn_bwd_gather has no query-side mask)")
    f_dims, so3_degree, Nq, Nk, scale, flags = cfg
    flags = flags & ~(native.FLAG_FUSED_KV | native.FLAG_KV_READY | native.FLAG_PREP_ONLY | native.FLAG_PERSIST)      # (GTA_FLAG_FP32_PRODUCTS stays: the X3 walks)
    dt = q.dtype
    dout = dout.to(dt)
    if not _kernel_layout_ok(dout):
        dout = dout.contiguous()
    B, H, Tq, dh = q.shape
    Tk = k.shape[2]
    # gradients in the projections' memory order (packed like the forward's q, k, v where those were packed)
    dq, dk, dv = _grad_buffers(q, k, v)
    # (both scalars are WRITTEN by the library -- the fixed-order reduction stores its sum -- so no zero-fill launch)
    dtc = torch.empty(1, device=q.device, dtype=torch.float32) if f_dims.get("se3", 0) > 0 else None
    desc = native.make_desc(q, k, v, out, f_dims, so3_degree, Nq, Nk, scale, flags)
    ws = torch.empty(native.attn_bwd_workspace_bytes(desc), device=q.device, dtype=torch.uint8)
    dta = torch.empty(1, device=q.device, dtype=torch.float32) if (want_dtau and ta is not None) else None
    if dlse is not None:
        dlse = dlse.to(torch.float32).contiguous()
        if q_live is not None:
            native.attn_bwd_qmask_dlse(desc, q, k, v, out, dout, lse, dlse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, key_idx, key_lens, q_live, q_lens,
                                       kv_images, dq, dk, dv, dtc, ws, dta)
        elif key_idx is not None:
            native.attn_bwd_gather_dlse(desc, q, k, v, out, dout, lse, dlse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, key_idx, key_lens, kv_images,
                                        dq, dk, dv, dtc, ws, dta)
        elif key_lens is not None:
            native.attn_bwd_varlen_dlse(desc, q, k, v, out, dout, lse, dlse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, key_lens, q_lens, kv_images,
                                        dq, dk, dv, dtc, ws, dta)
        else:
            native.attn_bwd_dlse(desc, q, k, v, out, dout, lse, dlse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, kv_images, dq, dk, dv, dtc, ws, dta)
    elif q_live is not None:
        native.attn_bwd_qmask(desc, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, key_idx, key_lens, q_live, q_lens, kv_images,
                              dq, dk, dv, dtc, ws, dta)
    elif key_idx is not None:
        native.attn_bwd_gather(desc, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, key_idx, key_lens, kv_images, dq, dk, dv, dtc, ws, dta)
    elif key_lens is not None:
        native.attn_bwd_varlen(desc, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, key_lens, q_lens, kv_images, dq, dk, dv, dtc, ws, dta)
    else:
        native.attn_bwd(desc, q, k, v, out, dout, lse, vrep_q, vrep_k, cs_q, cs_k, tc, ta, kv_images, dq, dk, dv, dtc, ws, dta)
    return dq, dk, dv, dtc, dta

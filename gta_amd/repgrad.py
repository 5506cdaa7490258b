"""Gradients of GTA attention w.r.t. its representations: camera poses and patch coordinates.

The reference applies its reps with differentiable einsums (gta.py:134-279), so ``loss.backward()`` reaches the extrinsics and the
token coordinates; only the Wigner-D blocks are cut (gta.py:194-197,267).  Here the attention backward returns dq, dk, dv as before;
when a table requires a gradient, one more pass (``gta_rep_grad_sums``, gta_repgrad.hip) reduces outer products of those with the
forward's operands into per-view 4x4 and per-token 2x2 / 3x3 sums, and the small-matrix algebra below maps them to the tables'
gradients (INTEGRATION.md "Gradients to poses and coordinates").

Sums of a b^T, per batch, over heads, the tokens of a view (se3) or one token (so2, t2) and the slab's channel groups:
    query side   (q, dq), (dout, out)       generic path: (q, dq'), (dout, o~)       [euclid se3: (dq', [q;1]) and (dout, [o~;1])]
    key side     (dk, k), (dv, v)           generic path: (dk', k), (dv', v)          [euclid se3: b homogenised]
the second pair only under v_transform.  ``direct`` marks sums taken in the transformed space (generic path): they are the gradients
of the matrices as applied; the fused path's sums are in the input space and go back through the matrix (A^-T, B^-T, R).

Batches that mix view counts (``key_views_backward=True``): the sums come from ``gta_rep_grad_sums_varlen`` over each scene's prefix, and
the algebra runs under masks built from the host view counts -- a padded view's matrix is never inverted, padded entries are selected to
exact zero.

Key and query masks (``key_mask_rep_grad=True``): the sums come from ``gta_rep_grad_sums_masked`` over the live tokens alone, and the
algebra runs under the device masks themselves -- a token is live when its byte is set, a view when one of its tokens is; nothing is
read back.
"""
from __future__ import annotations

import math

import torch

from . import native

TABLES = ("vrep_q", "vrep_k", "cs_q", "cs_k", "coord_q", "coord_k")
INV = slice(native.VREP_INV, native.VREP_INV + 16)
REP = slice(native.VREP_REP, native.VREP_REP + 16)


# --------------------------------------------------------------------------------------------
# which tables want a gradient
# --------------------------------------------------------------------------------------------
def split_tables(packed: dict):
    """packed tables -> (tables the kernels read, carriers).  A carrier is the tensor a table's gradient is returned for: the table
    itself when it requires grad (the builders of gta_amd.reps), or the reference-style dense tensor ``pack_reps`` put under
    ``grad_<name>`` (so2 rotation blocks [B,T,2F,2,2], t2 matrices [B,T,3,3]).  When no carrier wants a gradient: (packed, ())."""
    if not torch.is_grad_enabled():
        return packed, ()
    tables, carriers = dict(packed), []
    for name in TABLES:
        t, c = packed.get(name), packed.get("grad_" + name)
        if torch.is_tensor(t) and t.requires_grad:
            c = t if c is None else c
            tables[name] = t.detach()
        carriers.append(c if torch.is_tensor(c) and c.requires_grad else None)
    if all(c is None for c in carriers):
        return packed, ()
    return tables, tuple(carriers)


def carrier_meta(carriers):
    """(shape, dtype) of each carrier (what the backward needs of them), None where absent"""
    return tuple(None if c is None else (tuple(c.shape), c.dtype) for c in carriers)


# --------------------------------------------------------------------------------------------
# the algebra (fp64, per view / per token: tiny)
# --------------------------------------------------------------------------------------------
def scale_mask(tc, device) -> torch.Tensor:
    """gta.py:40-44 in fp64: ones, translation column (rows 0..2) = trans_coeff, last row [0,0,0,1]"""
    m = torch.ones(4, 4, dtype=torch.float64, device=device)
    m[3, :3] = 0.0
    if tc is not None:
        m[:3, 3] = tc.detach().double().reshape(-1)[0] if torch.is_tensor(tc) else float(tc)
    return m


def live_mask(counts, n: int, per: int, device) -> torch.Tensor:
    """[B, n * per] bool: entry i of scene b is live when i < counts[b] * per.  ``counts``: the validated HOST tuple of per-scene view
    counts (``key_views`` / ``query_views``); per = 1: a mask of the n views, per = P: of the n * P tokens.  Built on the device from the
    host tuple: nothing is read back."""
    lim = (torch.tensor(counts, dtype=torch.int64) * per).to(device, non_blocking=True)
    return torch.arange(n * per, device=device)[None, :] < lim[:, None]


def view_grad(side: int, S, vrep, tc, direct: bool, euclid: bool = False, S_out=None, live=None) -> torch.Tensor:
    """d vrep [B,N,72] (fp64; the E and inv(E) slots, zero elsewhere) from the view sums S [B,N,4,4].
    side 0: the q side's matrix A = E.m (q' = A^T q, out = A o~): dA = S A^-T (fused) or S (direct).
    side 1: B = inv(E_k).m (k' = B k, v' = B v): dB = B^-T S (fused) or S (direct).
    euclid (affine maps, generic path): S is the gradient of the matrix as applied -- query side S of (dq', [q;1]) for the
    inv(E_q) slot and S_out of (dout, [o~;1]) for the E_q slot; key side S of (dk', [k;1]) + (dv', [v;1]).
    live [B,N] bool (None: every view): a padded view's record may hold anything, a singular or non-finite matrix included -- the identity
    stands in for it before the inverse, and with its zero sums (gta_rep_grad_sums_varlen) the view's gradient is exact zero."""
    S = S.double()
    if live is not None:
        S = torch.where(live[..., None, None], S, torch.zeros((), dtype=torch.float64, device=S.device))
    msk = scale_mask(tc, S.device)
    g = torch.zeros(*S.shape[:2], native.VREP_STRIDE, dtype=torch.float64, device=S.device)
    if euclid:
        g[..., REP] = (S * msk).flatten(-2)
        if side == 0 and S_out is not None:
            g[..., INV] = (S_out.double() * msk).flatten(-2)
        return g
    slot = INV if side == 0 else REP
    M = vrep[..., slot].double().reshape(S.shape) * msk
    if live is not None:
        M = torch.where(live[..., None, None], M, torch.eye(4, dtype=torch.float64, device=S.device))
    if direct:
        dM = S
    elif side == 0:
        dM = S @ torch.linalg.inv(M).transpose(-1, -2)
    else:
        dM = torch.linalg.inv(M).transpose(-1, -2) @ S
    g[..., slot] = (dM * msk).flatten(-2)
    return g


def so2_grad(side: int, T, cs, direct: bool, live=None) -> torch.Tensor:
    """dR [B,T,nb,2,2] (fp64) of the rotation blocks R = [[c,-s],[s,c]] from the per-token sums T [B,T,nb,2,2].
    q side (q' = R q, out = R^T o~): dR = R T^T (fused) or T^T (direct); k side (k' = R k, v' = R v): R T or T.
    live [B,T] bool (None: every token): a padded token's (cos, sin) may hold anything; its dR is selected to exact zero, not multiplied."""
    T = T.double()
    if side == 0:
        T = T.transpose(-1, -2)
    if not direct:
        c, s = cs[..., 0].double(), cs[..., 1].double()
        R = torch.stack([torch.stack([c, -s], -1), torch.stack([s, c], -1)], -2)
        T = R @ T
    return _select(live, T, 3)


def _select(live, x, trailing: int) -> torch.Tensor:
    """x where live ([B,T] bool, broadcast over ``trailing`` more dimensions), exact zero elsewhere; live None: x"""
    if live is None:
        return x
    return torch.where(live[(...,) + (None,) * trailing], x, torch.zeros((), dtype=x.dtype, device=x.device))


def so2_packed(dR, live=None) -> torch.Tensor:
    """dR of R = [[c,-s],[s,c]] [B,T,nb,2,2] -> d (cos, sin) [B,T,nb,2]; live [B,T] bool: exact zero at padded tokens"""
    return _select(live, torch.stack([dR[..., 0, 0] + dR[..., 1, 1], dR[..., 1, 0] - dR[..., 0, 1]], -1), 2)


def t2_packed(side: int, dM, live=None) -> torch.Tensor:
    """dM of the t2 matrix [B,T,3,3] -> d (cx, cy): q side A = inv(T) holds -c in row 2, k side T holds c; live as in so2_packed"""
    d = dM[..., 2, :2]
    return _select(live, -d if side == 0 else d, 1)


def table_grads(desc, tables: dict, meta, tc, q_pairs, k_pairs, direct: bool, euclid: bool = False, q_view_pairs=None,
                views=(None, None), lens=(None, None), masks=(None, None)):
    """The carriers' gradients (list of six, None where no gradient is asked): the sums of both sides through ``gta_rep_grad_sums``
    (one launch per side; under euclid two more for the query side's view sums), then the algebra above.
    views, lens: per side (query, key) the validated host tuple of per-scene view counts (``query_views`` / ``key_views``) with the device
    tensor of valid tokens built from it (``q_lens`` / ``key_lens``), or None for a side without padding.  A side that has them takes its
    sums through ``gta_rep_grad_sums_varlen`` -- nothing of a padded view is read -- and the algebra works under masks built from the
    host tuple: padded views' matrices are never inverted, and padded entries get exact zeros.
    masks: per side (query, key) a device bool [B, T] (True = a live token of that side), or None for a side without a mask.  A side that
    has one takes its sums through ``gta_rep_grad_sums_masked`` -- nothing of a dead token is read -- and the algebra works under
    live_t = mask, live_v = "the view has a live token", both built on the device without a sync: a view without a live token never has
    its matrix inverted and gets exact zeros, and so do a dead token's so2 / coordinate entries.  Not with ``views`` on the same side."""
    out = [None] * 6
    for side, mask in enumerate(masks):          # said by name, for either side, before anything is launched
        if mask is None:
            continue
        T, N = (desc.Tk, desc.Nk) if side else (desc.Tq, desc.Nq)
        if views[side] is not None:
            raise native.GtaError("table_grads: views= and masks= on the same side (a side has per-scene view counts or a mask, not both)")
        if euclid:
            raise native.GtaError("table_grads: masks= does not serve euclid layouts")
        if direct:
            raise native.GtaError("table_grads: masks= does not serve direct sums (the generic path): the fused layouts only")
        if T % N != 0:
            raise native.GtaError(f"table_grads: masks= needs tokens that split evenly into views: T % N != 0 (T = {T}, N = {N})")
        if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (desc.B, T):
            raise native.GtaError(f"table_grads: masks[{side}] is a bool [B, T] = [{desc.B}, {T}] tensor")
    for side, pairs in ((0, q_pairs), (1, k_pairs)):
        mv, mc, mo = meta[side], meta[2 + side], meta[4 + side]
        if mv is None and mc is None and mo is None:
            continue
        want_view, want_so2, want_t2 = mv is not None and desc.d_se3 > 0, mc is not None and desc.d_so2 > 0, mo is not None and desc.d_t2 > 0
        S = S_out = T2 = T3 = live_v = live_t = None
        if views[side] is not None:
            if euclid or direct or lens[side] is None:
                raise native.GtaError("table_grads: per-scene view counts serve the fused layouts, with the device lens beside the host counts")
            T, N = (desc.Tk, desc.Nk) if side else (desc.Tq, desc.Nq)
            dev = pairs[0][0].device
            live_v, live_t = live_mask(views[side], N, 1, dev), live_mask(views[side], N, T // N, dev)
        mask = masks[side]
        if mask is not None:
            T, N = (desc.Tk, desc.Nk) if side else (desc.Tq, desc.Nq)
            live_t, live_v = mask, mask.view(desc.B, N, T // N).any(-1)
        view_here = want_view and not (euclid and side == 0)
        if view_here or want_so2 or want_t2:
            S, T2, T3 = native.rep_grad_sums(desc, side, pairs, view=view_here, so2=want_so2, t2=want_t2,
                                             lens=lens[side] if views[side] is not None else None,
                                             **({} if mask is None else {"live": mask}))
        if want_view and not view_here:
            S = native.rep_grad_sums(desc, 0, q_view_pairs[:1], view=True)[0]
            if len(q_view_pairs) > 1:
                S_out = native.rep_grad_sums(desc, 0, q_view_pairs[1:], view=True)[0]
        if mv is not None:
            g = (view_grad(side, S, tables[TABLES[side]], tc, direct, euclid, S_out, live=live_v) if want_view
                 else torch.zeros(mv[0], dtype=torch.float64, device=q_pairs[0][0].device))
            out[side] = g.to(mv[1])
        if mc is not None:
            shape, dt = mc
            if not want_so2:
                out[2 + side] = torch.zeros(shape, dtype=dt, device=q_pairs[0][0].device)
            else:
                dR = so2_grad(side, T2, tables[TABLES[2 + side]], direct, live=live_t)
                out[2 + side] = (dR if len(shape) == 5 else so2_packed(dR, live_t)).reshape(shape).to(dt)
        if mo is not None:
            shape, dt = mo
            if not want_t2:
                out[4 + side] = torch.zeros(shape, dtype=dt, device=q_pairs[0][0].device)
            else:
                dM = _select(live_t, T3.double(), 2)  # t2 runs on the generic path only: sums in the transformed space
                out[4 + side] = (dM if len(shape) == 4 else t2_packed(side, dM, live_t)).reshape(shape).to(dt)
    return out


# --------------------------------------------------------------------------------------------
# the rep builders' chain rules
# --------------------------------------------------------------------------------------------
def extrinsic_grad(E, dvrep) -> torch.Tensor:
    """dE (fp64) from d vrep: the E slot directly, the inv(E) slot through d inv(E) = -inv(E) dE inv(E).
    A view whose incoming gradient is entirely zero (the padded views of a call with per-scene view counts) takes the identity for E
    before the inverse: exact for any call (-E^-T 0 E^-T = 0), and such a view's extrinsic may then hold anything, all zeros included."""
    E = E.double()
    shape = E.shape
    dinv = dvrep[..., INV].double().reshape(shape)
    drep = dvrep[..., REP].double().reshape(shape)
    idle = ((dinv == 0) & (drep == 0)).flatten(-2).all(-1)
    Ei = torch.linalg.inv(torch.where(idle[..., None, None], torch.eye(shape[-1], dtype=torch.float64, device=E.device), E))
    return dinv - Ei.transpose(-1, -2) @ drep @ Ei.transpose(-1, -2)


def so2_weights(nfreqs: int, max_freq_h: float, max_freq_w: float, shared_freqs: bool, device) -> torch.Tensor:
    """w [F, 2] with theta_{t, 2f+d} = w[f, d] coord_d  (gta.py:57-68; oracle/gta_oracle.py:40-60)"""
    f = torch.ones(nfreqs, dtype=torch.float64, device=device) if shared_freqs else \
        2.0 ** torch.arange(1, nfreqs + 1, dtype=torch.float64, device=device) / 2.0 ** nfreqs
    mf = torch.tensor([max_freq_h, max_freq_w], dtype=torch.float64, device=device)
    return 2.0 * math.pi * f[:, None] * mf[None, :]


def coord_grad(coord, dcs, nfreqs: int, max_freq_h: float, max_freq_w: float, shared_freqs: bool) -> torch.Tensor:
    """d coord [..., 2] (fp64) from d (cos, sin) [..., 2F, 2]: d theta = -sin dcos + cos dsin, then through theta = w coord.
    A token whose incoming gradient is entirely zero (padded tokens under per-scene view counts) takes coordinate 0 for the sines: its
    coordinates may hold anything, NaN and Inf included, and its gradient is exact zero."""
    w = so2_weights(nfreqs, max_freq_h, max_freq_w, shared_freqs, coord.device)
    dcs = dcs.double()
    idle = (dcs == 0).flatten(-2).all(-1)
    coord = torch.where(idle[..., None], torch.zeros((), dtype=torch.float64, device=coord.device), coord.double())
    th = (coord[..., None, :] * w).flatten(-2)                            # [..., 2F], block 2f + d
    dth = -torch.sin(th) * dcs[..., 0] + torch.cos(th) * dcs[..., 1]
    return (dth.unflatten(-1, (nfreqs, 2)) * w).sum(-2)


class ViewReps(torch.autograd.Function):
    """native.build_view_reps with the extrinsics' gradient (the Wigner-D slots carry none)."""

    @staticmethod
    def forward(ctx, E, so3_degree):
        ctx.save_for_backward(E)
        return native._build_view_reps(E, so3_degree)

    @staticmethod
    def backward(ctx, dvrep):
        E, = ctx.saved_tensors
        return extrinsic_grad(E, dvrep).to(E.dtype), None


class So2Table(torch.autograd.Function):
    """native.build_so2_table with the coordinates' gradient."""

    @staticmethod
    def forward(ctx, coord, nfreqs, mfh, mfw, shared):
        ctx.save_for_backward(coord)
        ctx.args = (nfreqs, mfh, mfw, shared)
        return native._build_so2_table(coord, nfreqs, mfh, mfw, shared)

    @staticmethod
    def backward(ctx, dcs):
        coord, = ctx.saved_tensors
        return coord_grad(coord, dcs, *ctx.args).to(coord.dtype), None, None, None, None


class Reps(torch.autograd.Function):
    """native.build_reps (both tables in one launch) with the extrinsics' and the coordinates' gradients."""

    @staticmethod
    def forward(ctx, E, coord, so3_degree, nfreqs, mfh, mfw, shared):
        ctx.save_for_backward(E, coord)
        ctx.args = (nfreqs, mfh, mfw, shared)
        return native._build_reps(E, so3_degree, coord, nfreqs, mfh, mfw, shared)

    @staticmethod
    def backward(ctx, dvrep, dcs):
        E, coord = ctx.saved_tensors
        dE = extrinsic_grad(E, dvrep).to(E.dtype) if ctx.needs_input_grad[0] else None
        dc = coord_grad(coord, dcs, *ctx.args).to(coord.dtype) if ctx.needs_input_grad[1] else None
        return dE, dc, None, None, None, None, None

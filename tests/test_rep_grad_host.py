"""CPU checks of the pose / coordinate gradient algebra (gta_amd.repgrad) and of the argument checks of gta_rep_grad_sums.

The sums the kernel produces are emulated here with einsum in fp64; fed to the algebra they must reproduce autograd through the oracle
(the reference's own differentiation) for the extrinsics, the coordinates and the dense tensors."""
import ctypes
from ctypes import c_int64, c_void_p

import pytest
import torch

from gta_amd import native
from gta_amd import repgrad as R
from oracle import gta_oracle as O
from tests import _repgrad_sums as S

# the sums the kernel produces, in fp64 (each emulator also returns its absprod twin, which the algebra has no use for)
_view_sums = lambda *a, **kw: S._view_sums(*a, **kw)[0]
_so2_sums = lambda *a: S._so2_sums(*a)[0]
_t2_sums = lambda *a: S._t2_sums(*a)[0]


def _close(got, ref, name):
    ref = torch.zeros_like(got) if ref is None else ref
    err = (got - ref).abs().max().item()
    assert err <= 1e-9 * max(1.0, ref.abs().max().item()), (name, err, ref.abs().max().item())


def _setup(f_dims, cross, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, Nk, Pk = 2, 3, 2, 6
    Nq, Pq = (3, 4) if cross else (Nk, Pk)
    ak = {"f_dims": f_dims, "so2": f_dims.get("so2", 0) // 4, "so3": 0, "max_freq_h": 1.0, "max_freq_w": 2.0}
    Ein = O.random_extrinsics(B, Nk, g, torch.float64).requires_grad_()
    cin = torch.rand(B, Nk * Pk, 2, generator=g, dtype=torch.float64).requires_grad_()
    ex = {"input_transforms": Ein, "input_coord": cin}
    leaves = {"Ein": Ein, "cin": cin}
    if cross:
        leaves["Et"] = ex["target_transforms"] = O.random_extrinsics(B, Nq, g, torch.float64).requires_grad_()
        leaves["ct"] = ex["target_coord"] = torch.rand(B, Nq * Pq, 2, generator=g, dtype=torch.float64).requires_grad_()
    dh = sum(f_dims.values())
    q = torch.randn(B, H, Nq * Pq, dh, generator=g, dtype=torch.float64).requires_grad_()
    k = torch.randn(B, H, Nk * Pk, dh, generator=g, dtype=torch.float64).requires_grad_()
    v = torch.randn(B, H, Nk * Pk, dh, generator=g, dtype=torch.float64).requires_grad_()
    return ak, ex, leaves, (q, k, v), (Nq, Nk), g


def _vrep(E):
    vr = torch.zeros(*E.shape[:2], native.VREP_STRIDE, dtype=torch.float64)
    vr[..., R.INV] = E.detach().reshape(*E.shape[:2], 16)
    vr[..., R.REP] = torch.linalg.inv(E.detach()).reshape(*E.shape[:2], 16)
    return vr


def _cs(coord, ak):
    th = O.so2_angles(coord.detach(), ak["so2"], (ak["max_freq_h"], ak["max_freq_w"]))
    return torch.stack([torch.cos(th), torch.sin(th)], -1)


@pytest.mark.parametrize("mode", ["fused", "generic", "euclid"])
@pytest.mark.parametrize("cross", [False, True])
def test_algebra_reproduces_oracle_autograd(mode, cross):
    euclid = mode == "euclid"
    if mode == "fused":
        f_dims = {"triv": 4, "se3": 8, "so2": 8}
    elif mode == "generic":
        f_dims = {"triv": 2, "se3": 8, "so2": 8, "t2": 6}
    else:
        f_dims = {"triv": 2, "se3": 6, "so2": 8}
    ak, ex, leaves, (q, k, v), (Nq, Nk), g = _setup(f_dims, cross, 1)
    reps = O.encoder_reps(ak, ex)
    if cross:
        reps = O.decoder_reps(ak, ex, reps)
    for key in ("se3rep_k", "so2rep_q", "so2rep_k", "t2rep_k", "inv_t2rep_q"):
        if key in reps and not reps[key].is_leaf:
            reps[key].retain_grad()
    tc = 0.7
    scale = 0.3
    qt, kt, vt = O.transform_qkv(q, k, v, f_dims, reps, tc, True, euclid)
    for t in (qt, kt, vt):
        t.retain_grad()
    o, _ = O.softmax_attention(qt, kt, vt, scale, 1.0, euclid)
    o.retain_grad()
    out = O.inverse_transform_out(o, f_dims, reps, tc, euclid)
    w = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * w).sum().backward()

    lo_se3, lo_so2 = f_dims["triv"], f_dims["triv"] + f_dims["se3"]
    lo_t2 = lo_so2 + f_dims["so2"]
    n_so2 = f_dims["so2"] // 2
    tct = torch.tensor([tc], dtype=torch.float64)
    direct = mode != "fused"
    if direct:
        qpairs, kpairs = [(q, qt.grad), (w, o)], [(kt.grad, k), (vt.grad, v)]
    else:
        qpairs, kpairs = [(q, q.grad), (w, out.detach())], [(k.grad, k), (v.grad, v)]
    qpairs = [(a.detach(), b.detach()) for a, b in qpairs]
    kpairs = [(a.detach(), b.detach()) for a, b in kpairs]
    Eq = leaves["Et"] if cross else leaves["Ein"]
    cq = leaves["ct"] if cross else leaves["cin"]
    W = 3 if euclid else 4
    if euclid:
        Sq = _view_sums([(qpairs[0][1], qpairs[0][0])], lo_se3, f_dims["se3"] // 3, 3, Nq, homog=True)
        Sq_out = _view_sums([qpairs[1]], lo_se3, f_dims["se3"] // 3, 3, Nq, homog=True)
    else:
        Sq, Sq_out = _view_sums(qpairs, lo_se3, f_dims["se3"] // 4, 4, Nq), None
    Sk = _view_sums(kpairs, lo_se3, f_dims["se3"] // W, W, Nk, homog=euclid)
    dvq = R.view_grad(0, Sq, _vrep(Eq), tct, direct, euclid, Sq_out)
    dvk = R.view_grad(1, Sk, _vrep(leaves["Ein"]), tct, direct, euclid)
    # the extrinsics (inv_se3rep_q IS the leaf E, so E.grad is what checks both slots); se3rep_k = inv(E_in) on its own
    if cross or not euclid:                         # (euclid self-attention applies se3rep_q = se3rep_k on the q side too)
        _close(dvk[..., R.REP].reshape(reps["se3rep_k"].shape), reps["se3rep_k"].grad, "d se3rep_k")
    if cross:
        _close(R.extrinsic_grad(Eq, dvq), Eq.grad, "d target_transforms")
        _close(R.extrinsic_grad(leaves["Ein"], dvk), leaves["Ein"].grad, "d input_transforms")
    else:
        _close(R.extrinsic_grad(Eq, dvq + dvk), Eq.grad, "d input_transforms")
    # so2: dense blocks and, through (cos, sin), the coordinates
    dRq = R.so2_grad(0, _so2_sums(qpairs, lo_so2, n_so2), _cs(cq, ak), direct)
    dRk = R.so2_grad(1, _so2_sums(kpairs, lo_so2, n_so2), _cs(leaves["cin"], ak), direct)
    args = (ak["so2"], ak["max_freq_h"], ak["max_freq_w"], False)
    dcq = R.coord_grad(cq, R.so2_packed(dRq), *args)
    dck = R.coord_grad(leaves["cin"], R.so2_packed(dRk), *args)
    if "t2" in f_dims:
        Tq, Tk = _t2_sums(qpairs, lo_t2, 2), _t2_sums(kpairs, lo_t2, 2)
        _close(Tq, reps["inv_t2rep_q"].grad, "d inv_t2rep_q")
        if cross:                                   # (self-attention: inv_t2rep_q = inv(t2rep_k) adds to t2rep_k's grad)
            _close(Tk, reps["t2rep_k"].grad, "d t2rep_k")
        dcq = dcq + R.t2_packed(0, Tq)
        dck = dck + R.t2_packed(1, Tk)
    if cross:
        _close(dRq, reps["so2rep_q"].grad, "d so2rep_q")
        _close(dcq, cq.grad, "d target_coord")
        _close(dck, leaves["cin"].grad, "d input_coord")
    else:
        _close(dRq + dRk, reps["so2rep_q"].grad, "d so2rep")
        _close(dcq + dck, cq.grad, "d input_coord")


def test_coord_grad_matches_autograd_of_the_angles():
    g = torch.Generator().manual_seed(3)
    c = torch.rand(2, 7, 2, generator=g, dtype=torch.float64).requires_grad_()
    for shared in (False, True):
        th = O.so2_angles(c, 3, (1.5, 0.5), shared)
        cs = torch.stack([torch.cos(th), torch.sin(th)], -1)
        d = torch.randn(cs.shape, generator=g, dtype=torch.float64)
        ref, = torch.autograd.grad((cs * d).sum(), c)
        _close(R.coord_grad(c, d, 3, 1.5, 0.5, shared), ref, "d coord")


def _args(desc, side=0, n_pairs=1, a0=16, view=64, so2=None, t2=None, ws=None, ws_bytes=0):
    st = (c_int64 * 3)(64, 32, 8)
    a = c_void_p(a0) if a0 is not None else None
    return (ctypes.byref(desc) if desc is not None else None, side, n_pairs, a, st, c_void_p(16), st, None, None, None, None,
            c_void_p(view) if view else None, c_void_p(so2) if so2 else None, c_void_p(t2) if t2 else None,
            c_void_p(ws) if ws else None, ws_bytes, None)


def test_abi_entry_rejects_bad_arguments_without_a_gpu():
    L = native.lib()
    desc = lambda **kw: native.make_desc_from(kw.pop("dtype", torch.bfloat16), (1, kw.pop("H", 2), 8, 8), 8,
                                              [(64, 32, 8)] * 4, kw.pop("f", {"se3": 4, "so2": 4}), 0, 1, 1, 0.3, kw.pop("flags", 0))
    call = lambda *a: L.gta_rep_grad_sums(*a)
    assert call(*_args(None)) == -1                                            # null descriptor
    d = desc()
    d.abi_version = 99
    assert call(*_args(d)) == -1                                               # another ABI
    d = desc()
    d.dtype = 7
    assert call(*_args(d, ws=256, ws_bytes=1 << 20)) == -1                     # dtype
    assert call(*_args(desc(), side=2)) == -1
    assert call(*_args(desc(), n_pairs=3)) == -1
    assert call(*_args(desc(), n_pairs=2)) == -1                               # second pair missing
    assert call(*_args(desc(), a0=None)) == -1                                 # null operand
    assert call(*_args(desc(), a0=17, ws=256, ws_bytes=1 << 20)) == -1         # misaligned bf16 operand
    assert call(*_args(desc(), view=None)) == -1                               # nothing asked
    assert call(*_args(desc())) == -1                                          # view sums without a workspace
    assert call(*_args(desc(f={"se3": 0, "so2": 8}), ws=256, ws_bytes=1 << 20)) == -1      # view sums of an empty slab
    assert call(*_args(desc(f={"se3": 6, "so2": 2}), ws=256, ws_bytes=1 << 20)) == -2      # 6 channels: not 4-channel groups
    assert call(*_args(desc(H=300), ws=256, ws_bytes=1 << 20)) == -3                       # more heads than a workgroup's threads
    assert b"256 heads" in L.gta_strerror(-3)
    assert L.gta_rep_grad_workspace_bytes(ctypes.byref(desc()), 0) == 1 * 1 * 1 * 16 * 4
    assert L.gta_rep_grad_workspace_bytes(ctypes.byref(desc()), 5) == -1

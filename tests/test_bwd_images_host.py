"""CPU: the model of the backward's workspace (tests/_bwd_images.py) -- the layout arithmetic against hand-computed offsets, the decoder's
round trip, the split of d trans_coeff into pre-pass / dQ / dK/dV terms against autograd through the oracle, rho_q against the oracle's q-side
transform, and the proof that the bars of tests/test_gpu_bwd_prep.py catch what they are meant to: a host-made workspace (the pre-pass emulated
in fp32, the walk slots from the bf16 emulation) passes every rule, and each deliberate defect fails exactly its own."""
import functools

import pytest
import torch

from oracle import gta_oracle as O
from tests import _bwd_images as W
from tests import _images as I


def test_layout_against_hand_computed_offsets():
    # B = H = 3, Tq = Tk = 150, dh = 64: stage = 2 * 64 * 64 * 2 = 16384; 27 tiles of it = 442368 (aligned); 27 * 512 B of statistics ->
    # 456192 (aligned); 27 + 18 + 18 = 63 partials = 252 B -> 456444, aligned 456448; 18 d tau slots = 72 B -> 456520, aligned 456704; then
    # 27 key tiles of 16384 -> 899072
    L = W.bwd_layout(3, 3, 150, 150, 64)
    assert (L.off_qimg, L.off_stats, L.off_dc, L.off_dt, L.off_kv, L.total) == (0, 442368, 456192, 456448, 456704, 899072)
    assert (L.n_prep, L.n_dq, L.n_dkv, L.stage) == (27, 18, 18, 16384)
    assert L.gaps == ((442368, 442368), (456192, 456192), (456444, 456448), (456520, 456704))
    # B = 1, H = 2, Tq = 140, Tk = 150, dh = 40 (padded 64), X3: stage = 4 * 8192 = 32768; 6 tiles = 196608; 6 * 512 -> 199680; 6 + 4 + 4 = 14
    # partials = 56 B -> 199736, aligned 199936; 4 d tau slots -> 199952, aligned 200192; 6 key tiles of 32768 -> 396800
    L = W.bwd_layout(1, 2, 140, 150, 40, x3=True)
    assert (L.off_qimg, L.off_stats, L.off_dc, L.off_dt, L.off_kv, L.total) == (0, 196608, 199680, 199936, 200192, 396800)
    assert (L.n_prep, L.n_dq, L.n_dkv, L.stage, L.dhp, L.nimg) == (6, 4, 4, 32768, 64, 4)


@pytest.mark.parametrize("x3", [False, True])
def test_decode_round_trip(x3):
    L = W.bwd_layout(2, 3, 100, 70, 40, x3=x3)
    g = torch.Generator().manual_seed(3)
    bits = I.bf16_bits(torch.randn(2, 3, L.n_qt, L.nimg, 64, L.dhp, generator=g))
    r = lambda *s: torch.randn(*s, generator=g)
    a, b, p, dq, dkv, dt = r(2, 3, L.n_qt * 64), r(2, 3, L.n_qt * 64), r(2, 3, L.n_qt), r(2, 3, L.n_q128), r(2, 3, L.n_k128), r(2, 3, L.n_q128)
    ws = W.encode_bwd(L, bits, a, b, p, dq, dkv, dt)
    assert ws.numel() == L.total
    d = W.decode_bwd(ws, L)
    assert torch.equal(d.bits, bits) and d.gaps_keep_fill
    assert torch.equal(d.q2, I.bits_to_f32(bits[:, :, :, 0]).reshape(2, 3, -1, L.dhp))
    assert torch.equal(d.do, I.bits_to_f32(bits[:, :, :, 1]).reshape(2, 3, -1, L.dhp))
    if x3:
        assert torch.equal(d.do_lo, I.bits_to_f32(bits[:, :, :, 3]).reshape(2, 3, -1, L.dhp))
    for got, want in ((d.neg_lse2, a), (d.neg_D, b), (d.dc_prep, p), (d.dc_dq, dq), (d.dc_dkv, dkv), (d.dt, dt)):
        assert torch.equal(got, want)
    # one unit by hand: unit c of row r of image i of tile (b, h, j) lies at its tile's base + i * img + (r * chp + swz(chp, r, c)) * 16
    b_, h_, j_, i_, r_, c_ = 1, 2, 1, L.nimg - 1, 37, 5
    off = ((b_ * 3 + h_) * L.n_qt + j_) * L.stage + i_ * L.img + (r_ * L.chp + I.swz(L.chp, r_, c_)) * 16
    assert torch.equal(ws[off:off + 16].view(torch.int16), bits[b_, h_, j_, i_, r_, 8 * c_:8 * c_ + 8])
    assert bool((W.decode_bwd(W.encode_bwd(L, bits, a, b, p, dq, dkv), L).dt_raw == -1).all())


LAYOUTS = {"se3+so2": ({"se3": 16, "so2": 16}, 0), "se3+so3+so2": ({"se3": 8, "so3": 8, "so2": 16}, 2), "triv": ({"triv": 8, "se3": 16, "so2": 8}, 0)}


def _oracle_dtc(c, tc, scale, tau, dlse=None):
    """autograd's d trans_coeff (and d tau) through oracle.gta_oracle in fp64"""
    reps64 = {n: ([t.double() for t in r] if isinstance(r, list) else r.double()) for n, r in c.reps.items()}
    tco = torch.tensor([tc], dtype=torch.float64, requires_grad=True)
    tauo = torch.tensor([1.0 if tau is None else tau], dtype=torch.float64, requires_grad=True)
    out, _ = O.gta_attention(c.q.double(), c.k.double(), c.v.double(), c.f_dims, reps64, tco, True, False, scale, tauo)
    (out * c.dout.double()).sum().backward()
    return float(tco.grad), float(tauo.grad), out.detach()


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_partials_sum_to_autograd_dtrans_coeff(layout, cross):
    """pre-pass partials + dQ groups + dK/dV groups == autograd's d trans_coeff to 1e-9 relative, and -sum(dt) / tau == autograd's d tau: the
    split into kernels is right.  trans_coeff = 0.25: the view record's fp32 product with a power of two is exact, so the model's fp32
    tables and the oracle's fp64 ones are the same numbers."""
    f, so3 = LAYOUTS[layout]
    c = W.bwd_case(f, so3, torch.float32, B=2, H=2, Nk=3, Pk=20, seed=11, **(dict(Nq=2, Pq=35) if cross else {}))
    tc, tau, scale = 0.25, 0.8, c.dh ** -0.5
    want, want_tau, out = _oracle_dtc(c, tc, scale, tau)
    lse = torch.zeros(c.B, c.H, c.Tq)
    prep = W.ref_bwd_prep(c.q, c.dout, out, lse, c.packed, c.f_dims, c.Nq, c.so3, tc, scale, tau)
    walk = W.ref_walk_partials(c.q, c.k, c.v, c.dout, c.packed, c.f_dims, c.Nq, c.Nk, c.so3, tc, scale, tau)
    got = float(prep.dc.sum() + walk.dq.sum() + walk.dkv.sum())
    print(f"BWD_PREP host {layout} cross={cross}: d trans_coeff {got!r} autograd {want!r}; d tau {-float(walk.dt.sum()) / tau!r} autograd {want_tau!r}")
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert abs(-float(walk.dt.sum()) / tau - want_tau) <= 1e-9 * abs(want_tau)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_rho_q_is_the_oracles_query_transform(layout):
    f, so3 = LAYOUTS[layout]
    c = W.bwd_case(f, so3, torch.float32, B=2, H=2, Nk=3, Pk=20, seed=12, Nq=2, Pq=35)
    reps64 = {n: ([t.double() for t in r] if isinstance(r, list) else r.double()) for n, r in c.reps.items()}
    qt, _, _ = O.transform_qkv(c.q.double(), c.k.double(), c.v.double(), c.f_dims, reps64, 0.37)
    M, ident = W.rho_q(c.packed, c.f_dims, c.Tq, c.Nq, c.so3, 0.37)
    got = torch.einsum("btij,bhtj->bhti", M, c.q.double())
    absprod = torch.einsum("btij,bhtj->bhti", M.abs(), c.q.double().abs())
    assert bool(((got - qt).abs() <= 2.0 ** -23 * absprod).all())                    # (the fp32 trans_coeff product: one rounding per entry)
    assert torch.equal(got[..., ident], c.q.double()[..., ident]) and int(ident.sum()) == f.get("triv", 0)


# ---- a host-made workspace under the GPU tests' rules ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _host_case():
    """fp32, X3, se3 | so2 at dh 32, B = H = 2, 3 views of 50 rows with tau: out and lse from the oracle in fp64, rounded to fp32"""
    cs = W._cs("host", W.half(32), W.FP32, x3=True, tau=0.8, shape=dict(B=2, H=2), seed=13)
    c = W.case_inputs(cs)
    _, _, out = _oracle_dtc(c, c.tc, c.scale, cs.tau)
    qt, kt, _ = O.transform_qkv(c.q.double(), c.k.double(), c.v.double(), c.f_dims,
                                {n: ([t.double() for t in r] if isinstance(r, list) else r.double()) for n, r in c.reps.items()}, c.tc)
    lse = torch.logsumexp(c.scale / cs.tau * qt @ kt.transpose(-1, -2), -1).float()
    out = out.float()
    return cs, c, out, lse, W.case_refs(cs, c, out, lse)


def _host_workspace(defect=None):
    cs, c, out, lse, (ref, walk, emu) = _host_case()
    L = W.bwd_layout(c.B, c.H, c.Tq, c.T, c.dh, x3=True)
    bits, nl, nd, dc = W.emulate_prep(c.q, c.dout, out, lse, c.packed, c.f_dims, c.Nq, c.so3, c.tc, c.scale, cs.tau, True, True, defect)
    dq = emu.dq.clone().float()
    if defect == "dq_slot":
        dq.view(torch.int32)[1, 0, 1] = -1                                           # one dQ slot left at the 0xFF fill
    d = W.decode_bwd(W.encode_bwd(L, bits, nl, nd, dc, dq, emu.dkv, emu.dt), L)
    return W.check_workspace(f"host {defect}", d, ref, dh=c.dh, q=c.q, dout=c.dout, walk=walk, emu=emu, want_dt=True)


def test_clean_emulation_passes_every_rule():
    assert _host_workspace() == []


@pytest.mark.parametrize("defect,rules", [("truncate", {"image"}), ("share", {"D"}), ("lo_unscaled", {"hilo"}), ("pad_row", {"zero"}),
                                          ("hi_block", {"prep-partial"}), ("dq_slot", {"fill", "walk"})])
def test_each_defect_fails_its_own_rule(defect, rules):
    """(a slot left at the fill is a NaN: it fails the finiteness rule and the slot's own 6 sigma bar, nothing else)"""
    fails = _host_workspace(defect)
    assert {r for r, _ in fails} == rules, fails


WALK_CASES = sorted(n for n, cs in W.CASES.items() if cs.walk)


@pytest.mark.parametrize("name", WALK_CASES)
def test_walk_bar_sees_a_missing_term(name):
    """At every shape whose slots the GPU tests hold to 6 sigma: the V term of the dK/dV slots, and one se3 block's term of the dQ and of the
    dK/dV slots (the smallest block, by RMS over the slots), exceed 6 sigma (RMS over the slots: a missing term is missing from all of them)."""
    cs = W.CASES[name]
    c = W.case_inputs(cs)
    args = (c.q, c.k, c.v, c.dout, c.packed, c.f_dims, c.Nq, c.Nk, c.so3, c.tc, c.scale, cs.tau, cs.vt, c.dlse, cs.key_lens, cs.q_lens)
    walk = W.ref_walk_partials(*args)
    emu = W.ref_walk_partials(*args, emulate="x3" if cs.x3 else "bf16", out_dtype=cs.dtype)
    pairs = bool(cs.pairs)
    sig = W.walk_sigma(walk, emu, pairs)
    f = W._pair if pairs else (lambda x: x)
    rms = lambda x: float(f(x).pow(2).mean().sqrt())
    one_block = min(rms(b) for b in walk.dq_blocks)
    print(f"BWD_PREP host {name}: sigma dq {sig['dq']:.3e} dkv {sig['dkv']:.3e} dt {sig['dt']:.3e}; rms V term {rms(walk.dv):.3e}, smallest dQ block term {one_block:.3e}")
    if cs.vt:
        assert rms(walk.dv) > 6.0 * sig["dkv"], (rms(walk.dv), sig)
    assert one_block > 6.0 * sig["dq"], (one_block, sig)
    assert min(rms(b) for b in walk.dk_blocks) > 6.0 * sig["dkv"], sig

"""GPU: the backward's workspace itself -- the Q'' / dO~ tile images, the per-row statistics [-lse * log2e | -D] and the d trans_coeff partial
of `gta_bwd_prep_kernel`, the slots the dQ and dK/dV kernels add, and `gta_reduce_kernel`'s sums -- against fp64, element by element.

Every case: a real forward (`native.attn_fwd*` with a workspace: out and lse are the forward's own), the backward workspace filled with 0xFF
bytes (a NaN as fp32, -1 as a word), ONE backward call through `native.attn_bwd` / `attn_bwd_dlse` / `attn_bwd_varlen` with kv_images=None,
the workspace and the results copied back once, and everything compared on the CPU with tests/_bwd_images.py (the model of the layout, the
references and the rules: `check_workspace`, `check_reduce`; tests/test_bwd_images_host.py proves on the CPU that each rule catches its
defect).  The cases and their shapes are `_bwd_images.CASES`.

Bars (ulp(x) = 2^(floor(log2 |x|) - 7); absprod = sum_j |M_ij| |x_j|, Q'''s times qscale; pack8 rounds to nearest even):
  untouched channels       dO~ bits == bf16_bits(dout) (every channel without V_TRANSFORM); Q'' bits == bf16_bits(fp32(q) * qscale32), qscale32 =
                           (scale * LOG2E) / tau in fp32: the library is built without fast-math and its fp32 quotient is correctly rounded,
                           so this holds bit for bit with tau too (no case needs the ulp/2 + 4 * 2^-24 |ref| fallback)
  transformed channels     |img - ref64| <= ulp(ref64) / 2 + 16 * 2^-24 * absprod (a dot product of at most 5 terms, the trans_coeff product,
                           the three roundings of qscale and its product)
  X3                       hi as above; |hi + lo - ref64| <= 2^-16 |ref64| + the same fp32 term, for both images
  zero bytes               padded channels, rows past Tq, rows at or past q_lens[b] -- including the tiles wholly past the prefix
  statistics               valid rows: |neg_lse2 - ref| <= 4 * 2^-24 |ref|, |neg_D - ref| <= (dhp / 4 + 4) * 2^-24 * sum |dout * out| (+ 2^-24 |dlse|
                           for the DLSE entry); rows past Tq or the prefix: exactly (-1e30f, 0.0)
  fill                     every word of dc[0 : dc_total) finite; dt[0 : n_dq) finite with tau and dtau, else untouched; the alignment gaps untouched
  pre-pass partial         |got - ref| <= (n + 8) * 2^-24 * sum |addend|, n = 2 * dhp / 32 + 9: a thread adds the two block terms of each of its
                           dhp / 32 chunks, wg_sum256 six shuffle levels and three wave sums; 8 for the roundings inside a term; exactly 0.0
                           without V_TRANSFORM or an se3 slab
  reduce                   dtrans_coeff (dtau: -sum / tau) against the fp64 sum of the partials read back: (ceil(n / 1024) + 14) * 2^-24 * sum |partial|
  dQ, dK/dV, d tau slots   6 sigma, sigma = RMS over the case's slots of (the fp64 formulas with bf16 operands, P and dS -- hi + lo pairs under X3 --
                           minus their fp64 value); a generated stream's pair of slots as their sum, its second slot exactly 0.0.  The
                           emulation takes out and lse as the backward call was handed them (P = exp2(S2 - lse2), D = <dout, out>), as the
                           kernels do: a row's dS carries the common-mode error the forward left in them (gta_bwd.hip, the X3 dQ epilogue's
                           comment).  An emulation that normalised P by its own row sum and took D from its own P V' missed
                           that term: against it the X3 dh 40 dQ slots stood at 5.3 / 5.7 / 6.08 sigma (x3-dh40, -dlse, -tau-dlse); with it
                           the worst slot of the file is 5.74 sigma (x3-dh40-dlse, dQ), the next 4.54 (DESIGN.md 4.6b has the table)

The default shape's compiled pair runs as two launches (n_dkv = 18 is no multiple of 8): "ms96-joint" (B = 4, H = 2) is the joint launch.
FLAG_BWD_KEYS32 / KEYS64 / SPLIT select among kernels at dhp 96 bf16 only, so the launch forms run on the MSN layout."""
import functools
import time
from types import SimpleNamespace

import pytest
import torch

from gta_amd import native
from tests import _bwd_images as W

pytestmark = pytest.mark.gpu

VT, X3F = native.FLAG_V_TRANSFORM, native.FLAG_FP32_PRODUCTS


def _i32(x):
    return None if x is None else torch.tensor(list(x), device="cuda", dtype=torch.int32)


def _call(cs, c, q, k, v, dout, out, lse, packed, *, dlse=None, key_lens=None, q_lens=None, Nq=None, Nk=None):
    """one backward call on a 0xFF-filled workspace -> its bytes, dtrans_coeff and dtau on the CPU"""
    flags = (VT if cs.vt else 0) | (X3F if cs.x3 else 0)
    for f in cs.flags:
        flags |= getattr(native, f)
    B, H, Tq, dh = q.shape
    desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, Nq or c.Nq, Nk or c.Nk, c.scale, flags)
    L = W.bwd_layout(B, H, Tq, k.shape[2], dh, cs.x3)
    need = native.attn_bwd_workspace_bytes(desc)
    assert need == L.total, (need, L.total)
    ws = torch.full((need,), W.FILL, device="cuda", dtype=torch.uint8)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    nan1 = lambda: torch.full((1,), float("nan"), device="cuda")
    tc = torch.tensor([c.tc], device="cuda") if c.tc is not None else None
    tau = torch.tensor([cs.tau], device="cuda") if cs.tau else None
    dtc, dta = (nan1() if tc is not None else None), (nan1() if tau is not None else None)
    t = [packed.get(n) for n in ("vrep_q", "vrep_k", "cs_q", "cs_k")]
    if key_lens is not None:
        native.attn_bwd_varlen(desc, q, k, v, out, dout, lse, *t, tc, tau, _i32(key_lens), _i32(q_lens), None, dq, dk, dv, dtc, ws, dta)
    elif dlse is not None:
        native.attn_bwd_dlse(desc, q, k, v, out, dout, lse, dlse, *t, tc, tau, None, dq, dk, dv, dtc, ws, dta)
    else:
        native.attn_bwd(desc, q, k, v, out, dout, lse, *t, tc, tau, None, dq, dk, dv, dtc, ws, dta)
    torch.cuda.synchronize()
    return SimpleNamespace(ws=ws.cpu(), L=L, dtc=None if dtc is None else dtc.item(), dtau=None if dta is None else dta.item())


@functools.lru_cache(maxsize=None)
def _gpu(name, entry=None):
    """forward + backward of a case (entry: run a "dlse" case through the plain entry instead) -> inputs, device tensors, out / lse, the call"""
    cs = W.CASES[name]
    if entry:
        cs = SimpleNamespace(**{**vars(cs), "entry": entry})
    c = W.case_inputs(cs)
    dev = lambda t: t.to(cs.dtype).cuda()
    q, k, v, dout = dev(c.q), dev(c.k), dev(c.v), dev(c.dout)
    assert q.stride() == (c.Tq * c.H * c.dh, c.dh, c.H * c.dh, 1)                     # token-major
    packed = {n: t.cuda() for n, t in c.packed.items()}
    kl, ql = cs.key_lens, cs.q_lens
    if kl is not None:                                                                 # everything past a key prefix is NaN from the start
        for b, n in enumerate(kl):
            k[b, :, n:] = float("nan")
            v[b, :, n:] = float("nan")
    out = torch.empty(c.B, c.Tq, c.H, c.dh, device="cuda", dtype=cs.dtype).permute(0, 2, 1, 3)
    lse = torch.empty(c.B, c.H, c.Tq, device="cuda", dtype=torch.float32)
    fdesc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, c.Nk, c.scale, (VT if cs.vt else 0) | (X3F if cs.x3 else 0))
    rc = native.attn_fwd_supported(fdesc)
    if rc:
        print(f"BWD_PREP {name}: attn_fwd_supported refuses the layout: {native.lib().gta_strerror(rc)}")
        pytest.skip(f"attn_fwd_supported refuses {c.f_dims}")
    wsf = torch.empty(native.attn_fwd_workspace_bytes(fdesc), device="cuda", dtype=torch.uint8)
    tc = torch.tensor([c.tc], device="cuda") if c.tc is not None else None
    tau = torch.tensor([cs.tau], device="cuda") if cs.tau else None
    t = [packed.get(n) for n in ("vrep_q", "vrep_k", "cs_q", "cs_k")]
    if kl is not None:
        native.attn_fwd_varlen(fdesc, q, k, v, *t, tc, tau, _i32(kl), out, lse, wsf)
    else:
        native.attn_fwd(fdesc, q, k, v, *t, tc, tau, out, lse, wsf)
    torch.cuda.synchronize()
    out_c, lse_c = out.float().cpu(), lse.cpu()
    if ql is not None:                                                                 # ... and everything past a query prefix before the backward
        for b, n in enumerate(ql):
            for x in (q, dout, out):
                x[b, :, n:] = float("nan")
            lse[b, :, n:] = float("nan")
    dlse = c.dlse.cuda() if cs.entry == "dlse" else None
    r = _call(cs, c, q, k, v, dout, out, lse, packed, dlse=dlse, key_lens=kl, q_lens=ql)
    return SimpleNamespace(cs=cs, c=c, q=q, k=k, v=v, dout=dout, out=out, lse=lse, packed=packed, out_c=out_c, lse_c=lse_c, r=r)


@pytest.mark.parametrize("name", sorted(W.CASES))
def test_backward_workspace(name):
    t0 = time.perf_counter()
    g = _gpu(name)
    cs, c, r = g.cs, g.c, g.r
    ref, walk, emu = W.case_refs(cs, c, g.out_c, g.lse_c)
    d = W.decode_bwd(r.ws, r.L)
    fails = W.check_workspace(name, d, ref, dh=c.dh, q=c.q, dout=c.dout, walk=walk, emu=emu, want_dt=cs.tau is not None, pairs=cs.pairs,
                              dlse_abs=None if c.dlse is None else c.dlse.double().abs(), lens=cs.q_lens)
    fails += W.check_reduce(name, d, r.dtc, r.dtau, cs.tau)
    if cs.key_lens is not None:                      # blocks wholly past a prefix: exactly 0.0
        for b, n in enumerate(cs.key_lens):
            if not bool((d.dc_dkv[b, :, (n + 127) // 128:].contiguous().view(torch.int32) == 0).all()):
                fails.append(("walk", f"{name}: [walk] scene {b}: the partial of a key block past the prefix is not exactly 0.0"))
        for b, n in enumerate(cs.q_lens or ()):
            if not bool((d.dc_dq[b, :, (n + 127) // 128:].contiguous().view(torch.int32) == 0).all()):
                fails.append(("walk", f"{name}: [walk] scene {b}: the partial of a query block past the prefix is not exactly 0.0"))
    print(f"BWD_PREP {name}: {time.perf_counter() - t0:.2f} s")
    assert not fails, "\n".join(m for _, m in fails)


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_dlse_entry_changes_the_D_half_only(dt):
    """gta_attn_bwd_dlse against gta_attn_bwd on the same inputs: the images and the lse half of the statistics agree bit for bit"""
    a, b = _gpu(f"dlse-{dt}"), _gpu(f"dlse-{dt}", "bwd")
    da, db = W.decode_bwd(a.r.ws, a.r.L), W.decode_bwd(b.r.ws, b.r.L)
    assert torch.equal(da.bits, db.bits)
    assert torch.equal(da.stats_raw[:, :, :, 0], db.stats_raw[:, :, :, 0])
    assert not torch.equal(da.stats_raw[:, :, :, 1], db.stats_raw[:, :, :, 1])
    assert torch.equal(da.dc_raw[:a.r.L.n_prep], db.dc_raw[:a.r.L.n_prep])


@pytest.mark.parametrize("name", ["varlen-bf16", "varlen-fp32", "varlen-noq-bf16"])
def test_varlen_scene_is_the_scene_alone(name):
    """scene b's written tiles, statistics and pre-pass partials: byte for byte those of a plain call on that scene alone with both sides cut
    to the prefix (tile by tile: the strides differ)"""
    g = _gpu(name)
    cs, c = g.cs, g.c
    d = W.decode_bwd(g.r.ws, g.r.L)
    plain = SimpleNamespace(**{**vars(cs), "entry": "bwd"})
    for b, nk in enumerate(cs.key_lens):
        nq = cs.q_lens[b] if cs.q_lens is not None else c.Tq
        Nq, Nk = -(-nq // c.Pq), -(-nk // c.Pk)
        cut = {"vrep_q": Nq, "vrep_k": Nk, "cs_q": nq, "cs_k": nk}
        pk = {n: t[b:b + 1, :cut[n]].contiguous() for n, t in g.packed.items() if n in cut}
        sl = lambda x, n: x[b:b + 1, :, :n]
        r1 = _call(plain, c, sl(g.q, nq), sl(g.k, nk), sl(g.v, nk), sl(g.dout, nq), sl(g.out, nq), sl(g.lse, nq).contiguous(), pk, Nq=Nq, Nk=Nk)
        d1 = W.decode_bwd(r1.ws, r1.L)
        nt = r1.L.n_qt
        assert torch.equal(d.bits[b, :, :nt], d1.bits[0]), f"{name}: scene {b}: the images differ from those of the scene alone"
        assert torch.equal(d.stats_raw[b, :, :nt], d1.stats_raw[0]), f"{name}: scene {b}: the statistics differ from those of the scene alone"
        assert torch.equal(d.dc_prep[b, :, :nt].contiguous().view(torch.int32), d1.dc_prep[0].contiguous().view(torch.int32)), f"{name}: scene {b}: pre-pass partials"

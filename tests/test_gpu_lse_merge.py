"""GPU: `gta_attention(..., return_lse=True)` with a gradient for both outputs, `gta_attention_merge` (gta_merge.hip) and
`gta_attention_by_view_groups`.

Shapes are those of tests/test_gpu_key_views.py: 5 scenes, 2 heads, 13 views of 20 tokens, `clevrtr/gta` (dh 64) and `msn/gta_so3` (dh 96), a
decoder leg of 150 query rows and an encoder leg of 260; test 8 has 20 views of 8 tokens.  The merge kernels are checked alone at
n in {1, 2, 3, 8} partials and dh in {8, 64, 96, 128} (1, 2, 8, 12, 16, 24, 32 sixteen-byte units per row: every lane-group width) on 900 rows
(no multiple of the rows a workgroup takes per step), and past the cap of their grid (`merge_grid`: 2048 workgroups) at 3 partials on
32 811 to 1 049 859 rows, one size per lane-group width 32, 16, 16, 1: two full sweeps, five more steps and a ragged step of 3 rows, with a row
without keys (and NaN in its out row) in each of those regions (test_merge_past_the_grid_cap).

Bars (none new).  Merge against its fp64 formula: 1e-5 of max |ref| for fp32 operands (fp32 arithmetic: a few ulp of the largest term), one
bf16 rounding (2^-8 |ref| + 1e-6) for bf16 ones.  Attention against the fp64 oracle: forward REL_MAX / REL_RMS and the 2e-2 LSE bar of
tests/test_gpu_forward.py; gradients REL_MAX / REL_RMS of tests/test_gpu_backward.py with its 2 % (d trans_coeff) and 3 % (d tau, tau = 0.8)
bars; precise=True `_grad_check` of tests/test_gpu_precise.py with 2e-4 / 3e-4 for the two scalars."""
import functools
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import backward as BW
from gta_amd import gta as G2
from gta_amd import native
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests.test_gpu_backward import REL_MAX as G_MAX, REL_RMS as G_RMS, SHAPES
from tests.test_gpu_forward import REL_MAX, REL_RMS
from tests.test_gpu_key_views import B, H, NK, PK, KV, _abi, _case, _key_lens
from tests.test_gpu_precise import _grad_check
from tests.test_gpu_run_configs import RUNS

pytestmark = pytest.mark.gpu

FUSED = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
TAU = 0.8


def _call(c, grad=False, qkv=None, tc=None, tau=None, groups=None, **kw):
    """gta_attention (or, with `groups`, gta_attention_by_view_groups) on a case"""
    q, k, v = qkv or c.dev
    args = dict(so3_degree=c.so3, trans_coeff=c.tc if tc is None else tc, scale=c.scale, euclid=c.euclid, tau=tau, **kw)
    with torch.enable_grad() if grad else torch.no_grad():
        if groups is not None:
            return gta_amd.gta_attention_by_view_groups(q, k, v, c.f_dims, c.packed, views_per_call=groups, **args)
        return gta_amd.gta_attention(q, k, v, c.f_dims, c.packed, **args)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. return_lse, forward: every route returns the kernels' own lse and leaves out as it was
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED)
def test_return_lse_fused_route(run, dtype):
    for cc in (_case(run, "enc", dtype), _case(run, "dec", dtype)):      # (Tq = 260: the two-stage plan; 150: the single kernel)
        q, k, v = cc.dev
        flags = G2.attention_route(tuple(q.shape), k.shape[2], dtype, cc.f_dims, cc.so3, cc.Nq, NK)
        out = torch.empty(B, cc.Tq, H, cc.dh, device="cuda", dtype=dtype).permute(0, 2, 1, 3)
        lse = torch.empty(B, H, cc.Tq, device="cuda", dtype=torch.float32)
        desc = native.make_desc(q, k, v, out, cc.f_dims, cc.so3, cc.Nq, NK, cc.scale, flags)
        ws = None if flags & native.FLAG_FUSED_KV else torch.empty(native.attn_fwd_workspace_bytes(desc), device="cuda", dtype=torch.uint8)
        native.attn_fwd(desc, q, k, v, cc.packed.get("vrep_q"), cc.packed.get("vrep_k"), cc.packed.get("cs_q"), cc.packed.get("cs_k"), cc.tc, None,
                        out, lse, ws)
        got, got_lse = _call(cc, return_lse=True)
        plain = _call(cc)
        torch.cuda.synchronize()
        assert got_lse.dtype == torch.float32 and tuple(got_lse.shape) == (B, H, cc.Tq) and torch.isfinite(got_lse).all()
        assert torch.equal(got_lse, lse) and torch.equal(got, out) and torch.equal(got, plain)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED + ["clevrtr/gta_euclid", "msn/gta_t2"])
def test_return_lse_varlen_and_staged_routes(run, dtype):
    c = _case(run, "dec", dtype)
    out, lse, _ = _abi(c, _key_lens())                 # the varlen entry of the family (fused layouts: gta_attn_fwd_varlen)
    got, got_lse = _call(c, key_views=KV, return_lse=True)
    plain = _call(c, key_views=KV)
    torch.cuda.synchronize()
    assert torch.equal(got_lse, lse) and torch.equal(got, out) and torch.equal(got, plain)
    if not c.fused:                                    # the staged route without key_views
        q, k, v = c.dev
        assert G2.generic_route(tuple(q.shape), k.shape[2], dtype, c.f_dims, c.so3, c.Nq, NK, euclid=c.euclid) == "staged"
        out = torch.empty(B, c.Tq, H, c.dh, device="cuda", dtype=dtype).permute(0, 2, 1, 3)
        lse = torch.empty(B, H, c.Tq, device="cuda", dtype=torch.float32)
        desc = native.make_desc(q, k, v, out, c.f_dims, c.so3, c.Nq, NK, c.scale, G2._layout_flags(True, c.euclid))
        ws = torch.empty(native.attn_fwd_staged_workspace_bytes(desc), device="cuda", dtype=torch.uint8)
        native.attn_fwd_staged(desc, q, k, v, *[c.packed.get(t) for t in ("vrep_q", "vrep_k", "cs_q", "cs_k", "coord_q", "coord_k")], c.tc, None,
                               out, lse, ws)
        got, got_lse = _call(c, return_lse=True)
        plain = _call(c)
        torch.cuda.synchronize()
        assert torch.equal(got_lse, lse) and torch.equal(got, out) and torch.equal(got, plain)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2 - 4. the merge kernels alone
# ------------------------------------------------------------------------------------------------------------------------------------
MB, MH, MT = 2, 3, 150


@functools.lru_cache(maxsize=None)
def _partials(n, dh, dtype):
    return _partials_of(n, dh, dtype, MB, MH, MT)


def _partials_of(n, dh, dtype, MB, MH, MT, empty=None):
    """n partial attentions as strided views of [B,Tq,H,dh] memory (masters on the CPU, rounded to dtype), weights for a loss, and the fp64
    formula with its autograd gradients.  `empty` = (i, [(b, h, t), ...]): partial i saw no key on those rows (lse_i = -inf; its out_i row is
    zero in these masters, so the formula stays finite: the caller puts NaN there on the device)"""
    g = torch.Generator().manual_seed(1000 * n + dh)
    outs = [torch.randn(MB, MT, MH, dh, generator=g).to(dtype).float() for _ in range(n)]
    lses = [3.0 * torch.randn(MB, MH, MT, generator=g) for _ in range(n)]
    if empty is not None:
        for b_, h_, t_ in empty[1]:
            outs[empty[0]][b_, t_, h_] = 0.0
            lses[empty[0]][b_, h_, t_] = float("-inf")
    w, u = torch.randn(MB, MT, MH, dh, generator=g).to(dtype).float(), torch.randn(MB, MH, MT, generator=g)
    o64 = [t.double().permute(0, 2, 1, 3).requires_grad_() for t in outs]
    l64 = [t.double().requires_grad_() for t in lses]
    a = torch.softmax(torch.stack(l64), 0)
    ref_out = (a[..., None] * torch.stack(o64)).sum(0)
    ref_lse = torch.logsumexp(torch.stack(l64), 0)
    ((ref_out * w.double().permute(0, 2, 1, 3)).sum() + (ref_lse * u.double()).sum()).backward()
    return SimpleNamespace(outs=outs, lses=lses, w=w, u=u, ref_out=ref_out.detach(), ref_lse=ref_lse.detach(), d_outs=[t.grad for t in o64],
                           d_lses=[t.grad for t in l64])


def _close(got, ref, dtype, name):
    """fp32 operands: 1e-5 of max |ref|; bf16 operands: one rounding"""
    got, ref = got.double().cpu(), ref.double()
    assert torch.isfinite(got).all(), name
    err = (got - ref).abs()
    if dtype == torch.float32:
        assert err.max().item() <= 1e-5 * ref.abs().max().item(), (name, err.max().item(), ref.abs().max().item())
    else:
        assert bool((err <= 2.0 ** -8 * ref.abs() + 1e-6).all()), (name, (err - 2.0 ** -8 * ref.abs()).max().item())


def _device_partials(p, dtype, grad=False):
    outs = [t.to(dtype).cuda().permute(0, 2, 1, 3).requires_grad_(grad) for t in p.outs]
    lses = [t.cuda().requires_grad_(grad) for t in p.lses]
    return outs, lses


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dh", [8, 64, 96, 128])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
def test_merge_forward_and_backward_vs_fp64_formula(n, dh, dtype):
    p = _partials(n, dh, dtype)
    outs, lses = _device_partials(p, dtype, grad=True)
    assert not outs[0].is_contiguous() and outs[0].stride(3) == 1
    out, lse = gta_amd.gta_attention_merge(outs, lses)
    ((out.float() * p.w.cuda().permute(0, 2, 1, 3)).sum() + (lse * p.u.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert out.dtype == dtype and lse.dtype == torch.float32 and tuple(out.shape) == (MB, MH, MT, dh)
    _close(out, p.ref_out, dtype, "out")
    lse_err = (lse.double().cpu() - p.ref_lse).abs()
    assert bool((lse_err <= 1e-5 * p.ref_lse.abs().clamp_min(1.0)).all()), lse_err.max().item()
    if n == 1:
        assert torch.equal(out, outs[0]) and torch.equal(lse, lses[0])
    for i in range(n):
        _close(outs[i].grad, p.d_outs[i], dtype, f"dout_{i}")
        _close(lses[i].grad, p.d_lses[i], torch.float32, f"dlse_{i}")


@pytest.mark.parametrize("dh,dtype,rpb", [(128, torch.float32, 8), (96, torch.bfloat16, 16), (64, torch.float32, 16), (8, torch.bfloat16, 256)])
def test_merge_past_the_grid_cap(dh, dtype, rpb):
    """`merge_grid` caps at 2048 workgroups of rpb = 256 / (lane-group width) rows per step: R = 2 2048 rpb + 5 rpb + 3 rows are two full
    sweeps of the grid, five more steps and a ragged step of 3 rows (in the backward every lane of that workgroup still takes the step).
    The fp64 formula and the `_close` bars of test_merge_forward_and_backward_vs_fp64_formula with both dout and dlse; one row of each region
    (first sweep, second sweep, ragged step) is without keys in partial 1, whose out row holds NaN there, as in
    test_merge_selects_out_partials_without_keys."""
    Hh, n = 3, 3
    U = dh * (2 if dtype == torch.bfloat16 else 4) // 16
    assert rpb == 256 >> (U - 1).bit_length()                # (the lane group of gta_merge.hip's merge_map)
    R = 2 * 2048 * rpb + 5 * rpb + 3
    assert R % Hh == 0
    Tq = R // Hh
    empty_rows = [7, 2048 * rpb + 11, R - 2]                 # in memory order: row r is (t, h) = (r // H, r % H)
    empty = [(0, r % Hh, r // Hh) for r in empty_rows]
    p = _partials_of(n, dh, dtype, 1, Hh, Tq, empty=(1, empty))
    mem = [t.to(dtype).cuda() for t in p.outs]               # [B,Tq,H,dh]
    for b_, h_, t_ in empty:
        mem[1][b_, t_, h_] = float("nan")
    outs = [t.permute(0, 2, 1, 3).requires_grad_() for t in mem]
    lses = [t.cuda().requires_grad_() for t in p.lses]
    out, lse = gta_amd.gta_attention_merge(outs, lses)
    ((out.float() * p.w.cuda().permute(0, 2, 1, 3)).sum() + (lse * p.u.cuda()).sum()).backward()
    torch.cuda.synchronize()
    assert out.dtype == dtype and tuple(out.shape) == (1, Hh, Tq, dh) and tuple(lse.shape) == (1, Hh, Tq)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    _close(out, p.ref_out, dtype, "out")
    lse_err = (lse.double().cpu() - p.ref_lse).abs()
    assert bool((lse_err <= 1e-5 * p.ref_lse.abs().clamp_min(1.0)).all()), lse_err.max().item()
    for i in range(n):
        assert not torch.isnan(outs[i].grad).any() and not torch.isnan(lses[i].grad).any(), i
        _close(outs[i].grad, p.d_outs[i], dtype, f"dout_{i}")
        _close(lses[i].grad, p.d_lses[i], torch.float32, f"dlse_{i}")
    for b_, h_, t_ in empty:
        assert bool((outs[1].grad[b_, h_, t_] == 0).all()) and lses[1].grad[b_, h_, t_].item() == 0.0, (h_, t_)


def test_merge_with_one_output_unused():
    """either of (dout, dlse) may be missing"""
    p = _partials(3, 96, torch.float32)
    for use_out in (True, False):
        outs, lses = _device_partials(p, torch.float32, grad=True)
        out, lse = gta_amd.gta_attention_merge(outs, lses)
        ref_outs, ref_lses = _device_partials(p, torch.float32, grad=True)
        out2, lse2 = gta_amd.gta_attention_merge(ref_outs, ref_lses)
        if use_out:
            (out * p.w.cuda().permute(0, 2, 1, 3)).sum().backward()
            ((out2 * p.w.cuda().permute(0, 2, 1, 3)).sum() + (lse2 * 0.0).sum()).backward()
        else:
            (lse * p.u.cuda()).sum().backward()
            ((out2 * 0.0).sum() + (lse2 * p.u.cuda()).sum()).backward()
        torch.cuda.synchronize()
        for a, b_ in zip(outs + lses, ref_outs + ref_lses):
            assert torch.equal(a.grad, b_.grad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_selects_out_partials_without_keys(dtype):
    p = _partials(3, 96, dtype)
    outs, lses = _device_partials(p, dtype)
    dead = [0, 7, MT - 1]                                  # query rows without a key in ANY partial
    for l in lses:
        l[:, :, dead] = float("-inf")
    want, want_lse = gta_amd.gta_attention_merge([outs[0], outs[2]], [lses[0], lses[2]])
    outs[1] = torch.full_like(outs[1], float("nan"))
    lses[1] = torch.full_like(lses[1], float("-inf"))
    outs, lses = [t.requires_grad_() for t in outs], [t.requires_grad_() for t in lses]
    out, lse = gta_amd.gta_attention_merge(outs, lses)
    ((out.float() * p.w.cuda().permute(0, 2, 1, 3)).sum() + (lse[:, :, 1:7] * p.u.cuda()[:, :, 1:7]).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(lse, want_lse)
    assert not torch.isnan(out).any() and not torch.isnan(lse).any()
    assert bool((out[:, :, dead] == 0).all()) and bool((lse[:, :, dead] == float("-inf")).all())
    assert bool((outs[1].grad == 0).all()) and bool((lses[1].grad == 0).all())
    for t in outs + lses:
        assert not torch.isnan(t.grad).any()
        assert bool((t.grad[:, :, dead] == 0).all())


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. gta_attn_bwd_dlse with dlse = 0 is gta_attn_bwd, bit for bit
# ------------------------------------------------------------------------------------------------------------------------------------
def _bwd_twice(q, k, v, f_dims, packed, so3, Nq, Nk, tc, tau, dtype, precise=False, kv_mode="auto"):
    scale = q.shape[-1] ** -0.5
    with torch.no_grad():
        out, lse = gta_amd.gta_attention(q, k, v, f_dims, packed, so3_degree=so3, trans_coeff=tc, tau=tau, scale=scale, precise=precise,
                                         kv_mode=kv_mode, return_lse=True)
    flags = G2.attention_route(tuple(q.shape), k.shape[2], dtype, f_dims, so3, Nq, Nk, precise=precise, needs_grad=True, kv_mode=kv_mode)
    cfg = ({n: int(x) for n, x in f_dims.items()}, so3, Nq, Nk, scale, flags)
    dout = torch.randn(out.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(5)).to(dtype)
    tables = [packed.get(t) for t in ("vrep_q", "vrep_k", "cs_q", "cs_k")]
    run = lambda dlse: BW.attn_bwd(cfg, q, k, v, out, dout, lse, tc, tau, *tables, want_dtau=tau is not None, dlse=dlse)
    a, b_ = run(None), run(torch.zeros_like(lse))
    c_ = run(torch.ones_like(lse))
    torch.cuda.synchronize()
    for name, x, y in zip(("dq", "dk", "dv", "dtc", "dtau"), a, b_):
        assert (x is None) == (y is None), name
        if x is not None:
            assert torch.equal(x, y), name
    assert not torch.equal(a[0], c_[0])                # (and a non-zero dlse does reach the kernels)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("run", FUSED)
def test_zero_dlse_is_the_plain_backward(run, dtype):
    c = _case(run, "dec", dtype)
    _bwd_twice(*c.dev, c.f_dims, c.packed, c.so3, c.Nq, NK, c.tc, torch.tensor([TAU], device="cuda"), dtype)


def test_zero_dlse_is_the_plain_backward_x3():
    c = _case("clevrtr/gta", "dec", torch.float32)
    _bwd_twice(*c.dev, c.f_dims, c.packed, c.so3, c.Nq, NK, c.tc, torch.tensor([TAU], device="cuda"), torch.float32, precise=True)


def test_zero_dlse_is_the_plain_backward_generated_streams():
    """bf16, dh = 96, the MS-enc geometry cut to 2 views of 256 tokens, the generated 64-row streams by name (no d tau: the dQ stream has none)"""
    _, Hh, _, Pq, _, Pk, f_dims, so2, so3 = SHAPES["MS-enc"]
    q, k, v, ex, ak, cross = C.synth_inputs(1, Hh, 2, Pq, 2, Pk, f_dims, so2, so3, torch.bfloat16, seed=7)
    exd = {kk: vv.cuda() for kk, vv in ex.items()}
    gta_amd.pre_compute_reps_encoder(ak, exd)
    packed = gta_amd.pack_reps(exd, f_dims)
    qd, kd, vd = (t.bfloat16().cuda() for t in (q, k, v))
    _bwd_twice(qd, kd, vd, f_dims, packed, exd.get("gta_so3_degree", 0), 2, 2, torch.tensor([0.37], device="cuda"), None, torch.bfloat16,
               kv_mode="prepass_bwd_keys64")


# ------------------------------------------------------------------------------------------------------------------------------------
# 6 - 8. gradients through lse, split = whole, more than 16 views: against fp64 autograd through the oracle
# ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case20(dtype):
    """`_case` of tests/test_gpu_key_views.py for clevrtr/gta with 20 views of 8 tokens and the decoder leg of 150 rows"""
    from gta_amd import synth
    run, nk, pk, Tq = "clevrtr/gta", 20, 8, 150
    dh, _mixed, enc, dec = RUNS[run]
    g = torch.Generator().manual_seed(2020)
    ex = {"input_transforms": synth.random_extrinsics(B, nk, g), "input_coord": torch.rand(B, nk, pk, 2, generator=g),
          "target_transforms": synth.random_extrinsics(B, 1, g), "target_coord": torch.rand(B, 1, Tq, 2, generator=g)}
    q, k, v = (torch.randn(B, H, T, dh, generator=g) for T in (Tq, nk * pk, nk * pk))
    if dtype == torch.bfloat16:
        q, k, v = (t.bfloat16().float() for t in (q, k, v))
    exd = {kk: vv.cuda() for kk, vv in ex.items()}
    gta_amd.pre_compute_reps_encoder(enc, exd)
    gta_amd.pre_compute_reps_decoder(dec, exd)
    f_dims = dec["f_dims"]
    packed = {kk: vv.clone() for kk, vv in gta_amd.pack_reps(exd, f_dims).items()}
    return SimpleNamespace(run=run, side="dec", dtype=dtype, dh=dh, q=q, k=k, v=v, ex=ex, enc=enc, dec=dec, f_dims=f_dims, packed=packed, euclid=False,
                           so3=G2._so3_degree(f_dims, packed, exd), scale=dh ** -0.5, dev=tuple(t.to(dtype).cuda() for t in (q, k, v)),
                           tc=torch.tensor([0.01], device="cuda"), Tq=Tq, Nq=1, fused=True)


def _weights(c, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(c.q.shape, generator=g), torch.randn(c.q.shape[:3], generator=g)


_REF = {}


def _oracle_eval(c, reps, qkv, wu=None):
    """fp64 oracle on every key view: out, lse and, with weights (w, u), the gradients of sum(w out) + sum(u lse) in q, k, v, trans_coeff, tau"""
    q, k, v = (t.double().requires_grad_() for t in qkv)
    tc = torch.tensor([float(c.tc.item()) if c.tc is not None else 1.0], dtype=torch.float64, requires_grad=True)
    tau = torch.tensor([TAU], dtype=torch.float64, requires_grad=True)
    out, _ = O.gta_attention(q, k, v, c.f_dims, reps, tc, True, c.euclid, scale=c.scale, tau=tau)
    qt, kt, _ = O.transform_qkv(q, k, v, c.f_dims, reps, tc, True, c.euclid)
    sim = c.scale * qt @ kt.transpose(-1, -2)
    if c.euclid:
        sim = sim - 0.5 * c.scale * kt.pow(2).sum(-1)[..., None, :]
    lse = torch.logsumexp(sim / tau, -1)
    return out, lse, (q, k, v, tc, tau)


def _oracle_grads(c):
    """The reference of a case, once: out, lse and the gradients at tau = 0.8, with the draw of the loss weights (w, u).

    The draw.  d trans_coeff and d tau are single numbers summed over every (row, key) with both signs; at these sizes they come out anywhere
    between 0 and +-200 while what bf16 operands leave of them does not depend on the value: under 2^-9 relative perturbations of q, k, v the
    ORACLE's own scalars move by 0.05 .. 1.2 (`_dtc_sensitivity` of tests/test_gpu_backward.py, which adds three times that to its 2 % bar for
    the cancelling fixtures).  Here the bars stay the plain 2 % / 3 % of max(1, |ref|); the draw is instead the first seed from 77 up at which
    they can be about the kernels.  `sens` = the largest move of the oracle's scalar over three perturbed evaluations (fixed seed) estimates ONE
    rounding stage of size 2^-9, about 1.3 sigma of it; the default arithmetic has four such stages in a row (the inputs, the rho'd operand
    images, P, dS -- each rounded to bf16 once), so 3 sigma of their sum is 3 * sqrt(4) / 1.3 = 4.6 sens: the draw is accepted when 6 sens
    fits inside the bar (a third of headroom), for both scalars.  The criterion looks at the fp64 reference alone."""
    key = (c.run, c.side, c.dtype, c.k.shape[2])
    if key not in _REF:
        ex64 = {kk: vv.double() for kk, vv in c.ex.items()}
        reps = O.encoder_reps(c.enc, {kk: vv for kk, vv in ex64.items() if kk.startswith("input")})
        if c.side == "dec":
            reps = O.decoder_reps(c.dec, ex64, reps)
        out, lse, leaves = _oracle_eval(c, reps, (c.q, c.k, c.v))
        gp = torch.Generator().manual_seed(1)
        shaken = []
        for _ in range(3):
            qkv = [t.double() * (1 + (torch.rand(t.shape, generator=gp, dtype=torch.float64) - 0.5) * 2.0 ** -8) for t in (c.q, c.k, c.v)]
            shaken.append(_oracle_eval(c, reps, qkv))
        scalars = lambda o, l, lv, w, u: [float(x) for x in torch.autograd.grad((o * w).sum() + (l * u).sum(), lv[3:], retain_graph=True)]
        for seed in range(77, 141):
            w, u = (t.double() for t in _weights(c, seed))
            base = scalars(out, lse, leaves, w, u)
            sens = [max(abs(s_[i] - base[i]) for s_ in (scalars(*sh, w, u) for sh in shaken)) for i in range(2)]
            if 6 * sens[0] <= 2e-2 * max(1.0, abs(base[0])) and 6 * sens[1] <= 3e-2 * max(1.0, abs(base[1])):
                break
        else:
            raise AssertionError("no draw of (w, u) in 64 seeds at which the scalars' bars are above the reference's own sensitivity")
        dq, dk, dv, dtc, dtau = torch.autograd.grad((out * w).sum() + (lse * u).sum(), leaves)
        _REF[key] = SimpleNamespace(out=out.detach(), lse=lse.detach(), dq=dq, dk=dk, dv=dv, seed=seed,
                                    dtc=float(dtc.item()) if c.tc is not None else None, dtau=float(dtau.item()))
    return _REF[key]


def _check_against_oracle(c, precise=False, groups=None, forward_bars=False, **kw):
    ref = _oracle_grads(c)
    q, k, v = (t.clone().requires_grad_() for t in c.dev)
    tc = c.tc.clone().requires_grad_() if c.tc is not None else None
    tau = torch.tensor([TAU], device="cuda", requires_grad=True)
    out, lse = _call(c, grad=True, qkv=(q, k, v), tc=tc, tau=tau, return_lse=True, groups=groups, **({"precise": True} if precise else {}), **kw)
    w, u = _weights(c, ref.seed)
    ((out.float() * w.cuda()).sum() + (lse * u.cuda()).sum()).backward()
    torch.cuda.synchronize()
    st = C.err_stats(out.detach().float(), ref.out)
    lse_err = (lse.detach().double().cpu() - ref.lse).abs().max().item()
    print(f"LSE_MERGE {c.run} {c.side} {c.dtype} precise={precise} groups={groups} seed={ref.seed}: out {st} | lse max_abs {lse_err:.3e}")
    if forward_bars:                                   # tests/test_gpu_forward.py: _check, test_lse_matches_logsumexp
        assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] and st["rel_rms"] <= REL_RMS, st
        assert lse_err < 2e-2, lse_err
    for name, t, r in (("dq", q, ref.dq), ("dk", k, ref.dk), ("dv", v, ref.dv)):
        gs = C.err_stats(t.grad.float(), r)
        print(f"LSE_MERGE   {name} {gs}")
        if precise:
            _grad_check(t.grad.float().cpu(), r.float(), name)
        else:                                          # tests/test_gpu_backward.py: _check
            assert gs["finite"] and gs["max_abs"] <= G_MAX * gs["ref_max"] + 1e-6 and gs["rel_rms"] <= G_RMS, (name, gs)
    print(f"LSE_MERGE   dtc {None if tc is None else tc.grad.item()} ref {ref.dtc} | dtau {tau.grad.item()} ref {ref.dtau}")
    if tc is not None:
        assert abs(tc.grad.item() - ref.dtc) <= (2e-4 if precise else 2e-2) * max(1.0, abs(ref.dtc)), (tc.grad.item(), ref.dtc)
    assert abs(tau.grad.item() - ref.dtau) <= (3e-4 if precise else 3e-2) * max(1.0, abs(ref.dtau)), (tau.grad.item(), ref.dtau)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", FUSED)
def test_gradient_through_lse(run, side, dtype):
    _check_against_oracle(_case(run, side, dtype))


@pytest.mark.parametrize("side", ["dec", "enc"])
def test_gradient_through_lse_precise(side):
    _check_against_oracle(_case("clevrtr/gta", side, torch.float32), precise=True)


def test_gradient_through_lse_rho_apply_route():
    c = _case("clevrtr/gta_euclid", "dec", torch.float32)
    q, k, _ = c.dev
    assert G2.generic_route(tuple(q.shape), k.shape[2], torch.float32, c.f_dims, c.so3, c.Nq, NK, euclid=True, needs_grad=True) == "apply"
    _check_against_oracle(c)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["dec", "enc"])
@pytest.mark.parametrize("run", FUSED)
def test_split_equals_whole(run, side, dtype):
    """key views [0:4], [4:5], [5:13]: 80 keys (two tiles, ragged), 20 keys (one tile: the true-row-max rule), 160 keys (three tiles, a tail)"""
    _check_against_oracle(_case(run, side, dtype), groups=(4, 1, 8), forward_bars=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_more_than_sixteen_views(dtype):
    """20 views of 8 tokens in groups of 16 + 4 views (128 + 32 keys); one call of 20 views has no fused kernel"""
    c = _case20(dtype)
    route = lambda nk: G2.attention_route(tuple(c.dev[0].shape), nk * 8, dtype, c.f_dims, c.so3, 1, nk, needs_grad=True)
    assert route(20) is None and route(16) is not None and route(4) is not None
    _check_against_oracle(c, groups=16, forward_bars=True)

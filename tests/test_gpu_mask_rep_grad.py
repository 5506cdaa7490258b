"""GPU: pose and coordinate gradients under key and query masks (`gta_attention(..., key_mask=, key_mask_backward=True,
key_mask_rep_grad=True, query_mask=)` with tables that require grad; `gta_rep_grad_sums_masked` + the algebra of gta_amd/repgrad.py under the
device masks).  Modelled on tests/test_gpu_key_views_rep_grad.py.

Small shapes: those of tests/test_gpu_key_views.py (imported): B = 5, H = 2, 13 views x 20 tokens, layouts clevrtr/gta and msn/gta_so3, bf16
and fp32.  Decoder leg (Tq = 150): key mask only.  Encoder leg: key mask plus query_mask of the same tokens, one shared table in both roles.
Leaves: input_transforms, input_coord and, on the decoder leg, target_transforms and target_coord.

Masks, one per scene (`_mask_set`):
  bern     Bernoulli 0.9 / 0.5 / 0.5 / 0.25 / 0.1 (fixed seed), scene 2 with its views 5 and 6 wholly masked on top
  struct   every token | view 6 missing in the middle | view n padded inside its slot to 20 - n tokens | the first 13 tokens of views 0 .. 3
           and nothing else | view 12 whole and token 5 of view 0
  prefix   the leading views of key_views = [1, 3, 4, 7, 13]

Bars (none new).
  * Exact consistency and never-read: bit for bit.
  * Prefix masks against `key_views_backward` with the same counts: tests/test_gpu_key_mask_bwd.py holds dq, dk, dv bit-equal between a key
    mask of leading views and `key_views` without `query_views` (test_a_mask_of_leading_views_is_key_views_backward), on both legs -- so on
    those calls (key mask alone, both legs) the bar is the 1e-6 of max |ref| of `test_scene_alone` (tests/test_gpu_key_views_rep_grad.py).
    With `query_mask` beside it against `query_views` no existing test holds the activations' gradients bit-equal: REL_MAX / REL_RMS.
  * Oracle parity: REL_MAX / REL_RMS of tests/test_gpu_rep_grad.py at the two shapes of tests/test_gpu_key_views_rep_grad.py's PARITY.  A
    reference is used only where it is not a cancellation: under relative perturbations of q, k, v of bf16 rounding size (2^-9 times a
    uniform draw in [-1, 1], what bf16 inputs carry before any kernel runs) the oracle's own gradient of every leaf moves by at most
    HALF of the REL_MAX bar (`test_oracle_parity` asserts it); the loss weights' seed per (shape, mask) is the first of 0, 1, 2, ... that
    meets this (PARITY_SEEDS; found with the fp64 oracle alone, on the CPU).
  * Whole model: the fp32 bound of `_srt_grad_check` (tests/test_gpu_modules.py), 5e-2 * max(ref_max, 1e-4) + 1e-6, against the same model run
    scene by scene with the masked views physically removed -- for the mask of leading views, the one this fixture can remove (a convolution
    encodes whole views: tokens masked inside a view cannot be cut out of it).  Under the structured mask (a missing middle view, a view
    padded inside its slot) the first two checks alone: finite, exact zeros."""
import functools

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native, repgrad
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests.test_gpu_key_views import B, H, NK, PK, KV, TK, _case
from tests.test_gpu_key_views_bwd import _w
from tests.test_gpu_key_views_rep_grad import PARITY, _parity_inputs
from tests.test_gpu_rep_grad import REL_MAX, REL_RMS

pytestmark = pytest.mark.gpu

LAYOUTS = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
SIDES = ["dec", "enc"]
MASKS = ["bern", "struct"]
FILLS = (0.0, 0.5, float("nan"), float("inf"))
CASES = [(r, s, d, m) for r in LAYOUTS for s in SIDES for d in DTYPES for m in MASKS]


@functools.lru_cache(maxsize=None)
def _mask_set(name):
    """bool [B, TK] on the CPU"""
    m = torch.zeros(B, TK, dtype=torch.bool)
    if name == "bern":
        g = torch.Generator().manual_seed(2024)
        for b, p in enumerate((0.9, 0.5, 0.5, 0.25, 0.1)):
            m[b] = torch.rand(TK, generator=g) < p
        m[2, 5 * PK:7 * PK] = False
    elif name == "struct":
        m[0] = True
        m[1] = True
        m[1, 6 * PK:7 * PK] = False
        for n in range(NK):
            m[2, n * PK:n * PK + PK - n] = True
        for n in range(4):
            m[3, n * PK:n * PK + 13] = True
        m[4, 12 * PK:] = True
        m[4, 5] = True
    elif name == "prefix":
        for b, n in enumerate(KV):
            m[b, :n * PK] = True
    assert bool(m.any(1).all())
    return m


def _live_views(mask):
    return mask.view(B, NK, PK).any(-1)


def test_masks_hold_what_they_say():
    for name in MASKS:
        m = _mask_set(name)
        lv = _live_views(m)
        assert bool((~lv).any()) and bool(lv.any(1).all()) and not bool(m.all()), name
        # a wholly masked view between live ones, and a live view with masked tokens
        assert any(bool(~lv[b, n]) and bool(lv[b, :n].any()) and bool(lv[b, n + 1:].any()) for b in range(B) for n in range(1, NK - 1)), name
        assert bool((lv & ~m.view(B, NK, PK).all(-1)).any()), name
    assert _mask_set("prefix").sum(1).tolist() == [n * PK for n in KV]


def _leaf_names(side):
    return ("input_transforms", "input_coord") + (("target_transforms", "target_coord") if side == "dec" else ())


def _tables(c, ex):
    """the case's leaves -> packed tables, as a model builds them"""
    gta_amd.pre_compute_reps_encoder(c.enc, ex)
    if c.side == "dec":
        gta_amd.pre_compute_reps_decoder(c.dec, ex)
    return gta_amd.pack_reps(ex, c.f_dims)


def _run(c, mask, fill=None, query_mask=None, how="mask", spy=None):
    """one forward + backward with every leaf requiring grad.  ``mask``: the key mask; ``query_mask``: None = the leg's own (encoder leg: the
    key mask, decoder leg: none), False = none.  ``fill``: what everything a masked token or wholly masked view owns holds -- k, v rows,
    coordinates, extrinsics and (with a query mask) the dead q and dout rows.  how='views': under key_views = KV with key_views_backward
    (and query_views = KV where a query mask is asked).  -> ({leaf: grad}, (dq, dk, dv))"""
    if query_mask is None:
        query_mask = mask if c.side == "enc" else False
    qm = None if query_mask is False else query_mask
    ex = {n: c.ex[n].clone() for n in _leaf_names(c.side)}
    q, k, v = (t.detach().clone() for t in c.dev)
    w = _w(c).cuda()
    if fill is not None:
        dead_t, dead_v = (~mask).cuda(), ~_live_views(mask)
        ex["input_transforms"][dead_v] = fill
        ex["input_coord"][(~mask).view(B, NK, PK)] = fill
        k.permute(0, 2, 1, 3)[dead_t] = fill
        v.permute(0, 2, 1, 3)[dead_t] = fill
        if qm is not None:
            q.permute(0, 2, 1, 3)[(~qm).cuda()] = fill
            w.permute(0, 2, 1, 3)[(~qm).cuda()] = fill
    leaves = {n: t.cuda().requires_grad_() for n, t in ex.items()}
    packed = _tables(c, dict(leaves))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    if how == "mask":
        kw = dict(key_mask=mask.cuda(), key_mask_backward=True, key_mask_rep_grad=True, **({} if qm is None else {"query_mask": qm.cuda()}))
    else:
        kw = dict(key_views=KV, key_views_backward=True, **({} if qm is None else {"query_views": KV}))
    real = repgrad.table_grads
    if spy is not None:
        def wrapped(*a, **k_):
            res = real(*a, **k_)
            spy.append((a, k_, res))
            return res
        G2._repgrad.table_grads = wrapped
    try:
        out = gta_amd.gta_attention(q, k, v, c.f_dims, packed, so3_degree=c.so3, trans_coeff=c.tc, scale=c.scale, **kw)
        out.backward(w.to(out.dtype))
        torch.cuda.synchronize()
    finally:
        G2._repgrad.table_grads = real
    return {n: t.grad for n, t in leaves.items()}, (q.grad, k.grad, v.grad)


@functools.lru_cache(maxsize=None)
def _got(run, side, dtype, masks):
    return _run(_case(run, side, dtype), _mask_set(masks))


@pytest.mark.parametrize("run, side, dtype, masks", CASES)
def test_every_leaf_gets_a_finite_gradient(run, side, dtype, masks):
    """1. the call no longer raises with the keyword; every leaf gets a finite gradient that is not all zero"""
    grads, _ = _got(run, side, dtype, masks)
    for n in _leaf_names(side):
        g = grads[n]
        assert g is not None and g.shape == _case(run, side, dtype).ex[n].shape, n
        assert bool(torch.isfinite(g).all()) and bool(g.abs().max() > 0), (run, side, dtype, masks, n)


def test_without_the_keyword_the_call_still_refuses():
    c = _case("clevrtr/gta", "dec", torch.bfloat16)
    leaves = {n: c.ex[n].clone().cuda().requires_grad_() for n in _leaf_names("dec")}
    packed = _tables(c, dict(leaves))
    with pytest.raises(native.GtaError, match="no pose / coordinate gradients under a key mask yet"):
        gta_amd.gta_attention(*c.dev, c.f_dims, packed, so3_degree=c.so3, trans_coeff=c.tc, scale=c.scale, key_mask=_mask_set("bern").cuda(),
                              key_mask_backward=True)


@pytest.mark.parametrize("run, side, dtype, masks", CASES)
def test_masked_views_and_tokens_get_exactly_zero(run, side, dtype, masks):
    """2. extrinsics of views without a live token and coordinates of masked tokens: exactly zero (encoder leg: in both roles of the table)"""
    grads, _ = _got(run, side, dtype, masks)
    mask = _mask_set(masks)
    lv = _live_views(mask).cuda()
    mt = mask.view(B, NK, PK).cuda()
    gE, gC = grads["input_transforms"], grads["input_coord"]
    assert torch.count_nonzero(gE[~lv]) == 0 and torch.count_nonzero(gC[~mt]) == 0, (run, side, dtype, masks)
    for b in range(B):
        assert bool(gE[b][lv[b]].abs().max() > 0) and bool(gC[b][mt[b]].abs().max() > 0), (run, side, dtype, masks, b)


@pytest.mark.parametrize("run, side, dtype, masks", CASES)
def test_masked_content_is_never_read(run, side, dtype, masks):
    """3. 0.0, 0.5, NaN and Inf in everything a masked token or wholly masked view owns (encoder leg: the dead query rows too): every leaf
    gradient and dq, dk, dv bit-identical across the fills"""
    c = _case(run, side, dtype)
    mask = _mask_set(masks)
    ref_g, ref_qkv = _run(c, mask, FILLS[0])
    for fill in FILLS[1:]:
        g, qkv = _run(c, mask, fill)
        for n in _leaf_names(side):
            assert bool(torch.isfinite(g[n]).all()) and torch.equal(g[n], ref_g[n]), (run, side, dtype, masks, fill, n)
        for name, a, r in zip(("dq", "dk", "dv"), qkv, ref_qkv):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, r), (run, side, dtype, masks, fill, name)
    own_g, own_qkv = _got(run, side, dtype, masks)                  # and the content the case came with (valid poses, random rows)
    for n in _leaf_names(side):
        assert torch.equal(own_g[n], ref_g[n]), (run, side, dtype, masks, n)
    assert torch.equal(own_qkv[1], ref_qkv[1]) and torch.equal(own_qkv[2], ref_qkv[2])


@pytest.mark.parametrize("run, side, dtype, masks", CASES)
def test_exact_consistency_with_the_unmasked_pass(run, side, dtype, masks):
    """4. `table_grads` with masks against `table_grads` without masks on the same dq / dk / dv with the dead rows of q, k, v, out, dout set to
    zero: bit for bit at every view with a live token and every live token; zeros elsewhere"""
    c = _case(run, side, dtype)
    mask = _mask_set(masks)
    spy = []
    _run(c, mask, spy=spy)
    assert len(spy) == 1
    (desc, tables, meta, tc, q_pairs, k_pairs), kw, got = spy[0]
    q_live, k_live = kw["masks"]
    assert kw["direct"] is False and torch.equal(k_live.cpu(), mask) and (q_live is None) == (side == "dec")
    assert q_live is None or torch.equal(q_live.cpu(), mask)

    def zeroed(pairs, live):
        if live is None:
            return pairs
        keep = live[:, None, :, None]
        return tuple(tuple(torch.where(keep, t, torch.zeros((), dtype=t.dtype, device=t.device)) for t in ab) for ab in pairs)

    for pairs, live in ((q_pairs, q_live), (k_pairs, k_live)):          # the gradients' own dead rows are zeros already
        if live is not None:
            grad = pairs[0][1] if pairs is q_pairs else pairs[0][0]
            assert torch.count_nonzero(grad.permute(0, 2, 1, 3)[~live]) == 0
    ref = repgrad.table_grads(desc, tables, meta, tc, zeroed(q_pairs, q_live), zeroed(k_pairs, k_live), direct=False)
    torch.cuda.synchronize()
    n_checked = 0
    for i, (g, r) in enumerate(zip(got, ref)):
        if g is None:
            assert r is None
            continue
        live = (q_live, k_live)[i % 2]
        if live is None:
            assert torch.equal(g, r), (run, side, dtype, masks, repgrad.TABLES[i])
        else:
            T, N = live.shape[1], (desc.Nq, desc.Nk)[i % 2]
            sel = live.view(B, N, T // N).any(-1) if i < 2 else live
            assert torch.equal(g[sel], r[sel]) and bool(g[sel].abs().max() > 0), (run, side, dtype, masks, repgrad.TABLES[i])
            assert torch.count_nonzero(g[~sel]) == 0, (run, side, dtype, masks, repgrad.TABLES[i])
        n_checked += 1
    assert n_checked == 4


@pytest.mark.parametrize("run, side, dtype", [(r, s, d) for r in LAYOUTS for s in SIDES for d in DTYPES])
def test_prefix_masks_against_key_views_backward(run, side, dtype):
    """5. a mask of leading views against key_views with the same counts.  Key mask alone (both legs): 1e-6 of max |ref| per leaf.  With the
    query mask beside it (encoder leg) against query_views: REL_MAX / REL_RMS"""
    c = _case(run, side, dtype)
    mask = _mask_set("prefix")
    got, _ = _run(c, mask, query_mask=False)
    ref, _ = _run(c, mask, query_mask=False, how="views")
    for n in _leaf_names(side):
        r, g = ref[n].double(), got[n].double()
        err, bar = (g - r).abs().max().item(), 1e-6 * r.abs().max().item()
        print(f"MASK_REP_GRAD prefix {run} {side} {dtype} {n}: max err {err:.3e}, bar {bar:.3e}")
        assert r.abs().max().item() > 0 and err <= bar, (run, side, dtype, n, err, bar)
    if side == "enc":
        got, _ = _run(c, mask)
        ref, _ = _run(c, mask, how="views")
        for n in _leaf_names(side):
            st = C.err_stats(got[n].double().cpu(), ref[n].double().cpu())
            print(f"MASK_REP_GRAD prefix+queries {run} {dtype} {n}: max {st['max_abs'] / st['ref_max']:.2e} rms {st['rel_rms']:.2e}")
            assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS, (run, dtype, n, st)


# ---- oracle parity ----------------------------------------------------------------------------------------------------------------------------
PARITY_MASKS = ("bern", "struct")
PARITY_SEEDS = {("ms-enc", "bern"): 0, ("ms-enc", "struct"): 0, ("cl-dec", "bern"): 0, ("cl-dec", "struct"): 0}


def _parity_mask(name, kind):
    """bool [3, Nk * Pk]: Bernoulli 0.5 tokens; or a missing middle view / views padded inside their slots / a single view"""
    (_, _, _, _, Nk, Pk, *_), _, _ = PARITY[name]
    m = torch.zeros(3, Nk * Pk, dtype=torch.bool)
    if kind == "bern":
        m[:] = torch.rand(3, Nk * Pk, generator=torch.Generator().manual_seed(7)) < 0.5
    else:
        m[0] = True
        m[0, Pk:2 * Pk] = False                                # view 1 missing, views 0 and 2 live
        for n in range(Nk):
            m[1, n * Pk:n * Pk + Pk - 37 * (n + 1)] = True     # padded inside their slots
        m[2, (Nk - 1) * Pk:] = True                            # the last view alone
    return m


def _oracle_masked(ak, ex, qkv, w, mask, self_attn, tc, jitter=None):
    """fp64 autograd through the oracle's differentiable reps, scene by scene, the valid key columns selected (and, in self-attention, the
    loss taken over the live query rows) -- formed as tests/test_gpu_key_mask_bwd.py's `_oracle_scene`.  jitter: a generator; q, k, v get
    relative perturbations of bf16 rounding size"""
    grads = {k_: [] for k_ in ex}
    for b in range(mask.shape[0]):
        ex_b = {k_: v_[b:b + 1].clone().requires_grad_() for k_, v_ in ex.items()}
        reps = O.encoder_reps(ak, ex_b)
        if not self_attn:
            reps = O.decoder_reps(ak, ex_b, reps)
        q, k, v = (t[b:b + 1] for t in qkv)
        if jitter is not None:
            q, k, v = (t * (1 + 2.0 ** -9 * (2 * torch.rand(t.shape, generator=jitter, dtype=torch.float64) - 1)) for t in (q, k, v))
        cols = mask[b].nonzero().flatten()
        qt, kt, vt = O.transform_qkv(q, k, v, ak["f_dims"], reps, tc, True, False)
        o, _ = O.softmax_attention(qt, kt[:, :, cols], vt[:, :, cols], q.shape[-1] ** -0.5)
        out = O.inverse_transform_out(o, ak["f_dims"], reps, tc, False)
        loss = out * w[b:b + 1]
        (loss[:, :, cols] if self_attn else loss).sum().backward()
        for k_, v_ in ex_b.items():
            grads[k_].append(v_.grad)
    return {k_: torch.cat(v_) for k_, v_ in grads.items()}


@pytest.mark.parametrize("kind", PARITY_MASKS)
@pytest.mark.parametrize("name", list(PARITY))
def test_oracle_parity(name, kind):
    ak, ex, qkv, w, _, self_attn, Pk, Pq = _parity_inputs(name, seed=PARITY_SEEDS[(name, kind)])
    mask = _parity_mask(name, kind)
    ref = _oracle_masked(ak, ex, qkv, w, mask, self_attn, 0.3)
    moved = _oracle_masked(ak, ex, qkv, w, mask, self_attn, 0.3, jitter=torch.Generator().manual_seed(99))
    for key, r in ref.items():                                  # the reference is not a cancellation (docstring)
        shift, bar = (moved[key] - r).abs().max().item(), REL_MAX * r.abs().max().item()
        print(f"MASK_REP_GRAD parity {name} {kind} d {key}: the oracle moves by {shift / bar:.3f} of the bar under bf16-size input noise")
        assert r.abs().max().item() > 0 and shift <= 0.5 * bar, (name, kind, key, shift, bar)
    exd = {k_: v_.float().cuda().requires_grad_() for k_, v_ in ex.items()}
    leaves = dict(exd)
    q, k, v = (t.to(torch.bfloat16).cuda().requires_grad_() for t in qkv)
    gta_amd.pre_compute_reps_encoder(ak, exd)
    if not self_attn:
        gta_amd.pre_compute_reps_decoder(ak, exd)
    packed = gta_amd.pack_reps(exd, ak["f_dims"])
    out = gta_amd.gta_attention(q, k, v, ak["f_dims"], packed, so3_degree=exd.get("gta_so3_degree", 0), trans_coeff=torch.tensor([0.3], device="cuda"),
                                key_mask=mask.cuda(), key_mask_backward=True, key_mask_rep_grad=True,
                                **({"query_mask": mask.cuda()} if self_attn else {}))
    wd = w.float().cuda()
    if self_attn:                                               # (dead rows' dout is never read; the product below must stay finite)
        wd = torch.where(mask.cuda()[:, None, :, None], wd, torch.zeros((), device="cuda"))
    (out.float() * wd).sum().backward()
    torch.cuda.synchronize()
    failures = []
    Nk = mask.shape[1] // Pk
    for key, r in ref.items():
        g = leaves[key].grad.detach().double().cpu()
        st = C.err_stats(g, r.double())
        print(f"MASK_REP_GRAD parity {name} {kind} d {key}: max {st['max_abs'] / st['ref_max']:.4f} rms {st['rel_rms']:.4f}")
        if not (st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS):
            failures.append((name, kind, key, st))
    lv = mask.view(3, Nk, Pk).any(-1)
    assert torch.count_nonzero(leaves["input_transforms"].grad.cpu()[~lv]) == 0
    assert torch.count_nonzero(leaves["input_coord"].grad.cpu().reshape(3, Nk * Pk, 2)[~mask]) == 0
    assert not failures, failures


# ---- whole model ---------------------------------------------------------------------------------------------------------------------------
def _srt():
    from gta_amd import srt
    method = {"method": {"name": "gta", "args": {"f_dims": {"triv": 0, "se3": 16, "so2": 8}, "so2": 2, "max_freq_h": 1, "max_freq_w": 1}}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 48, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 48, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
                              "attn_args": method}}
    torch.manual_seed(0)
    return srt, srt.TransformingSRT(cfg).cuda().eval()


def test_whole_model_pose_gradients_under_input_masks():
    """the tiny fused-layout TransformingSRT of tests/test_gpu_key_views_rep_grad.py (fp32) with input_mask, input_mask_backward,
    input_mask_rep_grad and input_mask_queries, all four extras leaves requiring grad.  Leading views [2, 3]: against the same model run
    scene by scene with the masked views physically removed.  A structured mask (scene 0: its middle view missing; scene 1: view 1 padded
    inside its slot): finite, and exact zeros at wholly masked views and masked tokens"""
    srt, model = _srt()
    nb, NV, views, npix = 2, 3, [2, 3], 40
    data = srt.synthetic_batch(nb, n_in=NV, n_tgt=1, image=32, points_per_view=8, device="cuda", seed=1)
    P = data["input_coord"].shape[2]
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, 1, npix, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 1, 1, 3, generator=g).cuda().expand(-1, 1, npix, -1)
    coord = torch.from_numpy(G2.make_2dcoord(16, 20)).cuda().flatten(0, 1)[:npix]
    w = torch.randn(nb, npix, 3, generator=g).cuda()
    names = ("input_transforms", "input_coord", "target_transforms", "target_coord")

    def fresh(mask=None):
        lv = {"input_transforms": data["input_transforms"].detach().clone(), "input_coord": data["input_coord"].detach().clone(),
              "target_transforms": data["target_transforms"][:, :1].detach().clone(), "target_coord": coord[None, None].expand(nb, 1, -1, -1).clone()}
        if mask is not None:                               # zero-filled extrinsics of wholly masked views, coordinates of masked tokens
            lv["input_transforms"][~mask.any(-1)] = 0.0
            lv["input_coord"][~mask] = 0.0
        return {k_: v_.float().requires_grad_() for k_, v_ in lv.items()}

    def step(lv, sl, n, mask):
        nb_ = data["input_images"][sl].shape[0]
        extras = {"input_transforms": lv["input_transforms"][sl, :n], "input_coord": lv["input_coord"][sl, :n],
                  "target_transforms": lv["target_transforms"][sl], "target_coord": lv["target_coord"][sl]}
        images = data["input_images"][sl, :n]
        how = {}
        if mask is not None:
            images = torch.where(mask.any(-1)[:, :, None, None, None], images, torch.zeros((), device="cuda"))
            how = dict(input_mask=mask, input_mask_backward=True, input_mask_rep_grad=True, input_mask_queries=True)
        pix, _ = model(images, data["input_camera_pos"][sl, :n], data["input_rays"][sl, :n], cam[sl], rays[sl], extras, **how)
        (pix.reshape(nb_, npix, 3).float() * w[sl]).sum().backward()

    alone = fresh()
    for b, n in enumerate(views):
        step(alone, slice(b, b + 1), n, None)
    lead = torch.zeros(nb, NV, P, dtype=torch.bool, device="cuda")
    for b, n in enumerate(views):
        lead[b, :n] = True
    struct = torch.ones(nb, NV, P, dtype=torch.bool, device="cuda")
    struct[0, 1] = False
    struct[1, 1, P // 2:] = False
    for kind, mask in (("leading", lead), ("struct", struct)):
        batched = fresh(mask)
        step(batched, slice(0, nb), NV, mask)
        torch.cuda.synchronize()
        for name in names:
            got = batched[name].grad
            assert got is not None and bool(torch.isfinite(got).all()) and bool(got.abs().max() > 0), (kind, name)
        assert torch.count_nonzero(batched["input_transforms"].grad[~mask.any(-1)]) == 0, kind
        assert torch.count_nonzero(batched["input_coord"].grad[~mask]) == 0, kind
        if kind != "leading":
            continue
        for name in names:
            ref, got = alone[name].grad, batched[name].grad
            ref_max = ref.abs().max().item()
            err = (got - ref).abs().max().item()
            bound = 5e-2 * max(ref_max, 1e-4) + 1e-6
            print(f"MASK_REP_GRAD srt d {name}: max err {err:.3e}, ref max {ref_max:.3e}, bound {bound:.3e}")
            assert ref_max > 0 and err <= bound, (name, err, bound)

"""GPU: pose and coordinate gradients on batches that mix view counts (`gta_attention(..., key_views=, key_views_backward=True,
query_views=)` with tables that require grad; `gta_rep_grad_sums_varlen` + the masked algebra of gta_amd/repgrad.py).

Small shapes: those of tests/test_gpu_key_views.py (imported): B = 5, H = 2, 13 views x 20 tokens, key_views = [1, 3, 4, 7, 13], layouts
clevrtr/gta and msn/gta_so3, bf16 and fp32, decoder leg (Tq = 150) and encoder leg (query_views = key_views, one shared table in both
roles).  Leaves: input_transforms, input_coord and, on the decoder leg, target_transforms and target_coord, through
pre_compute_reps_encoder / _decoder + pack_reps.

Bars (none new).  Scene alone: the sums are bit-identical by construction, the fp64 algebra may batch differently and is rounded once to
fp32 (one ulp is 1.2e-7 of the element): 1e-6 of max |ref| per leaf.  Oracle parity: REL_MAX / REL_RMS of tests/test_gpu_rep_grad.py at two
of its SHAPES.  Whole model: the fp32 bound `_srt_grad_check` (tests/test_gpu_modules.py) applies to parameters,
5e-2 * max(ref_max, 1e-4) + 1e-6."""
import functools
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native, repgrad
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests.test_gpu_key_views import B, H, NK, PK, KV, _case, _tc
from tests.test_gpu_key_views_bwd import _w
from tests.test_gpu_rep_grad import REL_MAX, REL_RMS, SHAPES, _dense_leaves, _oracle_grads

pytestmark = pytest.mark.gpu

LAYOUTS = ["clevrtr/gta", "msn/gta_so3"]
DTYPES = [torch.float32, torch.bfloat16]
SIDES = ["dec", "enc"]
FILLS = (0.0, 0.5, float("nan"), float("inf"))
CASES = [(r, s, d) for r in LAYOUTS for s in SIDES for d in DTYPES]


def _leaf_names(side):
    return ("input_transforms", "input_coord") + (("target_transforms", "target_coord") if side == "dec" else ())


def _tables(c, ex):
    """the case's leaves -> packed tables, as a model builds them"""
    gta_amd.pre_compute_reps_encoder(c.enc, ex)
    if c.side == "dec":
        gta_amd.pre_compute_reps_decoder(c.dec, ex)
    return gta_amd.pack_reps(ex, c.f_dims)


def _run(c, fill=None):
    """one forward + backward under key_views with every leaf requiring grad; ``fill``: what everything that belongs to a padded view
    holds -- k, v rows, extrinsics, coordinates and (encoder leg) q and dout rows.  -> ({leaf: grad}, (dq, dk, dv))"""
    ex = {n: c.ex[n].clone() for n in _leaf_names(c.side)}
    q, k, v = (t.detach().clone() for t in c.dev)
    w = _w(c).cuda()
    if fill is not None:
        for b, n in enumerate(KV):
            ex["input_transforms"][b, n:] = fill
            ex["input_coord"][b, n:] = fill
            k[b, :, n * PK:] = fill
            v[b, :, n * PK:] = fill
            if c.side == "enc":
                q[b, :, n * PK:] = fill
                w[b, :, n * PK:] = fill
    leaves = {n: t.cuda().requires_grad_() for n, t in ex.items()}
    packed = _tables(c, dict(leaves))
    q, k, v = (t.requires_grad_() for t in (q, k, v))
    out = gta_amd.gta_attention(q, k, v, c.f_dims, packed, so3_degree=c.so3, trans_coeff=c.tc, scale=c.scale, key_views=KV,
                                key_views_backward=True, **({"query_views": KV} if c.side == "enc" else {}))
    out.backward(w.to(out.dtype))
    torch.cuda.synchronize()
    return {n: t.grad for n, t in leaves.items()}, (q.grad, k.grad, v.grad)


@functools.lru_cache(maxsize=None)
def _got(run, side, dtype):
    return _run(_case(run, side, dtype))


@pytest.mark.parametrize("run, side, dtype", CASES)
def test_every_leaf_gets_a_finite_gradient(run, side, dtype):
    """1. the call no longer raises; every leaf gets a finite gradient that is not all zero"""
    grads, _ = _got(run, side, dtype)
    for n in _leaf_names(side):
        g = grads[n]
        assert g is not None and g.shape == _case(run, side, dtype).ex[n].shape, n
        assert bool(torch.isfinite(g).all()) and bool(g.abs().max() > 0), (run, side, dtype, n)


@pytest.mark.parametrize("run, side, dtype", CASES)
def test_padded_views_get_exactly_zero(run, side, dtype):
    """2. gradients of padded views' extrinsics and padded tokens' coordinates are exactly zero (encoder leg: in both roles of the table)"""
    grads, _ = _got(run, side, dtype)
    for b, n in enumerate(KV):
        for name in ("input_transforms", "input_coord"):
            assert torch.count_nonzero(grads[name][b, n:]) == 0, (run, side, dtype, b, name)
            assert bool(grads[name][b, :n].abs().max() > 0), (run, side, dtype, b, name)


@pytest.mark.parametrize("run, side, dtype", CASES)
def test_padding_is_never_read(run, side, dtype):
    """3. 0.0, 0.5, NaN and Inf in everything that belongs to a padded view: every leaf gradient, dq, dk, dv equal bit for bit"""
    c = _case(run, side, dtype)
    ref_g, ref_qkv = _run(c, FILLS[0])
    for fill in FILLS[1:]:
        g, qkv = _run(c, fill)
        for n in _leaf_names(side):
            assert bool(torch.isfinite(g[n]).all()) and torch.equal(g[n], ref_g[n]), (run, side, dtype, fill, n)
        for name, a, r in zip(("dq", "dk", "dv"), qkv, ref_qkv):
            assert bool(torch.isfinite(a).all()) and torch.equal(a, r), (run, side, dtype, fill, name)
    own_g, own_qkv = _got(run, side, dtype)                         # and the padding the case came with (valid poses, random rows)
    for n in _leaf_names(side):
        assert torch.equal(own_g[n], ref_g[n]), (run, side, dtype, n)
    assert torch.equal(own_qkv[1], ref_qkv[1]) and torch.equal(own_qkv[2], ref_qkv[2])


@pytest.mark.parametrize("run, side, dtype", CASES)
def test_scene_alone(run, side, dtype):
    """4. against the unmasked `_FusedAttn` on scene b alone with keys, queries (encoder leg) and tables cut to the prefixes, on the same kernels (the
    flags of test_bits_of_the_scene_alone): each leaf gradient within 1e-6 of max |ref|"""
    c = _case(run, side, dtype)
    grads, _ = _got(run, side, dtype)
    w = _w(c).cuda()
    flags = native.FLAG_V_TRANSFORM | native.FLAG_ROWS32 | native.FLAG_FWD2_GENERIC | native.FLAG_BWD_KEYS32
    for b, n in enumerate(KV):
        rows = c.Tq if side == "dec" else n * PK
        leaves = {name: (c.ex[name][b:b + 1, :n] if name.startswith("input") else c.ex[name][b:b + 1]).clone().cuda().requires_grad_()
                  for name in _leaf_names(side)}
        packed, carriers = repgrad.split_tables(_tables(c, dict(leaves)))
        assert carriers
        q, k, v = c.dev
        q, k, v = (t.detach().clone().requires_grad_() for t in (q[b:b + 1, :, :rows], k[b:b + 1, :, :n * PK], v[b:b + 1, :, :n * PK]))
        cfg = ({k_: int(v_) for k_, v_ in c.f_dims.items()}, int(c.so3), 1 if side == "dec" else n, n, float(c.scale), flags)
        out = G2._FusedAttn.apply(q, k, v, c.tc, None, (cfg, None, G2._Mask()), packed.get("vrep_q"), packed.get("vrep_k"), packed.get("cs_q"),
                                  packed.get("cs_k"), *carriers)
        out.backward(w[b:b + 1, :, :rows].to(out.dtype))
        torch.cuda.synchronize()
        for name in _leaf_names(side):
            ref = leaves[name].grad[0].double()
            got = (grads[name][b, :n] if name.startswith("input") else grads[name][b]).double()
            err, bar = (got - ref).abs().max().item(), 1e-6 * ref.abs().max().item()
            print(f"KEY_VIEWS_REP_GRAD alone {run} {side} {dtype} scene {b} ({n} views) {name}: max err {err:.3e}, bar {bar:.3e}")
            assert ref.abs().max().item() > 0 and err <= bar, (run, side, dtype, b, name, err, bar)


@pytest.mark.parametrize("run, side, dtype", [("clevrtr/gta", "dec", torch.bfloat16), ("clevrtr/gta", "enc", torch.float32),
                                              ("msn/gta_so3", "dec", torch.float32), ("msn/gta_so3", "enc", torch.bfloat16)])
def test_dense_reference_style_leaves(run, side, dtype):
    """5. the reference's dense reps tensors (se3rep_k, so2rep_k, ...) as leaves, through the drop-in operator: gradients under key_views,
    exactly zero on the padded slices"""
    c = _case(run, side, dtype)
    ex64 = {n: c.ex[n].double() for n in _leaf_names(side)}
    reps = O.encoder_reps(c.enc, ex64)
    if side == "dec":
        reps = O.decoder_reps(c.dec, ex64, reps)
    leaves = _dense_leaves(reps, "cuda", torch.float32)
    q, k, v = (t.detach().clone().requires_grad_() for t in c.dev)
    out, _ = gta_amd.multihead_geometric_transform_attention(
        q, k, v, attn_fn=SimpleNamespace(scale=c.scale, tau=None), f_dims=c.f_dims, reps=leaves, trans_coeff=c.tc, key_views=KV,
        key_views_backward=True, query_views=KV if side == "enc" else None)
    out.backward(_w(c).cuda().to(out.dtype))
    torch.cuda.synchronize()
    checked = set()
    for key in ("se3rep_k", "so2rep_k") + (("se3rep_q", "inv_se3rep_q", "so2rep_q") if side == "enc" else ()):
        if key not in leaves or not leaves[key].requires_grad:
            continue
        g = leaves[key].grad
        assert g is not None and bool(torch.isfinite(g).all()), key
        per = 1 if "se3" in key else PK
        for b, n in enumerate(KV):
            assert torch.count_nonzero(g[b, n * per:]) == 0 and bool(g[b, :n * per].abs().max() > 0), (run, side, key, b)
        checked.add(key)
    assert {"se3rep_k", "so2rep_k"} <= checked, checked


# ---- oracle parity at shapes where the bars are known to hold -------------------------------------------------------------------------------
PARITY = {"ms-enc": (SHAPES["ms-enc"], [2, 5, 3], True), "cl-dec": (SHAPES["cl-dec"][:4] + (3,) + SHAPES["cl-dec"][5:], [1, 3, 2], False)}


def _parity_inputs(name, nb=3, seed=0):
    (_, Hh, Nq, Pq, Nk, Pk, f_dims, so2, so3), views, self_attn = PARITY[name]
    g = torch.Generator().manual_seed(seed)
    ak = {"f_dims": f_dims, "so2": so2, "so3": so3, "max_freq_h": 1, "max_freq_w": 1}
    ex = {"input_transforms": O.random_extrinsics(nb, Nk, g, torch.float64), "input_coord": torch.rand(nb, Nk * Pk, 2, generator=g, dtype=torch.float64)}
    if not self_attn:
        ex["target_transforms"] = O.random_extrinsics(nb, Nq, g, torch.float64)
        ex["target_coord"] = torch.rand(nb, Nq * Pq, 2, generator=g, dtype=torch.float64)
    dh = sum(f_dims.values())
    qkv = [torch.randn(nb, Hh, n, dh, generator=g, dtype=torch.float64) for n in (Nq * Pq, Nk * Pk, Nk * Pk)]
    w = torch.randn(nb, Hh, Nq * Pq, dh, generator=g, dtype=torch.float64)
    return ak, ex, qkv, w, views, self_attn, Pk, Pq


def _hip(ak, ex, qkv, w, cross, tc, dtype, key_views=None, query_views=None):
    """`_hip_grads` of tests/test_gpu_rep_grad.py with the view counts"""
    ex = {k_: v_.float().cuda().requires_grad_() for k_, v_ in ex.items()}
    leaves = dict(ex)
    q, k, v = (t.to(dtype).cuda().requires_grad_() for t in qkv)
    gta_amd.pre_compute_reps_encoder(ak, ex)
    if cross:
        gta_amd.pre_compute_reps_decoder(ak, ex)
    packed = gta_amd.pack_reps(ex, ak["f_dims"])
    kw = {} if key_views is None else dict(key_views=key_views, key_views_backward=True, **({} if query_views is None else {"query_views": query_views}))
    out = gta_amd.gta_attention(q, k, v, ak["f_dims"], packed, so3_degree=ex.get("gta_so3_degree", 0), trans_coeff=torch.tensor([tc], device="cuda"), **kw)
    (out.float() * w.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    return {k_: v_.grad for k_, v_ in leaves.items()}


@pytest.mark.parametrize("name", list(PARITY))
def test_oracle_parity(name):
    """fp64 oracle autograd scene by scene on the prefixes, at the bars of tests/test_gpu_rep_grad.py; the statistics of the existing
    unmasked route on each scene alone are printed beside them"""
    ak, ex, qkv, w, views, self_attn, Pk, Pq = _parity_inputs(name)
    got = _hip(ak, ex, qkv, w, not self_attn, 0.3, torch.bfloat16, key_views=views, query_views=views if self_attn else None)
    failures = []
    for b, n in enumerate(views):
        rows = n * Pq if self_attn else qkv[0].shape[2]
        ex_b = {k_: (v_[b:b + 1, :n * (Pk if k_ == "input_coord" else 1)] if k_.startswith("input") else v_[b:b + 1]) for k_, v_ in ex.items()}
        qkv_b = [qkv[0][b:b + 1, :, :rows], qkv[1][b:b + 1, :, :n * Pk], qkv[2][b:b + 1, :, :n * Pk]]
        w_b = w[b:b + 1, :, :rows]
        ref = _oracle_grads(ak, ex_b, qkv_b, w_b, not self_attn, 0.3, True)
        alone = _hip(ak, ex_b, qkv_b, w_b, not self_attn, 0.3, torch.bfloat16)
        for key, r in ref.items():
            g = got[key][b:b + 1, :n * (Pk if key == "input_coord" else 1)] if key.startswith("input") else got[key][b:b + 1]
            st = C.err_stats(g.detach().double().cpu(), r.double())
            st1 = C.err_stats(alone[key].detach().double().cpu(), r.double())
            print(f"KEY_VIEWS_REP_GRAD parity {name} scene {b} ({n} views) d {key}: masked max {st['max_abs'] / st['ref_max']:.4f} rms {st['rel_rms']:.4f}"
                  f" | unmasked scene alone max {st1['max_abs'] / st1['ref_max']:.4f} rms {st1['rel_rms']:.4f}")
            if not (st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] + 1e-6 and st["rel_rms"] <= REL_RMS):
                failures.append((name, b, key, st))
        for key in ("input_transforms", "input_coord"):
            assert torch.count_nonzero(got[key][b, n * (Pk if key == "input_coord" else 1):]) == 0, (name, b, key)
    assert not failures, failures


# ---- whole model ---------------------------------------------------------------------------------------------------------------------------
def test_whole_model_pose_gradients_with_mixed_input_views():
    """the tiny fused-layout TransformingSRT of test_whole_model_step_with_mixed_input_views (fp32), input_views = [2, 3], all four extras
    leaves requiring grad: the leaf gradients of one batched step against the same model run scene by scene on its valid views"""
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
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, 1, npix, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 1, 1, 3, generator=g).cuda().expand(-1, 1, npix, -1)
    coord = torch.from_numpy(G2.make_2dcoord(16, 20)).cuda().flatten(0, 1)[:npix]
    w = torch.randn(nb, npix, 3, generator=g).cuda()
    names = ("input_transforms", "input_coord", "target_transforms", "target_coord")

    def fresh(zero_padding):
        lv = {"input_transforms": data["input_transforms"].detach().clone(), "input_coord": data["input_coord"].detach().clone(),
              "target_transforms": data["target_transforms"][:, :1].detach().clone(), "target_coord": coord[None, None].expand(nb, 1, -1, -1).clone()}
        if zero_padding:                                   # zero-filled padded extrinsics and coordinates are legal
            for b, n in enumerate(views):
                lv["input_transforms"][b, n:] = 0.0
                lv["input_coord"][b, n:] = 0.0
        return {k_: v_.float().requires_grad_() for k_, v_ in lv.items()}

    def step(lv, sl, n, input_views):
        nb_ = data["input_images"][sl].shape[0]
        extras = {"input_transforms": lv["input_transforms"][sl, :n], "input_coord": lv["input_coord"][sl, :n],
                  "target_transforms": lv["target_transforms"][sl], "target_coord": lv["target_coord"][sl]}
        pix, _ = model(data["input_images"][sl, :n], data["input_camera_pos"][sl, :n], data["input_rays"][sl, :n], cam[sl], rays[sl], extras,
                       input_views=input_views, input_views_backward=input_views is not None)
        (pix.reshape(nb_, npix, 3).float() * w[sl]).sum().backward()

    alone = fresh(False)
    for b, n in enumerate(views):
        step(alone, slice(b, b + 1), n, None)
    batched = fresh(True)
    step(batched, slice(0, nb), NV, views)
    torch.cuda.synchronize()
    for name in names:
        ref, got = alone[name].grad, batched[name].grad
        assert ref is not None and got is not None and bool(torch.isfinite(got).all()), name
        ref_max = ref.abs().max().item()
        err = (got - ref).abs().max().item()
        bound = 5e-2 * max(ref_max, 1e-4) + 1e-6
        print(f"KEY_VIEWS_REP_GRAD srt d {name}: max err {err:.3e}, ref max {ref_max:.3e}, bound {bound:.3e}")
        assert ref_max > 0 and err <= bound, (name, err, bound)
    for b, n in enumerate(views):
        for name in ("input_transforms", "input_coord"):
            assert torch.count_nonzero(batched[name].grad[b, n:]) == 0, (name, b)

"""GPU: gradients to camera poses and patch coordinates through GTA attention (gta_rep_grad_sums + gta_amd.repgrad) against fp64
autograd through the CPU oracle -- the reference's own differentiation (so3 blocks detached, gta.py:194-197,267).
Bars are relative to each gradient tensor's own magnitude, as in test_gpu_backward.py."""
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import native
from oracle import gta_oracle as O
from tests import _golden as G
from tests import _hip_cases as C

pytestmark = pytest.mark.gpu

REL_MAX, REL_RMS = 4e-2, 2e-2
DENSE = ("se3rep_q", "se3rep_k", "inv_se3rep_q", "so2rep_q", "so2rep_k", "t2rep_q", "t2rep_k", "inv_t2rep_q")


def _check(got, ref, name, rel_max=REL_MAX, rel_rms=REL_RMS):
    got = torch.zeros_like(ref) if got is None else got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    st = C.err_stats(got, ref)
    assert st["finite"], (name, st)
    assert st["max_abs"] <= rel_max * st["ref_max"] + 1e-6, (name, st)
    if rel_rms is not None:
        assert st["rel_rms"] <= rel_rms, (name, st)


def _dense_leaves(ex, device, dtype):
    """the fixture's dense tensors as fresh leaves (distinct objects per key, shared where the reference shares them)"""
    out, seen = {}, {}
    for key, t in ex.items():
        if key in DENSE:
            ident = id(t)
            if ident not in seen:
                seen[ident] = t.detach().to(dtype).to(device).requires_grad_()
            out[key] = seen[ident]
        elif isinstance(t, list):
            out[key] = [u.to(dtype).to(device) for u in t]
        else:
            out[key] = t.to(dtype).to(device)
    return out


@pytest.mark.parametrize("kv_mode", ["prepass", "fused"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("case", G.list_cases("op_"))
def test_operator_fixture_table_gradients(case, dtype, kv_mode):
    d, meta = G.load("op_" + case)
    exd = G.extras_of(d, torch.float64)
    ref_leaves = _dense_leaves(exd, "cpu", torch.float64)
    hip_leaves = _dense_leaves(exd, "cuda", torch.float32)
    q64, k64, v64 = (torch.from_numpy(d[n]).double() for n in "qkv")
    w = torch.from_numpy(d["w"]).double()
    tc = float(d["trans_coeff"])
    tau = G.tau_of(d, torch.float64, grad=False)
    out, _ = O.gta_attention(q64, k64, v64, meta["f_dims"], ref_leaves, tc, meta["v_transform"], meta["euclid"], float(d["scale"]),
                             1.0 if tau is None else tau)
    (out * w).sum().backward()
    q, k, v = (torch.from_numpy(d[n]).to(dtype).cuda() for n in "qkv")
    out, _ = gta_amd.multihead_geometric_transform_attention(
        q, k, v, attn_fn=SimpleNamespace(scale=float(d["scale"]), tau=G.tau_of(d, torch.float32, "cuda", grad=False)),
        f_dims=meta["f_dims"], reps=hip_leaves, trans_coeff=torch.tensor([tc], device="cuda"),
        v_transform=meta["v_transform"], euclid=meta["euclid"], kv_mode=kv_mode)
    (out.float() * w.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    checked = 0
    for key in DENSE:
        if key in ref_leaves and ref_leaves[key].grad is not None:
            _check(hip_leaves[key].grad, ref_leaves[key].grad, f"{case} d {key}")
            checked += 1
    assert checked > 0
    for D in hip_leaves.get("so3rep_q", []) + hip_leaves.get("so3rep_k", []):
        assert D.grad is None                                                  # detached, as in the reference


SHAPES = {   # (B, H, Nq, Pq, Nk, Pk, f_dims, so2, so3): BASELINE shapes at B = 1 (test_gpu_backward.py)
    "ms-enc": (1, 8, 5, 256, 5, 256, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}, 6, 2),
    "ms-dec": (1, 8, 5, 512, 5, 256, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}, 6, 2),
    "cl-enc": (1, 6, 2, 300, 2, 300, {"se3": 32, "so2": 32}, 8, 0),
    "cl-dec": (1, 6, 3, 853, 2, 300, {"se3": 32, "so2": 32}, 8, 0),
    "dit": (1, 6, 1, 256, 1, 256, {"so2": 64}, 16, 0),
}


def _shape_inputs(name, seed=0):
    B, H, Nq, Pq, Nk, Pk, f_dims, so2, so3 = SHAPES[name]
    cross = name.endswith("dec")
    g = torch.Generator().manual_seed(seed)
    ak = {"f_dims": f_dims, "so2": so2, "so3": so3, "max_freq_h": 1, "max_freq_w": 1}
    ex = {"input_transforms": O.random_extrinsics(B, Nk, g, torch.float64), "input_coord": torch.rand(B, Nk * Pk, 2, generator=g, dtype=torch.float64)}
    if cross:
        ex["target_transforms"] = O.random_extrinsics(B, Nq, g, torch.float64)
        ex["target_coord"] = torch.rand(B, Nq * Pq, 2, generator=g, dtype=torch.float64)
    dh = sum(f_dims.values())
    qkv = [torch.randn(B, H, n, dh, generator=g, dtype=torch.float64) for n in (Nq * Pq, Nk * Pk, Nk * Pk)]
    w = torch.randn(B, H, Nq * Pq, dh, generator=g, dtype=torch.float64)
    return ak, ex, qkv, w, cross


def _oracle_grads(ak, ex, qkv, w, cross, tc, qkv_grad):
    ex = {k_: v_.clone().requires_grad_() for k_, v_ in ex.items()}
    q, k, v = (t.clone().requires_grad_(qkv_grad) for t in qkv)
    reps = O.encoder_reps(ak, ex)
    if cross:
        reps = O.decoder_reps(ak, ex, reps)
    out, _ = O.gta_attention(q, k, v, ak["f_dims"], reps, tc)
    (out * w).sum().backward()
    return {k_: v_.grad for k_, v_ in ex.items()}


def _hip_grads(ak, ex, qkv, w, cross, tc, qkv_grad, dtype, kv_mode="auto", precise=None):
    ex = {k_: v_.float().cuda().requires_grad_() for k_, v_ in ex.items()}
    leaves = dict(ex)
    q, k, v = (t.to(dtype).cuda().requires_grad_(qkv_grad) for t in qkv)
    gta_amd.pre_compute_reps_encoder(ak, ex)
    if cross:
        gta_amd.pre_compute_reps_decoder(ak, ex)
    packed = gta_amd.pack_reps(ex, ak["f_dims"])
    tct = torch.tensor([tc], device="cuda") if ak["f_dims"].get("se3", 0) > 0 else None
    out = gta_amd.gta_attention(q, k, v, ak["f_dims"], packed, so3_degree=ex.get("gta_so3_degree", 0), trans_coeff=tct,
                                kv_mode=kv_mode, precise=precise)
    (out.float() * w.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    return {k_: v_.grad for k_, v_ in leaves.items()}


@pytest.mark.parametrize("qkv_grad", [True, False])
@pytest.mark.parametrize("name", list(SHAPES))
def test_baseline_shapes_pose_and_coordinate_gradients(name, qkv_grad):
    ak, ex, qkv, w, cross = _shape_inputs(name)
    ref = _oracle_grads(ak, ex, qkv, w, cross, 0.3, True)
    got = _hip_grads(ak, ex, qkv, w, cross, 0.3, qkv_grad, torch.bfloat16)
    for key, r in ref.items():
        if r is None:
            assert got[key] is None or not got[key].abs().any(), key
            continue
        assert got[key] is not None, (name, key)
        _check(got[key], r, f"{name} d {key}")


def test_precise_fp32_matches_and_trans_coeff_entries_contract_to_d_trans_coeff():
    """fp32-faithful mode: tight bar on d E; the trans_coeff-carrying entries of d inv_se3rep_q / d se3rep_k, contracted with the
    reps, give the existing kernels' d trans_coeff (dense leaves, separate q and k tensors)."""
    ak, ex, qkv, w, cross = _shape_inputs("cl-dec")
    ref = _oracle_grads(ak, ex, qkv, w, cross, 0.3, True)
    got = _hip_grads(ak, ex, qkv, w, cross, 0.3, True, torch.float32, kv_mode="fused", precise=True)
    for key in ("input_transforms", "target_transforms"):
        _check(got[key], ref[key], key, rel_max=1e-4, rel_rms=None)
    Et, Ein = ex["target_transforms"].float().cuda(), ex["input_transforms"].float().cuda()
    reps = {"inv_se3rep_q": Et.clone().requires_grad_(), "se3rep_q": torch.linalg.inv(Et),
            "se3rep_k": torch.linalg.inv(Ein).requires_grad_()}
    q, k, v = (t.float().cuda() for t in qkv)
    tc = torch.tensor([0.3], device="cuda", requires_grad=True)
    out, _ = gta_amd.multihead_geometric_transform_attention(q, k, v, f_dims={"se3": 32, "so2": 0, "triv": 32}, reps=reps,
                                                             trans_coeff=tc, precise=True, kv_mode="fused")
    (out * w.float().cuda()).sum().backward()
    contr = sum((reps[n].grad[..., :3, 3] * reps[n].detach()[..., :3, 3]).double().sum() for n in ("inv_se3rep_q", "se3rep_k")) / 0.3
    assert abs(contr.item() - tc.grad.item()) <= 1e-3 * max(1.0, abs(tc.grad.item())), (contr.item(), tc.grad.item())


def test_packed_and_dense_so2_paths_give_the_same_coordinate_gradient():
    ak, ex, qkv, w, cross = _shape_inputs("cl-enc")
    q, k, v = (t.float().cuda() for t in qkv)
    res = []
    for dense in (False, True):
        c = ex["input_coord"].float().cuda().requires_grad_()
        if dense:
            R = O.make_so2_reps(c, ak["so2"])
            reps = {"so2rep_q": R, "so2rep_k": R}
        else:
            cs = native.build_so2_table(c, ak["so2"], 1.0, 1.0)
            reps = {"gta_cs_q": cs, "gta_cs_k": cs}
        out, _ = gta_amd.multihead_geometric_transform_attention(q, k, v, f_dims={"triv": 32, "so2": 32}, reps=reps, precise=True,
                                                                 kv_mode="fused")
        (out * w.float().cuda()).sum().backward()
        res.append(c.grad.double().cpu())
    _check(res[0], res[1], "d coord packed vs dense", rel_max=1e-4, rel_rms=None)


def test_pose_gradients_are_deterministic():
    ak, ex, qkv, w, cross = _shape_inputs("ms-dec")
    a = _hip_grads(ak, ex, qkv, w, cross, 0.3, False, torch.bfloat16)
    b = _hip_grads(ak, ex, qkv, w, cross, 0.3, False, torch.bfloat16)
    for key in a:
        assert torch.equal(a[key], b[key]), key


@pytest.mark.parametrize("fused_blocks", [True, False])
def test_transformer_pose_gradients_vs_oracle_transformer(fused_blocks):
    ak, ex, _, _, _ = _shape_inputs("cl-enc")
    args = {"method": {"name": "gta", "args": ak}}
    torch.manual_seed(0)
    om = O.OracleTransformer(64, 2, 6, 64, 128, 0.0, True, None, False, args).double()
    tr = gta_amd.Transformer(64, 2, 6, 64, 128, 0.0, True, None, False, args)
    tr.load_state_dict({k_: v_.float() for k_, v_ in om.state_dict().items()}, strict=True)
    tr = tr.cuda()
    tr.fused_blocks = fused_blocks
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 600, 64, generator=g, dtype=torch.float64)
    w = torch.randn(1, 600, 64, generator=g, dtype=torch.float64)
    E = ex["input_transforms"].clone().requires_grad_()
    c = ex["input_coord"].clone().requires_grad_()
    (om(x, None, O.encoder_reps(ak, {"input_transforms": E, "input_coord": c})) * w).sum().backward()
    Eh, ch = E.detach().float().cuda().requires_grad_(), c.detach().float().cuda().requires_grad_()
    exh = {"input_transforms": Eh, "input_coord": ch}
    gta_amd.pre_compute_reps_encoder(ak, exh)
    (tr(x.float().cuda(), None, exh) * w.float().cuda()).sum().backward()
    _check(Eh.grad, E.grad, "d input_transforms")
    _check(ch.grad, c.grad, "d input_coord")


def test_no_table_gradient_leaves_the_route_unchanged(monkeypatch):
    """With no table requiring grad the new entry is never called: forward and backward of the MSN and CLEVR-TR layouts."""
    def boom(*a, **k):
        raise AssertionError("gta_rep_grad_sums called without a table that requires grad")
    monkeypatch.setattr(native, "rep_grad_sums", boom)
    for name in ("ms-dec", "cl-enc"):
        ak, ex, qkv, w, cross = _shape_inputs(name)
        q, k, v = (t.to(torch.bfloat16).cuda().requires_grad_() for t in qkv)
        exh = {k_: v_.float().cuda() for k_, v_ in ex.items()}
        gta_amd.pre_compute_reps_encoder(ak, exh)
        if cross:
            gta_amd.pre_compute_reps_decoder(ak, exh)
        packed = gta_amd.pack_reps(exh, ak["f_dims"])
        tc = torch.tensor([0.3], device="cuda", requires_grad=True)
        out = gta_amd.gta_attention(q, k, v, ak["f_dims"], packed, so3_degree=exh.get("gta_so3_degree", 0), trans_coeff=tc)
        (out.float() * w.float().cuda()).sum().backward()
        torch.cuda.synchronize()
        assert q.grad is not None and tc.grad is not None


LEAVES = ("input_transforms", "target_transforms", "input_coord", "target_coord")
# Through a whole model the pose gradient also carries the error of every upstream activation gradient.  In the fp32-faithful mode that
# error is gone and the gradients must meet the operator's 1e-4 bar.  In the default arithmetic and under autocast it is the bf16 rounding of
# each layer's operands; the coordinates' gradient (a per-token torque summed over a few heads) shows it unaveraged.  There the bar is the
# operator's plus three times the ORACLE's own sensitivity to bf16-size perturbations of the weights and images -- the rule
# test_gpu_backward.py applies to d trans_coeff (_dtc_sensitivity).


def _oracle_srt_grads(cfg, params, d, noise=None):
    """fp64 OracleSRT: d (rendering loss) / d (poses, coordinates); ``noise`` a generator: weights and images scaled by (1 + u 2^-8),
    u uniform in [-1/2, 1/2) (bf16-size relative perturbations)"""
    jig = (lambda t: t * (1 + (torch.rand(t.shape, generator=noise, dtype=torch.float64) - 0.5) * 2.0 ** -8)) if noise else (lambda t: t)
    om = O.OracleSRT(cfg)
    om.load_state_dict(params, strict=True)
    om = om.double()
    with torch.no_grad():
        for p in om.parameters():
            p.copy_(jig(p))
    ref = {n: torch.from_numpy(d["extras." + n]).double().requires_grad_() for n in LEAVES}
    pred = om(jig(torch.from_numpy(d["images"]).double()), None, None, None, torch.from_numpy(d["rays_t"]).double(), dict(ref))
    target = torch.from_numpy(d["target"]).double().flatten(1, 2)
    ((pred.reshape(target.shape) - target) ** 2).mean((1, 2)).sum().backward()
    return {n: ref[n].grad for n in LEAVES}


def _srt_pose_grads(fixture, mode):
    """d loss / d (poses, coordinates) of the whole TransformingSRT (srt.compute_loss) under the fixture's reference weights, and the same
    through OracleSRT in fp64.  input_transforms reach the loss through the encoder's shared q / k table and every decoder layer's k side,
    target_transforms through the decoder's q side."""
    import ast
    import numpy as np
    from gta_amd import layers, srt
    d, _ = G.load(fixture)
    cfg = ast.literal_eval(str(np.load(G.GOLDEN + f"/{fixture}.npz")["meta"]))
    params = {k_[len("param."):]: torch.from_numpy(v_).float() for k_, v_ in d.items() if k_.startswith("param.")}
    model = srt.TransformingSRT(cfg)
    model.load_state_dict(params, strict=True)
    model = model.cuda()
    for m in model.modules():
        if isinstance(m, layers.Attention):
            m.precise = mode == "precise"
    t = lambda n: torch.from_numpy(d[n]).float().cuda()
    data = {"input_images": t("images"), "input_camera_pos": t("cam_in"), "input_rays": t("rays_in"), "target_camera_pos": t("cam_t"),
            "target_rays": t("rays_t"), "target_pixels": t("target")}
    got = {n: t("extras." + n).requires_grad_() for n in LEAVES}
    data.update(got)
    loss, _ = srt.compute_loss(model, data, mixed_prec=mode == "mixed")
    loss.sum().backward()
    torch.cuda.synchronize()
    ref = _oracle_srt_grads(cfg, params, d)
    sens = {n: (0.0, 0.0) for n in LEAVES}                   # (max |change|, rms change / rms ref) of the oracle's gradient
    if mode != "precise" and fixture != "srt_ms_tiny":
        # (on the 10-ray fixture one LeakyReLU sign flip in the render MLP moves everything upstream -- test_gpu_modules.py,
        # test_srt_model_matches_reference: its sensitivity would make the bar vacuous, so it keeps the operator's bar)
        g = torch.Generator().manual_seed(1)
        for _ in range(3):
            alt = _oracle_srt_grads(cfg, params, d, noise=g)
            for n in LEAVES:
                st = C.err_stats(alt[n], ref[n])
                sens[n] = (max(sens[n][0], st["max_abs"]), max(sens[n][1], st["rel_rms"]))
    return {n: got[n].grad for n in LEAVES}, ref, sens


@pytest.mark.parametrize("fixture,mode", [("srt_ms_tiny", "fp32"), ("srt_ms_rays", "fp32"), ("srt_cl_rays", "fp32"),
                                          ("srt_ms_rays", "mixed"), ("srt_cl_rays", "precise")])
def test_srt_pose_and_coordinate_gradients_vs_oracle_srt(fixture, mode):
    """Pose refinement through a trained model: the gradients of the rendering loss w.r.t. both extrinsics and both coordinate sets,
    fp32 (default arithmetic: bf16 products), bf16 autocast (the reference's mixed_prec: True) and the fp32-faithful mode."""
    got, ref, sens = _srt_pose_grads(fixture, mode)
    for n in LEAVES:
        assert got[n] is not None and ref[n] is not None, n
        st = C.err_stats(got[n], ref[n])
        print(fixture, mode, n, {k_: (round(v_, 8) if isinstance(v_, float) else v_) for k_, v_ in st.items()}, "sensitivity", sens[n])
        assert st["finite"], (n, st)
        if mode == "precise":
            assert st["max_abs"] <= 1e-4 * st["ref_max"] + 1e-9, (n, st)
        else:
            assert st["max_abs"] <= REL_MAX * st["ref_max"] + 3.0 * sens[n][0], (n, st, sens[n])
            assert st["rel_rms"] <= REL_RMS + 3.0 * sens[n][1], (n, st, sens[n])


@pytest.mark.parametrize("option", ["zeroout_so3", "id_so3"])
def test_so3_override_keeps_pose_gradients(option):
    """encoder.py:250-258: the so3 knobs write the builder's output in place; under autograd that stays legal and the pose gradient
    is the oracle's (whose D^l are replaced the same way, and detached)."""
    ak, ex, qkv, w, cross = _shape_inputs("ms-dec")
    ak = dict(ak, **{option: True})
    ref = _oracle_grads(ak, ex, qkv, w, cross, 0.3, True)
    got = _hip_grads(ak, ex, qkv, w, cross, 0.3, True, torch.float32)
    for key, r in ref.items():
        _check(got[key], r, f"{option} d {key}")

"""GPU: the mask index (`gta_mask_index`, gta_maskidx.hip; `gta_amd.mask_index`; `gta_attention(..., mask_index=)`;
`TransformingSRT(input_mask_index=True)`).

1. The kernel against the torch expressions of `key_index_tensors`, `query_mask_tensors` and `effective_key_mask(unvalidated=True)` on the CPU
   copy of the mask: every output exactly equal.  Row lengths around the wave (64) and the row loop's chunk (256 tokens a trip), the two
   configuration lengths 600 and 1280, and 777 = three full trips and an odd tail of 9; B = 1 and 3.  Every output buffer has 64 guard elements
   behind it and is pre-filled with a sentinel no result can equal.
2. Through the operator at the smallest shape with two key tiles, a masked tail and a dead scene-view on the query side: bit-identical to the
   same call without the record (the same kernels on equal inputs; the backward is bit-reproducible).
3. Through the model: `input_mask_index=True` against False, bit for bit, one launch per forward and no call of the torch index functions."""
import functools

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native
from tests.test_gpu_run_configs import RUNS

CHUNK = 256                                    # tokens per trip of the kernel's row loops (MASKIDX_CHUNK, gta_maskidx.hip)
SIZES = [1, 7, 63, 64, 65, 255, 256, 257, 600, 1280, 3 * CHUNK + 9]
BATCHES = [1, 3]
MASKS = ["all", "dead-row", "only-0", "only-last", "alternating", "bernoulli-0.5", "bernoulli-0.03", "leading-views", "behind-last-full-chunk"]
SIDES = ["key", "key-no-k_live", "query", "both-one-tensor", "both-two-tensors"]
GUARD = 64
SENTINEL = -7                                  # (int32 outputs; the bytes of k_live: 0xAB -- neither is a value the kernel writes)


@functools.lru_cache(maxsize=None)
def _mask(kind, B, T, seed=0):
    """bool [B, T] on the CPU"""
    g = torch.Generator().manual_seed(1000 * T + 10 * B + seed)
    t = torch.arange(T)
    m = torch.zeros(B, T, dtype=torch.bool)
    if kind == "all":
        m[:] = True
    elif kind == "dead-row":                   # a row with no live token (beside ordinary rows where there are more)
        m[:] = torch.rand(B, T, generator=g) < 0.5
        m[0] = False
    elif kind == "only-0":
        m[:, 0] = True
    elif kind == "only-last":
        m[:, T - 1] = True
    elif kind == "alternating":
        for b in range(B):
            m[b] = (t + b) % 2 == 0
    elif kind.startswith("bernoulli"):
        m[:] = torch.rand(B, T, generator=g) < float(kind.split("-")[1])
    elif kind == "leading-views":              # five views a scene where the row allows: the first b + 1 of them
        for b in range(B):
            m[b, :max(1, (b + 1) * T // 5)] = True
    elif kind == "behind-last-full-chunk":     # nothing live in any full trip of the row loop
        start = (T - 1) // CHUNK * CHUNK
        for b in range(B):
            m[b, start + b:] = True
    return m


def test_the_masks_hold_what_they_say():
    """(the fixtures themselves, on the CPU: not a GPU test)"""
    assert SIZES[-1] >= 2 * CHUNK + 1 and SIZES[-1] % CHUNK % 2 == 1
    assert not bool(_mask("dead-row", 3, 600)[0].any()) and bool(_mask("dead-row", 3, 600)[1:].any(1).all())
    assert _mask("only-0", 3, 257).sum(1).tolist() == [1] * 3 and bool(_mask("only-last", 3, 257)[:, 256].all())
    m = _mask("behind-last-full-chunk", 3, 777)
    assert not bool(m[:, :768].any()) and m.sum(1).tolist() == [9, 8, 7]
    assert _mask("leading-views", 3, 600).sum(1).tolist() == [120, 240, 360]
    assert 0 < int(_mask("bernoulli-0.03", 3, 1280).sum()) < 0.06 * 3 * 1280


@functools.lru_cache(maxsize=None)
def _reference(kind, B, T, seed=0):
    """the torch expressions on the CPU mask: (key_idx, key_lens, k_live as bytes, q_lens)"""
    m = _mask(kind, B, T, seed)
    key_idx = torch.sort((~m).to(torch.uint8), dim=1, stable=True).indices.to(torch.int32)          # key_index_tensors
    key_lens = m.sum(1, dtype=torch.int32)
    k_live = G2.effective_key_mask(m, "cpu", unvalidated=True).to(torch.uint8)
    q_lens = G2.query_mask_tensors(m, "cpu")[1]
    return key_idx, key_lens, k_live, q_lens


def _guarded(n, dtype, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("T", SIZES)
def test_kernel_equals_the_torch_expressions(T, B, kind):
    km = _mask(kind, B, T)
    qm_other = _mask("bernoulli-0.5" if kind != "bernoulli-0.5" else "alternating", B, T, seed=1)
    L, p = native.lib(), native._ptr
    for side in SIDES:
        with_key, with_query = side != "query", side in ("query", "both-one-tensor", "both-two-tensors")
        qm = qm_other if side == "both-two-tensors" else km
        qkind = ("bernoulli-0.5" if kind != "bernoulli-0.5" else "alternating", 1) if side == "both-two-tensors" else (kind, 0)
        d_km = km.cuda()
        d_qm = d_km if side == "both-one-tensor" else qm.cuda()
        key_idx, key_lens = _guarded(B * T, torch.int32, SENTINEL), _guarded(B, torch.int32, SENTINEL)
        k_live, q_lens = _guarded(B * T, torch.uint8, 0xAB), _guarded(B, torch.int32, SENTINEL)
        rc = L.gta_mask_index(p(d_km) if with_key else None, B, T if with_key else 0, p(key_idx), p(key_lens),
                              None if side == "key-no-k_live" else p(k_live), p(d_qm) if with_query else None, T if with_query else 0,
                              p(q_lens), native._stream())
        assert rc == 0, (side, L.gta_strerror(rc).decode())
        key_idx, key_lens, k_live, q_lens = (t.cpu() for t in (key_idx, key_lens, k_live, q_lens))
        want_idx, want_lens, want_live, _ = _reference(kind, B, T)
        want_q = _reference(qkind[0], B, T, qkind[1])[3]
        # the guards, and every buffer of a side that was not asked for
        assert bool((key_idx[B * T:] == SENTINEL).all()) and bool((key_lens[B:] == SENTINEL).all()), side
        assert bool((k_live[B * T:] == 0xAB).all()) and bool((q_lens[B:] == SENTINEL).all()), side
        if with_key:
            got = key_idx[:B * T].view(B, T)
            assert bool((got != SENTINEL).all()), side                                                     # every element written
            assert torch.equal(got.sort(1).values, torch.arange(T, dtype=torch.int32).expand(B, T)), side   # every row a permutation
            assert torch.equal(got, want_idx), side
            assert torch.equal(key_lens[:B], want_lens), (side, key_lens[:B], want_lens)
            if side == "key-no-k_live":
                assert bool((k_live == 0xAB).all()), side
            else:
                assert torch.equal(k_live[:B * T].view(B, T), want_live), side
        else:
            assert bool((key_idx == SENTINEL).all()) and bool((key_lens == SENTINEL).all()) and bool((k_live == 0xAB).all()), side
        if with_query:
            assert torch.equal(q_lens[:B], want_q), (side, q_lens[:B], want_q)
        else:
            assert bool((q_lens == SENTINEL).all()), side


@pytest.mark.gpu
def test_the_record_of_mask_index_equals_the_torch_functions():
    """`gta_amd.mask_index` on a CUDA mask and on a CPU mask: the fields are what the three functions return, types and shapes included"""
    dev = torch.device("cuda", torch.cuda.current_device())
    km, qm = _mask("dead-row", 3, 600), _mask("bernoulli-0.03", 3, 600, seed=1)
    d_km, d_qm = km.cuda(), qm.cuda()
    mi = gta_amd.mask_index(d_km, d_qm, device=dev)
    idx, lens = G2.key_index_tensors(d_km, dev)
    q_live, q_lens = G2.query_mask_tensors(d_qm, dev)
    k_live = G2.effective_key_mask(d_km, dev)
    for got, want in ((mi.key_idx, idx), (mi.key_lens, lens), (mi.k_live, k_live), (mi.q_live, q_live), (mi.q_lens, q_lens)):
        assert got.dtype == want.dtype and got.shape == want.shape and got.device == want.device and got.is_contiguous()
        assert torch.equal(got, want)
    assert mi.key_mask is d_km and mi.query_mask is d_qm and mi.q_live is d_qm
    # a CPU key mask is looked at (and uploaded); one tensor for both sides
    with pytest.raises(native.GtaError, match="have no valid key"):
        gta_amd.mask_index(km, device=dev)
    ok = _mask("bernoulli-0.5", 3, 600)
    both = gta_amd.mask_index(ok, ok, device=dev)
    idx, lens = G2.key_index_tensors(ok, dev)
    assert torch.equal(both.key_idx, idx) and torch.equal(both.key_lens, lens) and torch.equal(both.k_live.cpu(), ok)
    assert both.q_live.is_cuda and torch.equal(both.q_live.cpu(), ok) and torch.equal(both.q_lens, G2.query_mask_tensors(ok, dev)[1])


# ---- 2. through the operator -------------------------------------------------------------------------------------------------------------------
OB, OH, ON, OP = 2, 2, 2, 40
OT = ON * OP


@functools.lru_cache(maxsize=None)
def _case():
    """CLEVR-TR layout (se3 32 | so2 32, dh 64), bf16, self-attention over 2 views of 40 tokens: two 64-key tiles, the second with a tail"""
    from gta_amd import synth
    dh, _mixed, enc, _dec = RUNS["clevrtr/gta"]
    g = torch.Generator().manual_seed(11)
    ex = {"input_transforms": synth.random_extrinsics(OB, ON, g), "input_coord": torch.rand(OB, ON, OP, 2, generator=g)}
    q, k, v = (torch.randn(OB, OH, OT, dh, generator=g).bfloat16().cuda() for _ in range(3))
    w = torch.randn(OB, OH, OT, dh, generator=g).bfloat16().cuda()
    km = torch.ones(OB, OT, dtype=torch.bool)
    km[0, OP:] = False                          # one whole view of scene 0: its second tile is all tail
    km[1, 5::9] = False                         # scattered tokens of scene 1
    qm = torch.ones(OB, OT, dtype=torch.bool)
    qm[1, :OP] = False                          # one fully dead scene-view
    qm[0, 3] = False
    return dict(dh=dh, enc=enc, ex=ex, q=q, k=k, v=v, w=w, km=km.cuda(), qm=qm.cuda())


def _operator(mode, record, rep_grad):
    """-> the tensors of one run: mode 'forward' (no_grad: out, lse) or 'backward' (out and the gradients)"""
    c = _case()
    leaves = {n: t.clone().cuda().requires_grad_(rep_grad and mode == "backward") for n, t in c["ex"].items()}
    ex = dict(leaves)
    gta_amd.pre_compute_reps_encoder(c["enc"], ex)
    f_dims = c["enc"]["f_dims"]
    packed = gta_amd.pack_reps(ex, f_dims)
    kw = dict(so3_degree=0, scale=c["dh"] ** -0.5, key_mask=c["km"], query_mask=c["qm"])
    if record is not None:
        kw["mask_index"] = record
    if mode == "forward":
        with torch.no_grad():
            out, lse = gta_amd.gta_attention(c["q"], c["k"], c["v"], f_dims, packed, trans_coeff=torch.tensor([0.01], device="cuda"),
                                             tau=torch.tensor([0.8], device="cuda"), return_lse=True, **kw)
        torch.cuda.synchronize()
        return dict(out=out, lse=lse)
    q, k, v = (c[n].clone().requires_grad_() for n in "qkv")
    tc, ta = torch.tensor([0.01], device="cuda", requires_grad=True), torch.tensor([0.8], device="cuda", requires_grad=True)
    out = gta_amd.gta_attention(q, k, v, f_dims, packed, trans_coeff=tc, tau=ta, key_mask_backward=True,
                                **(dict(key_mask_rep_grad=True) if rep_grad else {}), **kw)
    out.backward(c["w"])
    torch.cuda.synchronize()
    res = dict(out=out.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dtc=tc.grad, dta=ta.grad)
    if rep_grad:
        res.update({"d" + n: t.grad for n, t in leaves.items()})
    return res


@functools.lru_cache(maxsize=None)
def _operator_reference(mode, rep_grad):
    return _operator(mode, None, rep_grad)


def _bits_equal(got, want):
    assert set(got) == set(want)
    for name in want:
        assert got[name] is not None and got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert torch.equal(got[name], want[name]), name
        assert bool(torch.isfinite(got[name].float()).all()), name


@pytest.mark.gpu
def test_operator_is_bit_identical_with_the_record(monkeypatch):
    """forward (out, lse), backward (q, k, v, trans_coeff, tau) and the pose / coordinate gradients, the three runs on ONE record: one launch,
    and no torch index function is called beside it"""
    c = _case()
    want = [_operator_reference("forward", False), _operator_reference("backward", False), _operator_reference("backward", True)]
    assert bool((want[0]["out"][1, :, :OP] == 0).all()) and bool((want[1]["dq"][1, :, :OP] == 0).all())      # (the dead scene-view is one)
    assert bool((want[1]["dk"][0, :, OP:] == 0).all()) and bool(want[1]["dk"][0, :, :OP].any())                # (and the masked view)
    assert bool(want[2]["dinput_transforms"].any()) and bool(want[2]["dinput_coord"].any())
    launches = []
    real = native.mask_index
    monkeypatch.setattr(native, "mask_index", lambda *a: launches.append(1) or real(*a))
    mi = gta_amd.mask_index(c["km"], c["qm"], device=c["q"].device)
    for name in ("key_index_tensors", "query_mask_tensors", "effective_key_mask", "_all_keys_tensors"):
        monkeypatch.setattr(G2, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called beside a mask_index"))
    _bits_equal(_operator("forward", mi, False), want[0])
    _bits_equal(_operator("forward", mi, False), want[0])              # (two consecutive calls on the one record)
    _bits_equal(_operator("backward", mi, False), want[1])
    _bits_equal(_operator("backward", mi, True), want[2])
    assert launches == [1]


# ---- 3. through the model ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model():
    """the whole-model case of tests/test_gpu_query_mask.py (fp32; se3 16 | so2 8 at dh = 24; 3 views of 16 patches)"""
    from gta_amd import srt
    method = {"method": {"name": "gta", "args": {"f_dims": {"triv": 0, "se3": 16, "so2": 8}, "so2": 2, "max_freq_h": 1, "max_freq_w": 1}}}
    cfg = {"encoder": "isrt", "decoder": "isrt",
           "encoder_kwargs": {"dim": 48, "attdim": 48, "num_conv_blocks": 3, "num_att_blocks": 1, "heads": 2, "dropout": 0.0, "emb": False,
                              "attn_args": method},
           "decoder_kwargs": {"dim": 20, "num_att_blocks": 2, "z_dim": 48, "heads": 2, "dropout": 0.0, "emb": "const", "rmlp_dim": 32,
                              "attn_args": method}}
    torch.manual_seed(0)
    model = srt.TransformingSRT(cfg).cuda().eval()
    nb, NV, npix = 2, 3, 40
    data = srt.synthetic_batch(nb, n_in=NV, n_tgt=1, image=32, points_per_view=8, device="cuda", seed=1)
    P = data["input_coord"].shape[2]
    mask = torch.ones(nb, NV, P, dtype=torch.bool, device="cuda")
    mask[0, 2] = False                          # a missing view
    mask[1, 1, 3::4] = False                    # patches to ignore
    g = torch.Generator().manual_seed(3)
    rays = torch.nn.functional.normalize(torch.randn(nb, 1, npix, 3, generator=g), dim=-1).cuda()
    cam = torch.randn(nb, 1, 1, 3, generator=g).cuda().expand(-1, 1, npix, -1)
    coord = torch.from_numpy(G2.make_2dcoord(16, 20)).cuda().flatten(0, 1)[:npix]
    w = torch.randn(nb, npix, 3, generator=g).cuda()
    return model, data, mask, rays, cam, coord, w


def _model_step(**how):
    model, data, mask, rays, cam, coord, w = _model()
    nb, npix = w.shape[:2]
    extras = {"input_transforms": data["input_transforms"], "input_coord": data["input_coord"],
              "target_transforms": data["target_transforms"][:, :1], "target_coord": coord[None, None].expand(nb, 1, -1, -1)}
    model.zero_grad(set_to_none=True)
    # MIOpen's default weight-gradient kernels of the conv stem are not reproducible to the last digit (tests/test_gpu_ddp.py; two runs of
    # the SAME call differ in the five conv weights' gradients and in nothing else): both legs run its deterministic ones, so that every
    # parameter gradient can be held to torch.equal
    with torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        pix, _ = model(data["input_images"], data["input_camera_pos"], data["input_rays"], cam, rays, extras, input_mask=mask,
                       input_mask_backward=True, **how)
        loss = (pix.reshape(nb, npix, 3).float() * w).sum()
        loss.backward()
    torch.cuda.synchronize()
    res = {"pix": pix.detach().clone(), "loss": loss.detach().clone()}
    res.update({"grad." + name: prm.grad.detach().clone() for name, prm in model.named_parameters() if prm.grad is not None})
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("queries", [False, True], ids=["keys", "keys-and-queries"])
def test_model_is_bit_identical_with_one_build_per_forward(monkeypatch, queries):
    want = _model_step(input_mask_queries=queries)
    assert len(want) > 10 and bool(torch.isfinite(want["loss"]))
    launches = []
    real = native.mask_index
    monkeypatch.setattr(native, "mask_index", lambda *a: launches.append(1) or real(*a))
    for name in ("key_index_tensors", "query_mask_tensors", "effective_key_mask", "_all_keys_tensors"):
        monkeypatch.setattr(G2, name, lambda *a, _n=name, **k: pytest.fail(f"{_n} was called under input_mask_index=True"))
    got = _model_step(input_mask_queries=queries, input_mask_index=True)
    assert launches == [1]
    _bits_equal(got, want)

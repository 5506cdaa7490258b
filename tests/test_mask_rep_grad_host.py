"""Host side of pose and coordinate gradients under key and query masks (`gta_attention(..., key_mask_rep_grad=True)`): without the keyword
the old refusal stands word for word; the new refusals name their reasons before anything is launched (these tests run without a GPU, on CPU
tensors); `repgrad.table_grads(masks=)` on the CPU with `native.rep_grad_sums` replaced by a torch fp64 sum; the autograd wiring of
`_FusedAttn` under the masks with carriers, natives replaced; the effective key mask; the keyword's way through `layers.Attention` and `TransformingSRT`."""
from types import SimpleNamespace

import pytest
import torch

import gta_amd
from gta_amd import gta as G2
from gta_amd import native, repgrad
from tests.test_key_mask_bwd_host import B, CL, H, NK, PK, TK, TQ, _cpu_call, _mask

OLD = ("key_mask_backward: no pose / coordinate gradients under a key mask yet (gta_rep_grad_sums_varlen knows prefixes only): detach the rep "
       "tables and poses")


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_without_the_keyword_the_old_refusal_stands_verbatim():
    for kw in ({}, {"key_mask_rep_grad": False}):
        with pytest.raises(native.GtaError) as e:
            _cpu_call(key_mask_backward=True, packed_grad=True, **kw)
        assert str(e.value) == OLD
        with pytest.raises(native.GtaError) as e:
            _cpu_call(key_mask_backward=True, packed_grad=True, query_mask=torch.ones(B, TQ, dtype=torch.bool), **kw)
        assert str(e.value) == OLD


def test_new_refusals_name_their_reasons():
    with pytest.raises(native.GtaError, match="key_mask_rep_grad=True comes with key_mask_backward=True"):
        _cpu_call(key_mask_rep_grad=True, packed_grad=True)
    with torch.no_grad(), pytest.raises(native.GtaError, match="key_mask_rep_grad=True comes with key_mask_backward=True"):
        _cpu_call(key_mask_rep_grad=True)
    with pytest.raises(native.GtaError, match="key_mask_rep_grad=True comes with key_mask_backward=True"):
        _cpu_call(mask=False, key_mask_rep_grad=True)
    # carriers that are not CUDA tensors: before any launch, in the words of the key_views_backward refusal
    with pytest.raises(native.GtaError) as e:
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True, packed_grad=True)
    assert str(e.value) == ("key_mask_rep_grad: the gradients of rep tables or poses come from a GPU pass (gta_rep_grad_sums_masked): "
                            "tables and poses that require grad must be CUDA tensors")
    with pytest.raises(native.GtaError, match="key_mask_rep_grad: .*must be CUDA tensors"):
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True, packed_grad=True, query_mask=torch.ones(B, TQ, dtype=torch.bool))
    # token counts that do not split evenly into views
    q = torch.zeros(B, H, TQ, 64, requires_grad=True)
    k = torch.zeros(B, H, TK, 64)
    packed = {"vrep_q": torch.zeros(B, 4, native.VREP_STRIDE), "vrep_k": torch.zeros(B, 7, native.VREP_STRIDE, requires_grad=True)}
    with pytest.raises(native.GtaError, match=f"key_mask_rep_grad: {TK} key tokens do not split evenly into 7 views"):
        gta_amd.gta_attention(q, k, k, CL, packed, key_mask=_mask(), key_mask_backward=True, key_mask_rep_grad=True)
    packed["vrep_k"] = torch.zeros(B, NK, native.VREP_STRIDE, requires_grad=True)
    with pytest.raises(native.GtaError, match=f"key_mask_rep_grad: {TQ} query tokens do not split evenly into 4 views"):
        gta_amd.gta_attention(q, k, k, CL, packed, key_mask=_mask(), key_mask_backward=True, key_mask_rep_grad=True,
                              query_mask=torch.ones(B, TQ, dtype=torch.bool))
    # everything else the mask route refuses stays refused
    with pytest.raises(native.GtaError, match="return_lse under grad with key_mask_backward"):
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True, return_lse=True)
    with pytest.raises(native.GtaError, match="key_mask has no precise=True"):
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True, precise=True)
    with pytest.raises(native.GtaError, match="no gather pre-pass.*t2"):
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True, f_dims={"se3": 32, "t2": 30, "triv": 2})
    with pytest.raises(native.GtaError, match="key_mask with key_views"):
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True, key_views=[1] * B, key_views_backward=True)
    # without tables that require grad the keyword changes nothing: the call gets as far as the kernels' device check
    with pytest.raises(native.GtaError, match="cpu|CUDA"):
        _cpu_call(key_mask_backward=True, key_mask_rep_grad=True)


# ---- the algebra under device masks ---------------------------------------------------------------------------------------------------------------
B_, H_, N_, P_, NB = 3, 2, 4, 5, 3
T_ = N_ * P_
DH = 8 + 2 * NB                      # se3 8 | so2 6


def _desc():
    return SimpleNamespace(B=B_, H=H_, Tq=T_, Tk=T_, Nq=N_, Nk=N_, d_se3=8, d_so2=2 * NB, d_t2=0)


def _fake_sums(calls):
    """native.rep_grad_sums as a torch fp64 sum: dead rows are not read (they hold NaN), the sums of dead entries are zeros"""
    def sums(desc, side, pairs, view=False, so2=False, t2=False, lens=None, live=None):
        calls.append((side, live, lens))
        S = torch.zeros(B_, N_, 4, 4, dtype=torch.float64)
        T2 = torch.zeros(B_, T_, NB, 2, 2, dtype=torch.float64)
        for a, b in pairs:
            a, b = a.double(), b.double()
            if live is not None:
                assert live.dtype == torch.bool and tuple(live.shape) == (B_, T_)
                a = torch.where(live[:, None, :, None], a, torch.zeros((), dtype=torch.float64))
                b = torch.where(live[:, None, :, None], b, torch.zeros((), dtype=torch.float64))
            av, bv = a[..., :8].reshape(B_, H_, N_, P_, 2, 4), b[..., :8].reshape(B_, H_, N_, P_, 2, 4)
            S += torch.einsum("bhntgi,bhntgj->bnij", av, bv)
            T2 += torch.einsum("bhtgi,bhtgj->btgij", a[..., 8:].unflatten(-1, (NB, 2)), b[..., 8:].unflatten(-1, (NB, 2)))
        return (S.float() if view else None), (T2.float() if so2 else None), None
    return sums


def _tables(g):
    E = torch.eye(4).repeat(B_, N_, 1, 1)
    E[..., :3, :] += 0.3 * torch.randn(B_, N_, 3, 4, generator=g)
    vrep = torch.zeros(B_, N_, native.VREP_STRIDE)
    vrep[..., repgrad.INV] = torch.linalg.inv(E.double()).float().flatten(-2)
    vrep[..., repgrad.REP] = E.flatten(-2)
    th = torch.rand(B_, T_, NB, generator=g, dtype=torch.float64) * 6.28
    return vrep, torch.stack([torch.cos(th), torch.sin(th)], -1).float()


def _masks(g):
    m = torch.rand(B_, T_, generator=g) < 0.6
    m[0, P_:2 * P_] = False                              # a wholly dead view between live ones
    m[0, 0] = m[0, 2 * P_] = True
    m[1] = False                                         # a scene without a live token
    m[2] = True                                          # a scene with all of them
    return m


@pytest.mark.parametrize("fill", ["singular", float("nan"), float("inf")], ids=str)
def test_table_grads_under_masks_on_the_cpu(monkeypatch, fill):
    calls = []
    monkeypatch.setattr(native, "rep_grad_sums", _fake_sums(calls))
    g = torch.Generator().manual_seed(11)
    vrep, cs = _tables(g)
    qm, km = _masks(g), _masks(g)
    ops = [torch.randn(B_, H_, T_, DH, generator=g) for _ in range(8)]
    meta = (((B_, N_, native.VREP_STRIDE), torch.float32),) * 2 + (((B_, T_, NB, 2), torch.float32),) * 2 + (None, None)
    poisoned = {}
    for side, m in ((0, qm), (1, km)):                   # what dead entries hold: anything
        dead_v = ~m.view(B_, N_, P_).any(-1)
        assert bool(dead_v.any()) and bool((~dead_v).any())
        v = vrep.clone()
        v[dead_v] = 0.0 if fill == "singular" else fill
        c = cs.clone()
        c[~m] = 0.0 if fill == "singular" else fill
        poisoned[side] = (v, c)
    nan_ops = [torch.where((qm if i < 4 else km)[:, None, :, None], x, torch.full((), float("nan"))) for i, x in enumerate(ops)]
    zero_ops = [torch.where((qm if i < 4 else km)[:, None, :, None], x, torch.zeros(())) for i, x in enumerate(ops)]
    pairs = lambda o: (((o[0], o[1]), (o[2], o[3])), ((o[4], o[5]), (o[6], o[7])))
    tables = dict(vrep_q=poisoned[0][0], vrep_k=poisoned[1][0], cs_q=poisoned[0][1], cs_k=poisoned[1][1])
    got = repgrad.table_grads(_desc(), tables, meta, 0.3, *pairs(nan_ops), direct=False, masks=(qm, km))
    assert [c[0] for c in calls] == [0, 1] and calls[0][1] is qm and calls[1][1] is km and calls[0][2] is None
    # the unmasked algebra on the zeroed operands and the clean tables
    calls.clear()
    ref = repgrad.table_grads(_desc(), dict(vrep_q=vrep, vrep_k=vrep, cs_q=cs, cs_k=cs), meta, 0.3, *pairs(zero_ops), direct=False)
    assert all(c[1] is None for c in calls)
    for side, m in ((0, qm), (1, km)):
        live_v = m.view(B_, N_, P_).any(-1)
        gv, gc = got[side], got[2 + side]
        assert gv.shape == (B_, N_, native.VREP_STRIDE) and gc.shape == (B_, T_, NB, 2)
        assert bool(torch.isfinite(gv).all()) and bool(torch.isfinite(gc).all()), (side, fill)
        assert torch.count_nonzero(gv[~live_v]) == 0 and torch.count_nonzero(gc[~m]) == 0, (side, fill)
        assert torch.equal(gv[live_v], ref[side][live_v]) and bool(gv[live_v].abs().max() > 0), (side, fill)
        assert torch.equal(gc[m], ref[2 + side][m]) and bool(gc[m].abs().max() > 0), (side, fill)
    assert got[4] is None and got[5] is None
    # one side masked, the other not (a decoder leg, or self-attention without query_mask)
    calls.clear()
    half = repgrad.table_grads(_desc(), dict(tables, vrep_q=vrep, cs_q=cs), meta, 0.3, pairs(zero_ops)[0], pairs(nan_ops)[1], direct=False,
                               masks=(None, km))
    assert calls[0][1] is None and calls[1][1] is km
    assert torch.equal(half[0], ref[0]) and torch.equal(half[1], got[1]) and torch.equal(half[3], got[3])


def test_table_grads_refuses_by_name():
    m = torch.ones(B_, T_, dtype=torch.bool)
    meta = (((B_, N_, native.VREP_STRIDE), torch.float32),) * 2 + (None,) * 4
    z = torch.zeros(B_, H_, T_, DH)
    pairs = ((z, z),)
    tables = dict(vrep_q=torch.zeros(B_, N_, 72), vrep_k=torch.zeros(B_, N_, 72))
    with pytest.raises(native.GtaError, match="views= and masks= on the same side"):
        repgrad.table_grads(_desc(), tables, meta, 0.3, pairs, pairs, direct=False, views=((1,) * B_, None), lens=(torch.zeros(B_), None),
                            masks=(m, None))
    with pytest.raises(native.GtaError, match="masks= does not serve euclid"):
        repgrad.table_grads(_desc(), tables, meta, 0.3, pairs, pairs, direct=False, euclid=True, masks=(None, m))
    with pytest.raises(native.GtaError, match="masks= does not serve direct sums"):
        repgrad.table_grads(_desc(), tables, meta, 0.3, pairs, pairs, direct=True, masks=(None, m))
    d = _desc()
    d.Nk = 3
    with pytest.raises(native.GtaError, match="T % N != 0"):
        repgrad.table_grads(d, tables, meta, 0.3, pairs, pairs, direct=False, masks=(None, m))
    with pytest.raises(native.GtaError, match=r"masks\[1\] is a bool \[B, T\]"):
        repgrad.table_grads(_desc(), tables, meta, 0.3, pairs, pairs, direct=False, masks=(None, m.to(torch.uint8)))


# ---- the effective key mask -------------------------------------------------------------------------------------------------------------------------
def test_effective_key_mask():
    m = torch.zeros(4, 6, dtype=torch.bool)
    m[0] = True
    m[1, 3] = True
    m[3, 0] = True                                       # scene 2: no valid key
    eff = G2.effective_key_mask(m, "cpu", unvalidated=True)           # a CUDA-style mask: its values were not looked at
    assert eff.dtype == torch.bool and eff.is_contiguous() and eff is not m
    want = m.clone()
    want[2, 0] = True                                    # ... attends its token 0 (the kernels clamp the count to 1): live for the sums too
    assert torch.equal(eff, want) and not bool(m[2].any())            # (the caller's mask is not written)
    idx, lens = G2.key_index_tensors(want, "cpu")
    assert int(idx[2, 0]) == 0 and int(lens[2]) == 1
    # a CPU mask is validated to have a valid key per scene and is used as it is
    ok = m.clone()
    ok[2, 4] = True
    assert torch.equal(G2.effective_key_mask(ok, "cpu"), ok)


# ---- autograd wiring --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_query_mask", [False, True])
def test_autograd_wiring(monkeypatch, with_query_mask):
    """`_FusedAttn` under the masks with carriers, the native calls and `table_grads` replaced: the backward hands table_grads the pairs (q, dq), (dout, out)
    and (dk, k), (dv, v), direct=False and masks=(q_live, k_live) -- the objects the forward was given --, and its six results come back as the
    carriers' gradients beside the five others"""
    seen = {}

    def fwd(desc, q, k, v, vq, vk, cq, ck, tc, ta, key_idx, key_lens, *rest):
        seen["fwd"] = rest[-1]
        rest[-3].zero_()

    def bwd(desc, q, k, v, out, dout, lse, vq, vk, cq, ck, tc, ta, key_idx, key_lens, *rest):
        dq, dk, dv, dtc, _, dta = rest[-6:]                 # (..., kv_images, dq, dk, dv, dtc, ws, dta)
        seen["bwd"] = (dq, dk, dv, rest[:-7])
        for t, val in ((dq, 1.0), (dk, 2.0), (dv, 3.0), (dtc, 4.0), (dta, 5.0)):
            t.fill_(val)

    def grads(desc, tables, meta, tc, q_pairs, k_pairs, direct, **kw):
        seen["tg"] = (desc, tables, meta, q_pairs, k_pairs, direct, kw)
        return [None if m is None else torch.full(m[0], 6.0 + i, dtype=m[1]) for i, m in enumerate(meta)]

    for name in ("attn_fwd_gather", "attn_fwd_qmask"):
        monkeypatch.setattr(native, name, fwd)
    for name in ("attn_bwd_gather", "attn_bwd_qmask"):
        monkeypatch.setattr(native, name, bwd)
    monkeypatch.setattr(G2, "_check_tables", lambda *a, **k: None)
    monkeypatch.setattr(G2._repgrad, "table_grads", grads)
    q, k, v = (torch.zeros(B, H, T, 64, requires_grad=True) for T in (TQ, TK, TK))
    tc, ta = torch.tensor([0.5], requires_grad=True), torch.tensor([0.8], requires_grad=True)
    vrep_q, vrep_k = torch.zeros(B, 1, native.VREP_STRIDE, requires_grad=True), torch.zeros(B, NK, native.VREP_STRIDE, requires_grad=True)
    cs_q, cs_k = torch.zeros(B, TQ, 16), torch.zeros(B, TK, 16, requires_grad=True)
    packed, carriers = repgrad.split_tables(dict(vrep_q=vrep_q, vrep_k=vrep_k, cs_q=cs_q, cs_k=cs_k))
    assert len(carriers) == 6 and carriers[2] is None and carriers[0] is vrep_q and not packed["vrep_k"].requires_grad
    km = _mask()
    key_idx, key_lens = G2.key_index_tensors(km, "cpu")
    k_live = G2.effective_key_mask(km, "cpu")
    q_live, q_lens = G2.query_mask_tensors(torch.ones(B, TQ, dtype=torch.bool), "cpu") if with_query_mask else (None, None)
    flags = G2.attention_route((B, H, TQ, 64), TK, torch.float32, CL, 0, 1, NK, key_mask=True, needs_grad=True, key_mask_backward=True)
    cfg = (dict(CL), 0, 1, NK, 0.125, flags)
    mask = G2._Mask("gather", key_idx=key_idx, key_lens=key_lens, q_live=q_live, q_lens=q_lens, k_live=k_live)
    out = G2._FusedAttn.apply(q, k, v, tc, ta, (cfg, None, mask), packed["vrep_q"], packed["vrep_k"], packed["cs_q"], packed["cs_k"], *carriers)
    out.sum().backward()
    desc, tables, meta, q_pairs, k_pairs, direct, kw = seen["tg"]
    assert direct is False and set(kw) == {"masks"} and kw["masks"][0] is q_live and kw["masks"][1] is k_live
    assert (desc.Tq, desc.Tk, desc.Nq, desc.Nk) == (TQ, TK, 1, NK)
    assert tables["vrep_k"] is packed["vrep_k"] and tables["cs_k"] is packed["cs_k"]
    assert [m is not None for m in meta] == [True, True, False, True, False, False]
    dq, dk, dv, _ = seen["bwd"]
    assert len(q_pairs) == 2 and q_pairs[0][1] is dq and q_pairs[0][0].shape == q.shape and q_pairs[1][0].shape == out.shape
    assert len(k_pairs) == 2 and k_pairs[0][0] is dk and k_pairs[1][0] is dv and k_pairs[0][1].shape == k.shape
    for t, val in ((q, 1.0), (k, 2.0), (v, 3.0), (tc, 4.0), (ta, 5.0), (vrep_q, 6.0), (vrep_k, 7.0), (cs_k, 9.0)):
        assert t.grad is not None and t.grad.shape == t.shape and bool((t.grad == val).all()), val
    assert cs_q.grad is None


def _mask_and_carriers(args):
    """of the arguments `_FusedAttn.apply` got: the mask record of its one non-tensor argument (cfg, kv_cache, mask), and the carriers"""
    (cfg, kv_cache, mask), = [a for a in args if isinstance(a, tuple)]
    assert mask.kind == "gather" and kv_cache is None
    return mask, tuple(args[G2._FusedAttn.CARRIERS:])


def test_gta_attention_uploads_the_mask_once_and_hands_it_on(monkeypatch):
    """the public call: k_live is built beside key_idx / key_lens (None for the all-True mask of a query_mask-only call), the carriers go in"""
    got = []
    monkeypatch.setattr(G2._FusedAttn, "apply", staticmethod(lambda *a: got.append(a) or torch.zeros(1)))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))             # (the carriers' device check, nothing else here)
    monkeypatch.setattr(G2, "attention_route", lambda *a, **k: native.FLAG_V_TRANSFORM)
    q = torch.zeros(B, H, TK, 64, requires_grad=True)
    packed = {"vrep_q": torch.zeros(B, NK, native.VREP_STRIDE, requires_grad=True), "vrep_k": torch.zeros(B, NK, native.VREP_STRIDE)}
    km, qm = _mask(), torch.ones(B, TK, dtype=torch.bool)
    real = G2.effective_key_mask
    monkeypatch.setattr(G2, "effective_key_mask", lambda m, dev: real(m, dev, unvalidated=True))
    for kw, want_k, want_q in (({"key_mask": km}, True, False), ({"key_mask": km, "query_mask": qm}, True, True), ({"query_mask": qm}, False, True)):
        got.clear()
        gta_amd.gta_attention(q, q, q, CL, packed, key_mask_backward=True, key_mask_rep_grad=True, **kw)
        mask, carriers = _mask_and_carriers(got[0])
        assert len(carriers) == 6 and carriers[0] is packed["vrep_q"] and carriers[1] is None
        assert (mask.q_live is not None) == want_q and (mask.k_live is not None) == want_k
        if want_k:
            assert torch.equal(mask.k_live, km) and mask.k_live.dtype == torch.bool
    # without tables that require grad nothing is built
    got.clear()
    gta_amd.gta_attention(q, q, q, CL, {k_: v_.detach() for k_, v_ in packed.items()}, key_mask=km, key_mask_backward=True, key_mask_rep_grad=True)
    mask, carriers = _mask_and_carriers(got[0])
    assert carriers == () and mask.k_live is None and mask.q_live is None and mask.q_lens is None


# ---- the keyword's way down ---------------------------------------------------------------------------------------------------------------------------
def test_layers_hand_the_keyword_on(monkeypatch):
    from gta_amd import layers
    args = {"f_dims": CL, "so2": 8, "max_freq_h": 1, "max_freq_w": 1}
    att = layers.Attention(128, heads=2, dim_head=64, attn_args={"method": {"name": "gta", "args": args}})
    seen = []

    def fake(q, k, v, f_dims, packed, **kw):
        seen.append(kw)
        return torch.zeros(q.shape[0], q.shape[2], q.shape[1], q.shape[3]).permute(0, 2, 1, 3)

    monkeypatch.setattr(layers._gta, "gta_attention", fake)
    monkeypatch.setattr(layers._gta, "pack_reps", lambda extras, f_dims: {})
    monkeypatch.setattr(layers._gta, "_so3_degree", lambda *a: 0)
    q = torch.zeros(2, 2, 8, 64)
    m = torch.ones(2, 8, dtype=torch.bool)
    att.core(q, q, q, {"key_mask": m, "key_mask_backward": True, "key_mask_rep_grad": True})
    att.core(q, q, q, {"key_mask": m, "key_mask_backward": True})
    att.core(q, q, q, {})
    assert seen[0]["key_mask_rep_grad"] is True and seen[0]["key_mask_backward"] is True
    assert "key_mask_rep_grad" not in seen[1] and "key_mask_rep_grad" not in seen[2]


def test_srt_sets_the_keyword_in_its_copy_of_extras():
    from gta_amd import srt
    model = srt.TransformingSRT.__new__(srt.TransformingSRT)
    torch.nn.Module.__init__(model)
    seen = {}

    def encoder(images, pos, rays, extras):
        seen["enc"] = dict(extras)
        return torch.zeros(1), extras

    model.encoder = encoder
    model.decode = lambda z, pos, rays, extras=None: seen.setdefault("dec", dict(extras))
    mask = torch.ones(2, 3, 4, dtype=torch.bool)
    mine = {"input_transforms": torch.zeros(1)}
    model.forward(None, None, None, None, None, mine, input_mask=mask, input_mask_backward=True, input_mask_rep_grad=True, input_mask_queries=True)
    assert seen["enc"]["key_mask_rep_grad"] is True and seen["enc"]["key_mask_backward"] is True and "query_mask" in seen["enc"]
    assert seen["dec"]["key_mask_rep_grad"] is True and "query_mask" not in seen["dec"]
    assert "key_mask_rep_grad" not in mine and "key_mask" not in mine
    seen.clear()
    model.forward(None, None, None, None, None, mine, input_mask=mask, input_mask_backward=True)
    assert "key_mask_rep_grad" not in seen["enc"] and "key_mask_rep_grad" not in seen["dec"]
    for kw in (dict(input_mask=mask), dict(), dict(input_mask=mask, input_mask_queries=True)):
        with pytest.raises(native.GtaError, match="input_mask_rep_grad=True comes with input_mask_backward=True"):
            model.forward(None, None, None, None, None, mine, input_mask_rep_grad=True, **kw)

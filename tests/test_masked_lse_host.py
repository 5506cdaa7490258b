"""Host: the lse gradient under key_views, key_mask and query_mask (`masked_lse_backward`; `gta_attn_bwd_varlen_dlse`, `gta_attn_bwd_gather_dlse`,
`gta_attn_bwd_qmask_dlse`) -- the six ABI symbols, the refusals that stay what they were without the opt-in, and the routes under the opt-in,
on CPU tensors with the spies of tests/_call_routes.py, extended by spies of the same kind on the three new entries (no launch, no GPU)."""
import contextlib
import ctypes
import inspect
import os
import re

import pytest
import torch

import gta_amd
from gta_amd import backward as BW
from gta_amd import gta as G
from gta_amd import native
from tests import _call_routes as R

HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gta_hip.h")).read()
BASES = ("gta_attn_bwd_varlen", "gta_attn_bwd_gather", "gta_attn_bwd_qmask")
F_DIMS = R.LAYOUTS["fused"]["f_dims"]


def _decl(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    L = native.lib()
    for base in BASES:
        for s in (base + "_dlse", base + "_dlse_supported"):
            assert s in native.ABI_SYMBOLS and hasattr(L, s), s
            assert len(getattr(L, s).argtypes) == len(_decl(s)), s
        # the base entry's arguments with `const float* dlse` behind lse
        args, ref = _decl(base + "_dlse"), _decl(base)
        i = [a.split()[-1] for a in args].index("dlse")
        assert args[i] == "const float* dlse" and args[i - 1].split()[-1] == "lse" and args[:i] + args[i + 1:] == ref, base
        at = getattr(L, base + "_dlse").argtypes
        assert getattr(L, base).argtypes == at[:i] + at[i + 1:] and at[i] == ctypes.c_void_p, base
        assert _decl(base + "_dlse_supported") == ["const GtaAttnDesc* desc"]
    assert native.GTA_ABI_VERSION == 2 and L.gta_abi_version() == 2


def test_supported_queries_answer_like_their_base_entries():
    def desc(f_dims, flags, dh=64, dtype=torch.bfloat16):
        qs = (2 * 32 * dh, 32 * dh, dh)
        return native.make_desc_from(dtype, (1, 2, 32, dh), 32, (qs, qs, qs, qs), f_dims, 0, 1, 1, 1.0, flags)
    cl = {"se3": 32, "so2": 32}
    descs = [desc(cl, native.FLAG_V_TRANSFORM), desc(cl, native.FLAG_V_TRANSFORM, dtype=torch.float32),
             desc(cl, native.FLAG_V_TRANSFORM | native.FLAG_FP32_PRODUCTS, dtype=torch.float32),
             desc(cl, native.FLAG_V_TRANSFORM | native.FLAG_PRETRANSFORMED), desc(cl, native.FLAG_V_TRANSFORM | native.FLAG_FUSED_KV),
             desc({"se3": 32, "t2": 30, "triv": 2}, native.FLAG_V_TRANSFORM)]
    for kind in ("varlen", "gather", "qmask"):
        base, twin = getattr(native, f"attn_bwd_{kind}_supported"), getattr(native, f"attn_bwd_{kind}_dlse_supported")
        answers = [base(d) for d in descs]
        assert answers == [twin(d) for d in descs], kind
        assert answers[0] == 0 and answers[1] == 0 and all(a != 0 for a in answers[2:]), (kind, answers)


def test_null_dlse_is_badarg_before_any_launch():
    """every other pointer is a non-null dummy: the entry answers before it touches one"""
    L = native.lib()
    dh = 64
    qs = (2 * 32 * dh, 32 * dh, dh)
    desc = native.make_desc_from(torch.bfloat16, (1, 2, 32, dh), 32, (qs, qs, qs, qs), {"se3": 32, "so2": 32}, 0, 1, 1, 1.0, native.FLAG_V_TRANSFORM)
    p = ctypes.c_void_p(256)
    st9, st3 = (ctypes.c_int64 * 9)(*(qs * 3)), (ctypes.c_int64 * 3)(*qs)
    for base, n_lens in (("gta_attn_bwd_varlen", 2), ("gta_attn_bwd_gather", 2), ("gta_attn_bwd_qmask", 4)):
        head = [ctypes.byref(desc)] + [p] * 6                     # q, k, v, out, dout, lse
        tail = [p] * 6 + [p] * n_lens + [p] * 4 + [st9, st3, p, p, p, 1 << 40, None]
        rc = getattr(L, base + "_dlse")(*head, None, *tail)
        assert rc == -1 and "null dlse" in L.gta_strerror(rc).decode(), base


# ---- the spies -------------------------------------------------------------------------------------------------------------------------------
NEW = ("attn_bwd_varlen_dlse", "attn_bwd_gather_dlse", "attn_bwd_qmask_dlse")


def test_the_new_entries_are_served_by_name_and_stay_out_of_the_recorded_entry_list():
    """tests/_call_routes.py holds its frozen record against every ``attn_bwd*`` name of ``dir(native)``; the three are reached by name"""
    for name in NEW:
        assert callable(getattr(native, name)) and name not in dir(native) and name not in R.ENTRIES
    with pytest.raises(AttributeError):
        native.attn_bwd_nothing_dlse


@contextlib.contextmanager
def _spies(log):
    """``R.spies`` plus spies of the same kind on the three new entries (notes in its format: name, flags, views, the optional operands)"""
    def spy_of(name):
        sig = inspect.signature(getattr(native, name))

        def spy(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            args = args.arguments
            desc = args["desc"]
            log.append(f"{name} flags={desc.flags:#x} Nq={desc.Nq} Nk={desc.Nk} ops=" + ",".join(o for o in R.OPERANDS if args.get(o) is not None))
            for out, val in R.FILL.items():
                if torch.is_tensor(args.get(out)):
                    args[out].fill_(val)
        return spy
    with R.spies(log):
        for name in NEW:
            setattr(native, name, spy_of(name))
        try:
            yield
        finally:
            for name in NEW:
                delattr(native, name)


def _record(kw, grad=True, tables_grad=False, cuda_carriers=False):
    """`R.record` of a fused-layout call under `_spies`: calls, returns, outputs_with_grad, grads -- or raises"""
    leaves, packed = R.inputs(F_DIMS, tables_grad=tables_grad)
    log, rec = [], {}
    with _spies(log), (contextlib.nullcontext() if grad else torch.no_grad()):
        if cuda_carriers:
            torch.Tensor.is_cuda = property(lambda self: True)
        try:
            ret = gta_amd.gta_attention(leaves["q"], leaves["k"], leaves["v"], F_DIMS, packed, trans_coeff=leaves["trans_coeff"], tau=leaves["tau"], **kw)
            rec["returns"] = "pair" if isinstance(ret, tuple) else "tensor"
            outs = ret if isinstance(ret, tuple) else (ret,)
            if any(o.requires_grad for o in outs):
                sum(o.sum() for o in outs if o.requires_grad).backward()
                rec["outputs_with_grad"] = sum(o.requires_grad for o in outs)
        except Exception as e:  # noqa: BLE001 -- the exception is the record
            rec["raises"] = f"{type(e).__name__}: {e}"
        finally:
            if cuda_carriers:
                del torch.Tensor.is_cuda
    rec["calls"] = log
    rec["grads"] = " ".join(f"{n}{list(t.grad.shape)}" for n, t in leaves.items() if t.grad is not None)
    return rec


# ---- defaults unchanged -----------------------------------------------------------------------------------------------------------------------
def _attend(kw, grad=True, **how):
    leaves, packed = R.inputs(F_DIMS, **how)
    with _spies([]), (contextlib.nullcontext() if grad else torch.no_grad()):
        return gta_amd.gta_attention(leaves["q"], leaves["k"], leaves["v"], F_DIMS, packed, trans_coeff=leaves["trans_coeff"], tau=leaves["tau"], **kw)


VIEWS = dict(key_views=[1, R.NK], key_views_backward=True)
VIEWS_Q = dict(key_views=[1, R.NK], query_views=[1, 1], key_views_backward=True)
GATHER = dict(key_mask_backward=True)        # (+ key_mask / query_mask: fresh tensors per call, below)


def _masks(kind):
    kw = {}
    if "key_mask" in kind:
        kw["key_mask"] = R.key_mask()
    if "query_mask" in kind:
        kw["query_mask"] = R.query_mask()
    return dict(kw, **(GATHER if kw else {}))


def test_without_the_opt_in_the_refusals_are_what_they_were():
    with pytest.raises(native.GtaError, match=r"return_lse under grad with key_views_backward: gta_attn_bwd_varlen takes no gradient of the log-sum-exp "
                                              r"\(drop return_lse, or call under torch.no_grad\(\)\)"):
        _attend(dict(VIEWS, return_lse=True))
    with pytest.raises(native.GtaError, match="return_lse under grad with key_views_backward"):
        _attend(dict(VIEWS_Q, return_lse=True))
    for kind in ("key_mask", "query_mask", "key_mask+query_mask"):
        with pytest.raises(native.GtaError, match=r"return_lse under grad with key_mask_backward: gta_attn_bwd_gather takes no gradient of the log-sum-exp "
                                                  r"\(drop return_lse, or call under torch.no_grad\(\)\)"):
            _attend(dict(_masks(kind), return_lse=True))
        with pytest.raises(native.GtaError, match="return_lse under grad with key_mask_backward"):
            _attend(dict(_masks(kind), return_lse=True, masked_lse_backward=False))


def test_the_opt_in_alone_is_refused():
    for kw in (dict(), dict(return_lse=True), dict(key_views=[1, R.NK]), dict(key_mask=R.key_mask()), dict(query_mask=R.query_mask())):
        for grad in (False, True):
            with pytest.raises(native.GtaError, match="masked_lse_backward=True comes with key_views_backward=True or key_mask_backward=True"):
                _attend(dict(kw, masked_lse_backward=True), grad=grad)


def test_the_opt_in_lifts_nothing_else():
    on = dict(return_lse=True, masked_lse_backward=True)
    for name, mask in (("key_views", VIEWS), ("key_mask", _masks("key_mask")), ("key_mask", _masks("key_mask+query_mask"))):
        with pytest.raises(native.GtaError, match=f"{name} has no precise=True"):
            _attend(dict(mask, precise=True, **on))
        with pytest.raises(native.GtaError, match=f"{name} with pretransformed=True"):
            _attend(dict(mask, pretransformed=True, **on))
        with pytest.raises(native.GtaError, match=f"{name} runs the two-stage plan: kv_mode='fused'"):
            _attend(dict(mask, kv_mode="fused", **on))
        with pytest.raises(native.GtaError, match="kv_cache is an inference feature" if "query_mask" not in mask else "query_mask with kv_cache"):
            _attend(dict(mask, kv_cache={}, **on))
    staged = R.LAYOUTS["staged"]["f_dims"]
    leaves, packed = R.inputs(staged)
    for mask, words in ((VIEWS, "key_views"), (_masks("key_mask"), "key_mask")):
        with _spies([]), pytest.raises(native.GtaError, match=words):
            gta_amd.gta_attention(leaves["q"], leaves["k"], leaves["v"], staged, packed, trans_coeff=leaves["trans_coeff"], **mask, **on)
    assert "masked_lse_backward" not in G.MASK_OPT_INS and "masked_lse_backward" not in G.MASK_KEYWORDS


def test_without_return_lse_or_without_grad_the_flag_changes_no_call():
    for mask in (lambda: VIEWS, lambda: VIEWS_Q, lambda: _masks("key_mask"), lambda: _masks("query_mask"), lambda: _masks("key_mask+query_mask")):
        for extra, grad in ((dict(), True), (dict(), False), (dict(return_lse=True), False)):
            a = _record(dict(mask(), **extra), grad=grad)
            b = _record(dict(mask(), masked_lse_backward=True, **extra), grad=grad)
            assert a == b and "raises" not in a, (a, b)
            assert not any("_dlse" in n for n in a["calls"])


# ---- routes -----------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _watch():
    """counts the applications of the two autograd Functions and notes what backward.attn_bwd is handed"""
    seen = dict(lse=0, plain=0, bwd=[])
    lse_apply, plain_apply, attn_bwd = G._FusedAttnLse.apply, G._FusedAttn.apply, BW.attn_bwd

    def wrap(name, fn):
        def f(*a, **kw):
            seen[name] += 1
            return fn(*a, **kw)
        return f

    def bwd(*a, **kw):
        seen["bwd"].append(kw)
        return attn_bwd(*a, **kw)
    G._FusedAttnLse.apply, G._FusedAttn.apply, BW.attn_bwd = wrap("lse", lse_apply), wrap("plain", plain_apply), bwd
    try:
        yield seen
    finally:
        G._FusedAttnLse.apply, G._FusedAttn.apply, BW.attn_bwd = lse_apply, plain_apply, attn_bwd


ROUTES = [("views", lambda: VIEWS, "varlen", ("key_lens",)),
          ("views+query_views", lambda: VIEWS_Q, "varlen", ("key_lens", "q_lens")),
          ("gather", lambda: _masks("key_mask"), "gather", ("key_idx", "key_lens")),
          ("gather+query_mask", lambda: _masks("key_mask+query_mask"), "qmask", ("key_idx", "key_lens", "q_live", "q_lens")),
          ("query_mask", lambda: _masks("query_mask"), "qmask", ("key_idx", "key_lens", "q_live", "q_lens"))]


@pytest.mark.parametrize("name,mask,entry,tensors", ROUTES, ids=[r[0] for r in ROUTES])
def test_routes_under_the_opt_in(name, mask, entry, tensors):
    with _watch() as seen:
        rec = _record(dict(mask(), return_lse=True, masked_lse_backward=True))
    assert "raises" not in rec, rec
    assert rec["returns"] == "pair" and rec["outputs_with_grad"] == 2
    assert seen["lse"] == 1 and seen["plain"] == 0
    (kw,) = seen["bwd"]                                    # one backward, with the mask's tensors and a dlse
    assert torch.is_tensor(kw["dlse"]) and tuple(kw["dlse"].shape) == (R.B, R.H, R.TQ)
    for t in ("key_lens", "q_lens", "key_idx", "q_live"):
        assert (kw[t] is not None) == (t in tensors), (name, t)
    fwd = {"varlen": "attn_fwd_varlen", "gather": "attn_fwd_gather", "qmask": "attn_fwd_qmask"}[entry]
    calls = [c.split()[0] for c in rec["calls"]]
    assert calls == [fwd, f"attn_bwd_{entry}_dlse"], rec["calls"]
    ops = re.search(r"ops=(\S*)", rec["calls"][1]).group(1).split(",")
    assert "dlse" in ops and "kv_images" in ops and all(t in ops for t in tensors), rec["calls"]
    assert kw["kv_images"] is not None                       # the forward's images serve the backward
    assert rec["grads"] == "q[2, 2, 8, 64] k[2, 2, 72, 64] v[2, 2, 72, 64] trans_coeff[1] tau[1]", rec["grads"]
    # without return_lse: the entry without dlse, through _FusedAttn, the flag notwithstanding
    with _watch() as seen:
        rec = _record(dict(mask(), masked_lse_backward=True))
    assert seen["lse"] == 0 and seen["plain"] == 1 and seen["bwd"][0]["dlse"] is None
    assert [c.split()[0] for c in rec["calls"]] == [fwd, f"attn_bwd_{entry}"], rec["calls"]


def test_attn_bwd_picks_the_entry_by_dlse():
    """backward.attn_bwd itself, per mask kind: with dlse the *_dlse twin, without it the entry it always called"""
    leaves, packed = R.inputs(F_DIMS)
    q, k, v = (leaves[n].detach() for n in "qkv")
    cfg = ({n: int(x) for n, x in F_DIMS.items()}, 0, 1, R.NK, 0.125, native.FLAG_V_TRANSFORM)
    out, lse = torch.zeros_like(q), torch.zeros(R.B, R.H, R.TQ)
    i32 = lambda *shape: torch.zeros(shape, dtype=torch.int32)
    kinds = {"": dict(), "_varlen": dict(key_lens=i32(R.B), q_lens=i32(R.B)), "_gather": dict(key_lens=i32(R.B), key_idx=i32(R.B, R.TK)),
             "_qmask": dict(key_lens=i32(R.B), key_idx=i32(R.B, R.TK), q_live=R.query_mask(), q_lens=i32(R.B))}
    for suffix, mask in kinds.items():
        for dlse in (None, torch.ones(R.B, R.H, R.TQ)):
            log = []
            with _spies(log):
                BW.attn_bwd(cfg, q, k, v, out, torch.ones_like(q), lse, leaves["trans_coeff"].detach(), None, packed["vrep_q"], packed["vrep_k"],
                            packed["cs_q"], packed["cs_k"], dlse=dlse, **mask)
            assert [c.split()[0] for c in log] == ["attn_bwd" + suffix + ("_dlse" if dlse is not None else "")], (suffix, log)


def test_view_groups_hand_the_keyword_to_every_group():
    leaves, packed = R.inputs(F_DIMS)
    qm = R.query_mask()
    seen = []

    def attention(q, k, v, f_dims, sub, **kw):
        seen.append((k.shape[2], sub["vrep_k"].shape[1], kw))
        return torch.zeros_like(q), torch.zeros(q.shape[:3])
    saved = G.gta_attention, G.gta_attention_merge
    G.gta_attention, G.gta_attention_merge = attention, (lambda outs, lses: (outs[0], lses[0]))
    try:
        out = gta_amd.gta_attention_by_view_groups(leaves["q"], leaves["k"], leaves["v"], F_DIMS, packed, views_per_call=2, query_mask=qm,
                                                   key_mask_backward=True, key_mask_rep_grad=True, masked_lse_backward=True)
    finally:
        G.gta_attention, G.gta_attention_merge = saved
    assert torch.is_tensor(out) and [(tk, nk) for tk, nk, _ in seen] == [(2 * R.PK, 2), (R.PK, 1)]
    for _, _, kw in seen:
        assert kw["masked_lse_backward"] is True and kw["key_mask_backward"] is True and kw["key_mask_rep_grad"] is True
        assert kw["query_mask"] is qm and kw["return_lse"] is True
    # ... and each such call is served under grad (the spied entries; the merge needs a GPU and is not run here)
    rec = _record(dict(query_mask=R.query_mask(), key_mask_backward=True, key_mask_rep_grad=True, masked_lse_backward=True, return_lse=True),
                  tables_grad=True, cuda_carriers=True)
    assert "raises" not in rec and [c.split()[0] for c in rec["calls"]] == ["attn_fwd_qmask", "attn_bwd_qmask_dlse", "table_grads"], rec
    # the refusals of the key-side masks stay
    for kw in (dict(key_mask=R.key_mask()), dict(key_views=[1, R.NK]), dict(mask_index=G.MaskIndex())):
        with pytest.raises(native.GtaError, match="gta_attention_by_view_groups takes no"):
            gta_amd.gta_attention_by_view_groups(leaves["q"], leaves["k"], leaves["v"], F_DIMS, packed, views_per_call=2, masked_lse_backward=True, **kw)

"""Recorder of the routes ``gta_attention`` takes, on CPU tensors and without a GPU: every native launch entry, the table checks in front of
them and ``repgrad.table_grads`` are replaced by spies, and each case of a grid over layout x mask x grad x return_lse x kv_cache (plus the
single extras, the illegal argument pairs and the routes' own refusals) is boiled down to one short record -- the exception with its full
message, or the entries called with their descriptor flags and optional operands, what ``table_grads`` was handed, the kind of the return
value, which leaves received a gradient, and what the call left in ``kv_cache``.

Only names that are part of the package's surface are used (``gta_amd.gta_attention``, the public helpers and routes of ``gta_amd.gta``,
``gta_amd.native.*``, ``gta_amd.repgrad.table_grads``), so the same recorder runs on any revision: ``tests/call_routes_expected.json`` was
written by it on the revision BEFORE the fused layouts were given one autograd Function, and ``tests/test_call_routes_host.py`` holds the
current tree against that file.  ``python -m tests._call_routes OUT.json`` writes the records of the tree it is run in."""
import contextlib
import inspect
import itertools
import json
import sys

import torch

import gta_amd
from gta_amd import gta as G
from gta_amd import native, repgrad

B, H, TQ, NK, PK, DH = 2, 2, 8, 3, 24, 64
TK = NK * PK
LAYOUTS = {
    "fused": dict(f_dims={"se3": 32, "so2": 32}),                            # the CL dict of the key-mask host tests
    "staged": dict(f_dims={"se3": 32, "t2": 30, "triv": 2}),
    "apply": dict(f_dims={"se3": 32, "t2": 30, "triv": 2}, precise=True),    # float32 + precise: the rho-apply route
}
MASKS = ("none", "key_views", "key_views+query_views", "key_mask", "query_mask", "key_mask+query_mask")
GRADS = ("no_grad", "grad", "grad+flag", "grad+flag+tables", "grad+flag+tables+rep_grad")
CACHES = ("none", "fresh", "second")
OPERANDS = ("key_idx", "key_lens", "q_live", "q_lens", "kv_images", "dlse", "workspace", "key_bias", "dkey_bias", "dtc_rows", "dtau")
FILL = dict(out=1.0, lse=0.5, dq=1.0, dk=2.0, dv=3.0, dtrans_coeff=4.0, dtau=5.0, y=1.0, dx=1.0, dtc_rows=0.25, dkey_bias=0.125, key_bias=0.0)
ENTRIES = sorted(n for n in dir(native) if n.startswith(("attn_fwd", "attn_bwd", "rep_apply")) and callable(getattr(native, n))
                 and not n.endswith(("_supported", "_workspace_bytes")))


@contextlib.contextmanager
def spies(log=None, cuda_carriers=False, native=native, repgrad=repgrad):
    """the native launch entries, ``check_table`` / ``check_scalar`` / ``_require_cuda`` and ``repgrad.table_grads`` replaced; with ``log`` (a
    list) every call is noted in it and the entries' outputs are filled with constants, without it they do nothing at all (the host-time
    measurement).  ``cuda_carriers``: every tensor answers ``is_cuda`` with True, so that the refusal of CPU carriers lets the call through.
    ``native``, ``repgrad``: the modules to patch (those of another copy of the package, for the measurement)."""
    saved, last_fwd = [], {}

    def patch(mod, name, fn):
        saved.append((mod, name, getattr(mod, name)))
        setattr(mod, name, fn)

    def entry_spy(name):
        sig = inspect.signature(getattr(native, name))

        def spy(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            args = args.arguments
            desc = args["desc"]
            note = f"{name} flags={desc.flags:#x} Nq={desc.Nq} Nk={desc.Nk}"
            if "mode" in args:
                note += f" mode={args['mode']}"
            note += " ops=" + ",".join(o for o in OPERANDS if args.get(o) is not None)
            if name.startswith("attn_fwd"):
                last_fwd.clear()
                last_fwd.update(args)
            elif name.startswith("attn_bwd") and last_fwd:
                fwd = dict(last_fwd, kv_images=last_fwd.get("workspace"))
                note += " same=" + ",".join(o for o in OPERANDS if args.get(o) is not None and args.get(o) is fwd.get(o))
            log.append(note)
            for out, val in FILL.items():
                if torch.is_tensor(args.get(out)):
                    args[out].fill_(val)
        return spy

    def table_grads(desc, tables, meta, tc, q_pairs, k_pairs, direct, **kw):
        slots = lambda name: "".join("01"[x is not None] for x in kw.get(name, (None, None)))
        log.append(f"table_grads direct={direct} kw={','.join(sorted(kw))} views={slots('views')} lens={slots('lens')} masks={slots('masks')} "
                   f"pairs={len(q_pairs)},{len(k_pairs)} meta={''.join('01'[m is not None] for m in meta)}")
        return [None if m is None else torch.full(m[0], 6.0 + i, dtype=m[1]) for i, m in enumerate(meta)]

    nothing = lambda *a, **kw: None
    for name in ENTRIES:
        patch(native, name, nothing if log is None else entry_spy(name))
    for name in ("check_table", "check_scalar", "_require_cuda"):
        patch(native, name, nothing)
    patch(repgrad, "table_grads", table_grads if log is not None else
          (lambda desc, tables, meta, *a, **kw: [None if m is None else torch.zeros(m[0], dtype=m[1]) for m in meta]))
    if cuda_carriers:
        torch.Tensor.is_cuda = property(lambda self: True)
    try:
        yield
    finally:
        if cuda_carriers:
            del torch.Tensor.is_cuda
        for mod, name, fn in reversed(saved):
            setattr(mod, name, fn)


def inputs(f_dims, dtype=torch.float32, tables_grad=False, tq=TQ, tk=TK, nq=1, nk=NK, dh=DH, only_tau=False):
    """leaves of one call: q, k, v, trans_coeff, tau (all requiring grad; ``only_tau``: tau alone) and the packed tables of the layout"""
    leaves = {n: torch.zeros(B, H, t, dh, dtype=dtype, requires_grad=not only_tau) for n, t in (("q", tq), ("k", tk), ("v", tk))}
    leaves["trans_coeff"] = torch.tensor([0.5], requires_grad=not only_tau)
    leaves["tau"] = torch.tensor([0.8], requires_grad=True)
    packed = {}
    if f_dims.get("se3", 0) or f_dims.get("so3", 0):
        packed.update(vrep_q=torch.zeros(B, nq, native.VREP_STRIDE), vrep_k=torch.zeros(B, nk, native.VREP_STRIDE))
    if f_dims.get("so2", 0):
        packed.update(cs_q=torch.zeros(B, tq, f_dims["so2"] // 2, 2), cs_k=torch.zeros(B, tk, f_dims["so2"] // 2, 2))
    if f_dims.get("t2", 0):
        packed.update(coord_q=torch.zeros(B, tq, 2), coord_k=torch.zeros(B, tk, 2))
    if tables_grad:
        for t in packed.values():
            t.requires_grad_(True)
    leaves.update(packed)
    return leaves, packed


def key_mask(tk=TK):
    m = torch.ones(B, tk, dtype=torch.bool)
    m[:, 1::3] = False
    return m


def query_mask(tq=TQ):
    m = torch.ones(B, tq, dtype=torch.bool)
    m[:, ::4] = False
    m[1] = False
    return m


def mask_kwargs(mask, grad):
    """the keywords of a mask kind at a grad mode (the opt-in flag of the kind, ``key_mask_rep_grad``)"""
    kw = {}
    if mask.startswith("key_views"):
        kw["key_views"] = [1, NK]
        if "query_views" in mask:
            kw["query_views"] = [1] * B
        if "flag" in grad or "query_views" in mask:      # (query_views without the flag is one of the illegal pairs, recorded below)
            kw["key_views_backward"] = True
    if "key_mask" in mask:
        kw["key_mask"] = key_mask()
    if "query_mask" in mask:
        kw["query_mask"] = query_mask()
    if "mask" in mask and "flag" in grad:
        kw["key_mask_backward"] = True
        if "rep_grad" in grad:
            kw["key_mask_rep_grad"] = True
    return kw


def describe(kw):
    return {k: (f"{v.dtype}{tuple(v.shape)}" if torch.is_tensor(v) else "dict" if isinstance(v, dict) else v) for k, v in sorted(kw.items())}


def record(f_dims, kw, grad=True, tables_grad=False, cache="none", cuda_carriers=False, dtype=torch.float32, **shape):
    """one case -> its record (a JSON-able dict)"""
    leaves, packed = inputs(f_dims, dtype, tables_grad, **shape)
    tensors = ("q", "k", "v", "trans_coeff", "tau")
    kw = dict(kw)
    if cache != "none" or "kv_cache" in kw:
        kw["kv_cache"] = {}          # (a dict of the case's own)
    log, rec = [], {}
    call = lambda: gta_amd.gta_attention(*(leaves[n] for n in "qkv"), f_dims, packed, **dict({n: leaves[n] for n in tensors[3:]}, **kw))
    with spies(log, cuda_carriers), (contextlib.nullcontext() if grad else torch.no_grad()):
        try:
            if cache == "second":
                call()
                rec["first"] = list(log)
                log.clear()
            ret = call()
            rec["returns"] = "pair" if isinstance(ret, tuple) else "tensor"
            outs = ret if isinstance(ret, tuple) else (ret,)
            if any(o.requires_grad for o in outs):
                sum(o.sum() for o in outs if o.requires_grad).backward()
                rec["outputs_with_grad"] = sum(o.requires_grad for o in outs)
        except Exception as e:  # noqa: BLE001 -- the exception IS the record
            rec["raises"] = f"{type(e).__name__}: {e}"
    grads = " ".join(f"{n}{list(t.grad.shape)}" for n, t in leaves.items() if t.grad is not None)
    rec.update({name: val for name, val in (("calls", log), ("grads", grads)) if val})          # (left out when empty: most cases are refusals)
    if "kv_cache" in kw:
        rec["kv_cache"] = {"keys": sorted(kw["kv_cache"]), "plan": str(kw["kv_cache"].get("plan"))}
    return rec


def route(fn, *a, **kw):
    try:
        return {"returns": getattr(G, fn)(*a, **kw)}
    except Exception as e:  # noqa: BLE001
        return {"raises": f"{type(e).__name__}: {e}"}


def cases():
    """name -> thunk of every case"""
    out, seen = {}, set()

    def add(name, layout="fused", kw=(), **how):
        lay = dict(LAYOUTS[layout])
        f_dims = how.pop("f_dims", lay.pop("f_dims"))
        kw = dict(lay, **dict(kw))
        key = json.dumps([f_dims, describe(kw), sorted(how.items(), key=str)], default=str, sort_keys=True)
        if key in seen:          # (exact duplicates: e.g. 'grad' and 'grad+flag' without a mask)
            return
        seen.add(key)
        assert name not in out, name
        out[name] = lambda: record(f_dims, kw, **how)

    # the grid
    for layout, mask, grad, lse, cache in itertools.product(LAYOUTS, MASKS, GRADS, (False, True), CACHES):
        kw = mask_kwargs(mask, grad)
        if lse:
            kw["return_lse"] = True
        tables = "tables" in grad
        for cuda in ((False, True) if tables and mask != "none" else (False,)):
            add(f"{layout}/{mask}/{grad}/lse={int(lse)}/cache={cache}" + ("/cuda_carriers" if cuda else ""), layout, kw,
                grad=grad != "no_grad", tables_grad=tables, cache=cache, cuda_carriers=cuda)
    # under grad with tau alone requiring it (q, k, v, trans_coeff detached): the kv_cache refusal does not look at tau, so these calls run
    # under grad WITH a cache -- the masked ones must leave it alone, the unmasked one fills and reuses it
    for layout, mask, lse, cache in itertools.product(LAYOUTS, MASKS, (False, True), CACHES):
        kw = mask_kwargs(mask, "grad+flag")
        if lse:
            kw["return_lse"] = True
        add(f"{layout}/{mask}/grad+flag,tau_only/lse={int(lse)}/cache={cache}", layout, kw, cache=cache, only_tau=True)
    # single extras, once per mask kind (without grad and under grad with the opt-in)
    for mask, grad, extra in itertools.product(MASKS, ("no_grad", "grad+flag"), (dict(precise=True), dict(pretransformed=True), dict(kv_mode="fused"))):
        (name, val), = extra.items()
        add(f"extra/{mask}/{grad}/{name}={val}", "fused", dict(mask_kwargs(mask, grad), **extra), grad=grad != "no_grad")
    for extra in (dict(kv_mode="prepass"), dict(kv_mode="nonsense"), dict(use_dma=False), dict(precise=True, kv_cache={}), dict(v_transform=False),
                  dict(pretransformed=True, return_lse=True), dict(scale=0.2), dict(trans_coeff=0.5, tau=1.0)):
        for grad in (False, True):
            add(f"extra/none/grad={int(grad)}/" + ",".join(f"{k}={v}" for k, v in extra.items()), "fused", extra, grad=grad)
    add("extra/none/grad/tables/pretransformed", "fused", dict(pretransformed=True), tables_grad=True)
    add("extra/none/bfloat16", "fused", {}, dtype=torch.bfloat16)
    add("extra/none/float16", "fused", {}, dtype=torch.float16, grad=False)
    add("extra/key_views/float16", "fused", dict(key_views=[1, NK]), dtype=torch.float16, grad=False)
    add("extra/precise/bfloat16", "fused", dict(precise=True), dtype=torch.bfloat16, grad=False)
    add("extra/precise/dh=96/kv_cache", "fused", dict(precise=True, kv_cache={}), f_dims={"se3": 48, "so2": 48}, dh=96, grad=False)
    add("extra/euclid/key_mask", "fused", dict(key_mask=key_mask(), euclid=True), f_dims={"triv": 2, "se3": 30, "so2": 32}, grad=False)
    add("extra/euclid/key_views", "fused", dict(key_views=[1, NK], euclid=True), f_dims={"triv": 2, "se3": 30, "so2": 32}, grad=False)
    add("extra/euclid/key_views_backward", "fused", dict(key_views=[1, NK], euclid=True, key_views_backward=True), f_dims={"triv": 2, "se3": 30, "so2": 32})
    add("extra/dh=12/key_views", "fused", dict(key_views=[1, NK]), f_dims={"se3": 8, "so2": 4}, dh=12, grad=False)
    add("extra/dh=12/key_mask", "fused", dict(key_mask=key_mask()), f_dims={"se3": 8, "so2": 4}, dh=12, grad=False)
    add("extra/key_lens/given", "fused", dict(key_views=[1, NK], key_lens=G.key_lens_tensor((1, NK), PK, "cpu")), grad=False)
    add("extra/key_views/as_tensor", "fused", dict(key_views=torch.tensor([1, NK])), grad=False)
    for bad in ([1], [0, 1], [1.0, 2.0], 3):
        add(f"extra/key_views/bad={bad}", "fused", dict(key_views=bad), grad=False)
    add("extra/key_views/no_view_tables", "fused", dict(key_views=[1, 1]), f_dims={"so2": 64}, grad=False)
    add("extra/key_mask/empty_scene", "fused", dict(key_mask=torch.zeros(B, TK, dtype=torch.bool)), grad=False)
    add("extra/key_mask/wrong_shape", "fused", dict(key_mask=key_mask(TK + 1)), grad=False)
    add("extra/query_mask/wrong_shape", "fused", dict(query_mask=query_mask(TQ + 1)), grad=False)
    add("extra/query_mask/not_bool", "fused", dict(query_mask=query_mask().float()), grad=False)
    # tokens that do not split evenly into views
    add("uneven/key_views", "fused", dict(key_views=[1, NK]), tk=TK + 8, grad=False)
    add("uneven/query_views", "fused", dict(key_views=[1, NK], query_views=[1, 1], key_views_backward=True), nq=3)
    for mask in ("key_mask", "query_mask", "key_mask+query_mask"):
        kw = mask_kwargs(mask, "grad+flag+tables+rep_grad")
        if "key_mask" in kw:
            kw["key_mask"] = key_mask(TK + 8)
        add(f"uneven/{mask}/keys", "fused", kw, tk=TK + 8, tables_grad=True, cuda_carriers=True)
        add(f"uneven/{mask}/queries", "fused", mask_kwargs(mask, "grad+flag+tables+rep_grad"), nq=3, tables_grad=True, cuda_carriers=True)
    # the argument pairs refused at the top of gta_attention, each alone and against what could fire beside it
    km, qm, kv = key_mask(), query_mask(), [1, NK]
    lens = G.key_lens_tensor((1, NK), PK, "cpu")
    illegal = {
        "key_mask_backward/alone": dict(key_mask_backward=True),
        "key_mask_rep_grad/alone": dict(key_mask_rep_grad=True),
        "key_mask_rep_grad/key_mask": dict(key_mask=km, key_mask_rep_grad=True),
        "key_mask_rep_grad/key_mask_backward_alone": dict(key_mask_backward=True, key_mask_rep_grad=True),
        "query_mask/key_views": dict(query_mask=qm, key_views=kv),
        "query_mask/key_lens": dict(query_mask=qm, key_lens=lens),
        "query_mask/key_views_backward": dict(query_mask=qm, key_views_backward=True),
        "query_mask/query_views": dict(query_mask=qm, query_views=[1, 1]),
        "query_mask/key_mask/key_views": dict(query_mask=qm, key_mask=km, key_views=kv),
        "query_mask/kv_cache": dict(query_mask=qm, kv_cache={}),
        "query_mask/kv_cache/key_views": dict(query_mask=qm, kv_cache={}, key_views=kv),
        "key_mask/key_views": dict(key_mask=km, key_views=kv),
        "key_mask/key_lens": dict(key_mask=km, key_lens=lens),
        "key_mask/key_views_backward": dict(key_mask=km, key_views_backward=True),
        "key_mask/query_views": dict(key_mask=km, query_views=[1, 1]),
        "query_views/alone": dict(query_views=[1, 1]),
        "query_views/key_views": dict(key_views=kv, query_views=[1, 1]),
        "key_views_backward/alone": dict(key_views_backward=True),
        "key_lens/alone": dict(key_lens=lens),
        "key_lens/key_views_backward": dict(key_lens=lens, key_views_backward=True),
        "key_mask_backward/key_views": dict(key_mask_backward=True, key_views=kv),
    }
    for name, kw in illegal.items():
        for grad in (False, True):
            add(f"illegal/{name}/grad={int(grad)}", "fused", kw, grad=grad)
    # the routes, asked directly: the refusals gta_attention never lets them reach, and the answers
    shape, f_dims = (B, H, TQ, DH), LAYOUTS["fused"]["f_dims"]
    t2, small = LAYOUTS["staged"]["f_dims"], {"se3": 8, "so2": 4}
    fused = lambda **kw: route("attention_route", shape, kw.pop("tk", TK), kw.pop("dtype", torch.float32), kw.pop("f_dims", f_dims), 0, 1, NK, **kw)
    generic = lambda **kw: route("generic_route", kw.pop("shape", shape), TK, kw.pop("dtype", torch.float32), kw.pop("f_dims", t2), 0, 1, NK, **kw)
    asked = {"attention_route": fused, "generic_route": generic}
    how = [dict(), dict(needs_grad=True), dict(precise=True), dict(key_views=True), dict(key_views=True, needs_grad=True),
           dict(key_views=True, needs_grad=True, key_views_backward=True), dict(key_views=True, precise=True),
           dict(key_views=True, dtype=torch.float16), dict(dtype=torch.float16)]
    only_fused = [dict(key_mask=True), dict(key_mask=True, key_views=True), dict(key_mask=True, needs_grad=True),
                  dict(key_mask=True, needs_grad=True, key_mask_backward=True), dict(key_mask=True, precise=True),
                  dict(key_mask=True, pretransformed=True), dict(key_mask=True, kv_mode="fused"), dict(key_mask=True, f_dims=t2),
                  dict(key_mask=True, kv_mode="prepass_pg"), dict(key_mask=True, use_dma=False), dict(key_views=True, pretransformed=True),
                  dict(key_views=True, kv_mode="fused"), dict(key_views=True, kv_mode="prepass_pg"), dict(key_views=True, use_dma=False),
                  dict(key_views=True, f_dims=t2), dict(kv_mode="nonsense"), dict(precise=True, dtype=torch.bfloat16), dict(precise=True, needs_grad=True),
                  dict(precise=True, needs_grad=True, kv_mode="fused"), dict(precise=True, kv_cache=True), dict(kv_cache=True),
                  dict(pretransformed=True), dict(f_dims=t2), dict(kv_mode="prepass"), dict(kv_mode="fused"),
                  dict(key_views=True, tk=TK + 8), dict(key_mask=True, tk=TK + 8)]
    only_generic = [dict(key_views=True, f_dims=small, shape=(B, H, TQ, 12)), dict(f_dims=small, shape=(B, H, TQ, 12)), dict(euclid=True)]
    for fn, extra in (("attention_route", only_fused), ("generic_route", only_generic)):
        for kw in how + extra:
            name = f"{fn}/" + (",".join(f"{k}={v}" for k, v in kw.items()) or "plain")
            out[name] = (lambda fn=fn, kw=kw: asked[fn](**dict(kw)))
    return out


def record_all():
    return {name: thunk() for name, thunk in cases().items()}


def load(path):
    """the records of a file written by ``__main__`` below (most cases are one of a few dozen refusals: the file holds each message once)"""
    with open(path) as f:
        data = json.load(f)
    return {name: dict(rec, raises=data["messages"][rec["raises"]]) if "raises" in rec else rec for name, rec in data["cases"].items()}


if __name__ == "__main__":
    records = record_all()
    messages = sorted({rec["raises"] for rec in records.values() if "raises" in rec})
    for rec in records.values():
        if "raises" in rec:
            rec["raises"] = messages.index(rec["raises"])
    with open(sys.argv[1], "w") as f:
        json.dump({"messages": messages, "cases": records}, f, indent=0, sort_keys=True)
        f.write("\n")

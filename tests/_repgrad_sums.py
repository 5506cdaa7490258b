"""The rep-gradient sums (`gta_rep_grad_sums`, gta_repgrad.hip) as a test sees them: the fp64 reference, the two rules, the fill and guard
rules, the case table and a host emulation of the kernel's structure.  CPU only; tests/test_repgrad_sums_host.py proves on the CPU that
every rule fails on the defect it is meant for, tests/test_gpu_repgrad_sums.py holds the kernel to the same rules.

The operation: with (a, b) pairs of [B,H,T,dh] rows and the descriptor's slabs [triv | se3 | so3 | so2 | t2],
  view [B,N,4,4]        sum over pairs, heads, the view's P = T / N tokens and the se3 slab's groups of a_g b_g^T (euclid: 3-channel groups,
                        b homogenised by 1, a by 0: a zero fourth row)
  so2  [B,T,n_so2,2,2]  sum over pairs and heads of the block's a b^T
  t2   [B,T,3,3]        sum over pairs, heads and the t2 slab's 3-channel groups of a_g b_g^T

Rules (`check`):
  lattice data   every operand element is k/4, |k| <= 8: a product is a multiple of 1/16 of magnitude <= 4, so every partial sum of n
                 addends is a multiple of 1/16 of magnitude <= 4n -- exact in fp32 in any order, with or without FMA, while 64 n < 2^24
                 (`exact_ok`).  got == ref64, element for element.
  gaussian data  |got - ref64| <= (n + 1) * 2^-24 * absprod, absprod the same sum over |a|, |b| and n the element's addends
                 (`addends`): the dot-product bound gamma_n of fp32 accumulation in any order; the reference takes the operands as
                 rounded to the case's dtype, so nothing else enters.  With n <= 1024 a bf16 rounding of one workgroup's partial breaks it.
  fill           a requested output comes back finite everywhere from a NaN fill; one not requested is not passed (NULL)
  guards         the 64 words behind each output and the 256 bytes behind the workspace come back as they were"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

BF16, F32 = torch.bfloat16, torch.float32
NT = 256                     # threads of a workgroup (GTA_REPGRAD_THREADS)
SO2_PASS = 8                 # so2 blocks per pass of the kernel's LDS
GUARD = 64                   # guard words behind each output
WS_PAD = 256                 # guard bytes behind the workspace
NAN_WORD = 0x7FC12345        # the fill of outputs and guards: a quiet NaN no arithmetic produces
U = 2.0 ** -24
OUTS = ("view", "so2", "t2")


# ---- reference ---------------------------------------------------------------------------------------------------------------------------
def _view_sums(pairs, lo, n, W, N, homog=False):
    """per view: sum over heads, the view's tokens and the slab's n groups of W channels from channel lo of a b^T -> ([B,N,4,4], absprod)"""
    S = A = 0
    for a, b in pairs:
        B, H, T, _ = a.shape
        av = a[..., lo:lo + n * W].reshape(B, H, N, T // N, n, W)
        bv = b[..., lo:lo + n * W].reshape(B, H, N, T // N, n, W)
        if homog:
            av, bv = F.pad(av, (0, 1)), F.pad(bv, (0, 1), value=1.0)
        S = S + torch.einsum("bhntgi,bhntgj->bnij", av, bv)
        A = A + torch.einsum("bhntgi,bhntgj->bnij", av.abs(), bv.abs())
    return S, A


def _so2_sums(pairs, lo, n):
    """per token and so2 block: sum over heads of a b^T -> ([B,T,n,2,2], absprod)"""
    S = A = 0
    for a, b in pairs:
        av, bv = a[..., lo:lo + 2 * n].unflatten(-1, (n, 2)), b[..., lo:lo + 2 * n].unflatten(-1, (n, 2))
        S = S + torch.einsum("bhtgi,bhtgj->btgij", av, bv)
        A = A + torch.einsum("bhtgi,bhtgj->btgij", av.abs(), bv.abs())
    return S, A


def _t2_sums(pairs, lo, n):
    """per token: sum over heads and the slab's n groups of a b^T -> ([B,T,3,3], absprod)"""
    S = A = 0
    for a, b in pairs:
        av, bv = a[..., lo:lo + 3 * n].unflatten(-1, (n, 3)), b[..., lo:lo + 3 * n].unflatten(-1, (n, 3))
        S = S + torch.einsum("bhtgi,bhtgj->btij", av, bv)
        A = A + torch.einsum("bhtgi,bhtgj->btij", av.abs(), bv.abs())
    return S, A


def slabs(f_dims, euclid=False):
    """the descriptor's slab offsets and group counts as gta_rep_grad_sums derives them"""
    g = lambda k: int(f_dims.get(k, 0))
    W = 3 if euclid else 4
    assert g("se3") % W == 0 and g("so2") % 2 == 0 and g("t2") % 3 == 0
    off_so2 = g("triv") + g("se3") + g("so3")
    return SimpleNamespace(W=W, off_se3=g("triv"), n_se3=g("se3") // W, off_so2=off_so2, n_so2=g("so2") // 2,
                           off_t2=off_so2 + g("so2"), n_t2=g("t2") // 3, dh=sum(int(v) for v in f_dims.values()))


def addends(case):
    """the number of products an element of each output sums"""
    s = slabs(case.f_dims, case.euclid)
    return {"view": case.pairs * case.H * case.P * s.n_se3, "so2": case.pairs * case.H, "t2": case.pairs * case.H * s.n_t2}


def exact_ok(case):
    """the lattice rule's condition: 64 n < 2^24 for the largest n of the case"""
    return 64 * max(addends(case).values()) < 2 ** 24


def reference(case, vals):
    """{output: (ref64, absprod, n)} for every output the case's slabs allow"""
    s = slabs(case.f_dims, case.euclid)
    pairs = [(vals[2 * i], vals[2 * i + 1]) for i in range(case.pairs)]
    n = addends(case)
    ref = {}
    if s.n_se3:
        ref["view"] = _view_sums(pairs, s.off_se3, s.n_se3, s.W, case.N, homog=case.euclid) + (n["view"],)
    if s.n_so2:
        ref["so2"] = _so2_sums(pairs, s.off_so2, s.n_so2) + (n["so2"],)
    if s.n_t2:
        ref["t2"] = _t2_sums(pairs, s.off_t2, s.n_t2) + (n["t2"],)
    return ref


# ---- operands ----------------------------------------------------------------------------------------------------------------------------
def _logical(x, lay):
    if lay == "h0":
        return x[:, :1].expand_as(x)
    if lay == "b0":
        return x[:1].expand_as(x)
    return x


def values(case, family):
    """the 2 * pairs operands (a0, b0, a1, b1) as fp64 [B,H,T,dh], already rounded to the case's dtype; a function of case.seed, the
    shape and the family alone, so cases that share those hold the same values under different strides"""
    g = torch.Generator().manual_seed(case.seed + (7919 if family == "gauss" else 0))
    shape = (case.B, case.H, case.N * case.P, slabs(case.f_dims, case.euclid).dh)
    vals = []
    for i in range(2 * case.pairs):
        if family == "lattice":
            x = torch.randint(-8, 9, shape, generator=g).double() / 4
        else:
            x = torch.randn(shape, generator=g, dtype=torch.float64)
        x = x.to(case.dtype).double()
        vals.append(_logical(x, case.lay[i]))
    return vals


def place(x, lay, dtype, device="cpu"):
    """the [B,H,T,dh] view of layout ``lay`` that holds x; whatever its storage holds outside the view is NaN
      bhtd      contiguous                              bthd     [B,T,H,dh] storage
      packed<i> slot i of a packed [B,T,3,H,dh] buffer  h0 / b0  head / batch stride 0 (expand)
      choff     x[..., 1:dh+1] of a dh+8 wide buffer    pad<k>   x[..., :dh] of a dh+k wide buffer"""
    B, H, T, dh = x.shape
    nan = lambda *s: torch.full(s, float("nan"), dtype=dtype, device=device)
    src = x.to(dtype).to(device)
    if lay == "bhtd":
        v = nan(B, H, T, dh)
    elif lay == "bthd":
        v = nan(B, T, H, dh).permute(0, 2, 1, 3)
    elif lay.startswith("packed"):
        v = nan(B, T, 3, H, dh)[:, :, int(lay[6:])].permute(0, 2, 1, 3)
    elif lay == "h0":
        st = nan(B, 1, T, dh)
        st.copy_(src[:, :1])
        return st.expand(B, H, T, dh)
    elif lay == "b0":
        st = nan(1, H, T, dh)
        st.copy_(src[:1])
        return st.expand(B, H, T, dh)
    elif lay == "choff":
        v = nan(B, H, T, dh + 8)[..., 1:dh + 1]
    elif lay.startswith("pad"):
        v = nan(B, H, T, dh + int(lay[3:]))[..., :dh]
    else:
        raise ValueError(lay)
    v.copy_(src)
    return v


def instance(case, subset, ops=None):
    """the kernel instance (element size, EUCLID, VEC) `vec_ok` and `gta_repgrad_dispatch` select for the launch, read from gta_repgrad.hip;
    ``ops``: the placed operands (default: placed on the CPU, whose allocations are 64-byte aligned as the GPU's are 256-byte aligned).
    Documentation of the table and the key of the per-instance error report, not something a test asserts about the kernel."""
    s = slabs(case.f_dims, case.euclid)
    esz = 2 if case.dtype == BF16 else 4
    if ops is None:
        ops = [place(torch.zeros(case.B, case.H, case.N * case.P, s.dh), lay, case.dtype) for lay in case.lay[:2 * case.pairs]]
    vec = all((t.storage_offset() * esz) % 16 == 0 and all((st * esz) % 16 == 0 for st in t.stride()[:3]) for t in ops)
    if "view" in subset and (case.euclid or s.off_se3 % 8 or s.n_se3 % 2):
        vec = False
    if "so2" in subset and (s.off_so2 % 8 or s.n_so2 % 4):
        vec = False
    return (esz, False, True) if vec else (esz, case.euclid, False)


# ---- rules -------------------------------------------------------------------------------------------------------------------------------
def subsets(case):
    """the launches of a case: each output alone, and all its slabs allow together"""
    s = slabs(case.f_dims, case.euclid)
    have = [o for o, n in zip(OUTS, (s.n_se3, s.n_so2, s.n_t2)) if n]
    return [(o,) for o in have] + ([tuple(have)] if len(have) > 1 else [])


def out_shapes(case):
    s = slabs(case.f_dims, case.euclid)
    T = case.N * case.P
    return {"view": (case.B, case.N, 4, 4), "so2": (case.B, T, s.n_so2, 2, 2), "t2": (case.B, T, 3, 3)}


def tpb_chunks(case):
    tpb = NT // case.H
    return tpb, -(-case.P // tpb)


def workspace_bytes(case):
    return case.B * case.N * tpb_chunks(case)[1] * 64


def check(case, subset, family, res, ref):
    """Apply every rule to the result of one launch: res = {"view" / "so2" / "t2": fp32 tensor or None, "guard": {output: int32[GUARD]},
    "ws_tail": uint8[WS_PAD] or None}.  Returns {output: largest error / bound} on gaussian data ({} on lattice data)."""
    worst = {}
    tag = (case.name, "+".join(subset), family)
    for o in OUTS:
        got = res[o]
        if o not in subset:
            assert got is None, tag + (o, "not requested, yet produced")
            continue
        r, ap, n = ref[o]
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(r.shape) == out_shapes(case)[o], tag + (o, tuple(got.shape))
        fin = torch.isfinite(got)
        assert fin.all(), tag + (o, f"{int((~fin).sum())} of {got.numel()} words not finite (left at the fill?)",
                                 (~fin).nonzero()[0].tolist())
        g64 = got.double()
        if family == "lattice":
            assert exact_ok(case), tag
            bad = g64 != r
            if bad.any():
                i = tuple(bad.nonzero()[0].tolist())
                raise AssertionError(tag + (o, f"{int(bad.sum())} of {got.numel()} elements differ; first at {i}: got {g64[i].item()!r}, "
                                               f"ref {r[i].item()!r}"))
        else:
            bound = (n + 1) * U * ap
            err = (g64 - r).abs()
            ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0).double())
            worst[o] = ratio.max().item()
            if worst[o] > 1:
                i = tuple((ratio == ratio.max()).nonzero()[0].tolist())
                raise AssertionError(tag + (o, f"error {err[i].item():.3e} is {worst[o]:.2f} of the bound {bound[i].item():.3e} "
                                               f"(n = {n}) at {i}"))
        guard = res["guard"][o]
        assert guard.numel() == GUARD and bool((guard == NAN_WORD).all()), tag + (o, "guard words written")
    if "view" in subset:
        tail = res["ws_tail"]
        assert tail is not None and tail.numel() == WS_PAD and bool((tail == 0xFF).all()), tag + ("workspace tail written",)
    else:
        assert res["ws_tail"] is None, tag + ("a workspace without view sums",)
    return worst


# ---- host emulation of the kernel's structure ----------------------------------------------------------------------------------------------
DEFECTS = ("row_dropped", "chunk_last_token_dropped", "last_partial_skipped", "dead_threads_live", "transposed", "pair1_ignored",
           "no_homogeneous_one", "second_pass_at_f0_0", "head_left_out", "t2_first_group_only", "neighbour_view", "partial_bf16",
           "guard_written", "fill_left")


def applies(defect, case, subset, family):
    """whether the planted defect changes what this launch of this case computes"""
    s = slabs(case.f_dims, case.euclid)
    tpb, chunks = tpb_chunks(case)
    view, so2, t2 = ("view" in subset), ("so2" in subset), ("t2" in subset)
    return {
        "row_dropped": True,
        "chunk_last_token_dropped": True,
        "last_partial_skipped": view and chunks >= 2,
        "dead_threads_live": view and tpb * case.H < NT,
        "transposed": True,
        "pair1_ignored": case.pairs == 2,
        "no_homogeneous_one": view and case.euclid,
        "second_pass_at_f0_0": so2 and s.n_so2 > SO2_PASS,
        "head_left_out": so2 or t2,
        "t2_first_group_only": t2 and s.n_t2 > 1,
        "neighbour_view": view,
        "partial_bf16": view and family == "gauss",
        "guard_written": True,
        "fill_left": True,
    }[defect]


def emulate(case, vals, subset, defect=None):
    """The kernel's structure in fp32 on the host: per-(token, head) row sums over pairs then groups, the workgroup's tree over its 256
    threads (dead threads add zero), the finish sum over a view's partials in workgroup order, per-token sums in head order; so2 blocks in
    passes of SO2_PASS.  ``defect``: one of DEFECTS planted.  Returns a result for `check`."""
    s = slabs(case.f_dims, case.euclid)
    B, H, N, P = case.B, case.H, case.N, case.P
    T = N * P
    tpb, chunks = tpb_chunks(case)
    pairs = [(vals[2 * i].float(), vals[2 * i + 1].float()) for i in range(case.pairs)]
    if defect == "pair1_ignored":
        pairs = pairs[:1]

    def rows(off, n, W, homog=False, per_group=False):
        """fp32 row sums [B,H,T,(n,)W',W'] accumulated pair by pair, group by group"""
        Wp = W + 1 if homog else W
        acc = torch.zeros((B, H, T, n, Wp, Wp) if per_group else (B, H, T, Wp, Wp), dtype=torch.float32)
        for a, b in pairs:
            for g in range(n):
                x, y = a[..., off + g * W:off + (g + 1) * W], b[..., off + g * W:off + (g + 1) * W]
                if homog:
                    x, y = F.pad(x, (0, 1)), F.pad(y, (0, 1), value=0.0 if defect == "no_homogeneous_one" else 1.0)
                if defect == "transposed":
                    x, y = y, x
                term = x[..., :, None] * y[..., None, :]
                if per_group:
                    acc[:, :, :, g] += term
                else:
                    acc += term
        if defect == "row_dropped":
            acc[B - 1, H - 1, T // 2] = 0
        if defect == "chunk_last_token_dropped":
            for n_ in range(N):
                acc[:, :, n_ * P + min(tpb, P) - 1] = 0
        return acc

    def head_sum(r):
        out = torch.zeros(r.shape[:1] + r.shape[2:], dtype=torch.float32)
        for h in range(H - 1 if defect == "head_left_out" else H):
            out += r[:, h]
        return out

    res = {o: None for o in OUTS}
    if "view" in subset:
        r = rows(s.off_se3, s.n_se3, s.W, homog=case.euclid).reshape(B, H, N, P, 16)
        if defect == "neighbour_view":
            r = r.roll(-1, dims=2)
        r = F.pad(r, (0, 0, 0, chunks * tpb - P)).reshape(B, H, N, chunks, tpb, 16)
        wg = r.permute(0, 2, 3, 4, 1, 5).reshape(B, N, chunks, tpb * H, 16)       # thread tid = tl * H + h
        wg = F.pad(wg, (0, 0, 0, NT - tpb * H)).contiguous()
        if defect == "dead_threads_live":
            for tid in range(tpb * H, NT):
                wg[..., tid, :] = wg[..., tid % H, :]                              # token 0 of the chunk, head tid % H
        st = NT // 2
        while st > 0:
            wg[..., :st, :] = wg[..., :st, :] + wg[..., st:2 * st, :]
            st //= 2
        part = wg[..., 0, :].clone()                                               # [B,N,chunks,16]
        if defect == "partial_bf16":
            part[0, 0, 0] = part[0, 0, 0].bfloat16().float()
        view = torch.zeros(B, N, 16, dtype=torch.float32)
        for c in range(chunks - 1 if defect == "last_partial_skipped" else chunks):
            view += part[:, :, c]
        res["view"] = view.reshape(B, N, 4, 4)
    if "so2" in subset:
        full = head_sum(rows(s.off_so2, s.n_so2, 2, per_group=True))               # [B,T,n,2,2]
        if defect == "second_pass_at_f0_0":
            out = torch.full_like(full, float("nan"))
            for f0 in range(0, s.n_so2, SO2_PASS):
                nf = min(SO2_PASS, s.n_so2 - f0)
                out[:, :, :nf] = full[:, :, f0:f0 + nf]
            full = out
        res["so2"] = full
    if "t2" in subset:
        res["t2"] = head_sum(rows(s.off_t2, 1 if defect == "t2_first_group_only" else s.n_t2, 3))
    res["guard"] = {o: torch.full((GUARD,), NAN_WORD, dtype=torch.int32) for o in subset}
    res["ws_tail"] = torch.full((WS_PAD,), 0xFF, dtype=torch.uint8) if "view" in subset else None
    if defect == "guard_written":
        res["guard"][subset[-1]][17] = 0
    if defect == "fill_left":
        o = subset[-1]
        res[o].view(-1)[res[o].numel() // 2] = float("nan")
    return res


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
FV = {"se3": 8, "so2": 8}                               # dh 16: both slabs on 8-channel boundaries, n_se3 2, n_so2 4
FT = {"triv": 2, "se3": 4, "so2": 6, "t2": 6}           # dh 18: nothing aligned, n_se3 1, n_so2 3, two t2 groups


def _table():
    """name -> case.  The instance comments are `instance()`'s reading of vec_ok for the launches view / so2 / t2 / all, V = the 16-byte
    form <esz, false, true>, S = the scalar form <esz, false, false>, E = the scalar euclid form <esz, true, false>; alike for both dtypes
    unless said."""
    cases = {}

    def add(name, H, N, P, f_dims, *, B=2, pairs=1, lay=None, euclid=False, gauss=False, side=0, other=None, seed=None, twin=None,
            dtypes=(BF16, F32)):
        for dt in dtypes:
            full = f"{name}-{'bf16' if dt == BF16 else 'f32'}"
            lay4 = tuple(lay) if lay else ("bhtd",) * 4
            lay4 = (lay4 * 2)[:4] if len(lay4) == 2 else lay4
            c = SimpleNamespace(name=full, B=B, H=H, N=N, P=P, f_dims=dict(f_dims), euclid=euclid, dtype=dt, pairs=pairs, lay=lay4,
                                gauss=gauss, side=side, other=other or (N, P), seed=len(cases) + 100 if seed is None else seed, twin=twin)
            assert B <= 2 and N * P <= 600 and N >= 2 and full not in cases
            cases[full] = c

    # heads and dead threads, chunk edges (tpb = 256 / H tokens of a view per workgroup)
    add("h1-short", 1, 2, 5, FV)                            # tpb 256, one short chunk                              V V - V
    add("h1-t2", 1, 2, 5, FT)                               #                                                       S S S S
    add("h3-full", 3, 2, 85, FV)                            # tpb 85, 1 dead thread, P = tpb                        V V - V
    add("h3-plus1", 3, 2, 86, FT)                           # P = tpb + 1: the finish kernel adds two partials      S S S S
    add("h5-full", 5, 2, 51, FV)                            # tpb 51, 1 dead thread                                 V V - V
    add("h5-plus1", 5, 3, 52, FT, pairs=2)                  #                                                       S S S S
    add("h6-2c5", 6, 3, 89, FV)                             # tpb 42, 4 dead threads, P = 2 tpb + 5                 V V - V
    add("h6-plus1", 6, 2, 43, FT)                           #                                                       S S S S
    add("h6-short", 6, 2, 7, FT, pairs=2)                   #                                                       S S S S
    add("h8-short", 8, 2, 7, FV)                            # tpb 32                                                V V - V
    add("h8-full", 8, 2, 32, FV)
    add("h8-plus1", 8, 2, 33, FV)
    add("h8-2c5", 8, 2, 69, FV, pairs=2)
    add("h8t-short", 8, 2, 7, FT)                           #                                                       S S S S
    add("h8t-full", 8, 2, 32, FT, pairs=2)
    add("h8t-plus1", 8, 2, 33, FT)
    add("h8t-2c5", 8, 3, 69, FT)
    add("h256", 256, 2, 3, FV)                              # tpb 1: one workgroup per token, three partials a view V V - V
    add("h256-t2", 256, 2, 3, FT, pairs=2)                  #                                                       S S S S
    # se3: the 16-byte form needs off_se3 % 8 == 0 and an even n_se3, no euclid
    add("se3-vec8", 8, 2, 33, {"se3": 32, "so2": 8})                          # n_se3 8, dh 40                      V V - V
    add("se3-odd1", 8, 2, 33, {"se3": 4, "so3": 4, "so2": 8})                 # n_se3 1, aligned rows (dh 16)       S V - S
    add("se3-odd3", 6, 2, 43, {"se3": 12, "so3": 4, "so2": 16})               # n_se3 3, dh 32                      S V - S
    add("se3-off4", 8, 2, 33, {"triv": 4, "se3": 8, "so2": 8, "t2": 12})      # off_se3 4, off_so2 12, dh 32        S S V S
    add("eu-se3-3", 6, 2, 43, {"triv": 5, "se3": 3, "so2": 8}, euclid=True)   # dh 16, off_so2 8                    E V - E
    add("eu-se3-9", 8, 2, 33, {"triv": 1, "se3": 9, "so2": 8, "t2": 6}, euclid=True, pairs=2)     # dh 24           E E V E
    add("eu-t2", 5, 2, 20, {"triv": 2, "se3": 3, "so2": 8, "t2": 3}, euclid=True)                 # dh 16           E E V E
    # so2: the 16-byte form needs off_so2 % 8 == 0 and n_so2 % 4 == 0; n_so2 > 8 takes a second SO2_PASS trip
    for n in (4, 8, 12, 16):
        add(f"so2-vec{n}", 8, 2, 33, {"se3": 8, "so2": 2 * n})                # dh 16 / 24 / 32 / 40; 12: nf = 4    V V - V
    add("so2-n1", 8, 2, 33, {"se3": 8, "so2": 2, "t2": 6})                    # dh 16                               V S V S
    add("so2-n3", 6, 2, 43, {"se3": 8, "so2": 6, "t2": 18})                   # dh 32                               V S V S
    add("so2-n9", 8, 2, 33, {"se3": 8, "so2": 18, "t2": 6})                   # dh 32, second trip with nf = 1      V S V S
    add("so2-only16", 5, 2, 52, {"so2": 32}, pairs=2)                         # no se3 slab                         - V - -
    add("so2-only9", 8, 2, 33, {"triv": 2, "so2": 18})                        # dh 20                               - S - -
    # t2 alone: no view output, so no workspace
    add("t2-alone3", 8, 2, 33, {"triv": 5, "t2": 3})                          # dh 8                                - - V -
    add("t2-alone6", 6, 2, 43, {"triv": 2, "t2": 6}, pairs=2)                 # dh 8                                - - V -
    # strides: one set of values (seed 77) under six layouts, exact on lattice data and so equal to each other
    add("st-bhtd", 8, 2, 33, FV, seed=77, twin="st")                                           #                    V V - V
    add("st-bthd", 8, 2, 33, FV, lay=("bthd", "bthd"), seed=77, twin="st")                     #                    V V - V
    add("st-packed", 8, 2, 33, FV, lay=("packed1", "packed2"), seed=77, twin="st")             #                    V V - V
    add("st-pad8", 8, 2, 33, FV, lay=("pad8", "pad8"), seed=77, twin="st")                     # rows 24 wide       V V - V
    add("st-choff", 8, 2, 33, FV, lay=("choff", "choff"), seed=77, twin="st")                  # base off 16 bytes  S S - S
    add("st-pad2", 8, 2, 33, FV, lay=("pad2", "pad2"), seed=77, twin="st")                     # token stride 18    S S - S
    add("st-h0", 8, 2, 33, FV, lay=("h0", "bhtd"))                                             # head stride 0      V V - V
    add("st-b0", 8, 2, 33, FV, lay=("bthd", "b0"))                                             # batch stride 0     V V - V
    add("p2-mixed", 8, 2, 33, FV, pairs=2, lay=("bhtd", "bhtd", "bthd", "packed1"))            # pair 1 strided     V V - V
    add("p2-choff", 8, 2, 33, FV, pairs=2, lay=("bhtd", "bhtd", "bthd", "choff"))              # pair 1 misaligned  S S - S
    # both sides of a cross attention: Tq = 102 in 3 views, Tk = 90 in 2
    add("cross-q", 8, 3, 34, FV, side=0, other=(2, 45), pairs=2)                               #                    V V - V
    add("cross-k", 8, 2, 45, FV, side=1, other=(3, 34), pairs=2)                               #                    V V - V
    add("cross-k-t2", 6, 2, 45, FT, side=1, other=(3, 34))                                     #                    S S S S
    # gaussian data as well: every instance, two chunks (g-2chunk, g-euclid), n_so2 = 12; view addends n <= 1024
    add("g-vec", 4, 2, 8, FV, gauss=True)                                                      # n 64               V V - V
    add("g-2chunk", 8, 2, 33, FT, gauss=True)                                                  # n 264              S S S S
    add("g-euclid", 6, 2, 43, {"triv": 2, "se3": 3, "so2": 8, "t2": 3}, euclid=True, gauss=True)   # n 258          E E V E
    add("g-so2-12", 8, 2, 10, {"se3": 8, "so2": 24}, pairs=2, gauss=True)                      # n 320              V V - V
    return cases


CASES = _table()
GAUSS = tuple(n for n, c in CASES.items() if c.gauss)
RUNS = tuple((n, "lattice") for n in CASES) + tuple((n, "gauss") for n in GAUSS)

"""The rep-gradient sums under a per-token mask (`gta_rep_grad_sums_masked`, the MASKED instances of gta_repgrad.hip) as a test sees them:
tests/_repgrad_sums.py -- its fp64 reference, lattice / gaussian rules, fill and guard rules, host emulation -- with a bool [B, T] mask, the
way tests/_repgrad_sums_varlen.py adds a prefix.  CPU only; tests/test_repgrad_sums_masked_host.py proves on the CPU that every rule fails on
the defect it is meant for, tests/test_gpu_repgrad_sums_masked.py holds the kernel to the same rules.

A masked case is a case of `_repgrad_sums.CASES` plus ``mask`` (bool [B, T], True = the token is live).  A row (b, h, t) with mask[b, t]
False is dead.  The reference is `_repgrad_sums.reference` on the values with dead rows set to zero: zero rows add exact zero, and `addends`
stays an upper bound of an element's products, so the lattice rule (exact equality) and the gaussian rule ((n + 1) * 2^-24 * absprod) carry
over unchanged.

New rules:
  dead-zero     (`check`) per-token sums of dead tokens and view sums of views without a live token are +0.0: all 32 bits zero
  never-read    the launch runs on operands whose dead rows hold NaN in every channel of every pair, and every output is finite
  live-equal    (`check_same_bits`) EVERY word is, bit for bit, that of the unmasked entry on the operands with the dead rows set to zero
  prefix-equal  (`check_same_bits`) under a mask that is a prefix of every scene, every word is that of the VARLEN entry with those counts"""
from types import SimpleNamespace

import torch

from tests import _repgrad_sums as S
from tests import _repgrad_sums_varlen as V

OUTS = S.OUTS


def row_mask(case, mask=None):
    """[B,1,T,1] bool: live rows"""
    return (case.mask if mask is None else mask)[:, None, :, None]


def masked(case, vals, fill=0.0):
    """the operands with every dead row set to ``fill``"""
    m = row_mask(case)
    return [torch.where(m, x, torch.full((), fill, dtype=x.dtype)) for x in vals]


def reference(case, vals):
    return S.reference(case, masked(case, vals))


def dead_views(case):
    """[B,N] bool: views without a live token"""
    return ~case.mask.view(case.B, case.N, case.P).any(-1)


def dead_tokens(case):
    return ~case.mask


def workgroups(case):
    """[(b, n, c, t0, t1)]: the launch's workgroups and the tokens [t0, t1) each owns"""
    tpb, chunks = S.tpb_chunks(case)
    return [(b, n, c, n * case.P + c * tpb, min(n * case.P + (c + 1) * tpb, (n + 1) * case.P))
            for b in range(case.B) for n in range(case.N) for c in range(chunks)]


def dead_workgroups(case, mask=None):
    """the workgroups none of whose tokens is live"""
    mask = case.mask if mask is None else mask
    return [w for w in workgroups(case) if not bool(mask[w[0], w[3]:w[4]].any())]


def check(case, subset, family, res, ref):
    """every rule of `_repgrad_sums.check` (lattice / gaussian, fill -- which is never-read when the launch had NaN in its dead rows --,
    guards) and dead-zero.  Returns what `_repgrad_sums.check` returns."""
    worst = S.check(case, subset, family, res, ref)
    tag = (case.name, "+".join(subset), family)
    for o in subset:
        bits = res[o].contiguous().view(torch.int32)
        dead = dead_views(case) if o == "view" else dead_tokens(case)
        bad = bits[dead] != 0
        assert not bool(bad.any()), tag + (o, f"dead-zero: {int(bad.sum())} words of dead entries are not +0.0")
    return worst


def check_same_bits(case, subset, res, other, rule):
    """live-equal (``other``: the unmasked entry on the operands with zeroed dead rows) and prefix-equal (``other``: the VARLEN entry under
    the prefix's counts): every word, dead entries included"""
    for o in subset:
        a, b = res[o].contiguous().view(torch.int32), other[o].contiguous().view(torch.int32)
        assert torch.equal(a, b), (case.name, "+".join(subset), o, f"{rule}: {int((a != b).sum())} of {a.numel()} words differ")


# ---- what the masks of the table must contain (tests/test_repgrad_sums_masked_host.py asserts it) ------------------------------------------
def has_first_dead_later_live(case):
    """(a) a workgroup whose first token is dead and a later one live"""
    return any(not bool(case.mask[b, t0]) and bool(case.mask[b, t0 + 1:t1].any()) for b, n, c, t0, t1 in workgroups(case))


def has_dead_view_between_live(case):
    """(b) a wholly dead view between two live ones"""
    dv = dead_views(case)
    return any(bool(dv[b, n]) and not bool(dv[b, :n].all()) and not bool(dv[b, n + 1:].all())
               for b in range(case.B) for n in range(1, case.N - 1))


def has_dead_and_full_scene(case):
    """(c) a scene with no live token and a scene with all tokens live"""
    return bool((~case.mask.any(1)).any()) and bool(case.mask.all(1).any())


def has_last_partial_chunk_last_only(case):
    """(d) a last partial chunk (P % tpb != 0) whose only live token is its last"""
    tpb, chunks = S.tpb_chunks(case)
    if case.P % tpb == 0:
        return False
    return any(c == chunks - 1 and t1 - t0 >= 2 and bool(case.mask[b, t1 - 1]) and not bool(case.mask[b, t0:t1 - 1].any())
               for b, n, c, t0, t1 in workgroups(case))


def has_lone_live_token(case):
    """(e) a live token whose every neighbour in the workgroup is dead, with a neighbour on either side"""
    return any(bool(case.mask[b, t]) and not bool(case.mask[b, t - 1]) and not bool(case.mask[b, t + 1])
               for b, n, c, t0, t1 in workgroups(case) for t in range(t0 + 1, t1 - 1))


# ---- host emulation with a mask ----------------------------------------------------------------------------------------------------------
DEFECTS = ("mask_ignored", "scene0_mask_for_all", "mask_by_tl", "dead_by_first_token", "dead_wg_no_write", "dead_times_zero")


def _by_tl(case):
    """the mask a kernel sees that indexes live[] by the token's place in its workgroup instead of t0 + tl"""
    used = torch.zeros_like(case.mask)
    for b, n, c, t0, t1 in workgroups(case):
        used[b, t0:t1] = case.mask[b, :t1 - t0]
    return used


def _by_first_token(case):
    """the rows a kernel loads that calls a workgroup dead when its FIRST token is"""
    used = case.mask.clone()
    for b, n, c, t0, t1 in workgroups(case):
        if not bool(case.mask[b, t0]):
            used[b, t0:t1] = False
    return used


def applies(defect, case, subset, family):
    """whether the planted defect changes what this launch of this case computes"""
    some_dead = not bool(case.mask.all())
    return {
        "mask_ignored": some_dead,
        "scene0_mask_for_all": not torch.equal(case.mask, case.mask[:1].expand_as(case.mask)),
        "mask_by_tl": not torch.equal(_by_tl(case), case.mask),
        "dead_by_first_token": not torch.equal(_by_first_token(case), case.mask),
        "dead_wg_no_write": bool(dead_workgroups(case)),
        "dead_times_zero": some_dead,
    }[defect]


def emulate(case, vals, subset, defect=None):
    """`_repgrad_sums.emulate` (the kernel's structure in fp32 on the host) under the mask: dead rows hold NaN, as in a never-read launch,
    and the emulated kernel does not load them -- they add zero at their place in the workgroup's tree; a dead workgroup's partial and
    its per-token outputs are zeros.  ``defect``: one of DEFECTS planted."""
    used = case.mask
    if defect == "mask_ignored":
        used = torch.ones_like(case.mask)
    if defect == "scene0_mask_for_all":
        used = case.mask[:1].expand_as(case.mask)
    if defect == "mask_by_tl":
        used = _by_tl(case)
    if defect == "dead_by_first_token":
        used = _by_first_token(case)
    nan_vals = masked(case, vals, float("nan"))                              # what the buffers hold
    live = row_mask(case, used)
    loaded = [torch.where(live, x, torch.zeros((), dtype=x.dtype)) for x in nan_vals]
    if defect == "dead_times_zero":                                          # NaN * 0 is NaN
        loaded = [x * live.to(x.dtype) for x in nan_vals]
    res = S.emulate(case, loaded, subset)
    if defect == "dead_wg_no_write":                                         # the fills: a 0xFF workspace word is a NaN the finish kernel adds
        for b, n, c, t0, t1 in dead_workgroups(case):
            if "view" in subset:
                res["view"][b, n] = float("nan")
            for o in ("so2", "t2"):
                if o in subset:
                    res[o][b, t0:t1] = float("nan")
    return res


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# the bases of tests/_repgrad_sums_varlen.py: two chunks per view (h8-2c5: two pairs; h6-2c5 and h8t-2c5: three views, dead threads), H = 256
# (one workgroup per token), euclid, t2, and the key side of a cross attention; with the gaussian bases the six MASKED instances are reached
# on both kinds of data
BASES = V.BASES
GAUSS_BASES = V.GAUSS_BASES
PREFIXES = ("views", "inchunk")                           # names of `_repgrad_sums_varlen.lens_table`: the prefix masks "p-<name>"


def mask_table(N, P, tpb, seed):
    """name -> bool [2, T]"""
    T = N * P
    tv = torch.arange(T) % P                              # a token's place in its view
    tw = tv % tpb                                         # ... in its workgroup
    ntok = torch.minimum(torch.full((T,), tpb), P - (tv - tw))          # tokens of its workgroup
    last_of_view = tv == P - 1
    g = torch.Generator().manual_seed(seed)
    table = {
        # (a) every workgroup's first token dead, the rest live; only token 0 dead
        "firstdead": torch.stack([tw != 0, torch.arange(T) != 0]),
        # (c) a scene without a live token beside a scene with all of them
        "scenes": torch.stack([torch.zeros(T, dtype=torch.bool), torch.ones(T, dtype=torch.bool)]),
        # (d) the last token of each view alone: its last chunk's only live token, every other workgroup dead; the very last token alone
        "lastonly": torch.stack([last_of_view, torch.arange(T) == T - 1]),
        # (e) every third token of a view; the middle token of each workgroup
        "lone": torch.stack([tv % 3 == 1, tw == ntok // 2]),
        "bern": torch.rand(2, T, generator=g) < 0.5,
        "full": torch.ones(2, T, dtype=torch.bool),
    }
    if N >= 3:                                            # (b) a dead view between live ones; the middle views alone
        view = torch.arange(T) // P
        table["midview"] = torch.stack([view != 1, (view != 0) & (view != N - 1)])
    for name in PREFIXES:
        lens = V.lens_table(N, P, tpb)[name]
        table["p-" + name] = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    return table


def _table():
    cases = {}
    for base, names in [(b, None) for b in BASES] + [(b, ("bern", "lastonly", "p-inchunk")) for b in GAUSS_BASES]:
        for dt in ("bf16", "f32"):
            c0 = S.CASES[f"{base}-{dt}"]
            assert c0.B == 2 and all(l == "bhtd" for l in c0.lay)
            for mname, mask in mask_table(c0.N, c0.P, S.tpb_chunks(c0)[0], c0.seed).items():
                if names is not None and mname not in names:
                    continue
                c = SimpleNamespace(**vars(c0))
                c.name, c.base, c.mask, c.mask_name = f"{c0.name}@{mname}", c0.name, mask, mname
                c.prefix = V.CASES.get(f"{c0.name}@{mname[2:]}") if mname.startswith("p-") else None     # the VARLEN case of the same counts
                cases[c.name] = c
    return cases


CASES = _table()
RUNS = tuple((n, "lattice") for n in CASES) + tuple((n, "gauss") for n, c in CASES.items() if c.gauss)

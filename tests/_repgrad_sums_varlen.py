"""The rep-gradient sums with per-scene prefixes (`gta_rep_grad_sums_varlen`, the VARLEN instances of gta_repgrad.hip) as a test sees them:
tests/_repgrad_sums.py -- its fp64 reference, lattice / gaussian rules, fill and guard rules, host emulation -- with a mask.  CPU only;
tests/test_repgrad_sums_varlen_host.py proves on the CPU that every rule fails on the defect it is meant for,
tests/test_gpu_repgrad_sums_varlen.py holds the kernel to the same rules.

A varlen case is a case of `_repgrad_sums.CASES` plus ``lens`` (valid tokens of the case's side per scene, as handed to the entry, which
clamps them to 1..T).  A row (b, h, t) with t >= lens[b] is dead.  The reference is `_repgrad_sums.reference` on the values with dead rows
set to zero: zero rows add exact zero, and `addends` stays an upper bound of an element's products, so the lattice rule (exact equality)
and the gaussian rule ((n + 1) * 2^-24 * absprod) carry over unchanged.

New rules (`check`):
  dead-zero    per-token sums of dead tokens and view sums of wholly dead views are +0.0: all 32 bits zero
  never-read   the launch runs on operands whose dead rows hold NaN in every channel of every pair, and every output is finite
  live-equal   (`check_live_equal`) per-token sums of live tokens and view sums of wholly live views are, bit for bit, those of the
               unmasked entry on the same values"""
from types import SimpleNamespace

import torch

from tests import _repgrad_sums as S

OUTS = S.OUTS


def effective(case):
    """lens as the kernel uses them: clamped to 1..T"""
    T = case.N * case.P
    return tuple(min(max(int(l), 1), T) for l in case.lens)


def row_mask(case):
    """[B,1,T,1] bool: live rows"""
    T = case.N * case.P
    return (torch.arange(T)[None, :] < torch.tensor(effective(case))[:, None])[:, None, :, None]


def masked(case, vals, fill=0.0):
    """the operands with every dead row set to ``fill``"""
    m = row_mask(case)
    return [torch.where(m, x, torch.full((), fill, dtype=x.dtype)) for x in vals]


def reference(case, vals):
    return S.reference(case, masked(case, vals))


def dead_views(case):
    """[B,N] bool: views without a live token"""
    eff = torch.tensor(effective(case))
    return torch.arange(case.N)[None, :] * case.P >= eff[:, None]


def whole_views(case):
    """[B,N] bool: views whose tokens are all live"""
    eff = torch.tensor(effective(case))
    return (torch.arange(case.N)[None, :] + 1) * case.P <= eff[:, None]


def dead_tokens(case):
    return ~row_mask(case)[:, 0, :, 0]


def dead_workgroups(case):
    """[(b, n, c)] of the workgroups whose first token lies at or past the prefix"""
    tpb, chunks = S.tpb_chunks(case)
    eff = effective(case)
    return [(b, n, c) for b in range(case.B) for n in range(case.N) for c in range(chunks) if n * case.P + c * tpb >= eff[b]]


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


def check_live_equal(case, subset, res, plain):
    """live-equal: ``plain`` is the result of the unmasked entry on the same values (finite in the dead rows)"""
    for o in subset:
        live = whole_views(case) if o == "view" else ~dead_tokens(case)
        a, b = res[o].contiguous().view(torch.int32)[live], plain[o].contiguous().view(torch.int32)[live]
        assert torch.equal(a, b), (case.name, "+".join(subset), o, f"live-equal: {int((a != b).sum())} words differ from the unmasked entry")


# ---- host emulation with a mask ----------------------------------------------------------------------------------------------------------
DEFECTS = ("padded_row_read", "prefix_plus_one", "prefix_minus_one", "scene0_len_for_all", "dead_partial_at_fill", "dead_tokens_at_fill",
           "mask_pair0_only")


def applies(defect, case, subset, family):
    """whether the planted defect changes what this launch of this case computes"""
    T = case.N * case.P
    eff = effective(case)
    some_dead = any(l < T for l in eff)
    dead_wg = bool(dead_workgroups(case))
    return {
        "padded_row_read": some_dead,
        "prefix_plus_one": some_dead,
        "prefix_minus_one": any(l > 1 for l in eff),
        "scene0_len_for_all": len(set(eff)) > 1,
        "dead_partial_at_fill": dead_wg and "view" in subset,
        "dead_tokens_at_fill": dead_wg and ("so2" in subset or "t2" in subset),
        "mask_pair0_only": some_dead and case.pairs == 2,
    }[defect]


def emulate(case, vals, subset, defect=None):
    """`_repgrad_sums.emulate` (the kernel's structure in fp32 on the host) under the mask: dead rows hold NaN, as in a never-read launch,
    and the emulated kernel does not load them -- they add zero at their place in the workgroup's tree, a dead workgroup's partial and its
    per-token outputs are zeros.  ``defect``: one of DEFECTS planted."""
    T = case.N * case.P
    eff = list(effective(case))
    if defect == "prefix_plus_one":
        eff = [min(l + 1, T) for l in eff]
    if defect == "prefix_minus_one":
        eff = [max(l - 1, 1) if l > 1 else l for l in eff]
    if defect == "scene0_len_for_all":
        eff = [eff[0]] * case.B
    live = (torch.arange(T)[None, :] < torch.tensor(eff)[:, None])[:, None, :, None]
    nan_vals = masked(case, vals, float("nan"))                              # what the buffers hold
    loaded = [torch.where(live, x, torch.zeros((), dtype=x.dtype)) for x in nan_vals]
    if defect == "padded_row_read":                                          # the first dead row of the last scene that has one, head 0
        b = max(i for i, l in enumerate(effective(case)) if l < T)
        for x, src in zip(loaded, nan_vals):
            x[b, 0, effective(case)[b]] = src[b, 0, effective(case)[b]]
    if defect == "mask_pair0_only":
        loaded[2:] = nan_vals[2:]
    res = S.emulate(case, loaded, subset)
    tpb, chunks = S.tpb_chunks(case)
    for b, n, c in dead_workgroups(case):
        t0 = n * case.P + c * tpb
        t1 = min(t0 + tpb, (n + 1) * case.P)
        if defect == "dead_partial_at_fill" and "view" in subset:            # the 0xFF workspace word is a NaN, and the finish kernel adds it
            res["view"][b, n] = float("nan")
        if defect == "dead_tokens_at_fill":
            for o in ("so2", "t2"):
                if o in subset:
                    res[o][b, t0:t1] = float("nan")
    return res


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
# two chunks per view (h8-2c5: two pairs; h6-2c5: dead threads), H = 256 (one workgroup per token), euclid, t2, and the key side of a cross
# attention; with the gaussian bases the six VARLEN instances are reached on both kinds of data
BASES = ("h8-2c5", "h6-2c5", "h256", "eu-se3-9", "h8t-2c5", "cross-k")
GAUSS_BASES = ("g-vec", "g-2chunk", "g-euclid", "g-so2-12")


def lens_table(N, P, tpb):
    """name -> (lens of scene 0, of scene 1)"""
    T = N * P
    inside = max(1, min(P, tpb) // 2)
    table = {
        "views": (P, T),                                   # whole views: what the Python layer passes
        "full": (T, T),                                    # nothing padded
        "one": (1, P + 1),                                 # a single live row; one row into the second view
        "inchunk": (inside, P + inside + 1),               # a prefix that ends inside a chunk
        "viewedge": ((N - 1) * P, P),                      # ... exactly on a view edge
        "clamp": (0, T + 5),                               # clamped to 1 and T
    }
    if tpb < P:
        table["chunkedge"] = (tpb, P + tpb)                # ... exactly on a chunk edge
    return table


def _table():
    cases = {}
    for base, names in [(b, None) for b in BASES] + [(b, ("views", "inchunk", "clamp")) for b in GAUSS_BASES]:
        for dt in ("bf16", "f32"):
            c0 = S.CASES[f"{base}-{dt}"]
            assert c0.B == 2 and all(l == "bhtd" for l in c0.lay)
            seen = set()
            for lname, lens in lens_table(c0.N, c0.P, S.tpb_chunks(c0)[0]).items():
                if (names is not None and lname not in names) or lens in seen:
                    continue
                seen.add(lens)
                c = SimpleNamespace(**vars(c0))
                c.name, c.base, c.lens, c.lens_name = f"{c0.name}@{lname}", c0.name, lens, lname
                cases[c.name] = c
    return cases


CASES = _table()
RUNS = tuple((n, "lattice") for n in CASES) + tuple((n, "gauss") for n, c in CASES.items() if c.gauss)

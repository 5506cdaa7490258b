"""CPU: the rep-gradient sums under a per-token mask, without a GPU.
  * the rules of tests/_repgrad_sums_masked.py bite: the host emulation under the mask passes every rule on every case and launch (live-equal
    and prefix-equal included), and each planted mask defect fails them on every launch it applies to;
  * the masks of the table contain what the MASKED instances can get wrong (a) - (e);
  * `gta_rep_grad_sums_masked` is declared, listed, exported and bound, refuses a NULL ``live`` and answers every refusal row of
    `gta_rep_grad_sums` (tests/test_abi_refusals.py) alike."""
import ctypes
import functools
import os
import re

import pytest
import torch

from gta_amd import native
from tests import _repgrad_sums as S
from tests import _repgrad_sums_masked as M
from tests import _repgrad_sums_varlen as V
from tests import test_abi_refusals as R


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """the tensors here are tiny: on many intra-op threads the emulation is ten times slower than on one"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _data(name, family):
    case = M.CASES[name]
    vals = S.values(case, family)
    return case, vals, M.reference(case, vals)


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, family", M.RUNS, ids=lambda v: v)
def test_emulation_passes_every_rule(name, family):
    case, vals, ref = _data(name, family)
    zeroed = M.masked(case, vals)
    for subset in S.subsets(case):
        res = M.emulate(case, vals, subset)
        worst = M.check(case, subset, family, res, ref)                       # fp64 rules, never-read (NaN in the dead rows), dead-zero
        assert (family == "gauss") == bool(worst)
        M.check_same_bits(case, subset, res, S.emulate(case, zeroed, subset), "live-equal")
        if case.mask_name.startswith("p-"):
            assert case.prefix is not None and torch.equal(case.mask, V.row_mask(case.prefix)[:, 0, :, 0]), name
            M.check_same_bits(case, subset, res, V.emulate(case.prefix, vals, subset), "prefix-equal")


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_planted_defect_fails_its_rule(defect):
    hit, missed = [], []
    for name, family in M.RUNS:
        case, vals, ref = _data(name, family)
        for subset in S.subsets(case):
            if not M.applies(defect, case, subset, family):
                continue
            hit.append((name, subset, family))
            try:
                M.check(case, subset, family, M.emulate(case, vals, subset, defect), ref)
            except AssertionError:
                continue
            missed.append((name, subset, family))
    assert hit and not missed, (defect, len(hit), missed)
    assert {f for _, _, f in hit} == {"lattice", "gauss"}


def test_each_defect_fails_the_rule_meant_for_it():
    """which rule answers: the fill rule (never-read) for what reads a dead row or leaves a dead workgroup's words, the fp64 rule for
    what drops a live row"""
    case, vals, ref = _data("h8-2c5-bf16@firstdead", "lattice")
    subset = S.subsets(case)[-1]
    for defect, text in (("mask_ignored", "not finite"), ("dead_times_zero", "not finite"), ("dead_by_first_token", "elements differ")):
        with pytest.raises(AssertionError, match=text):
            M.check(case, subset, "lattice", M.emulate(case, vals, subset, defect), ref)
    case, vals, ref = _data("h8-2c5-bf16@lastonly", "lattice")
    with pytest.raises(AssertionError, match="not finite"):
        M.check(case, subset, "lattice", M.emulate(case, vals, subset, "dead_wg_no_write"), ref)
    # a mask taken from the wrong place reads a dead (NaN) row or drops a live one: either rule may answer first
    for defect in ("scene0_mask_for_all", "mask_by_tl"):
        with pytest.raises(AssertionError, match="not finite|elements differ"):
            M.check(case, subset, "lattice", M.emulate(case, vals, subset, defect), ref)


def test_dead_zero_and_same_bits_bite():
    """the rules no mask defect above reaches: a negative zero at a dead entry, and a word that differs from the other entry's"""
    case, vals, ref = _data("h6-2c5-bf16@midview", "lattice")
    subset = S.subsets(case)[-1]
    res = M.emulate(case, vals, subset)
    plain = S.emulate(case, M.masked(case, vals), subset)
    M.check(case, subset, "lattice", res, ref)
    for o in subset:
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}
        where = M.dead_views(case) if o == "view" else M.dead_tokens(case)
        i = tuple(where.nonzero()[0].tolist())
        bad[o][i] = -0.0
        with pytest.raises(AssertionError, match="dead-zero"):
            M.check(case, subset, "lattice", bad, ref)
        with pytest.raises(AssertionError, match="live-equal"):                # -0.0 at a dead entry: the unmasked entry gives +0.0 there
            M.check_same_bits(case, subset, bad, plain, "live-equal")
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}
        i = tuple((~where).nonzero()[0].tolist())
        bad[o][i] += 0.25
        with pytest.raises(AssertionError, match="prefix-equal"):
            M.check_same_bits(case, subset, bad, plain, "prefix-equal")


def test_masks_contain_what_the_kernel_can_get_wrong():
    cases = list(M.CASES.values())
    for what in (M.has_first_dead_later_live, M.has_dead_view_between_live, M.has_dead_and_full_scene,
                 M.has_last_partial_chunk_last_only, M.has_lone_live_token):
        have = [c.name for c in cases if what(c)]
        assert have, what.__name__
        # ... in both dtypes, on lattice data and on gaussian data where the mask family is run on both
        assert {n.split("@")[0].rsplit("-", 1)[1] for n in have} == {"bf16", "f32"}, (what.__name__, have)
    # (a) and (d) in a launch with two chunks per view and two pairs, and with dead threads (H = 6)
    for what in (M.has_first_dead_later_live, M.has_last_partial_chunk_last_only, M.has_lone_live_token):
        assert any(what(c) and c.pairs == 2 and S.tpb_chunks(c)[1] >= 2 for c in cases), what.__name__
        assert any(what(c) and c.H == 6 for c in cases), what.__name__
    assert any(M.has_last_partial_chunk_last_only(c) and c.gauss for c in cases)
    # dead workgroups beside live ones in one launch, a launch without a dead token, and every prefix mask has its VARLEN case
    assert any(M.dead_workgroups(c) and len(M.dead_workgroups(c)) < len(M.workgroups(c)) for c in cases)
    assert any(bool(c.mask.all()) for c in cases)
    assert all(c.prefix is not None for c in cases if c.mask_name.startswith("p-")) and any(c.prefix is not None for c in cases)
    B = [S.CASES[f"{b}-bf16"] for b in M.BASES]
    assert any(c.H == 256 for c in B) and any(c.euclid for c in B) and any(S.slabs(c.f_dims, c.euclid).n_t2 for c in B)
    assert any(c.side == 1 and c.other != (c.N, c.P) for c in B)
    # both kinds of data reach the six MASKED instances (the twins of the instances `_repgrad_sums.instance` reads from vec_ok)
    for family in ("lattice", "gauss"):
        inst = {S.instance(M.CASES[n], sub) for n, f in M.RUNS if f == family for sub in S.subsets(M.CASES[n])}
        assert len(inst) == 6, (family, inst)
    assert all(tuple(c.mask.shape) == (c.B, c.N * c.P) and c.mask.dtype == torch.bool and c.N * c.P <= 600 for c in cases)


def test_reference_is_the_sum_over_live_rows():
    case, vals, ref = _data("h6-2c5-f32@bern", "lattice")
    s = S.slabs(case.f_dims)
    a, b = vals[0], vals[1]
    for bi in range(case.B):
        want = torch.zeros(case.N, 4, 4, dtype=torch.float64)
        for t in case.mask[bi].nonzero().flatten().tolist():
            for g in range(s.n_se3):
                x, y = a[bi, :, t, s.off_se3 + 4 * g:s.off_se3 + 4 * g + 4], b[bi, :, t, s.off_se3 + 4 * g:s.off_se3 + 4 * g + 4]
                want[t // case.P] += torch.einsum("hi,hj->ij", x, y)
        assert torch.equal(ref["view"][0][bi], want)
        assert bool((ref["so2"][0][bi][~case.mask[bi]] == 0).all()) and bool((ref["so2"][0][bi][case.mask[bi]] != 0).any())


# ---- the entry ---------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_exported_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gta_hip.h")).read()
    m = re.search(r"^int gta_rep_grad_sums_masked\(([^;]*)\);", header, re.M)
    assert m, "gta_rep_grad_sums_masked is not declared in include/gta_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names[names.index("live") + 1] == "view_sums" and params[names.index("live")] == "const uint8_t* live"    # in front of the outputs
    varlen = re.search(r"^int gta_rep_grad_sums_varlen\(([^;]*)\);", header, re.M).group(1).replace("\n", " ")
    assert [p.strip() for p in varlen.split(",")] == [p if not p.endswith(" live") else "const int32_t* lens" for p in params]
    assert "gta_rep_grad_sums_masked" in native.ABI_SYMBOLS
    L = native.lib()
    assert hasattr(L, "gta_rep_grad_sums_masked")
    assert len(L.gta_rep_grad_sums_masked.argtypes) == len(L.gta_rep_grad_sums.argtypes) + 1 == len(params)
    assert L.gta_abi_version() == 2
    for word in ("Never-read", "Dead-zero", "Live-equal", "one OR over the whole workgroup"):
        assert word in header, word


def _masked(desc, live=R.X, **args):
    st = R._strides(R.H * R.TQ * 64, R.TQ * 64, 64)
    full = dict(side=0, n_pairs=2, a0=R.X, b0=R.X, a1=R.X, b1=R.X, a0_stride=st, b0_stride=st, a1_stride=st, b1_stride=st, view_sums=R.X,
                so2_sums=R.X, t2_sums=None, workspace=R.X, workspace_bytes=R.BIG, stream=None)
    full.update(args)
    vals = [full[name] for name in R.REPGRAD_ARGS]
    vals.insert(R.REPGRAD_ARGS.index("view_sums"), live)
    return native.lib().gta_rep_grad_sums_masked(None if desc is None else ctypes.byref(desc), *vals)


REFUSAL_ROWS = R.test_rep_grad_sums_refusal.pytestmark[0].args[1]


@pytest.mark.parametrize("desc, args, code, text", REFUSAL_ROWS)
def test_every_refusal_of_the_unmasked_entry(desc, args, code, text):
    if desc is not None:
        desc = dict(desc)
        raw = desc.pop("dtype_", None)
        desc = R._desc(**desc)
        if raw is not None:
            desc.dtype = raw
    rc = _masked(desc, **args)
    assert rc == code == R._rep_grad(desc, **args), (rc, native.lib().gta_strerror(rc).decode())
    assert text in native.lib().gta_strerror(rc).decode()


def test_null_live_is_refused_before_any_launch():
    assert len(REFUSAL_ROWS) >= 20
    rc = _masked(R._desc(), live=None)           # (placeholder operands nothing may read: a launch would fault, not return)
    assert rc == R.BADARG and "live" in native.lib().gta_strerror(rc).decode()
    for side in (0, 1):
        rc = _masked(R._desc(), live=None, side=side, n_pairs=1, view_sums=None, workspace=None, workspace_bytes=0)
        assert rc == R.BADARG and "live" in native.lib().gta_strerror(rc).decode()

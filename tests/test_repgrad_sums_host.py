"""CPU proof that the rules of tests/_repgrad_sums.py bite: a host emulation of the structure of `gta_rep_grad_sums` (fp32 row sums per
(token, head), the workgroup tree, the finish sum, head-order per-token sums) passes every rule on every case and launch, and each planted
defect fails them on every launch it applies to.  Also the conditions the rules rest on (64 n < 2^24 per lattice case, n <= 1024 per
gaussian case), the reference against a naive loop, and the shape of the case table."""
import functools
import itertools
from types import SimpleNamespace

import pytest
import torch

from tests import _repgrad_sums as S


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """the tensors here are tiny: on many intra-op threads the emulation is ten times slower than on one"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _data(name, family):
    case = S.CASES[name]
    vals = S.values(case, family)
    return case, vals, S.reference(case, vals)


@pytest.mark.parametrize("name, family", S.RUNS, ids=lambda v: v)
def test_emulation_passes_every_rule(name, family):
    case, vals, ref = _data(name, family)
    for subset in S.subsets(case):
        worst = S.check(case, subset, family, S.emulate(case, vals, subset), ref)
        assert (family == "gauss") == bool(worst)


@pytest.mark.parametrize("defect", S.DEFECTS)
def test_planted_defect_fails_its_rule(defect):
    hit, missed = [], []
    for name, family in S.RUNS:
        case, vals, ref = _data(name, family)
        for subset in S.subsets(case):
            if not S.applies(defect, case, subset, family):
                continue
            hit.append((name, subset, family))
            try:
                S.check(case, subset, family, S.emulate(case, vals, subset, defect), ref)
            except AssertionError:
                continue
            missed.append((name, subset, family))
    assert hit and not missed, (defect, len(hit), missed)
    if defect == "dead_threads_live":
        assert any(S.CASES[n].H == 6 for n, _, _ in hit)
    if defect == "partial_bf16":                       # every gaussian case shows that the bound catches a bf16 partial
        assert {n for n, _, _ in hit} == set(S.GAUSS)
    if defect == "second_pass_at_f0_0":                # nf = 4, 8 and 1 on the second trip
        assert {S.slabs(S.CASES[n].f_dims).n_so2 for n, _, _ in hit} >= {9, 12, 16}


def test_conditions_of_the_rules():
    for name, case in S.CASES.items():
        assert S.exact_ok(case), name
        n = S.addends(case)
        s = S.slabs(case.f_dims, case.euclid)
        assert n["view"] == case.pairs * case.H * case.P * s.n_se3 and n["so2"] == case.pairs * case.H
        assert case.B <= 2 and case.N * case.P <= 600
        if case.gauss:
            assert 0 < n["view"] <= 1024, (name, n)
    assert 6 <= len(S.GAUSS) <= 10


def test_lattice_values_are_quarters_and_survive_the_dtype():
    for name in ("h6-2c5-bf16", "st-h0-f32", "g-euclid-bf16"):
        case = S.CASES[name]
        for x in S.values(case, "lattice"):
            k = x * 4
            assert bool((k == k.round()).all()) and k.abs().max().item() <= 8
            assert torch.equal(x.to(case.dtype).double(), x)
        for x in S.values(case, "gauss"):
            assert torch.equal(x.to(case.dtype).double(), x)                       # the reference sees the rounded operands


def test_table_reaches_every_path():
    C = S.CASES.values()
    assert {c.H for c in C} >= {1, 3, 5, 6, 8, 256}
    edges = set()
    for c in C:
        tpb, chunks = S.tpb_chunks(c)
        edges |= {"short"} if c.P < tpb else {"full"} if c.P == tpb else {"plus1"} if c.P == tpb + 1 else set()
        edges |= {"2c5"} if c.P == 2 * tpb + 5 else set()
    assert edges == {"short", "full", "plus1", "2c5"}
    sl = [(c, S.slabs(c.f_dims, c.euclid)) for c in C]
    assert {s.n_se3 for c, s in sl if not c.euclid and s.off_se3 % 8 == 0} >= {1, 2, 3, 8}
    assert any(s.off_se3 == 4 for c, s in sl) and {s.n_se3 for c, s in sl if c.euclid} >= {1, 3}
    assert {s.n_so2 for c, s in sl if s.off_so2 % 8 == 0} >= {1, 3, 4, 8, 9, 12, 16}
    assert any(s.n_so2 and s.off_so2 % 8 for c, s in sl)
    assert {s.n_t2 for c, s in sl} >= {1, 2} and any(S.subsets(c) == [("t2",)] for c in C)
    assert {c.pairs for c in C} == {1, 2} and any(c.pairs == 2 and c.lay[:2] != c.lay[2:] for c in C)
    assert {l for c in C for l in c.lay[:2 * c.pairs]} >= {"bhtd", "bthd", "packed1", "h0", "b0", "choff", "pad2"}
    assert {c.side for c in C if c.other != (c.N, c.P)} == {0, 1}
    assert {c.dtype for c in C} == {S.BF16, S.F32}
    # the instances vec_ok is read to select: all six on gaussian data, each dtype's three on lattice data under every output subset
    inst = {S.instance(S.CASES[n], sub) for n in S.GAUSS for sub in S.subsets(S.CASES[n])}
    assert inst == set(itertools.product((2, 4), (False,), (True, False))) | {(2, True, False), (4, True, False)}
    # a misaligned base pointer or token stride alone must cost the 16-byte form
    for n in ("st-choff", "st-pad2", "p2-choff"):
        for dt in ("bf16", "f32"):
            assert S.instance(S.CASES[f"{n}-{dt}"], ("view", "so2"))[2] is False
    for n in ("st-bhtd", "st-bthd", "st-packed", "st-pad8", "st-h0", "st-b0", "p2-mixed"):
        for dt in ("bf16", "f32"):
            assert S.instance(S.CASES[f"{n}-{dt}"], ("view", "so2"))[2] is True


def test_placed_operands_hold_the_values_under_the_layouts_strides():
    case = S.CASES["p2-choff-bf16"]
    vals = S.values(case, "lattice")
    ops = [S.place(x, lay, case.dtype) for x, lay in zip(vals, case.lay)]
    for x, t in zip(vals, ops):
        assert t.stride(3) == 1 and torch.equal(t.double(), x)
    assert ops[2].stride()[:3] == (33 * 2 * 8 * 16, 16, 8 * 16) and ops[3].storage_offset() == 1 and ops[3].stride(2) == 24
    for lay, st in (("h0", 1), ("b0", 0)):
        c = S.CASES[f"st-{lay}-f32"]
        v = S.values(c, "lattice")
        i = c.lay.index(lay)
        t = S.place(v[i], lay, c.dtype)
        assert t.stride(st) == 0 and torch.equal(t.double(), v[i])
    t = S.place(S.values(S.CASES["st-packed-f32"], "lattice")[0], "packed1", S.F32)
    assert t.stride()[:3] == (66 * 3 * 8 * 16, 16, 3 * 8 * 16) and t.storage_offset() == 8 * 16


def test_reference_against_a_naive_loop():
    for euclid in (False, True):
        f = {"triv": 1, "se3": 6 if euclid else 8, "so2": 4, "t2": 6}
        case = SimpleNamespace(name="tiny", B=2, H=2, N=2, P=2, f_dims=f, euclid=euclid, dtype=S.F32, pairs=2, lay=("bhtd",) * 4, seed=5)
        vals = S.values(case, "gauss")
        ref = S.reference(case, vals)
        s = S.slabs(f, euclid)
        view, so2, t2 = torch.zeros(2, 2, 4, 4).double(), torch.zeros(2, 4, s.n_so2, 2, 2).double(), torch.zeros(2, 4, 3, 3).double()
        aview = torch.zeros_like(view)
        for p, b, h, t in itertools.product(range(2), range(2), range(2), range(4)):
            x, y = vals[2 * p][b, h, t], vals[2 * p + 1][b, h, t]
            for g in range(s.n_se3):
                xs = x[s.off_se3 + g * s.W:s.off_se3 + (g + 1) * s.W].tolist() + ([0.0] if euclid else [])
                ys = y[s.off_se3 + g * s.W:s.off_se3 + (g + 1) * s.W].tolist() + ([1.0] if euclid else [])
                for i, j in itertools.product(range(4), range(4)):
                    view[b, t // 2, i, j] += xs[i] * ys[j]
                    aview[b, t // 2, i, j] += abs(xs[i]) * abs(ys[j])
            for g in range(s.n_so2):
                for i, j in itertools.product(range(2), range(2)):
                    so2[b, t, g, i, j] += x[s.off_so2 + 2 * g + i] * y[s.off_so2 + 2 * g + j]
            for g in range(s.n_t2):
                for i, j in itertools.product(range(3), range(3)):
                    t2[b, t, i, j] += x[s.off_t2 + 3 * g + i] * y[s.off_t2 + 3 * g + j]
        for got, want in ((ref["view"][0], view), (ref["view"][1], aview), (ref["so2"][0], so2), (ref["t2"][0], t2)):
            assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())
        assert ref["view"][2] == 2 * 2 * 2 * s.n_se3 and ref["so2"][2] == 4 and ref["t2"][2] == 2 * 2 * s.n_t2
        if euclid:
            assert bool((ref["view"][0][..., 3, :] == 0).all()) and bool((ref["view"][1][..., 3, :] == 0).all())


def test_workspace_bytes_match_the_library():
    import ctypes
    from gta_amd import native
    for case in S.CASES.values():
        Nq, Pq = (case.N, case.P) if case.side == 0 else case.other
        Nk, Pk = case.other if case.side == 0 else (case.N, case.P)
        dh = S.slabs(case.f_dims, case.euclid).dh
        d = native.make_desc_from(case.dtype, (case.B, case.H, Nq * Pq, dh), Nk * Pk, [(0, 0, 0)] * 4, case.f_dims, 0, Nq, Nk, 1.0,
                                  native.FLAG_EUCLID if case.euclid else 0)
        tpb, chunks = S.tpb_chunks(case)
        assert native.lib().gta_rep_grad_workspace_bytes(ctypes.byref(d), case.side) == case.B * case.N * chunks * 64 == S.workspace_bytes(case)

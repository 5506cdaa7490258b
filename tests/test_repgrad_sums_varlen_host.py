"""CPU: the masked rep-gradient sums and the algebra behind them, without a GPU.
  * the rules of tests/_repgrad_sums_varlen.py bite: the host emulation under the mask passes every rule on every case and launch, and each
    planted mask defect fails them on every launch it applies to;
  * `gta_rep_grad_sums_varlen` is declared, listed, exported and bound, refuses a NULL ``lens`` and answers every refusal row of
    `gta_rep_grad_sums` (tests/test_abi_refusals.py) alike;
  * `gta_amd.repgrad`: view_grad, so2_grad with so2_packed, extrinsic_grad and coord_grad give exact zeros at padded entries whatever the
    tables hold there (0.0, 0.5, NaN, Inf), raise nothing, and at live entries return the bits of the call on the live slice alone."""
import ctypes
import functools
import os
import re

import pytest
import torch

from gta_amd import native, repgrad
from tests import _repgrad_sums as S
from tests import _repgrad_sums_varlen as V
from tests import test_abi_refusals as R

FILLS = (0.0, 0.5, float("nan"), float("inf"))


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """the tensors here are tiny: on many intra-op threads the emulation is ten times slower than on one"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _data(name, family):
    case = V.CASES[name]
    vals = S.values(case, family)
    return case, vals, V.reference(case, vals)


# ---- the rules ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, family", V.RUNS, ids=lambda v: v)
def test_emulation_passes_every_rule(name, family):
    case, vals, ref = _data(name, family)
    plain_vals = S.values(case, family)
    for subset in S.subsets(case):
        res = V.emulate(case, vals, subset)
        worst = V.check(case, subset, family, res, ref)
        assert (family == "gauss") == bool(worst)
        V.check_live_equal(case, subset, res, S.emulate(case, plain_vals, subset))


@pytest.mark.parametrize("defect", V.DEFECTS)
def test_planted_defect_fails_its_rule(defect):
    hit, missed = [], []
    for name, family in V.RUNS:
        case, vals, ref = _data(name, family)
        for subset in S.subsets(case):
            if not V.applies(defect, case, subset, family):
                continue
            hit.append((name, subset, family))
            try:
                V.check(case, subset, family, V.emulate(case, vals, subset, defect), ref)
            except AssertionError:
                continue
            missed.append((name, subset, family))
    assert hit and not missed, (defect, len(hit), missed)
    assert {f for _, _, f in hit} == {"lattice", "gauss"}


def test_dead_zero_and_live_equal_bite():
    """the two rules no mask defect above reaches: a negative zero at a dead entry, and a live word that differs from the unmasked entry"""
    case, vals, ref = _data("h8-2c5-bf16@views", "lattice")
    subset = S.subsets(case)[-1]
    res = V.emulate(case, vals, subset)
    plain = S.emulate(case, S.values(case, "lattice"), subset)
    V.check(case, subset, "lattice", res, ref)
    V.check_live_equal(case, subset, res, plain)
    for o in subset:
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}
        where = V.dead_views(case) if o == "view" else V.dead_tokens(case)
        i = tuple(where.nonzero()[0].tolist())
        bad[o][i] = -0.0
        with pytest.raises(AssertionError, match="dead-zero"):
            V.check(case, subset, "lattice", bad, ref)
        bad = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in res.items()}
        live = V.whole_views(case) if o == "view" else ~V.dead_tokens(case)
        i = tuple(live.nonzero()[0].tolist())
        bad[o][i] += 0.25
        with pytest.raises(AssertionError, match="live-equal"):
            V.check_live_equal(case, subset, bad, plain)


def test_table_covers_the_prefixes_the_kernel_can_get_wrong():
    for base in V.BASES:
        for dt in ("bf16", "f32"):
            mine = [c for c in V.CASES.values() if c.base == f"{base}-{dt}"]
            c0 = mine[0]
            T, (tpb, chunks) = c0.N * c0.P, S.tpb_chunks(c0)
            lens = {c.lens for c in mine}
            assert {(c0.P, T), (T, T), (1, c0.P + 1), (0, T + 5), ((c0.N - 1) * c0.P, c0.P)} <= lens, base
            # (H = 256: one token per workgroup, so no prefix ends inside a chunk)
            assert tpb == 1 or any(l % c0.P % tpb for ls in lens for l in ls), base                        # ends inside a chunk
            assert any(l % c0.P and l % c0.P % tpb == 0 for ls in lens for l in ls) or tpb >= c0.P, base   # on a chunk edge inside a view
            # a straddling workgroup and a wholly dead one, in the same launch
            assert tpb == 1 or any(V.dead_workgroups(c) and any(l % c.P % tpb for l in V.effective(c)) for c in mine), base
    B = [S.CASES[f"{b}-bf16"] for b in V.BASES]
    assert any(S.tpb_chunks(c)[1] >= 2 and c.pairs == 2 for c in B) and any(c.H == 6 and S.tpb_chunks(c)[1] >= 2 for c in B)
    assert any(c.H == 256 for c in B) and any(c.euclid for c in B) and any(S.slabs(c.f_dims, c.euclid).n_t2 for c in B)
    assert any(c.side == 1 and c.other != (c.N, c.P) for c in B)
    # both kinds of data reach the six VARLEN instances (the twins of the instances `_repgrad_sums.instance` reads from vec_ok)
    for family in ("lattice", "gauss"):
        inst = {S.instance(V.CASES[n], sub) for n, f in V.RUNS if f == family for sub in S.subsets(V.CASES[n])}
        assert len(inst) == 6, (family, inst)
    assert all(V.effective(c) == tuple(min(max(l, 1), c.N * c.P) for l in c.lens) for c in V.CASES.values())
    assert all(c.N * c.P <= 600 and c.B == 2 for c in V.CASES.values())


def test_reference_is_the_sum_over_live_rows():
    case, vals, ref = _data("h6-2c5-f32@inchunk", "lattice")
    eff = V.effective(case)
    s = S.slabs(case.f_dims)
    a, b = vals[0], vals[1]
    for bi in range(case.B):
        want = torch.zeros(case.N, 4, 4, dtype=torch.float64)
        for t in range(eff[bi]):
            for g in range(s.n_se3):
                x, y = a[bi, :, t, s.off_se3 + 4 * g:s.off_se3 + 4 * g + 4], b[bi, :, t, s.off_se3 + 4 * g:s.off_se3 + 4 * g + 4]
                want[t // case.P] += torch.einsum("hi,hj->ij", x, y)
        assert torch.equal(ref["view"][0][bi], want)
        assert bool((ref["so2"][0][bi, eff[bi]:] == 0).all()) and bool((ref["so2"][0][bi, :eff[bi]] != 0).any())


# ---- the entry ---------------------------------------------------------------------------------------------------------------------------
def test_entry_is_declared_listed_exported_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "gta_hip.h")).read()
    m = re.search(r"^int gta_rep_grad_sums_varlen\(([^;]*)\);", header, re.M)
    assert m, "gta_rep_grad_sums_varlen is not declared in include/gta_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names[names.index("lens") + 1] == "view_sums" and params[names.index("lens")] == "const int32_t* lens"    # in front of the outputs
    plain = re.search(r"^int gta_rep_grad_sums\(([^;]*)\);", header, re.M).group(1).replace("\n", " ")
    assert [p.strip() for p in plain.split(",")] == [p for p in params if not p.endswith(" lens")]
    assert "gta_rep_grad_sums_varlen" in native.ABI_SYMBOLS
    L = native.lib()
    assert hasattr(L, "gta_rep_grad_sums_varlen")
    assert len(L.gta_rep_grad_sums_varlen.argtypes) == len(L.gta_rep_grad_sums.argtypes) + 1 == len(params)
    assert L.gta_abi_version() == 2


def _varlen(desc, lens=R.X, **args):
    st = R._strides(R.H * R.TQ * 64, R.TQ * 64, 64)
    full = dict(side=0, n_pairs=2, a0=R.X, b0=R.X, a1=R.X, b1=R.X, a0_stride=st, b0_stride=st, a1_stride=st, b1_stride=st, view_sums=R.X,
                so2_sums=R.X, t2_sums=None, workspace=R.X, workspace_bytes=R.BIG, stream=None)
    full.update(args)
    vals = [full[name] for name in R.REPGRAD_ARGS]
    vals.insert(R.REPGRAD_ARGS.index("view_sums"), lens)
    return native.lib().gta_rep_grad_sums_varlen(None if desc is None else ctypes.byref(desc), *vals)


REFUSAL_ROWS = R.test_rep_grad_sums_refusal.pytestmark[0].args[1]


@pytest.mark.parametrize("desc, args, code, text", REFUSAL_ROWS)
def test_every_refusal_of_the_unmasked_entry(desc, args, code, text):
    if desc is not None:
        desc = dict(desc)
        raw = desc.pop("dtype_", None)
        desc = R._desc(**desc)
        if raw is not None:
            desc.dtype = raw
    rc = _varlen(desc, **args)
    assert rc == code == R._rep_grad(desc, **args), (rc, native.lib().gta_strerror(rc).decode())
    assert text in native.lib().gta_strerror(rc).decode()


def test_null_lens_is_refused_before_any_launch():
    assert len(REFUSAL_ROWS) >= 20
    rc = _varlen(R._desc(), lens=None)           # (placeholder operands nothing may read: a launch would fault, not return)
    assert rc == R.BADARG and "lens" in native.lib().gta_strerror(rc).decode()
    for side in (0, 1):
        rc = _varlen(R._desc(), lens=None, side=side, n_pairs=1, view_sums=None, workspace=None, workspace_bytes=0)
        assert rc == R.BADARG and "lens" in native.lib().gta_strerror(rc).decode()


# ---- the algebra at padded entries ---------------------------------------------------------------------------------------------------------
B_, N_, P_, NB = 3, 4, 5, 3
VIEWS = (2, 4, 1)


def _rot(g, *shape):
    th = torch.rand(*shape, generator=g, dtype=torch.float64) * 6.28
    return torch.stack([torch.cos(th), torch.sin(th)], -1).float()


def _poses(g, *shape):
    E = torch.eye(4).repeat(*shape, 1, 1)
    E[..., :3, :] += 0.3 * torch.randn(*shape, 3, 4, generator=g)
    return E


def _vrep(E):
    v = torch.zeros(*E.shape[:-2], native.VREP_STRIDE)
    v[..., repgrad.INV] = torch.linalg.inv(E.double()).float().flatten(-2)
    v[..., repgrad.REP] = E.flatten(-2)
    return v


@pytest.mark.parametrize("fill", FILLS, ids=str)
@pytest.mark.parametrize("side", [0, 1])
def test_view_grad_at_padded_views(side, fill):
    g = torch.Generator().manual_seed(3)
    live = repgrad.live_mask(VIEWS, N_, 1, "cpu")
    assert live.tolist() == [[n < v for n in range(N_)] for v in VIEWS]
    vrep = torch.where(live[..., None], _vrep(_poses(g, B_, N_)), torch.full((), fill))
    Ssum = torch.where(live[..., None, None], torch.randn(B_, N_, 4, 4, generator=g), torch.zeros(()))
    got = repgrad.view_grad(side, Ssum, vrep, 0.3, False, live=live)
    assert got.shape == (B_, N_, native.VREP_STRIDE) and bool(torch.isfinite(got).all())
    assert bool((got[~live] == 0).all())
    for b, n in enumerate(VIEWS):
        assert torch.equal(got[b, :n], repgrad.view_grad(side, Ssum[b:b + 1, :n], vrep[b:b + 1, :n], 0.3, False)[0])


@pytest.mark.parametrize("fill", FILLS, ids=str)
@pytest.mark.parametrize("side", [0, 1])
def test_so2_grad_at_padded_tokens(side, fill):
    g = torch.Generator().manual_seed(4)
    live = repgrad.live_mask(VIEWS, N_, P_, "cpu")
    assert live.shape == (B_, N_ * P_) and live.sum(1).tolist() == [v * P_ for v in VIEWS]
    cs = torch.where(live[..., None, None], _rot(g, B_, N_ * P_, NB), torch.full((), fill))
    Tsum = torch.where(live[..., None, None, None], torch.randn(B_, N_ * P_, NB, 2, 2, generator=g), torch.zeros(()))
    dR = repgrad.so2_grad(side, Tsum, cs, False, live=live)
    dcs = repgrad.so2_packed(dR, live)
    for got in (dR, dcs):
        assert bool(torch.isfinite(got).all()) and bool((got[~live] == 0).all())
    for b, n in enumerate(VIEWS):
        alone = repgrad.so2_grad(side, Tsum[b:b + 1, :n * P_], cs[b:b + 1, :n * P_], False)
        assert torch.equal(dR[b, :n * P_], alone[0]) and torch.equal(dcs[b, :n * P_], repgrad.so2_packed(alone)[0])
    # a gradient that is not zero at a padded token is still selected out, not multiplied by zero
    assert bool((repgrad.so2_packed(torch.full((B_, N_ * P_, NB, 2, 2), float("nan"), dtype=torch.float64), live)[~live] == 0).all())
    assert bool((repgrad.t2_packed(side, torch.full((B_, N_ * P_, 3, 3), float("inf"), dtype=torch.float64), live)[~live] == 0).all())


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_extrinsic_grad_at_padded_views(fill):
    g = torch.Generator().manual_seed(5)
    live = repgrad.live_mask(VIEWS, N_, 1, "cpu")
    E = torch.where(live[..., None, None], _poses(g, B_, N_), torch.full((), fill))
    dvrep = torch.where(live[..., None], torch.randn(B_, N_, native.VREP_STRIDE, generator=g), torch.zeros(()))
    got = repgrad.extrinsic_grad(E, dvrep)
    assert got.shape == (B_, N_, 4, 4) and bool(torch.isfinite(got).all()) and bool((got[~live] == 0).all())
    for b, n in enumerate(VIEWS):
        assert torch.equal(got[b, :n], repgrad.extrinsic_grad(E[b:b + 1, :n], dvrep[b:b + 1, :n])[0])
    # through the builders' autograd functions, as a model's backward reaches it
    Eg = E.clone().requires_grad_(True)
    dE = repgrad.ViewReps.backward(type("ctx", (), {"saved_tensors": (Eg,)})(), dvrep)[0]
    assert dE.dtype == E.dtype and bool((dE[~live] == 0).all()) and bool(torch.isfinite(dE).all())


@pytest.mark.parametrize("fill", FILLS, ids=str)
def test_coord_grad_at_padded_tokens(fill):
    g = torch.Generator().manual_seed(6)
    live = repgrad.live_mask(VIEWS, N_, P_, "cpu")
    nf = 4
    coord = torch.where(live[..., None], torch.rand(B_, N_ * P_, 2, generator=g), torch.full((), fill))
    dcs = torch.where(live[..., None, None], torch.randn(B_, N_ * P_, 2 * nf, 2, generator=g), torch.zeros(()))
    for shared in (False, True):
        got = repgrad.coord_grad(coord, dcs, nf, 1.0, 2.0, shared)
        assert got.shape == (B_, N_ * P_, 2) and bool(torch.isfinite(got).all()) and bool((got[~live] == 0).all())
        for b, n in enumerate(VIEWS):
            assert torch.equal(got[b, :n * P_], repgrad.coord_grad(coord[b:b + 1, :n * P_], dcs[b:b + 1, :n * P_], nf, 1.0, 2.0, shared)[0])
        assert bool((got[live] != 0).any())

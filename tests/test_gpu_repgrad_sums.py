"""GPU: what `gta_rep_grad_sums` (gta_repgrad.hip: gta_repgrad_kernel, gta_repgrad_finish_kernel) itself computes, against fp64.

Every launch goes to the C entry through ctypes on buffers the test owns: each requested output filled with NaN words and followed by
64 guard words, the workspace of exactly `gta_rep_grad_workspace_bytes` filled with 0xFF and followed by 256 guard bytes, an output that
is not requested passed as NULL (and no workspace without view sums).  One call, one synchronize, everything copied back, and the rules
of tests/_repgrad_sums.py applied on the CPU: exact equality with the fp64 reference on lattice data (every case), the dot-product bound
(n + 1) * 2^-24 * absprod on gaussian data (`_repgrad_sums.GAUSS`); tests/test_repgrad_sums_host.py shows that each rule catches its
defect.  A case runs each output alone and all its slabs allow together (`_repgrad_sums.subsets`): the sections of the kernel share
one LDS array and none may depend on an earlier one having run.  The cases and the kernel instance each launch selects: `_repgrad_sums._table`."""
import ctypes
import functools
import time

import pytest
import torch

from gta_amd import native
from tests import _repgrad_sums as S

pytestmark = pytest.mark.gpu

WORST = {}                      # kernel instance -> (largest gaussian error / bound, case, launch, output)
SPENT = [0.0, 0]                # seconds in launches and copies, launches
RAN = set()                     # gaussian runs done


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """the references are einsums over tiny tensors: many intra-op threads only slow them down"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _data(name, family):
    case = S.CASES[name]
    vals = S.values(case, family)
    return case, vals, S.reference(case, vals)


def _desc(case):
    Nq, Pq = (case.N, case.P) if case.side == 0 else case.other
    Nk, Pk = case.other if case.side == 0 else (case.N, case.P)
    dh = S.slabs(case.f_dims, case.euclid).dh
    Tq, Tk = Nq * Pq, Nk * Pk
    qs, ks = (case.H * Tq * dh, Tq * dh, dh), (case.H * Tk * dh, Tk * dh, dh)
    return native.make_desc_from(case.dtype, (case.B, case.H, Tq, dh), Tk, (qs, ks, ks, qs), case.f_dims, 0, Nq, Nk, dh ** -0.5,
                                 native.FLAG_EUCLID if case.euclid else 0)


@functools.lru_cache(maxsize=None)
def _operands(name, family):
    case, vals, _ = _data(name, family)
    return [S.place(x, lay, case.dtype, "cuda") for x, lay in zip(vals, case.lay)]


def _raw(name, family, subset):
    """one call of the C entry on guarded buffers -> the result `_repgrad_sums.check` reads, on the CPU"""
    case, _, _ = _data(name, family)
    ops = _operands(name, family)
    desc = _desc(case)
    t0 = time.perf_counter()
    shapes = S.out_shapes(case)
    numel = {o: int(torch.Size(shapes[o]).numel()) for o in subset}
    bufs = {o: torch.full((numel[o] + S.GUARD,), S.NAN_WORD, device="cuda", dtype=torch.int32) for o in subset}
    need = native.lib().gta_rep_grad_workspace_bytes(ctypes.byref(desc), case.side)
    assert need == S.workspace_bytes(case), (name, need)
    ws = torch.full((need + S.WS_PAD,), 0xFF, device="cuda", dtype=torch.uint8) if "view" in subset else None
    args = []
    for i in range(4):
        t = ops[i] if i < 2 * case.pairs else None
        args += [native._ptr(t), None if t is None else native._strides(t)]
    rc = native.lib().gta_rep_grad_sums(ctypes.byref(desc), case.side, case.pairs, *args, native._ptr(bufs.get("view")),
                                        native._ptr(bufs.get("so2")), native._ptr(bufs.get("t2")), native._ptr(ws),
                                        need if ws is not None else 0, native._stream())
    assert rc == 0, (name, subset, rc, native.lib().gta_strerror(rc).decode())
    torch.cuda.synchronize()
    res = {o: None for o in S.OUTS}
    res["guard"] = {}
    for o, b in bufs.items():
        b = b.cpu()
        res[o] = b[:numel[o]].view(torch.float32).reshape(shapes[o])
        res["guard"][o] = b[numel[o]:]
    res["ws_tail"] = None if ws is None else ws[need:].cpu()
    SPENT[0] += time.perf_counter() - t0
    SPENT[1] += 1
    return res, ops, desc


@pytest.mark.parametrize("name, family", S.RUNS, ids=lambda v: v)
def test_sums_against_fp64(name, family):
    case, _, ref = _data(name, family)
    for subset in S.subsets(case):
        res, ops, _ = _raw(name, family, subset)
        worst = S.check(case, subset, family, res, ref)
        inst = S.instance(case, subset, ops)
        for o, ratio in worst.items():
            print(f"REPGRAD_SUMS {name} {'+'.join(subset)} {o}: instance {inst}, error / bound {ratio:.4f}")
            if ratio > WORST.get(inst, (-1.0,))[0]:
                WORST[inst] = (ratio, name, "+".join(subset), o)
    if family == "gauss":
        RAN.add(name)


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_strides_do_not_change_a_bit(dt):
    """one set of lattice values under six layouts, two of which fall to the scalar instance: every run is exact, so all are equal"""
    twins = [n for n, c in S.CASES.items() if c.twin == "st" and n.endswith(dt)]
    assert len(twins) == 6
    first = _raw(twins[0], "lattice", ("view", "so2"))[0]
    for n in twins[1:]:
        res = _raw(n, "lattice", ("view", "so2"))[0]
        for o in ("view", "so2"):
            assert torch.equal(res[o].view(torch.int32), first[o].view(torch.int32)), (n, o)


@pytest.mark.parametrize("name", ["g-2chunk-bf16", "g-2chunk-f32", "g-euclid-bf16", "g-vec-f32"])
def test_two_runs_same_bits(name):
    case = S.CASES[name]
    subset = S.subsets(case)[-1]
    a, b = _raw(name, "gauss", subset)[0], _raw(name, "gauss", subset)[0]
    for o in subset:
        assert torch.equal(a[o].view(torch.int32), b[o].view(torch.int32)), (name, o)


@pytest.mark.parametrize("name, family", S.RUNS, ids=lambda v: v)
def test_wrapper_returns_the_raw_calls_tensors(name, family):
    case = S.CASES[name]
    subset = S.subsets(case)[-1]
    res, ops, desc = _raw(name, family, subset)
    pairs = [(ops[2 * i], ops[2 * i + 1]) for i in range(case.pairs)]
    got = native.rep_grad_sums(desc, case.side, pairs, view="view" in subset, so2="so2" in subset, t2="t2" in subset)
    torch.cuda.synchronize()
    for o, t in zip(S.OUTS, got):
        if o in subset:
            assert tuple(t.shape) == S.out_shapes(case)[o] and torch.equal(t.cpu().view(torch.int32), res[o].view(torch.int32)), (name, o)
        else:
            assert t is None


def test_workspace_bytes():
    for name, case in S.CASES.items():
        tpb, chunks = 256 // case.H, -(-case.P // (256 // case.H))
        assert native.lib().gta_rep_grad_workspace_bytes(ctypes.byref(_desc(case)), case.side) == case.B * case.N * chunks * 64, name


def test_report():
    """the figures of this file's run (largest gaussian error as a fraction of its bound per instance, time); when the gaussian runs
    came before it, they reached all six instances"""
    if RAN == set(S.GAUSS):
        assert len(WORST) == 6 and all(w[0] <= 1 for w in WORST.values()), WORST
    for inst in sorted(WORST):
        print(f"REPGRAD_SUMS worst {inst}: {WORST[inst][0]:.4f} of the bound ({WORST[inst][1]}, {WORST[inst][2]}, {WORST[inst][3]})")
    print(f"REPGRAD_SUMS {SPENT[1]} launches, {SPENT[0]:.2f} s in launches and copies, {len(S.CASES)} cases, {len(S.RUNS)} runs")

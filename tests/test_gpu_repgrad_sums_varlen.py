"""GPU: what `gta_rep_grad_sums_varlen` (the VARLEN instances of gta_repgrad_kernel, gta_repgrad_finish_kernel) itself computes, against fp64.

The harness of tests/test_gpu_repgrad_sums.py: every launch goes to the C entry through ctypes on buffers the test owns -- each requested
output filled with NaN words and followed by 64 guard words, the workspace of exactly `gta_rep_grad_workspace_bytes` filled with 0xFF and
followed by 256 guard bytes, an output that is not requested passed as NULL --, one call, one synchronize, everything copied back, and the
rules of tests/_repgrad_sums_varlen.py applied on the CPU (tests/test_repgrad_sums_varlen_host.py shows that each catches its defect).  The
operands of the masked launch hold NaN in every dead row (never-read); the last launch of a case is repeated on operands that are finite
there, which must not change a bit, and compared with the existing `gta_rep_grad_sums` on those buffers (live-equal)."""
import ctypes
import functools

import pytest
import torch

from gta_amd import native
from tests import _repgrad_sums as S
from tests import _repgrad_sums_varlen as V
from tests.test_gpu_repgrad_sums import _desc

pytestmark = pytest.mark.gpu

WORST = {}                      # kernel instance -> (largest gaussian error / bound, case, launch, output)
REACHED = {"lattice": set(), "gauss": set()}
SPENT = [0]                     # launches
RAN = set()                     # runs of test_masked_sums_against_fp64 done


@pytest.fixture(autouse=True, scope="module")
def _one_thread():
    """the references are einsums over tiny tensors: many intra-op threads only slow them down"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@functools.lru_cache(maxsize=None)
def _data(name, family):
    case = V.CASES[name]
    vals = S.values(case, family)
    return case, vals, V.reference(case, vals)


@functools.lru_cache(maxsize=None)
def _operands(name, family, padding):
    """the placed operands; padding 'nan': NaN in every dead row, 'finite': the values themselves"""
    case, vals, _ = _data(name, family)
    if padding == "nan":
        vals = V.masked(case, vals, float("nan"))
    return [S.place(x, lay, case.dtype, "cuda") for x, lay in zip(vals, case.lay)]


@functools.lru_cache(maxsize=None)
def _lens(name):
    return torch.tensor(V.CASES[name].lens, dtype=torch.int32, device="cuda")


def _raw(name, family, subset, padding="nan", masked=True):
    """one call of the C entry (masked: gta_rep_grad_sums_varlen, else gta_rep_grad_sums) on guarded buffers -> the result `check` reads"""
    case, _, _ = _data(name, family)
    ops = _operands(name, family, padding)
    desc = _desc(case)
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
    outs = (native._ptr(bufs.get("view")), native._ptr(bufs.get("so2")), native._ptr(bufs.get("t2")), native._ptr(ws),
            need if ws is not None else 0, native._stream())
    if masked:
        rc = native.lib().gta_rep_grad_sums_varlen(ctypes.byref(desc), case.side, case.pairs, *args, native._ptr(_lens(name)), *outs)
    else:
        rc = native.lib().gta_rep_grad_sums(ctypes.byref(desc), case.side, case.pairs, *args, *outs)
    assert rc == 0, (name, subset, rc, native.lib().gta_strerror(rc).decode())
    torch.cuda.synchronize()
    res = {o: None for o in S.OUTS}
    res["guard"] = {}
    for o, b in bufs.items():
        b = b.cpu()
        res[o] = b[:numel[o]].view(torch.float32).reshape(shapes[o])
        res["guard"][o] = b[numel[o]:]
    res["ws_tail"] = None if ws is None else ws[need:].cpu()
    SPENT[0] += 1
    return res, ops, desc


def _same_bits(a, b, subset, tag):
    for o in subset:
        assert torch.equal(a[o].view(torch.int32), b[o].view(torch.int32)), tag + (o,)


@pytest.mark.parametrize("name, family", V.RUNS, ids=lambda v: v)
def test_masked_sums_against_fp64(name, family):
    case, _, ref = _data(name, family)
    for subset in S.subsets(case):
        res, ops, _ = _raw(name, family, subset)                                   # NaN in the dead rows: never-read
        worst = V.check(case, subset, family, res, ref)                            # fp64 rules, fill, guards, dead-zero
        inst = S.instance(case, subset, ops)
        REACHED[family].add(inst)
        for o, ratio in worst.items():
            print(f"REPGRAD_SUMS_VARLEN {name} {'+'.join(subset)} {o}: instance {inst} + VARLEN, error / bound {ratio:.4f}")
            if ratio > WORST.get(inst, (-1.0,))[0]:
                WORST[inst] = (ratio, name, "+".join(subset), o)
    # the last launch (every output together) again on finite padding: not a bit may move; and the existing entry on those buffers
    fin = _raw(name, family, subset, padding="finite")[0]
    _same_bits(res, fin, subset, (name, "finite padding changes the masked result"))
    V.check(case, subset, family, fin, ref)
    plain = _raw(name, family, subset, padding="finite", masked=False)[0]
    V.check_live_equal(case, subset, fin, plain)
    RAN.add((name, family))


@pytest.mark.parametrize("name", ["g-2chunk-bf16@inchunk", "g-2chunk-f32@views", "g-euclid-bf16@inchunk", "g-vec-f32@clamp",
                                  "g-so2-12-bf16@inchunk", "g-euclid-f32@views"])
def test_two_runs_same_bits(name):
    case = V.CASES[name]
    subset = S.subsets(case)[-1]
    a, b = _raw(name, "gauss", subset)[0], _raw(name, "gauss", subset)[0]
    _same_bits(a, b, subset, (name,))


def test_full_prefix_is_the_unmasked_entry():
    """lens = T in every scene: every word, view sums included, is the existing entry's"""
    for name in ("h8-2c5-bf16@full", "h6-2c5-f32@full", "eu-se3-9-f32@full", "h8t-2c5-bf16@full"):
        subset = S.subsets(V.CASES[name])[-1]
        _same_bits(_raw(name, "lattice", subset)[0], _raw(name, "lattice", subset, masked=False)[0], subset, (name,))


@pytest.mark.parametrize("name, family", [r for r in V.RUNS if r[0].endswith(("@views", "@inchunk"))], ids=lambda v: v)
def test_wrapper_returns_the_raw_calls_tensors(name, family):
    case = V.CASES[name]
    subset = S.subsets(case)[-1]
    res, ops, desc = _raw(name, family, subset)
    pairs = [(ops[2 * i], ops[2 * i + 1]) for i in range(case.pairs)]
    got = native.rep_grad_sums(desc, case.side, pairs, view="view" in subset, so2="so2" in subset, t2="t2" in subset, lens=_lens(name))
    torch.cuda.synchronize()
    for o, t in zip(S.OUTS, got):
        if o in subset:
            assert tuple(t.shape) == S.out_shapes(case)[o] and torch.equal(t.cpu().view(torch.int32), res[o].view(torch.int32)), (name, o)
        else:
            assert t is None
    with pytest.raises(native.GtaError, match="lens"):
        native.rep_grad_sums(desc, case.side, pairs, view="view" in subset, so2="so2" in subset, lens=_lens(name).long())


def test_report():
    """the figures of this file's run; when the masked runs came before it, each kind of data reached all six VARLEN instances"""
    if RAN == set(V.RUNS):
        assert len(REACHED["lattice"]) == 6 and len(REACHED["gauss"]) == 6, REACHED
        assert len(WORST) == 6 and all(w[0] <= 1 for w in WORST.values()), WORST
    for inst in sorted(WORST):
        print(f"REPGRAD_SUMS_VARLEN worst {inst} + VARLEN: {WORST[inst][0]:.4f} of the bound ({WORST[inst][1]}, {WORST[inst][2]}, {WORST[inst][3]})")
    print(f"REPGRAD_SUMS_VARLEN {SPENT[0]} launches, {len(V.CASES)} cases, {len(V.RUNS)} runs")

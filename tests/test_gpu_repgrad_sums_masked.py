"""GPU: what `gta_rep_grad_sums_masked` (the MASKED instances of gta_repgrad_kernel, gta_repgrad_finish_kernel) itself computes, against fp64.

The harness of tests/test_gpu_repgrad_sums_varlen.py: every launch goes to the C entry through ctypes on buffers the test owns -- each
requested output filled with NaN words and followed by 64 guard words, the workspace of exactly `gta_rep_grad_workspace_bytes` filled with
0xFF and followed by 256 guard bytes, an output that is not requested passed as NULL --, one call, one synchronize, everything copied back,
and the rules of tests/_repgrad_sums_masked.py applied on the CPU (tests/test_repgrad_sums_masked_host.py shows that each catches its defect).
The operands of the masked launch hold NaN in every dead row (never-read).  The last launch of a case is compared, every word, with the
existing `gta_rep_grad_sums` on operands whose dead rows hold zeros (live-equal) and, under a prefix mask, with `gta_rep_grad_sums_varlen`
under the prefix's counts (prefix-equal)."""
import ctypes
import functools

import pytest
import torch

from gta_amd import native
from tests import _repgrad_sums as S
from tests import _repgrad_sums_masked as M
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
    case = M.CASES[name]
    vals = S.values(case, family)
    return case, vals, M.reference(case, vals)


@functools.lru_cache(maxsize=None)
def _operands(name, family, padding):
    """the placed operands; padding 'nan': NaN in every dead row, 'zero': zeros there"""
    case, vals, _ = _data(name, family)
    vals = M.masked(case, vals, float("nan") if padding == "nan" else 0.0)
    return [S.place(x, lay, case.dtype, "cuda") for x, lay in zip(vals, case.lay)]


@functools.lru_cache(maxsize=None)
def _live(name):
    return M.CASES[name].mask.to(torch.uint8).contiguous().cuda()


@functools.lru_cache(maxsize=None)
def _lens(name):
    return torch.tensor(M.CASES[name].prefix.lens, dtype=torch.int32, device="cuda")


def _raw(name, family, subset, padding="nan", entry="masked"):
    """one call of a C entry (masked / plain: gta_rep_grad_sums / varlen) on guarded buffers -> the result `check` reads"""
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
    if entry == "masked":
        live = _live(name)
        assert tuple(live.shape) == (case.B, case.N * case.P) and live.is_contiguous()
        rc = native.lib().gta_rep_grad_sums_masked(ctypes.byref(desc), case.side, case.pairs, *args, native._ptr(live), *outs)
    elif entry == "varlen":
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


@pytest.mark.parametrize("name, family", M.RUNS, ids=lambda v: v)
def test_masked_sums_against_fp64(name, family):
    case, _, ref = _data(name, family)
    for subset in S.subsets(case):
        res, ops, _ = _raw(name, family, subset)                                   # NaN in the dead rows: never-read
        worst = M.check(case, subset, family, res, ref)                            # fp64 rules, fill, guards, dead-zero
        inst = S.instance(case, subset, ops)
        REACHED[family].add(inst)
        for o, ratio in worst.items():
            print(f"REPGRAD_SUMS_MASKED {name} {'+'.join(subset)} {o}: instance {inst} + MASKED, error / bound {ratio:.4f}")
            if ratio > WORST.get(inst, (-1.0,))[0]:
                WORST[inst] = (ratio, name, "+".join(subset), o)
    # the last launch (every output together): the unmasked entry on zeroed dead rows, and under a prefix mask the VARLEN entry
    plain = _raw(name, family, subset, padding="zero", entry="plain")[0]
    M.check_same_bits(case, subset, res, plain, "live-equal")
    if case.mask_name.startswith("p-"):
        assert case.prefix is not None
        M.check_same_bits(case, subset, res, _raw(name, family, subset, entry="varlen")[0], "prefix-equal")
    RAN.add((name, family))


@pytest.mark.parametrize("name", ["g-2chunk-bf16@bern", "g-2chunk-f32@lastonly", "g-euclid-bf16@bern", "g-vec-f32@p-inchunk",
                                  "g-so2-12-bf16@bern", "g-euclid-f32@lastonly"])
def test_two_runs_same_bits(name):
    case = M.CASES[name]
    subset = S.subsets(case)[-1]
    a, b = _raw(name, "gauss", subset)[0], _raw(name, "gauss", subset)[0]
    M.check_same_bits(case, subset, a, b, "two runs")


def test_all_true_mask_is_the_unmasked_entry():
    """every token live: every word, view sums included, is the existing entry's on the same buffers"""
    for name in ("h8-2c5-bf16@full", "h6-2c5-f32@full", "eu-se3-9-f32@full", "h8t-2c5-bf16@full", "h256-bf16@full", "cross-k-f32@full"):
        case = M.CASES[name]
        assert bool(case.mask.all())
        subset = S.subsets(case)[-1]
        M.check_same_bits(case, subset, _raw(name, "lattice", subset)[0], _raw(name, "lattice", subset, entry="plain")[0], "all-true")


def test_prefix_masks_are_the_varlen_entry():
    """every prefix mask of the table, each launch: the VARLEN entry's words under the prefix's counts, on the same NaN-padded buffers"""
    names = [n for n, c in M.CASES.items() if c.mask_name.startswith("p-") and not c.gauss]
    assert len(names) >= 2 * len(M.BASES)
    for name in names:
        case = M.CASES[name]
        for subset in S.subsets(case):
            M.check_same_bits(case, subset, _raw(name, "lattice", subset)[0], _raw(name, "lattice", subset, entry="varlen")[0], "prefix-equal")


@pytest.mark.parametrize("name, family", [r for r in M.RUNS if r[0].endswith(("@bern", "@midview"))], ids=lambda v: v)
def test_wrapper_returns_the_raw_calls_tensors(name, family):
    case = M.CASES[name]
    subset = S.subsets(case)[-1]
    res, ops, desc = _raw(name, family, subset)
    pairs = [(ops[2 * i], ops[2 * i + 1]) for i in range(case.pairs)]
    want = dict(view="view" in subset, so2="so2" in subset, t2="t2" in subset)
    for live in (_live(name), _live(name).bool()):                              # uint8 and bool alike
        got = native.rep_grad_sums(desc, case.side, pairs, live=live, **want)
        torch.cuda.synchronize()
        for o, t in zip(S.OUTS, got):
            if o in subset:
                assert tuple(t.shape) == S.out_shapes(case)[o] and torch.equal(t.cpu().view(torch.int32), res[o].view(torch.int32)), (name, o)
            else:
                assert t is None
    live = _live(name)
    for bad in (live.long(), live[:, :-1].contiguous(), live[:1], live.t().contiguous().t(), live.cpu()):
        with pytest.raises(native.GtaError, match="live"):
            native.rep_grad_sums(desc, case.side, pairs, live=bad, **want)
    with pytest.raises(native.GtaError, match="lens and live"):
        native.rep_grad_sums(desc, case.side, pairs, live=live, lens=torch.ones(case.B, dtype=torch.int32, device="cuda"), **want)


def test_report():
    """the figures of this file's run; when the masked runs came before it, each kind of data reached all six MASKED instances"""
    if RAN == set(M.RUNS):
        assert len(REACHED["lattice"]) == 6 and len(REACHED["gauss"]) == 6, REACHED
        assert len(WORST) == 6 and all(w[0] <= 1 for w in WORST.values()), WORST
    for inst in sorted(WORST):
        print(f"REPGRAD_SUMS_MASKED worst {inst} + MASKED: {WORST[inst][0]:.4f} of the bound ({WORST[inst][1]}, {WORST[inst][2]}, {WORST[inst][3]})")
    print(f"REPGRAD_SUMS_MASKED {SPENT[0]} launches, {len(M.CASES)} cases, {len(M.RUNS)} runs")

"""GPU: the row and element-wise kernels of gta_block.hip at sizes where their loops take a second trip.

tests/test_gpu_block.py runs them where every loop makes at most one trip; here each case is sized by the constant that caps its grid:

    element-wise kernels   `ew_grid` caps at 8192 workgroups of 256 lanes, 8 elements per lane: N_EW = 8 (8192 256 + 1000 256 + 5)
                           elements give workgroups 0..999 a full second trip and workgroup 1000 a ragged one (5 of its 256 lanes)
    LayerNorm backward     `LN_BWD_MAX_WG` = 1024 workgroups of 4 rows: 8198 rows = two sweeps of 4096 and six rows of a third
    colsum_finish_kernel   four partials per row group and trip of its unrolled body (32 row groups): 97 partials (only row group 0
                           enters it), 200 (body, then tail), 1024 (eight trips), 141 column-sum strips (`COLSUM_MAX_STRIPS` = 512)

Each LayerNorm / column-sum case asserts its regime from the workspace size the library reports, so a changed constant fails the case
instead of quietly moving it back into the first trip.  References are fp64 PyTorch on the device; the dropout mask is the host
Philox of tests/_philox.py.  Bars (none new): those of test_gelu_and_colsum, test_dropout_kernels and test_layernorm_forward_backward."""
import functools

import pytest
import torch
import torch.nn.functional as F

from gta_amd import native_block as nb
from tests import _philox
from tests.test_gpu_block import BF, DEV, _check_layernorm, _err, _mask

pytestmark = pytest.mark.gpu

EW_CAP = 8 * 8192 * 256                            # elements of the first trip under ew_grid's cap
N_EW = 8 * (8192 * 256 + 1000 * 256 + 5)
SEED = 0x5DEECE66D1234                             # both halves of the key non-zero
WINDOWS = ((0, 1 << 20), (EW_CAP - (1 << 15), 1 << 16), (N_EW - (1 << 16), 1 << 16))     # (first element, length), multiples of 8


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_mask_past_the_grid_cap_is_the_host_philox(p, dt):
    """The keep factors dropout_add applies, against tests/_philox.py: the first 2^20 elements, 2^16 around the seam between the
    trips, the last 2^16 (the ragged workgroup)."""
    m = _mask((N_EW,), p, SEED, dt)
    scale = torch.tensor(float(_philox.keep_scale(p)), dtype=torch.float32).to(dt)
    for first, length in WINDOWS:
        assert first % 8 == 0 and 0 <= first and first + length <= N_EW
        keep = torch.from_numpy(_philox.keep_mask(length, p, SEED, first_unit=first // 8)).to(DEV)
        want = torch.where(keep, scale.to(DEV), torch.zeros((), device=DEV, dtype=dt))
        got = m[first:first + length]
        wrong = (got != want).nonzero()
        assert wrong.numel() == 0, (p, dt, first, wrong.numel(), first + int(wrong[0]))


@functools.lru_cache(maxsize=None)
def _ew_operands(dt):
    g = torch.Generator(device=DEV).manual_seed(17)
    x = (torch.randn(N_EW, device=DEV, generator=g) * 2).to(dt)
    dy = torch.randn(N_EW, device=DEV, generator=g).to(dt)
    return x, dy


def _by_trip(name, got, ref, bound):
    """|got - ref| <= bound (a number or a tensor) on the first-trip and the second-trip index range, each reported by itself"""
    over = (got.double() - ref).abs() - bound
    for trip, lo, hi in (("first trip", 0, EW_CAP), ("second trip", EW_CAP, N_EW)):
        worst, at = over[lo:hi].max().item(), lo + int(over[lo:hi].argmax())
        print(f"BLOCK_REGIMES {name} {trip}: max (|err| - bound) = {worst:.3e} at element {at}")
        assert worst <= 0, (name, trip, worst, at)


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("p", [0.0, 0.3])
def test_elementwise_kernels_past_the_grid_cap(p, dt):
    """gelu_fwd, gelu_bwd, dropout_bwd and dropout_add over all of N_EW against fp64 formulas times the mask (which the test above
    ties to the host generator).  Bars: test_gelu_and_colsum's (2e-6 / 2^-8 of max |ref|) for the two GELU kernels, test_dropout_kernels'
    for the two dropout kernels (allclose with its rtol 1e-5 and atol 1e-8 / 1e-6; the bf16 result equal to the rounded fp32 product)."""
    x, dy = _ew_operands(dt)
    m = _mask((N_EW,), p, SEED).double()
    xr = x.double().requires_grad_(True)
    yr = F.gelu(xr)
    yr.backward(dy.double())
    tol = 2.0 ** -8 if dt == BF else 2e-6
    ref = yr.detach() * m
    _by_trip("gelu_fwd", nb.gelu_fwd(x, p, SEED), ref, tol * ref.abs().max().item())
    ref = xr.grad * m
    _by_trip("gelu_bwd", nb.gelu_bwd(dy, x, p, SEED), ref, tol * ref.abs().max().item())
    ref = x.double() * m                               # exact in fp64 (at most 24 x 24 significant bits)
    _by_trip("dropout_bwd fp32", nb.dropout_bwd(x, torch.float32, p, SEED), ref, 1e-8 + 1e-5 * ref.abs())
    _by_trip("dropout_bwd bf16", nb.dropout_bwd(x, BF, p, SEED), ref.float().to(BF).double(), 0.0)
    z, skip = x.to(BF), dy.float()
    ref = skip.double() + z.double() * m
    _by_trip("dropout_add", nb.dropout_add(z, skip, p, SEED), ref, 1e-6 + 1e-5 * ref.abs())


@pytest.mark.parametrize("rows,d", [(r, d) for r in (388, 800, 8198) for d in (64, 180, 768)])
@pytest.mark.parametrize("xdt,ydt", [(torch.float32, BF), (torch.float32, torch.float32), (BF, BF)])
def test_layernorm_backward_regimes(rows, d, xdt, ydt):
    """test_layernorm_forward_backward's body, references and bars where the row walk and the finish pass take further trips"""
    partials = nb.lib().gta_ln_bwd_workspace_bytes(rows, d) / (8 * d)
    if rows == 388:
        assert partials == 97                        # colsum_finish_kernel: only row group 0 enters the unrolled body (0 + 96 < 97)
    elif rows == 800:
        assert partials == 200                       # every row group: the unrolled body once, then two or three tail steps
    else:
        assert partials == 1024 and 4 * 1024 < rows  # the grid is capped: every wave walks 2 rows, six of them 3; finish: 8 trips, no tail
    _check_layernorm(rows, d, xdt, ydt)


@pytest.mark.parametrize("dt", [torch.float32, BF])
@pytest.mark.parametrize("n", [264, 180])
def test_colsum_finish_unrolled_body_then_tail(n, dt):
    """9000 rows: 141 strips -- the finish pass runs its unrolled body, then its tail loop; n = 264: 8 columns per lane, 180: 4"""
    m = 9000
    strips = nb.lib().gta_colsum_workspace_bytes(m, n) / (4 * n)
    assert strips > 128, strips
    g = torch.Generator(device=DEV).manual_seed(n)
    a = torch.randn(m, n, device=DEV, generator=g).to(dt)
    assert _err(nb.colsum(a), a.double().sum(0)) <= 1e-5 * a.double().abs().sum(0).max().item()

"""CPU: the workspace model of tests/_images.py -- encode / decode are inverses at every padded head size, the unit map is the swizzle of
gta_common.h, the byte offsets and sizes are the library's own (`gta_attn_fwd_workspace_bytes`, `gta_attn_fwd_staged_workspace_bytes`: host code),
and `ref_rows` (the fp64 reference the GPU cases of tests/test_gpu_prep_images.py hold the pre-pass kernels to) agrees with the oracle's
`transform_qkv` on one layout of every kind those cases run."""
import numpy as np
import pytest
import torch

from gta_amd import native
from oracle import gta_oracle as O
from tests import _images as I
from tests import test_host_logic

VT, EU, X3 = native.FLAG_V_TRANSFORM, native.FLAG_EUCLID, native.FLAG_FP32_PRODUCTS


def _bf16_rows(B, H, n_tiles, dhp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, H, n_tiles * 64, dhp, generator=g).bfloat16().float()


@pytest.mark.parametrize("mode", ["fused", "x3", "staged"])          # (the staged route has no GTA_FLAG_FP32_PRODUCTS instances)
@pytest.mark.parametrize("dhp", [32, 64, 96, 128])
def test_decode_inverts_encode(dhp, mode):
    x3, staged = mode == "x3", mode == "staged"
    B, H, Tk = 2, 3, 150
    n_tiles = 3
    k, v = _bf16_rows(B, H, n_tiles, dhp, 1), _bf16_rows(B, H, n_tiles, dhp, 2)
    lo = (_bf16_rows(B, H, n_tiles, dhp, 3) * 2.0 ** -9, _bf16_rows(B, H, n_tiles, dhp, 4) * 2.0 ** -9) if x3 else (None, None)
    aux = torch.rand(B, H, n_tiles * 64 if staged else n_tiles)
    ws = I.encode(k, v, Tk, dhp, *lo, aux=aux, staged=staged, fill=0xFF)
    L = I.staged_layout(B, H, Tk, dhp) if staged else I.fused_layout(B, H, Tk, dhp, x3)
    assert ws.dtype == torch.uint8 and ws.numel() == L.total
    d = I.decode(ws, B, H, Tk, dhp, x3=x3, staged=staged)
    assert torch.equal(d.k, k) and torch.equal(d.v, v) and torch.equal(d.aux, aux)
    if x3:
        assert torch.equal(d.k_lo, lo[0]) and torch.equal(d.v_lo, lo[1])
    # ... and encode(decode(bytes)) gives the bytes back: the model covers every byte up to the end of the norms / bias but the alignment gap
    again = I.encode(d.k, d.v, Tk, dhp, d.k_lo, d.v_lo, aux=d.aux, staged=staged, fill=0xFF)
    assert torch.equal(again, ws)
    assert bool((ws[L.images:L.aux_off] == 0xFF).all()) and bool((ws[L.aux_end:] == 0xFF).all())
    # one element by hand: channel 8c + i of row r of image `image` of tile (b, h, j) is the bf16 at unit_offset + 2 i
    raw = ws.numpy()
    for (b, h, j, image, r, c, i) in ((0, 0, 0, 0, 0, 0, 0), (1, 2, 2, 1, 37, L.chp - 1, 5), (0, 1, 1, L.nimg - 1, 63, 1, 7)):
        o = I.unit_offset(L, b, h, j, image, r, c) + 2 * i
        got = torch.from_numpy(raw[o:o + 2].copy().view(np.int16))
        assert int(got) == int(d.bits[b, h, j, image, r, 8 * c + i])
        assert tuple(d.bits.shape) == (B, H, n_tiles, L.nimg, 64, dhp)


def test_encode_rounds_to_nearest_even():
    x = torch.zeros(1, 1, 64, 32)
    one = torch.tensor(1.0)
    x[0, 0, 0, 0] = one + 2.0 ** -8                  # a tie: to the even neighbour 1.0
    x[0, 0, 0, 1] = one + 2.0 ** -7 + 2.0 ** -8      # a tie: to the even neighbour 1 + 2^-6
    x[0, 0, 0, 2] = one + 2.0 ** -8 + 2.0 ** -20     # above the tie: up
    x[0, 0, 0, 3] = one + 2.0 ** -7 - 2.0 ** -20     # truncation would give 1.0
    d = I.decode(I.encode(x, x, 64, 32), 1, 1, 64, 32)
    assert d.k[0, 0, 0, :4].tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7]
    assert I.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, -0.75, 0.0])).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0]


@pytest.mark.parametrize("chp", [4, 8, 12, 16])
def test_unit_map_is_the_kernels_swizzle(chp):
    pos = I.unit_positions(chp)
    assert pos.shape == (64, chp)
    for r in range(64):
        assert sorted(pos[r].tolist()) == list(range(chp))                         # a permutation of the row's units
        for c in range(chp):
            assert pos[r, c] == test_host_logic.swz(chp, r, c) == I.swz(chp, r, c)
    assert test_host_logic.swz is I.swz                                            # one definition
    # swz_rot<UNITS> of gta_common.h, spelled out: the rotation of unit 0
    rot = {4: lambda r: (r >> 2) & 3, 8: lambda r: 4 * ((r >> 1) & 1) + ((r >> 2) & 3), 12: lambda r: (r >> 2) & 3,
           16: lambda r: 4 * (r & 3) + ((r >> 2) & 3)}[chp]
    for r in range(64):
        assert pos[r, 0] == rot(r) % chp and all(pos[r, c] == (c + rot(r)) % chp for c in range(chp))


def _desc(f_dims, dtype, B, H, Tq, Tk, Nq, Nk, flags, L=0):
    dh = sum(f_dims.values())
    qs, ks = (Tq * H * dh, dh, H * dh), (Tk * H * dh, dh, H * dh)                  # token-major storage
    return native.make_desc_from(dtype, (B, H, Tq, dh), Tk, (qs, ks, ks, qs), f_dims, L, Nq, Nk, dh ** -0.5, flags)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("dh", [16, 32, 40, 64, 96, 104, 128])
def test_fused_offsets_are_the_librarys(dh, dtype):
    esz = 2 if dtype == torch.bfloat16 else 4
    for (B, H, Nk, Pk, Nq) in ((3, 3, 3, 50, 3), (1, 1, 1, 40, 1), (4, 3, 4, 32, 2), (2, 5, 1, 64, 1)):
        f = {"se3": dh // 2, "so2": dh // 2}
        d = _desc(f, dtype, B, H, Nq * 10, Nk * Pk, Nq, Nk, VT)
        assert native.attn_fwd_supported(d) == 0
        L = I.fused_layout(B, H, Nk * Pk, dh, False, Nq, esz)
        assert native.attn_fwd_workspace_bytes(d) == L.total, (dh, B, H, Nk, Pk)
        assert L.aux_off % 256 == 0 and L.qtiles_off % 256 == 0 and L.aux_off >= L.images and L.qtiles_off >= L.aux_end
        assert L.images == B * H * L.n_tiles * 2 * 64 * L.dhp * 2 and L.dhp == (dh + 31) // 32 * 32
        assert I.tile_offset(L, B - 1, H - 1, L.n_tiles - 1, 1) + L.img == L.images       # the last image ends the image region
        if esz == 4 and dh <= 64:                  # the split-bf16 instances: four images per tile
            d.flags = VT | X3
            L3 = I.fused_layout(B, H, Nk * Pk, dh, True, Nq, esz)
            assert native.attn_fwd_workspace_bytes(d) == L3.total and L3.images == 2 * L.images
            assert I.tile_offset(L3, 0, 0, 1, 0) == 4 * L3.img and I.tile_offset(L3, 0, 0, 0, 2) == 2 * L3.img


@pytest.mark.parametrize("name", ["euclid", "t2", "t2-96"])
def test_staged_offsets_are_the_librarys(name):
    f, flags = {"euclid": ({"triv": 2, "se3": 30, "so2": 32}, VT | EU), "t2": ({"triv": 2, "se3": 32, "t2": 30}, VT),
                "t2-96": ({"se3": 48, "t2": 48}, VT)}[name]
    dh = sum(f.values())
    for dtype in (torch.bfloat16, torch.float32):
        for (B, H, Nk, Pk) in ((3, 3, 3, 50), (4, 3, 4, 32), (1, 2, 1, 64)):
            d = _desc(f, dtype, B, H, 70, Nk * Pk, 1, Nk, flags)
            assert native.attn_fwd_staged_supported(d) == 0
            L = I.staged_layout(B, H, Nk * Pk, dh)
            assert native.attn_fwd_staged_workspace_bytes(d) == L.total
            assert L.aux_off % 256 == 0 and L.aux_off >= L.images and L.aux_count == B * H * L.n_tiles * 64


# one layout of each kind the GPU cases run: (f_dims, so3 degree, euclid)
KINDS = {
    "se3|so2": ({"se3": 16, "so2": 16}, 0, False),
    "se3|so3|so2": ({"se3": 8, "so3": 8, "so2": 16}, 2, False),
    "so2": ({"so2": 32}, 0, False),
    "se3": ({"se3": 32}, 0, False),
    "mixed halves": ({"triv": 4, "se3": 12, "so2": 16}, 0, False),
    "triv": ({"triv": 32}, 0, False),
    "euclid": ({"triv": 2, "se3": 30, "so2": 32}, 0, True),
    "t2": ({"triv": 2, "se3": 32, "t2": 30}, 0, False),
}


@pytest.mark.parametrize("v_transform", [True, False])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_ref_rows_is_the_oracles_transform(kind, v_transform):
    """tables from the CPU packer (gta_amd.pack_reps on oracle reps); 1e-5 relative to the size of the terms (absprod) per element -- the
    observed difference is the fp32 rounding of trans_coeff times the translation column, 2^-24"""
    f, L, euclid = KINDS[kind]
    tc = 0.37
    c = I.key_side_case(f, L, torch.float32, B=2, H=2, Nk=3, Pk=7, seed=len(kind))
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, c.so3, tc if f.get("se3", 0) else None, v_transform, euclid)
    reps64 = {n: ([t.double() for t in r] if isinstance(r, list) else r.double()) for n, r in c.reps.items()}
    _, kt, vt = O.transform_qkv(c.k.double(), c.k.double(), c.v.double(), c.f_dims, reps64, tc, v_transform, euclid)
    assert ref.k.shape == kt.shape == (2, 2, 21, c.dh)
    for got, want, ap in ((ref.k, kt, ref.absprod_k), (ref.v, vt, ref.absprod_v)):
        assert bool((ap >= got.abs() * (1 - 1e-12)).all())
        assert bool(((got - want).abs() <= 1e-5 * ap + 1e-30).all()), (kind, ((got - want).abs() / ap.clamp_min(1e-30)).max())
    # the channels the transform leaves alone carry the input's value exactly
    assert torch.equal(ref.k[..., ref.ident_k], c.k.double()[..., ref.ident_k])
    assert torch.equal(ref.v[..., ref.ident_v], c.v.double()[..., ref.ident_v])
    assert bool(ref.ident_v.all()) == (not v_transform or kind == "triv")

"""The gather rule of the STAGED generic pre-pass as an executable statement (test infrastructure on top of tests/_images.py, which is
imported unchanged -- `decode(..., staged=True)`; plain numpy / torch on the CPU, no GPU, no kernel output).  Modelled on
tests/_gather_images.py, which states the same for the fused pre-pass.

`gta_attn_fwd_staged_gather` (the GATHER instances of `gta_gen_prep_kernel`, gta_amd/csrc/gta_fwd_gen.hip) leaves the workspace of the staged
generic forward (`_images.staged_layout`: [K' | V'] tile images, then 64 fp32 bias values per tile) with the valid keys of
every scene compacted:

  gather rule   image row r of tile j of scene b is `_images.ref_rows` of token tok = key_idx[b, 64 j + r] -- that token's K / V row under the
                record of view tok / P, that token's (cos, sin) row and its coord row --, for 64 j + r < key_lens[b]
  euclid bias   -0.5 scale |k'|^2 of that token at the COMPACTED position 64 j + r of (b, h) -- not at the token's own position
  zero rule     rows at or past key_lens[b] in the last written tile, and the padded channels of every written row, are zero bytes; the
                bias of such a row is exactly +0.0
  skip rule     tiles with 64 j >= key_lens[b] keep what the workspace held, images and bias; so does every byte outside images and bias;
                without euclid no bias is written at all

The bars are those of tests/test_gpu_prep_images.py (derived there; none new): untouched channels are the input's bits rounded to nearest
even; transformed ones lie within ulp(ref64) / 2 + err32 of ref64, err32 = 16 * 2^-24 * absprod; the bias within
0.5 scale (2 sum_i |k'_i| err32_i + (dh + 2) 2^-24 sum_i k'_i^2) of -0.5 scale sum_i k'_i^2 from ref_rows.

`emulate` is the host emulation of the kernel: the reference rows gathered, rounded by `_images.encode`, the bias of the gathered rows at the
compacted positions, with skipped tiles left at the fill.  `DEFECTS` are planted faults, each of which `check` must catch
(tests/test_key_mask_generic_host.py)."""
import numpy as np
import torch

from tests import _images as I
from tests._gather_images import FILL, gathered, index_tensors          # noqa: F401  (index_tensors: for the callers)


def _scale(dh, scale):
    return float(np.float32(dh ** -0.5 if scale is None else scale))


def check(name, ws, c, ref, key_idx, key_lens, euclid, scale=None):
    """every rule of the module docstring on one workspace (CPU uint8 tensor) written over FILL bytes; c: `_images.key_side_case`-like (B, H,
    T, dh, k, v fp32 masters); ref: `_images.ref_rows` of the WHOLE key side; key_idx [B, T], key_lens [B] (only idx[b, :lens[b]] is looked
    at); scale: the descriptor's (None: dh ** -0.5)"""
    B, H, T, dh = c.B, c.H, c.T, c.dh
    d = I.decode(ws, B, H, T, dh, staged=True)
    L = d.layout
    lens = [int(n) for n in key_lens]
    assert all(1 <= n <= T for n in lens), lens
    raw = ws.numpy()
    assert bool((raw[L.images:L.aux_off] == FILL).all()) and bool((raw[L.aux_end:] == FILL).all()), f"{name}: bytes outside the images and bias were written"
    rows = d.bits.permute(0, 1, 3, 2, 4, 5).reshape(B, H, L.nimg, L.n_tiles * 64, L.dhp)          # [B,H,image,position,channel]
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        assert bool((rows[b, :, :, nt * 64:] == -1).all()), f"{name}: scene {b}: an image of a tile past the count was written"
        assert bool((d.aux_raw[b, :, nt * 64:] == -1).all()), f"{name}: scene {b}: a bias of a tile past the count was written"
        assert bool((rows[b, :, :, n:nt * 64] == 0).all()), f"{name}: scene {b}: rows {n}..{nt * 64 - 1} are not zero rows in every image"
        assert bool((rows[b, :, :, :nt * 64, dh:] == 0).all()), f"{name}: scene {b}: padded channels are not zero"
    valid = torch.zeros(B, 1, T, 1, dtype=torch.bool)
    idx = torch.zeros(B, T, dtype=torch.int64)
    for b, n in enumerate(lens):
        valid[b, :, :n] = True
        idx[b, :n] = key_idx[b, :n].long()
        assert bool(((idx[b, :n] >= 0) & (idx[b, :n] < T)).all()), f"{name}: scene {b}: an index outside [0, Tk)"
    err32 = lambda ap: 16.0 * 2.0 ** -24 * ap
    for img_i, (what, x, r64, ap, ident) in enumerate((("K'", c.k, ref.k, ref.absprod_k, ref.ident_k), ("V'", c.v, ref.v, ref.absprod_v, ref.ident_v))):
        x, r64, ap = gathered(x, idx), gathered(r64, idx), gathered(ap, idx)
        bits = rows[:, :, img_i, :T, :dh]
        img = I.bits_to_f32(bits)
        same = (bits == I.bf16_bits(x)) | ~valid | ~ident
        assert bool(same.all()), f"{name} {what}: an untransformed element is not RNE(input of token key_idx[b, p]): first at flat index {int((~same).flatten().int().argmax())}"
        sel = (valid & ~ident).expand_as(r64)
        excess = (img.double() - r64).abs() - (I.ulp_bf16(r64) / 2 + err32(ap))
        excess = torch.where(sel, excess, torch.full_like(excess, -1.0))
        excess = torch.where(torch.isnan(excess), torch.full_like(excess, float("inf")), excess)
        w = int(excess.argmax())
        b, h, p, ch = np.unravel_index(w, tuple(r64.shape))
        print(f"STAGED_GATHER_IMAGES {name} {what}: worst |img - ref| - bar = {excess.flatten()[w].item():.3e}")
        assert excess.flatten()[w].item() <= 0.0, (f"{name} {what}: scene {b} head {h} tile {p // 64} row {p % 64} (token {int(idx[b, p])}) channel {ch}: "
                                                   f"ref64 {r64.flatten()[w].item()!r} img {img.flatten()[w].item()!r}")
    if not euclid:
        assert bool((d.aux_raw == -1).all()), f"{name}: a bias was written without euclid"
        return d
    sc = _scale(dh, scale)
    rk, apk = gathered(ref.k, idx), gathered(ref.absprod_k, idx)
    rb = -0.5 * sc * rk.pow(2).sum(-1)                                                              # [B,H,position]
    bar = 0.5 * sc * (2 * (rk.abs() * err32(apk)).sum(-1) + (dh + 2) * 2.0 ** -24 * rk.pow(2).sum(-1))
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        e = (d.aux[b, :, :n].double() - rb[b, :, :n]).abs() - bar[b, :, :n]
        w = int(torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e).argmax())
        h, p = np.unravel_index(w, tuple(e.shape))
        worst = float("inf") if bool(torch.isnan(e.flatten()[w])) else e.flatten()[w].item()
        print(f"STAGED_GATHER_IMAGES {name} bias scene {b}: worst err - bar {worst:.3e} (bar {bar[b, h, p].item():.3e})")
        assert worst <= 0.0, (f"{name}: bias of scene {b} head {h} position {p} (token {int(idx[b, p])}): {d.aux[b, h, p].item()!r} "
                              f"ref {rb[b, h, p].item()!r} bar {bar[b, h, p].item():.3e}")
        assert bool((d.aux_raw[b, :, n:nt * 64] == 0).all()), f"{name}: scene {b}: the bias of a row past the count is not +0.0"
    return d


def emulate(c, ref, key_idx, key_lens, euclid, total=None, defect=None, scale=None):
    """the workspace bytes the staged gather pre-pass leaves on a FILL-filled workspace (of `total` bytes; None: the layout's), from the
    reference rows; defect: one of DEFECTS, planted"""
    B, H, T, dh = c.B, c.H, c.T, c.dh
    L = I.staged_layout(B, H, T, dh)
    lens = [int(n) for n in key_lens]
    true_idx = key_idx.clone().long()
    idx = true_idx.clone()
    if defect == "prefix":                       # the gather ignored
        idx = torch.arange(T)[None].expand(B, -1).clone()
    elif defect == "off_by_one":
        idx = (idx + 1).clamp_max(T - 1)
    elif defect == "scene0":                     # scene 0's indices for every scene
        idx = idx[:1].expand(B, -1).clone()
    k = torch.zeros(B, H, L.n_tiles * 64, L.dhp)
    v = torch.zeros_like(k)
    sc = _scale(dh, scale)
    bias_bits = np.full((B, H, L.n_tiles * 64), -1, dtype=np.int32)         # (the fill: what no lane wrote)
    bias = bias_bits.view(np.float32)
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        k[b, :, :n, :dh] = ref.k[b][:, idx[b, :n]].float()
        v[b, :, :n, :dh] = ref.v[b][:, idx[b, :n]].float()
        if defect == "dead_row" and n % 64:
            v[b, :, n, 0] = 1.0
        if not euclid:
            continue
        if defect == "tile_past" and nt < L.n_tiles:
            bias_bits[b, :, nt * 64:(nt + 1) * 64] = 0                         # (the written all-zero tile comes with its bias)
        bias_bits[b, :, n:nt * 64] = 0
        val = (-0.5 * sc * ref.k[b][:, idx[b, :n]].pow(2).sum(-1)).float().numpy()          # [H, n]
        if defect == "bias_at_token":             # apply_row's own rule: the bias at the token's position, the compacted one never written
            bias[b][:, idx[b, :n].numpy()] = val
        else:
            bias[b, :, :n] = val
        if defect == "bias_dead" and n % 64:
            bias[b, :, n] = -1.0
    ws = I.encode(k, v, T, dh, aux=torch.from_numpy(bias.copy()), staged=True, total=total, fill=FILL)
    raw = ws.numpy()
    raw[L.aux_off:L.aux_end] = bias_bits.reshape(-1).view(np.uint8)         # (bit for bit: the fill is a NaN pattern)
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        if defect == "tile_past" and nt < L.n_tiles:
            nt += 1                               # a written (all-zero) tile past the count
        for h in range(H):                        # the skipped tiles of (b, h): the images stay as they were
            raw[I.tile_offset(L, b, h, 0) + nt * L.nimg * L.img:I.tile_offset(L, b, h, 0) + L.n_tiles * L.nimg * L.img] = FILL
    raw[L.images:L.aux_off] = FILL
    raw[L.aux_end:] = FILL
    return ws


DEFECTS = ("prefix", "off_by_one", "scene0", "dead_row", "tile_past", "bias_at_token", "bias_dead")

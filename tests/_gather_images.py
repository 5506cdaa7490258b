"""The gather rule of the K/V pre-pass as an executable statement (test infrastructure on top of tests/_images.py, which is imported
unchanged; plain numpy / torch on the CPU, no GPU, no kernel output).

`gta_attn_fwd_gather` (the GATHER instances of `gta_kv_prep_kernel`, gta_amd/csrc/gta_prep.hip) leaves the workspace of the two-stage plan
(`_images.fused_layout`) with the valid keys of every scene compacted:

  gather rule   image row r of tile j of scene b is `_images.ref_rows` of token key_idx[b, 64 j + r] -- that token's K / V row under that
                token's (cos, sin) row and its view's record --, for 64 j + r < key_lens[b]
  zero rule     rows at or past key_lens[b] in the last written tile, and the padded channels of every written row, are zero bytes
  skip rule     tiles with 64 j >= key_lens[b] keep what the workspace held, images and norm; so does every byte outside images and norms
  key norm      m <= kn <= m * 1.0001 * (1 + 2^-16), m = max over the tile's rows below key_lens[b] of |decoded K' row| in fp64

The element bars are those of tests/test_gpu_prep_images.py (derived there): untouched channels are the input's bits rounded to nearest even;
transformed ones lie within ulp(ref64) / 2 + 16 * 2^-24 * absprod of ref64.

`emulate` is the host emulation of the kernel: the reference rows gathered, rounded by `_images.encode`, with skipped tiles left at the fill.
`DEFECTS` are planted faults, each of which `check` must catch (tests/test_key_mask_host.py)."""
import numpy as np
import torch

from tests import _images as I

F_NORM = 1.0001


def index_tensors(mask):
    """bool [B, Tk] -> (key_idx [B, Tk], key_lens [B]) as int64 CPU tensors: the valid tokens first, ascending (a stable sort of ~mask)"""
    idx = torch.sort((~mask).to(torch.uint8), dim=1, stable=True).indices
    return idx, mask.sum(1)


def gathered(x, key_idx):
    """[B,H,T,...] -> the same with row p of scene b taken from token key_idx[b, p]"""
    B = x.shape[0]
    return torch.stack([x[b][:, key_idx[b].long()] for b in range(B)])


FILL = 0xFF                     # what the workspace holds before the call: an untouched 16- or 32-bit word reads -1


def check(name, ws, c, ref, key_idx, key_lens):
    """every rule of the module docstring on one workspace (CPU uint8 tensor) written over FILL bytes; c: `_images.key_side_case`-like (B, H,
    T, dh, k, v fp32 masters); ref: `_images.ref_rows` of the WHOLE key side; key_idx [B, T], key_lens [B] (only idx[b, :lens[b]] is looked at)"""
    B, H, T, dh = c.B, c.H, c.T, c.dh
    d = I.decode(ws, B, H, T, dh)
    L = d.layout
    lens = [int(n) for n in key_lens]
    assert all(1 <= n <= T for n in lens), lens
    raw = ws.numpy()
    untouched = aux_untouched = -1
    assert bool((raw[L.images:L.aux_off] == FILL).all()) and bool((raw[L.aux_end:] == FILL).all()), f"{name}: bytes outside the images and norms were written"
    rows = d.bits.permute(0, 1, 3, 2, 4, 5).reshape(B, H, L.nimg, L.n_tiles * 64, L.dhp)          # [B,H,image,position,channel]
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        assert bool((rows[b, :, :, nt * 64:] == untouched).all()), f"{name}: scene {b}: an image of a tile past the count was written"
        assert bool((d.aux_raw[b, :, nt:] == aux_untouched).all()), f"{name}: scene {b}: a norm of a tile past the count was written"
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
        print(f"GATHER_IMAGES {name} {what}: worst |img - ref| - bar = {excess.flatten()[w].item():.3e}")
        assert excess.flatten()[w].item() <= 0.0, (f"{name} {what}: scene {b} head {h} tile {p // 64} row {p % 64} (token {int(idx[b, p])}) channel {ch}: "
                                                   f"ref64 {r64.flatten()[w].item()!r} img {img.flatten()[w].item()!r}")
    kd = d.k.double()
    for b, n in enumerate(lens):
        for j in range((n + 63) // 64):
            m = kd[b, :, j * 64:min(n, (j + 1) * 64)].norm(dim=-1).max(dim=-1).values          # [H]
            kn = d.aux[b, :, j].double()
            ok = (m <= kn) & (kn <= m * F_NORM * (1 + 2.0 ** -16))
            assert bool(ok.all()), f"{name}: key norm of scene {b} tile {j}: m {m.tolist()} kn {kn.tolist()}"
    return d


def emulate(c, ref, key_idx, key_lens, total, defect=None):
    """the workspace bytes the gather pre-pass leaves on a FILL-filled workspace of `total` bytes, from the reference rows; defect: one of
    DEFECTS, planted"""
    B, H, T, dh = c.B, c.H, c.T, c.dh
    L = I.fused_layout(B, H, T, dh)
    lens = [int(n) for n in key_lens]
    idx = key_idx.clone().long()
    if defect == "prefix":                       # the gather ignored
        idx = torch.arange(T)[None].expand(B, -1).clone()
    elif defect == "off_by_one":
        idx = (idx + 1).clamp_max(T - 1)
    elif defect == "scene0":                     # scene 0's indices for every scene
        idx = idx[:1].expand(B, -1).clone()
    k = torch.zeros(B, H, L.n_tiles * 64, L.dhp)
    v = torch.zeros_like(k)
    for b, n in enumerate(lens):
        k[b, :, :n, :dh] = ref.k[b][:, idx[b, :n]].float()
        v[b, :, :n, :dh] = ref.v[b][:, idx[b, :n]].float()
        if defect == "dead_row" and n % 64:
            v[b, :, n, 0] = 1.0
    kb = I.bits_to_f32(I.bf16_bits(k)).double()
    kn = torch.zeros(B, H, L.n_tiles)
    for b, n in enumerate(lens):
        for j in range(L.n_tiles):
            hi = (j + 1) * 64 if defect == "norm_dead" else min(n, (j + 1) * 64)
            src = kb
            if defect == "norm_dead" and j == (n - 1) // 64 and n % 64:      # (a row that is not a key of the scene, as a norm over all 64 rows would see it)
                src = kb.clone()
                src[b, :, n] = 2.0 * kb[b, :, j * 64:n].abs().max() + 1.0
            if j * 64 < n:
                kn[b, :, j] = (src[b, :, j * 64:hi].norm(dim=-1).max(dim=-1).values * (1 + 2.0 ** -15)).float()
    ws = I.encode(k, v, T, dh, aux=kn, total=total, fill=FILL)
    raw = ws.numpy()
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        if defect == "tile_past" and nt < L.n_tiles:
            nt += 1                               # a written (all-zero) tile past the count
        for h in range(H):                        # the skipped tiles of (b, h): images and norms stay as they were
            raw[I.tile_offset(L, b, h, 0) + nt * L.nimg * L.img:I.tile_offset(L, b, h, 0) + L.n_tiles * L.nimg * L.img] = FILL
            a0 = L.aux_off + (b * H + h) * L.n_tiles * 4
            raw[a0 + nt * 4:a0 + L.n_tiles * 4] = FILL
    raw[L.images:L.aux_off] = FILL
    raw[L.aux_end:] = FILL
    return ws


DEFECTS = ("prefix", "off_by_one", "scene0", "dead_row", "tile_past", "norm_dead")

"""The K/V pre-pass workspace as an executable statement (test infrastructure; plain numpy / torch on the CPU, no GPU, no kernel output).

What `gta_kv_prep_kernel` (gta_amd/csrc/gta_prep.hip) and `gta_gen_prep_kernel` (gta_amd/csrc/gta_fwd_gen.hip) leave in the workspace, written
from the kernel sources:

  tile image    BN = 64 rows of CHP = dhp / 8 16-byte units, dhp = padded_dh(dh); unit c of row r holds channels 8c .. 8c+7 as bf16 and lies at
                byte (r * CHP + swz(CHP, r, c)) * 16 of the image (gta_common.h: swz_rot / swz)
  fused         tile (b, h, j) at ((b * H + h) * n_tiles + j) * nimg * IMG with IMG = 64 * dhp * 2 and the images [K' | V'] (nimg = 2), or
                [K'hi | V'hi | K'lo | V'lo] under GTA_FLAG_FP32_PRODUCTS (nimg = 4); behind the images, 256-byte aligned, B * H * n_tiles fp32
                key norms; behind those, 256-byte aligned, the q-side tiles (not modelled)     (gta_fwd2.hip: gta_fwd2_*_bytes, gta_abi.cpp: fwd_params)
  staged        [K' | V'] per tile in the same order; behind the images, 256-byte aligned, B * H * n_tiles * 64 fp32 bias values, value of key t
                of (b, h) at (b * H + h) * n_tiles * 64 + t, written under euclid only          (gta_fwd_gen.hip: gta_gen_*_bytes, gta_abi.cpp: staged_call)

`ref_rows` is the fp64 value of K' = rho_k K and V' = rho_k V computed from the very fp32 tables the kernels read (the view records with the
trans_coeff mask multiplied in fp32 as krec_source / apply_row do), so a comparison judges the pre-pass alone."""
from types import SimpleNamespace

import numpy as np
import torch

BN = 64
VREP_REP, VREP_D1, VREP_D2 = 16, 32, 41          # include/gta_hip.h: the slots of a packed view record the key side reads
GROUP_ORDER = ("triv", "se3", "so3", "so2", "t2")


def padded_dh(dh):
    """gta_abi.cpp: padded_dh"""
    return 32 if dh <= 32 else 64 if dh <= 64 else 96 if dh <= 96 else 128 if dh <= 128 else -1


def swz(units, r, u):
    """Python model of swz<UNITS>() in gta_amd/csrc/gta_common.h."""
    if units == 8:
        rot = 4 * ((r >> 1) & 1) + ((r >> 2) & 3)
    elif units == 16:
        rot = 4 * (r & 3) + ((r >> 2) & 3)
    else:
        tz = 4 if units % 16 == 0 else 3 if units % 8 == 0 else 2 if units % 4 == 0 else 1 if units % 2 == 0 else 0
        rot = (r >> (4 - tz)) & ((1 << tz) - 1)
    return (u + rot) % units


def unit_positions(chp):
    """[64, chp] int: the position (in 16-byte units within its row) of unit c of row r"""
    return np.array([[swz(chp, r, c) for c in range(chp)] for r in range(BN)], dtype=np.int64)


def _align256(n):
    return (n + 255) // 256 * 256


def fused_layout(B, H, Tk, dh, x3=False, Nq=0, esz=2):
    """byte offsets of the two-stage plan's workspace; total includes the q-side tiles of the one instance that has them (bf16 at dhp 96)"""
    dhp = padded_dh(dh)
    n_tiles = (Tk + BN - 1) // BN
    nimg, img = (4 if x3 else 2), BN * dhp * 2
    images = B * H * n_tiles * nimg * img
    norms_off = _align256(images)
    qtiles_off = norms_off + _align256(B * H * n_tiles * 4)
    total = qtiles_off + (B * Nq * 24 * 1024 if dhp == 96 and esz == 2 else 0)
    return SimpleNamespace(B=B, H=H, Tk=Tk, dh=dh, dhp=dhp, chp=dhp // 8, n_tiles=n_tiles, nimg=nimg, img=img, images=images, aux_off=norms_off,
                           aux_count=B * H * n_tiles, aux_end=norms_off + B * H * n_tiles * 4, qtiles_off=qtiles_off, total=total, staged=False)


def staged_layout(B, H, Tk, dh):
    """byte offsets of the staged generic forward's workspace"""
    dhp = padded_dh(dh)
    n_tiles = (Tk + BN - 1) // BN
    img = BN * dhp * 2
    images = B * H * n_tiles * 2 * img
    bias_off = _align256(images)
    total = bias_off + B * H * n_tiles * BN * 4
    return SimpleNamespace(B=B, H=H, Tk=Tk, dh=dh, dhp=dhp, chp=dhp // 8, n_tiles=n_tiles, nimg=2, img=img, images=images, aux_off=bias_off,
                           aux_count=B * H * n_tiles * BN, aux_end=total, qtiles_off=total, total=total, staged=True)


def tile_offset(L, b, h, j, image=0):
    """byte offset of image `image` of tile (b, h, j)"""
    return (((b * L.H + h) * L.n_tiles + j) * L.nimg + image) * L.img


def unit_offset(L, b, h, j, image, r, c):
    """byte offset of unit c (channels 8c .. 8c+7) of row r of that image"""
    return tile_offset(L, b, h, j, image) + (r * L.chp + swz(L.chp, r, c)) * 16


def _layout(B, H, Tk, dh, x3, staged):
    return staged_layout(B, H, Tk, dh) if staged else fused_layout(B, H, Tk, dh, x3)


def bf16_bits(x):
    """fp32 -> bf16 bits (int16), round to nearest even"""
    return x.to(torch.float32).to(torch.bfloat16).view(torch.int16)


def bits_to_f32(bits):
    return bits.view(torch.bfloat16).to(torch.float32)


def split_hi_lo(x):
    """the X3 pair of an fp32 value: hi = bf16(x), lo = bf16(x - hi)"""
    hi = x.to(torch.float32).to(torch.bfloat16).to(torch.float32)
    return hi, (x.to(torch.float32) - hi).to(torch.bfloat16).to(torch.float32)


def pad_rows(x, dhp=None):
    """[B,H,T,dh] -> [B,H,n_tiles*64,dhp], zero rows and zero channels added"""
    B, H, T, dh = x.shape
    dhp = dhp or padded_dh(dh)
    out = torch.zeros(B, H, (T + BN - 1) // BN * BN, dhp, dtype=x.dtype)
    out[:, :, :T, :dh] = x
    return out


def decode(ws, B, H, Tk, dh, x3=False, staged=False):
    """workspace bytes (CPU uint8 tensor or array) -> k, v (and k_lo, v_lo under x3) as fp32 [B,H,n_tiles*64,dhp]; bits: the bf16 bits of every
    image in logical order, int16 [B,H,n_tiles,nimg,64,dhp]; aux: the key norms [B,H,n_tiles] or the bias [B,H,n_tiles*64] as fp32, aux_raw: the
    same words as int32 (an untouched 0xFF fill reads -1)"""
    L = _layout(B, H, Tk, dh, x3, staged)
    raw = np.ascontiguousarray(ws.numpy() if torch.is_tensor(ws) else ws).view(np.uint8).reshape(-1)
    assert raw.size >= L.aux_end, (raw.size, L.aux_end)
    phys = raw[:L.images].view(np.int16).reshape(B, H, L.n_tiles, L.nimg, BN, L.chp, 8)
    pos = unit_positions(L.chp)
    logical = phys[:, :, :, :, np.arange(BN)[:, None], pos, :]                  # [..., 64, chp, 8]: unit c of row r
    bits = torch.from_numpy(np.ascontiguousarray(logical)).reshape(B, H, L.n_tiles, L.nimg, BN, L.dhp)
    f = bits_to_f32(bits)
    rows = lambda i: f[:, :, :, i].reshape(B, H, L.n_tiles * BN, L.dhp)
    aux_raw = torch.from_numpy(raw[L.aux_off:L.aux_end].copy().view(np.int32))
    shape = (B, H, L.n_tiles * BN) if staged else (B, H, L.n_tiles)
    return SimpleNamespace(k=rows(0), v=rows(1), k_lo=rows(2) if x3 else None, v_lo=rows(3) if x3 else None, bits=bits,
                           aux=aux_raw.view(torch.float32).reshape(shape), aux_raw=aux_raw.reshape(shape), layout=L)


def encode(k, v, Tk, dh, k_lo=None, v_lo=None, aux=None, staged=False, total=None, fill=0):
    """the inverse of decode: fp32 rows [B,H,n_tiles*64,dhp] (rounded to bf16, nearest even) and the norms / bias -> workspace bytes (uint8
    tensor of `total` bytes, at least the layout's; what the model does not cover holds `fill`)"""
    B, H = k.shape[:2]
    x3 = k_lo is not None
    L = _layout(B, H, Tk, dh, x3, staged)
    assert tuple(k.shape) == (B, H, L.n_tiles * BN, L.dhp) == tuple(v.shape), (k.shape, v.shape, L)
    imgs = [k, v] + ([k_lo, v_lo] if x3 else [])
    logical = torch.stack([bf16_bits(t).reshape(B, H, L.n_tiles, BN, L.chp, 8) for t in imgs], 3).numpy()
    phys = np.empty_like(logical)
    phys[:, :, :, :, np.arange(BN)[:, None], unit_positions(L.chp), :] = logical
    out = np.full(max(total or 0, L.total), fill, dtype=np.uint8)
    out[:L.images] = phys.reshape(-1).view(np.uint8)
    if aux is not None:
        a = aux.to(torch.float32).contiguous().reshape(-1).numpy()
        assert a.size == L.aux_count, (a.size, L.aux_count)
        out[L.aux_off:L.aux_end] = a.view(np.uint8)
    return torch.from_numpy(out)


def key_side_case(f_dims, so3_degree=0, dtype=torch.bfloat16, B=3, H=3, Nk=3, Pk=50, seed=0, Tq=0):
    """Seeded inputs of one key side: k, v fp32 masters rounded to `dtype`, as [B,H,T,dh] views of token-major [B,T,H,dh] storage (the packed
    projection's strides); oracle reps (fp32, self-attention; with Tq > 0 a decoder-like query side of one view of Tq rows, and q) and the
    tables gta_amd.pack_reps makes of them on the CPU"""
    import gta_amd
    from oracle import gta_oracle as O
    f_dims = {g: int(n) for g, n in f_dims.items()}
    dh, T = sum(f_dims.values()), Nk * Pk
    g = torch.Generator().manual_seed(1000 + seed)
    ex = {"input_transforms": O.random_extrinsics(B, Nk, g), "input_coord": torch.rand(B, Nk, Pk, 2, generator=g)}
    ak = {"f_dims": f_dims, "so2": f_dims.get("so2", 0) // 4, "so3": so3_degree, "max_freq_h": 1, "max_freq_w": 1}
    reps = O.encoder_reps(ak, ex)
    rnd = lambda t: t.to(dtype).to(torch.float32)
    k, v = (rnd(torch.randn(B, T, H, dh, generator=g)).permute(0, 2, 1, 3) for _ in range(2))
    q = None
    if Tq:
        ex["target_transforms"] = O.random_extrinsics(B, 2, g)[:, 1:]
        ex["target_coord"] = torch.rand(B, 1, Tq, 2, generator=g)
        reps = O.decoder_reps(ak, ex, reps)
        q = rnd(torch.randn(B, Tq, H, dh, generator=g)).permute(0, 2, 1, 3)
    packed = {name: t.clone() for name, t in gta_amd.pack_reps(dict(reps), f_dims).items()}
    return SimpleNamespace(f_dims=f_dims, so3=so3_degree if f_dims.get("so3", 0) > 0 else 0, dtype=dtype, B=B, H=H, Nk=Nk, Pk=Pk, T=T, dh=dh, Tq=Tq,
                           q=q, k=k, v=v, reps=reps, packed=packed, ak=ak)


def ulp_bf16(x):
    """spacing of the bf16 grid at x: 2^(floor(log2 |x|) - 7); 0 at 0"""
    a = x.double().abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7), torch.zeros_like(a))


def _mask(trans_coeff):
    """gta.py:40-44 as the kernels apply it (krec_source / apply_row): translation column times trans_coeff, last row [0 0 0 1]"""
    tc = torch.tensor(1.0 if trans_coeff is None else float(trans_coeff), dtype=torch.float32)
    m = torch.ones(4, 4, dtype=torch.float32)
    m[:3, 3] = tc
    m[3, :3] = 0.0
    return m


def rho_k(tables, f_dims, T, Nk, so3_degree=0, trans_coeff=None, euclid=False):
    """the key side's row transform x -> M x + off as fp64 [B,T,dh,dh], [B,T,dh] from the packed fp32 tables (vrep_k [B,Nk,72], cs_k
    [B,T,d_so2/2,2], coord_k [B,T,2]), and ident: the channels it leaves alone.  Slabs in GROUP_ORDER; per slab what chunk_apply / rot2_apply<false>
    (fused) and apply_row mode 1 (staged) compute -- the two agree wherever both serve a layout."""
    d = {g: int(f_dims.get(g, 0)) for g in GROUP_ORDER}
    dh = sum(d.values())
    some = next((t for t in (tables.get("vrep_k"), tables.get("cs_k"), tables.get("coord_k")) if t is not None), None)
    B = some.shape[0] if some is not None else 1
    M = torch.zeros(B, T, dh, dh, dtype=torch.float64)
    off = torch.zeros(B, T, dh, dtype=torch.float64)
    ident = torch.zeros(dh, dtype=torch.bool)
    view = torch.arange(T) // (T // Nk)
    ch = 0
    for _ in range(d["triv"]):
        M[:, :, ch, ch] = 1.0
        ident[ch] = True
        ch += 1
    if d["se3"] > 0:
        vrep = tables["vrep_k"].to(torch.float32)
        rec = (vrep[..., VREP_REP:VREP_REP + 16].reshape(B, Nk, 4, 4) * _mask(trans_coeff)).double()[:, view]      # fp32 product, as the kernels
        w = 3 if euclid else 4
        for _ in range(d["se3"] // w):
            M[:, :, ch:ch + w, ch:ch + w] = rec[..., :w, :w]
            if euclid:
                off[:, :, ch:ch + 3] = rec[..., :3, 3]                  # homogenisation: the translation column times 1
            ch += w
    if d["so3"] > 0:
        vrep = tables["vrep_k"].double()
        D = [(3, vrep[..., VREP_D1:VREP_D1 + 9].reshape(B, Nk, 3, 3)[:, view])]
        if so3_degree >= 2:
            D.append((5, vrep[..., VREP_D2:VREP_D2 + 25].reshape(B, Nk, 5, 5)[:, view]))
        for _ in range(d["so3"] // sum(w for w, _m in D)):
            for w, m in D:
                M[:, :, ch:ch + w, ch:ch + w] = m
                ch += w
    if d["so2"] > 0:
        cs = tables["cs_k"].double()
        assert cs.shape[1] == T and cs.shape[2] == d["so2"] // 2, (cs.shape, T, d["so2"])
        for blk in range(d["so2"] // 2):
            c, s = cs[:, :, blk, 0], cs[:, :, blk, 1]
            M[:, :, ch, ch], M[:, :, ch, ch + 1], M[:, :, ch + 1, ch], M[:, :, ch + 1, ch + 1] = c, -s, s, c
            ch += 2
    if d["t2"] > 0:
        co = tables["coord_k"].double()
        for _ in range(d["t2"] // 3):
            for i in range(3):
                M[:, :, ch + i, ch + i] = 1.0
            M[:, :, ch + 2, ch], M[:, :, ch + 2, ch + 1] = co[:, :, 0], co[:, :, 1]
            ident[ch] = ident[ch + 1] = True
            ch += 3
    assert ch == dh, (ch, dh)
    return M, off, ident


def ref_rows(k, v, tables, f_dims, Nk, so3_degree=0, trans_coeff=None, v_transform=True, euclid=False):
    """fp64 K' and V' [B,H,T,dh] of fp32 masters k, v [B,H,T,dh] (already rounded to the input type), absprod_k / absprod_v = sum_j |M_ij| |x_j|
    (+ |off_i|) per element, ident_k / ident_v: the channels whose value is the input's"""
    B, H, T, dh = k.shape
    M, off, ident = rho_k(tables, f_dims, T, Nk, so3_degree, trans_coeff, euclid)
    if M.shape[0] != B:
        M, off = M.expand(B, -1, -1, -1), off.expand(B, -1, -1)
    apply = lambda x: torch.einsum("btij,bhtj->bhti", M, x.double()) + off[:, None]
    absprod = lambda x: torch.einsum("btij,bhtj->bhti", M.abs(), x.double().abs()) + off.abs()[:, None]
    out = SimpleNamespace(k=apply(k), absprod_k=absprod(k), ident_k=ident, M=M, off=off)
    if v_transform:
        out.v, out.absprod_v, out.ident_v = apply(v), absprod(v), ident
    else:
        out.v, out.absprod_v, out.ident_v = v.double(), v.double().abs(), torch.ones(dh, dtype=torch.bool)
    return out

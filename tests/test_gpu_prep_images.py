"""GPU: the K/V pre-pass workspace itself -- the bf16 tile images of K' = rho_k K and V' = rho_k V, the per-tile key norms (two-stage plan,
`gta_kv_prep_kernel`) and the per-key euclid bias (staged route, `gta_gen_prep_kernel`) -- against fp64, element by element.

Every case calls a forward entry through ctypes with GTA_FLAG_PREP_ONLY on a workspace pre-filled with 0xFF bytes (q and out null), copies the
workspace back and decodes it with tests/_images.py, the model of the layout written from the kernel sources.  The reference is
`_images.ref_rows`: fp64 from the very fp32 tables the kernel reads.  The last test proves the decoder independently of the producer: a workspace
ENCODED on the host from the reference, handed to the attention kernels under GTA_FLAG_KV_READY, gives the oracle's attention.

Bars (derived; ulp(x) = 2^(floor(log2 |x|) - 7), err32 = 16 * 2^-24 * absprod with absprod = sum_j |M_ij| |x_j|: an fp32 dot product of at most
five terms errs by under 5 * 2^-24 of that, the view record's trans_coeff product by 2^-24 more):
  channels rho_k leaves alone   image bits == round-to-nearest-even bf16 of the input (for bf16 inputs: the input's bits)
  transformed channels          |img - ref64| <= ulp(ref64) / 2 + err32        (truncation errs by up to one ulp)
  X3 (FP32_PRODUCTS)            hi as above; |hi + lo - ref64| <= 2^-16 |ref64| + err32
  padded channels, rows past Tk, rows past key_lens[b] in the prefix's last tile: zero bytes in every image
  tiles wholly past key_lens[b] images, norms and bias keep the 0xFF fill; so does every byte behind the norms / bias and the alignment gap
  key norm                      m <= kn <= m * F * (1 + 2^-16), m = max over the tile's valid rows of |decoded K' row| in fp64 (hi + lo under
                                X3), F = 1.0001 (1.0002 under X3): the kernel's margin against its fp32 sum of at most 128 squares (< 1e-5)
  euclid bias                   |bias - ref| <= 0.5 scale (2 sum_i |k'_i| err32_i + (dh + 2) 2^-24 sum_i k'_i^2), ref = -0.5 scale sum_i k'_i^2
                                from ref_rows; exactly 0.0 for the rows past Tk or the prefix in a tile that is written
A failure names scene, head, tile, row and chunk of the worst element with its ref64, image value and absprod.

Shapes: B = 3, H = 3, 3 views of 50 tokens unless a case says otherwise -- Tk = 150 is tiles of 64, 64 and 22 rows with view boundaries inside
tiles (rows 50, 100), 9 row tiles (the work map's second group of 8 and its unused tail), K and V token-major ([B,T,H,dh] storage)."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch

from gta_amd import native
from oracle import gta_oracle as O
from tests import _hip_cases as C
from tests import _images as I
from tests.test_gpu_forward import REL_MAX, REL_RMS
from tests.test_gpu_staged import _bar as staged_bar

pytestmark = pytest.mark.gpu

TC = 0.37
VT, EU, X3F = native.FLAG_V_TRANSFORM, native.FLAG_EUCLID, native.FLAG_FP32_PRODUCTS
DTYPES = [torch.bfloat16, torch.float32]
_name = lambda dt: "bf16" if dt == torch.bfloat16 else "fp32"


def _half(dh):
    """se3 | so2 scaled from {"se3": dh/2, "so2": dh/2}, slabs rounded to multiples of 4"""
    se3 = int(round(dh / 2 / 4)) * 4
    return {"se3": se3, "so2": dh - se3}


@functools.lru_cache(maxsize=None)
def _case(f_items, so3, dtype, B=3, H=3, Nk=3, Pk=50, seed=0, Tq=0):
    """CPU masters, oracle reps and packed tables of one key side: built once, never written to"""
    return I.key_side_case(dict(f_items), so3, dtype, B, H, Nk, Pk, seed, Tq)


def _f(f_dims):
    return tuple(f_dims.items())


def _dev_kv(c, contiguous=False):
    k, v = (t.to(c.dtype).cuda() for t in (c.k, c.v))
    if contiguous:
        k, v = k.contiguous(), v.contiguous()
    else:
        assert k.stride() == (c.T * c.H * c.dh, c.dh, c.H * c.dh, 1)          # token-major: k_st = H * dh
    return k, v


def _prep(c, k, v, packed, *, staged=False, euclid=False, v_transform=True, x3=False, key_lens=None, tc=TC, Nk=None):
    """one PREP_ONLY call of the entry (fused / staged, plain / varlen) on a 0xFF-filled workspace -> its bytes on the CPU"""
    B, H, T, dh = k.shape
    Nk = Nk or c.Nk
    flags = (VT if v_transform else 0) | (EU if euclid else 0) | (X3F if x3 else 0) | native.FLAG_PREP_ONLY
    st = [tuple(k.stride()[:3]), tuple(k.stride()[:3]), tuple(v.stride()[:3]), tuple(k.stride()[:3])]
    desc = native.make_desc_from(c.dtype, (B, H, T, dh), T, st, c.f_dims, c.so3, Nk, Nk, dh ** -0.5, flags)
    L = native.lib()
    if staged:
        assert native.attn_fwd_staged_supported(desc) == 0
        need = native.attn_fwd_staged_workspace_bytes(desc)
        assert need == I.staged_layout(B, H, T, dh).total
    else:
        assert native.attn_fwd_supported(desc) == 0
        need = native.attn_fwd_workspace_bytes(desc)
        assert need == I.fused_layout(B, H, T, dh, x3, Nk, 2 if c.dtype == torch.bfloat16 else 4).total
    ws = torch.full((need,), 0xFF, device="cuda", dtype=torch.uint8)
    dev = {n: (t.cuda() if t is not None else None) for n, t in packed.items()}
    tcd = torch.tensor([tc], device="cuda") if c.f_dims.get("se3", 0) > 0 else None
    p = native._ptr
    vrep, cs, coord = p(dev.get("vrep_k")), p(dev.get("cs_k")), p(dev.get("coord_k"))      # (the q side of a PREP_ONLY call is never read)
    kl = torch.tensor(key_lens, device="cuda", dtype=torch.int32) if key_lens is not None else None
    if staged:
        if kl is None:
            rc = L.gta_attn_fwd_staged(ctypes.byref(desc), None, p(k), p(v), vrep, vrep, cs, cs, coord, coord, p(tcd), None, None, None,
                                       p(ws), ws.numel(), native._stream())
        else:
            rc = L.gta_attn_fwd_staged_varlen(ctypes.byref(desc), None, p(k), p(v), vrep, vrep, cs, cs, coord, coord, p(tcd), None, p(kl),
                                              None, None, p(ws), ws.numel(), native._stream())
    elif kl is None:
        rc = L.gta_attn_fwd(ctypes.byref(desc), None, p(k), p(v), vrep, vrep, cs, cs, p(tcd), None, None, None, p(ws), ws.numel(), native._stream())
    else:
        rc = L.gta_attn_fwd_varlen(ctypes.byref(desc), None, p(k), p(v), vrep, vrep, cs, cs, p(tcd), None, p(kl), None, None, p(ws), ws.numel(),
                                   native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    return ws.cpu()


def _where(idx, shape):
    """flat index idx into a [B,H,T,dh] tensor -> scene, head, tile, row and chunk as text"""
    b, h, t, ch = np.unravel_index(int(idx), shape)
    return f"scene {b} head {h} tile {t // 64} row {t % 64} (token {t}) chunk {ch // 8} channel {ch}"


def _assert_within(name, img, ref, bar, absprod, sel):
    """|img - ref| <= bar on the selected elements, or the worst element named"""
    excess = ((img.double() - ref).abs() - bar)
    excess = torch.where(sel, excess, torch.full_like(excess, -1.0))
    excess = torch.where(torch.isnan(excess), torch.full_like(excess, float("inf")), excess)
    worst = int(excess.argmax())
    err = (img.double() - ref).abs().flatten()[worst].item()
    print(f"PREP_IMAGES {name}: worst |img - ref| - bar = {excess.flatten()[worst].item():.3e} (err {err:.3e}, bar {bar.flatten()[worst].item():.3e})")
    assert excess.flatten()[worst].item() <= 0.0, (
        f"{name}: {_where(worst, tuple(ref.shape))}: ref64 {ref.flatten()[worst].item()!r} img {img.flatten()[worst].item()!r} "
        f"absprod {absprod.flatten()[worst].item()!r} err {err:.4e} bar {bar.flatten()[worst].item():.4e}")


def _check(name, ws, c, ref, *, lens=None, staged=False, euclid=False, x3=False):
    """every rule of the module docstring on one decoded workspace; lens: valid keys per scene (None: Tk everywhere)"""
    B, H, T, dh = c.B, c.H, c.T, c.dh
    d = I.decode(ws, B, H, T, dh, x3=x3, staged=staged)
    L = d.layout
    lens = [T] * B if lens is None else list(lens)
    raw = ws.numpy()
    assert bool((raw[L.images:L.aux_off] == 0xFF).all()) and bool((raw[L.aux_end:] == 0xFF).all()), f"{name}: bytes outside the images and norms / bias were written"
    rows = d.bits.permute(0, 1, 3, 2, 4, 5).reshape(B, H, L.nimg, L.n_tiles * 64, L.dhp)          # [B,H,image,token,channel]
    scale = float(np.float32(dh ** -0.5))
    err32 = lambda ap: 16.0 * 2.0 ** -24 * ap
    for b, n in enumerate(lens):
        nt = (n + 63) // 64
        # tiles wholly past the prefix: nobody wrote them
        assert bool((rows[b, :, :, nt * 64:] == -1).all()), f"{name}: scene {b}: an image of a tile past the prefix was written"
        aux_past = d.aux_raw[b, :, nt * 64:] if staged else d.aux_raw[b, :, nt:]
        assert bool((aux_past == -1).all()), f"{name}: scene {b}: a norm / bias of a tile past the prefix was written"
        # rows past the prefix (or Tk) in its last tile, and the padded channels of every written tile: zero bytes
        assert bool((rows[b, :, :, n:nt * 64] == 0).all()), f"{name}: scene {b}: rows {n}..{nt * 64 - 1} are not zero rows in every image"
        assert bool((rows[b, :, :, :nt * 64, dh:] == 0).all()), f"{name}: scene {b}: padded channels are not zero"
    for img_i, (what, x, r64, ap, ident) in enumerate((("K'", c.k, ref.k, ref.absprod_k, ref.ident_k), ("V'", c.v, ref.v, ref.absprod_v, ref.ident_v))):
        valid = torch.zeros(B, 1, T, 1, dtype=torch.bool)
        for b, n in enumerate(lens):
            valid[b, :, :n] = True
        hi_bits = rows[:, :, img_i, :T, :dh]
        hi = I.bits_to_f32(hi_bits)
        # untouched channels: the bits of the input rounded to nearest even
        same = (hi_bits == I.bf16_bits(x)) | ~valid | ~ident
        assert bool(same.all()), f"{name} {what}: an untransformed element is not RNE(input): {_where(int((~same).flatten().int().argmax()), tuple(x.shape))}"
        sel = (valid & ~ident).expand_as(r64)
        if bool(sel.any()):
            _assert_within(f"{name} {what}", hi, r64, I.ulp_bf16(r64) / 2 + err32(ap), ap, sel)
        if x3:
            lo_bits = rows[:, :, 2 + img_i, :T, :dh]
            lo = I.bits_to_f32(lo_bits)
            same = (lo_bits == I.bf16_bits(x - hi)) | ~valid | ~ident
            assert bool(same.all()), f"{name} {what}: lo of an untransformed element is not RNE(input - hi)"
            _assert_within(f"{name} {what} hi+lo", hi.double() + lo.double(), r64, 2.0 ** -16 * r64.abs() + err32(ap), ap, valid.expand_as(r64))
    if not staged:
        kd = d.k.double() + (d.k_lo.double() if x3 else 0.0)
        F = 1.0002 if x3 else 1.0001
        ratios = []
        for b, n in enumerate(lens):
            for j in range((n + 63) // 64):
                m = kd[b, :, j * 64:min(n, (j + 1) * 64)].norm(dim=-1).max(dim=-1).values          # [H]
                kn = d.aux[b, :, j].double()
                ok = (m <= kn) & (kn <= m * F * (1 + 2.0 ** -16))
                ratios += (kn / m - 1).tolist()
                assert bool(ok.all()), f"{name}: key norm of scene {b} tile {j}: m {m.tolist()} kn {kn.tolist()} (factor {F})"
        print(f"PREP_IMAGES {name} norms: kn / m - 1 in [{min(ratios):.6e}, {max(ratios):.6e}] (bar [0, {F * (1 + 2.0 ** -16) - 1:.6e}])")
    elif euclid:
        rb = -0.5 * scale * ref.k.pow(2).sum(-1)                                                    # [B,H,T]
        bar = 0.5 * scale * (2 * (ref.k.abs() * err32(ref.absprod_k)).sum(-1) + (dh + 2) * 2.0 ** -24 * ref.k.pow(2).sum(-1))
        for b, n in enumerate(lens):
            nt = (n + 63) // 64
            e = (d.aux[b, :, :n].double() - rb[b, :, :n]).abs() - bar[b, :, :n]
            w = int(torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e).argmax())
            h, t = np.unravel_index(w, tuple(e.shape))
            print(f"PREP_IMAGES {name} bias scene {b}: worst err - bar {e.flatten()[w].item():.3e} (bar {bar[b, h, t].item():.3e})")
            assert e.flatten()[w].item() <= 0.0, f"{name}: bias of scene {b} head {h} key {t}: {d.aux[b, h, t].item()!r} ref {rb[b, h, t].item()!r} bar {bar[b, h, t].item():.3e}"
            assert bool((d.aux_raw[b, :, n:nt * 64] == 0).all()), f"{name}: scene {b}: the bias of a row past the prefix is not 0.0"
    else:
        assert bool((d.aux_raw == -1).all()), f"{name}: a bias was written without euclid"
    return d


def _run(name, f_dims, so3, dtype, *, staged=False, euclid=False, v_transform=True, x3=False, contiguous=False, **shape):
    c = _case(_f(f_dims), so3, dtype, **shape)
    tc = TC if c.f_dims.get("se3", 0) > 0 else None
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, c.so3, tc, v_transform, euclid)
    k, v = _dev_kv(c, contiguous)
    t0 = time.perf_counter()
    ws = _prep(c, k, v, c.packed, staged=staged, euclid=euclid, v_transform=v_transform, x3=x3)
    _check(name, ws, c, ref, staged=staged, euclid=euclid, x3=x3)
    print(f"PREP_IMAGES {name}: {time.perf_counter() - t0:.2f} s")
    return ws


# ---- 1. the fused pre-pass, every instance -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("dh", [16, 32, 40, 64, 96, 104, 128])
def test_fused_every_instance(dh, dtype):
    """se3 | so2 at every padded size, with the head sizes that leave chunks unused (16: 2 of 4, 40: 5 of 8, 104: 13 of 16)"""
    _run(f"fused dh{dh} {_name(dtype)}", _half(dh), 0, dtype)


# ---- 2. each layout kind at its smallest padded size ---------------------------------------------------------------------------------------
KINDS = {
    "ms96": ({"se3": 48, "so3": 24, "so2": 24}, 2, True),                 # the compile-time MS layout
    "so3-32": ({"se3": 8, "so3": 8, "so2": 16}, 2, True),                 # the same kinds through the chunk table
    "so2": ({"so2": 32}, 0, True),
    "se3": ({"se3": 32}, 0, True),
    "mixed-halves": ({"triv": 4, "se3": 12, "so2": 16}, 0, True),         # chunks of two kinds: the generic body of the pre-pass
    "triv": ({"triv": 32}, 0, True),                                      # no tables passed
    "no-v-transform": ({"se3": 32, "so2": 32}, 0, False),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_fused_layout_kinds(kind, dtype):
    f, so3, xv = KINDS[kind]
    _run(f"fused {kind} {_name(dtype)}", f, so3, dtype, v_transform=xv, seed=1)


def test_contiguous_rows_give_the_same_bytes():
    """[B,H,T,dh] contiguous K and V against the token-major views: the row gather does not enter the result"""
    a = _run("fused dh64 bf16", _half(64), 0, torch.bfloat16)
    b = _run("fused dh64 bf16 contiguous", _half(64), 0, torch.bfloat16, contiguous=True)
    assert torch.equal(a, b)


# ---- 3. X3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dh", [32, 64])
def test_fused_split_bf16_images(dh):
    """GTA_FLAG_FP32_PRODUCTS: four images per tile, [K'hi | V'hi | K'lo | V'lo]"""
    _run(f"x3 dh{dh}", _half(dh), 0, torch.float32, x3=True, seed=2)


# ---- 4. tail shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tk", [40, 64, 71])
def test_fused_tail_shapes(Tk):
    """one scene, one head: one ragged tile, exactly one tile, one tile and seven rows"""
    _run(f"tail Tk{Tk}", _half(64), 0, torch.bfloat16, B=1, H=1, Nk=1, Pk=Tk, seed=3)


# ---- 5. / 6. per-scene key prefixes --------------------------------------------------------------------------------------------------------
KV_VIEWS = [1, 2, 3, 4]             # of 4 views of 32 tokens (Tk = 128, two tiles): mid-tile, exactly one tile, mid second tile, all


def _poisoned(c):
    """K, V and the key-side tables with everything of a padded view set to NaN"""
    k, v = (t.to(c.dtype).cuda().clone() for t in (c.k, c.v))
    pk = {n: t.clone() for n, t in c.packed.items()}
    for b, n in enumerate(KV_VIEWS):
        k[b, :, n * c.Pk:] = float("nan")
        v[b, :, n * c.Pk:] = float("nan")
        for name, cut in (("vrep_k", n), ("cs_k", n * c.Pk), ("coord_k", n * c.Pk)):
            if name in pk:
                pk[name][b, cut:] = float("nan")
    assert k.stride() == (c.T * c.H * c.dh, c.dh, c.H * c.dh, 1)
    return k, v, pk


def _varlen(name, f_dims, so3, dtype, staged=False, euclid=False):
    c = _case(_f(f_dims), so3, dtype, B=4, H=3, Nk=4, Pk=32, seed=4)
    tc = TC if c.f_dims.get("se3", 0) > 0 else None
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, c.so3, tc, True, euclid)            # (from the clean tables: the valid rows are theirs)
    lens = [n * c.Pk for n in KV_VIEWS]
    k, v, pk = _poisoned(c)
    t0 = time.perf_counter()
    ws = _prep(c, k, v, pk, staged=staged, euclid=euclid, key_lens=lens)
    d = _check(name, ws, c, ref, lens=lens, staged=staged, euclid=euclid)
    # scene b's tiles and norms / bias: byte for byte those of a call on the scene alone with its key side cut to the prefix
    for b, n in enumerate(KV_VIEWS):
        T = n * c.Pk
        cut = {"vrep_k": n, "cs_k": T, "coord_k": T}
        pk1 = {nm: t[b:b + 1, :cut[nm]].contiguous() for nm, t in pk.items() if nm in cut}
        ws1 = _prep(c, k[b:b + 1, :, :T], v[b:b + 1, :, :T], pk1, staged=staged, euclid=euclid, Nk=n)
        d1 = I.decode(ws1, 1, c.H, T, c.dh, staged=staged)
        nt = d1.layout.n_tiles
        assert torch.equal(d.bits[b, :, :nt], d1.bits[0]), f"{name}: scene {b}: the images differ from those of the scene alone"
        aux = d.aux_raw[b, :, :nt * 64] if staged else d.aux_raw[b, :, :nt]
        assert torch.equal(aux, d1.aux_raw[0]), f"{name}: scene {b}: the norms / bias differ from those of the scene alone"
    print(f"PREP_IMAGES {name}: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("dh", [64, 96])
def test_fused_varlen(dh, dtype):
    """gta_attn_fwd_varlen, padded views all NaN: zero rows, skipped tiles, and the bytes of the cut-down call"""
    f = {"se3": 32, "so2": 32} if dh == 64 else {"se3": 48, "so3": 24, "so2": 24}
    _varlen(f"varlen dh{dh} {_name(dtype)}", f, 2 if dh == 96 else 0, dtype)


STAGED = {
    "euclid64": ({"triv": 2, "se3": 30, "so2": 32}, True),
    "t2-64": ({"triv": 2, "se3": 32, "t2": 30}, False),
    "t2-96": ({"se3": 48, "t2": 48}, False),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("kind", sorted(STAGED))
def test_staged_images_and_bias(kind, dtype):
    f, euclid = STAGED[kind]
    _run(f"staged {kind} {_name(dtype)}", f, 0, dtype, staged=True, euclid=euclid, seed=5)


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_staged_varlen(dtype):
    """gta_attn_fwd_staged_varlen on the euclid layout with the prefixes of the fused case"""
    _varlen(f"staged varlen {_name(dtype)}", STAGED["euclid64"][0], 0, dtype, staged=True, euclid=True)


# ---- 7. the decoder is what the attention kernels read -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fused32", "fused64", "fused96", "euclid64"])
def test_attention_reads_a_host_encoded_workspace(kind):
    """A workspace encoded on the host from ref_rows (norms 1.0001 m; the bias under euclid), the full entry under GTA_FLAG_KV_READY with k and v
    junk, Tq = 70: out and LSE against the fp64 oracle under the bars of the file each family's bars come from -- tests/test_gpu_forward.py
    (REL_MAX, REL_RMS, LSE 2e-2; at its trans_coeff 0.01) and tests/test_gpu_staged.py (_bar and its LSE bound; trans_coeff 0.37).  No pre-pass
    runs, so the cases above cannot pass by a decoder fitted to the producer."""
    staged = kind == "euclid64"
    f = STAGED["euclid64"][0] if staged else _half(int(kind[5:]))
    tc = TC if staged else 0.01
    dtype, Tq = torch.bfloat16, 70
    c = _case(_f(f), 0, dtype, seed=6, Tq=Tq)
    B, H, T, dh, scale = c.B, c.H, c.T, c.dh, c.dh ** -0.5
    ref = I.ref_rows(c.k, c.v, c.packed, c.f_dims, c.Nk, 0, tc, True, staged)
    q, k, v = c.q.to(dtype).cuda(), *_dev_kv(c)
    junk = torch.full_like(k, 3.0)
    out = torch.empty(B, Tq, H, dh, device="cuda", dtype=dtype).permute(0, 2, 1, 3)
    lse = torch.empty(B, H, Tq, device="cuda", dtype=torch.float32)
    flags = VT | (EU if staged else 0) | native.FLAG_KV_READY
    desc = native.make_desc(q, junk, junk, out, c.f_dims, 0, 1, c.Nk, scale, flags)
    need = native.attn_fwd_staged_workspace_bytes(desc) if staged else native.attn_fwd_workspace_bytes(desc)
    kp, vp = I.pad_rows(ref.k.float()), I.pad_rows(ref.v.float())
    if staged:
        aux = torch.zeros(B, H, kp.shape[2])
        aux[:, :, :T] = (-0.5 * float(np.float32(scale)) * ref.k.pow(2).sum(-1)).float()
    else:
        rounded = I.bits_to_f32(I.bf16_bits(kp)).double()
        aux = (1.0001 * rounded.reshape(B, H, -1, 64, kp.shape[-1]).norm(dim=-1).max(dim=-1).values).float()
    ws = I.encode(kp, vp, T, dh, aux=aux, staged=staged, total=need, fill=0xFF).cuda()
    dev = {n: t.cuda() for n, t in c.packed.items()}
    tcd = torch.tensor([tc], device="cuda")
    p, L = native._ptr, native.lib()
    if staged:
        rc = L.gta_attn_fwd_staged(ctypes.byref(desc), p(q), p(junk), p(junk), p(dev["vrep_q"]), p(dev["vrep_k"]), p(dev["cs_q"]), p(dev["cs_k"]),
                                   None, None, p(tcd), None, p(out), p(lse), p(ws), ws.numel(), native._stream())
    else:
        rc = L.gta_attn_fwd(ctypes.byref(desc), p(q), p(junk), p(junk), p(dev["vrep_q"]), p(dev["vrep_k"]), p(dev["cs_q"]), p(dev["cs_k"]),
                            p(tcd), None, p(out), p(lse), p(ws), ws.numel(), native._stream())
    assert rc == 0, L.gta_strerror(rc)
    torch.cuda.synchronize()
    reps64 = {n: ([t.double() for t in r] if isinstance(r, list) else r.double()) for n, r in c.reps.items()}
    q64, k64, v64 = c.q.double(), c.k.double(), c.v.double()
    ref_out, _ = O.gta_attention(q64, k64, v64, c.f_dims, reps64, tc, True, staged, scale=scale)
    qt, kt, _ = O.transform_qkv(q64, k64, v64, c.f_dims, reps64, tc, True, staged)
    sim = scale * qt @ kt.transpose(-1, -2)
    if staged:
        sim = sim - 0.5 * scale * kt.pow(2).sum(-1)[..., None, :]
    ref_lse = torch.logsumexp(sim, -1)
    st = C.err_stats(out.float().cpu(), ref_out.float())
    lse_err = (lse.double().cpu() - ref_lse).abs().max().item()
    print(f"PREP_IMAGES kv_ready {kind}: {st} | lse max_abs {lse_err:.3e}")
    if staged:
        lse_bar = 1.01 * 2.0 ** -8 * scale * (qt.norm(dim=-1).max() * kt.norm(dim=-1).max()).item() + 1e-4          # (tests/test_gpu_staged.py)
        assert staged_bar(st), (kind, st)
        assert lse_err <= lse_bar, (kind, lse_err, lse_bar)
    else:
        assert st["finite"] and st["max_abs"] <= REL_MAX * st["ref_max"] and st["rel_rms"] <= REL_RMS, (kind, st)
        assert lse_err < 2e-2, (kind, lse_err)

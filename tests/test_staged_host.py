"""Host logic of the staged generic forward (no GPU): the three C entries exist, what `gta_attn_fwd_staged_supported` answers for the run
configs without a fused kernel and for the requests it refuses, the workspace-size rule, and the `generic_route` decision table."""
import os
import re

import pytest
import torch

from gta_amd import gta as G2
from gta_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

B, H, TQ, TK, NQ, NK = 4, 12, 640, 320, 2, 5
VT, EU = native.FLAG_V_TRANSFORM, native.FLAG_EUCLID


def _desc(f_dims, flags=VT, so3_degree=0, dtype=torch.bfloat16, Tq=TQ, Tk=TK, dh=None):
    dh = sum(f_dims.values()) if dh is None else dh
    qs, ks = (H * Tq * dh, Tq * dh, dh), (H * Tk * dh, Tk * dh, dh)
    return native.make_desc_from(dtype, (B, H, Tq, dh), Tk, (qs, ks, ks, qs), f_dims, so3_degree, NQ, NK, dh ** -0.5, flags)


def _reason(rc):
    return native.lib().gta_strerror(rc).decode()


# (f_dims, flags, so3 degree) of the four run configs the fused kernels refuse, the t2 / so2 mix and so3 of degree 1
SERVED = {
    "clevrtr/gta_euclid": ({"triv": 2, "se3": 30, "so2": 32}, VT | EU, 0),
    "clevrtr/gta_t2": ({"se3": 32, "t2": 30, "triv": 2}, VT, 0),
    "msn/gta_so3_euclid": ({"triv": 0, "se3": 48, "so2": 24, "so3": 24}, VT | EU, 2),
    "msn/gta_t2": ({"triv": 0, "se3": 48, "t2": 48}, VT, 0),
    "so2+t2": ({"so2": 8, "t2": 24}, VT, 0),
    "so3 degree 1": ({"se3": 48, "so3": 24, "so2": 24}, VT, 1),
}


def test_staged_symbols_in_header_library_and_bindings():
    header = open(ROOT + "/include/gta_hip.h").read()
    for name in ("gta_attn_fwd_staged", "gta_attn_fwd_staged_supported", "gta_attn_fwd_staged_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in native.ABI_SYMBOLS
        assert hasattr(native.lib(), name), name


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name", sorted(SERVED))
def test_staged_supported_layouts(name, dtype):
    f_dims, flags, L = SERVED[name]
    d = _desc(f_dims, flags, L, dtype)
    assert native.attn_fwd_staged_supported(d) == 0, _reason(native.attn_fwd_staged_supported(d))
    assert native.attn_fwd_supported(d) == -3               # the fused entry keeps refusing them
    d.flags = flags & ~VT
    assert native.attn_fwd_staged_supported(d) == 0


def test_staged_refusals_and_their_reasons():
    rc = native.attn_fwd_staged_supported(_desc({"se3": 6, "so2": 8}, VT | EU))
    assert rc == -3 and "dh % 8" in _reason(rc)
    rc = native.attn_fwd_staged_supported(_desc({"triv": 136}, VT))
    assert rc == -3 and "dh <= 128" in _reason(rc)
    served = SERVED["clevrtr/gta_t2"][0]
    rc = native.attn_fwd_staged_supported(_desc(served, VT | native.FLAG_FP32_PRODUCTS, dtype=torch.float32))
    assert rc == -3 and "GTA_FLAG_FP32_PRODUCTS" in _reason(rc)
    rc = native.attn_fwd_staged_supported(_desc(served, VT | native.FLAG_PRETRANSFORMED))
    assert rc == -3 and "GTA_FLAG_PRETRANSFORMED" in _reason(rc)
    assert native.attn_fwd_staged_supported(_desc({"se3": 32, "t2": 30}, VT, dh=64)) == -2          # slabs that do not sum
    assert native.attn_fwd_staged_supported(_desc({"se3": 32, "t2": 32}, VT)) == -2                 # t2 slab not 3-channel groups
    assert native.attn_fwd_staged_supported(_desc({"se3": 32, "so2": 32}, VT | EU)) == -2           # euclid: se3 slab of 3-vectors
    d = _desc(served, VT)
    d.q_stride[2] = 68                                                                                # rows off the 16-byte grid
    assert native.attn_fwd_staged_supported(d) == -1
    d = _desc(served, VT)
    d.abi_version = 1
    assert native.attn_fwd_staged_supported(d) == -1


def test_staged_workspace_size():
    """[K' image | V' image] of bf16 per 64-key tile at the padded head size, 256-byte aligned, + 64 fp32 bias values per tile; the query side,
    the input type and the flags do not enter; 0 for a refused descriptor"""
    for name, (f_dims, flags, L) in SERVED.items():
        dh = sum(f_dims.values())
        dhp = (dh + 31) // 32 * 32
        for Tk in (320, 300, 65):
            n_tiles = (Tk + 63) // 64
            want = (B * H * n_tiles * 2 * 64 * dhp * 2 + 255) // 256 * 256 + B * H * n_tiles * 64 * 4
            if Tk % NK:
                continue
            assert native.attn_fwd_staged_workspace_bytes(_desc(f_dims, flags, L, Tk=Tk)) == want, (name, Tk)
            assert native.attn_fwd_staged_workspace_bytes(_desc(f_dims, flags, L, torch.float32, Tq=2 * TQ, Tk=Tk)) == want
    assert native.attn_fwd_staged_workspace_bytes(_desc({"se3": 6, "so2": 8}, VT | EU)) == 0


def test_generic_route_table():
    for name, (f_dims, flags, L) in SERVED.items():
        dh = sum(f_dims.values())
        eu = bool(flags & EU)
        args = ((B, H, TQ, dh), TK, torch.bfloat16, f_dims, L, NQ, NK)
        assert G2.attention_route(*args, euclid=eu) is None, name
        assert G2.generic_route(*args, euclid=eu) == "staged", name
        assert G2.generic_route(*args, euclid=eu, v_transform=False) == "staged", name
        assert G2.generic_route(*args, euclid=eu, needs_grad=True) == "apply", name
        args32 = ((B, H, TQ, dh), TK, torch.float32, f_dims, L, NQ, NK)
        assert G2.generic_route(*args32, euclid=eu) == "staged", name
        assert G2.generic_route(*args32, euclid=eu, precise=True) == "apply", name
    # the fixture sizes of the ablation tests (dh % 8 != 0) keep today's route
    assert G2.generic_route((B, H, TQ, 14), TK, torch.float32, {"se3": 6, "so2": 8}, 0, NQ, NK, euclid=True) == "apply"
    assert G2.generic_route((B, H, TQ, 18), TK, torch.float32, {"se3": 8, "so2": 4, "t2": 6}, 0, NQ, NK) == "apply"
    assert G2.generic_route((B, H, TQ, 64), TK, torch.float16, SERVED["clevrtr/gta_t2"][0], 0, NQ, NK) == "apply"

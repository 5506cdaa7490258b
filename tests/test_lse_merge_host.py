"""Host side of `return_lse`, `gta_attention_merge` and `gta_attention_by_view_groups` (no GPU): the new entries are declared in the header,
exported by the library and bound with as many arguments as the header gives them; the combinations `return_lse` does not serve under grad
are refused by name before anything touches a device; `gta_attention_by_view_groups` refuses what a per-group call cannot honour."""
import ctypes
import os
import re

import pytest
import torch

import gta_amd
from gta_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "gta_hip.h")).read()
NEW = ("gta_attn_merge", "gta_attn_merge_bwd", "gta_attn_bwd_dlse", "gta_attn_bwd_dlse_supported")


def _decl(name):
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*?)\)\s*;", HEADER, re.M | re.S)
    assert m, name
    return [a.strip() for a in m.group(1).replace("\n", " ").split(",")]


def test_symbols_are_declared_exported_and_bound():
    L = native.lib()
    for s in NEW:
        assert s in native.ABI_SYMBOLS and hasattr(L, s), s
        assert len(getattr(L, s).argtypes) == len(_decl(s)), s
    assert native.GTA_ABI_VERSION == 2 and L.gta_abi_version() == 2
    # gta_attn_bwd_dlse: gta_attn_bwd's arguments with `const float* dlse` behind lse
    args, base = _decl("gta_attn_bwd_dlse"), _decl("gta_attn_bwd")
    i = [a.split()[-1] for a in args].index("dlse")
    assert args[i] == "const float* dlse" and args[i - 1].split()[-1] == "lse" and args[:i] + args[i + 1:] == base
    at = L.gta_attn_bwd_dlse.argtypes
    assert L.gta_attn_bwd.argtypes == at[:i] + at[i + 1:] and at[i] == ctypes.c_void_p
    assert _decl("gta_attn_bwd_dlse_supported") == ["const GtaAttnDesc* desc"]
    # the merges: six int32 sizes, then pointer / stride pairs, the stream last
    for s in ("gta_attn_merge", "gta_attn_merge_bwd"):
        args, at = _decl(s), getattr(L, s).argtypes
        assert [a.split()[-1] for a in args[:6]] == ["dtype", "n", "B", "H", "Tq", "dh"] and at[:6] == [ctypes.c_int32] * 6
        for a, t in zip(args[6:], at[6:]):
            if a.startswith("const int64_t*"):
                assert t == ctypes.POINTER(ctypes.c_int64), (s, a)
            elif "* const*" in a:
                assert t == ctypes.POINTER(ctypes.c_void_p), (s, a)
            else:
                assert t == ctypes.c_void_p, (s, a)


def test_bwd_dlse_supported_answers_like_the_backward():
    def desc(f_dims, flags, dh=64, dtype=torch.bfloat16):
        qs = (2 * 32 * dh, 32 * dh, dh)
        return native.make_desc_from(dtype, (1, 2, 32, dh), 32, (qs, qs, qs, qs), f_dims, 0, 1, 1, 1.0, flags)
    cl = {"se3": 32, "so2": 32}
    assert native.attn_bwd_dlse_supported(desc(cl, native.FLAG_V_TRANSFORM)) == 0
    assert native.attn_bwd_dlse_supported(desc(cl, native.FLAG_V_TRANSFORM | native.FLAG_FP32_PRODUCTS, dtype=torch.float32)) == 0
    for d in (desc(cl, native.FLAG_V_TRANSFORM | native.FLAG_PRETRANSFORMED),
              desc({"se3": 48, "so2": 48}, native.FLAG_V_TRANSFORM | native.FLAG_FP32_PRODUCTS, dh=96, dtype=torch.float32),
              desc({"se3": 30, "t2": 34}, native.FLAG_V_TRANSFORM | native.FLAG_EUCLID)):
        assert native.attn_bwd_dlse_supported(d) == native.E_UNSUPPORTED
        assert native.lib().gta_strerror(native.E_UNSUPPORTED).decode()


def test_merge_argument_checks_need_no_launch():
    L = native.lib()
    one = (ctypes.c_void_p * 1)(16)
    st = (ctypes.c_int64 * 3)(64, 8, 8)
    call = lambda dtype, n, dh: L.gta_attn_merge(dtype, n, 1, 1, 8, dh, one, st, one, st, ctypes.c_void_p(16), st, ctypes.c_void_p(16), st, None)
    assert call(7, 1, 8) == -1 and call(0, 0, 8) == -1 and call(0, 9, 8) == -1        # GTA_E_BADARG: dtype, n
    assert call(0, 1, 12) == native.E_UNSUPPORTED and call(0, 1, 136) == native.E_UNSUPPORTED


def test_return_lse_refusals_under_grad_name_it():
    q = torch.randn(1, 2, 8, 96, requires_grad=True)
    # float32 at dh = 96 with precise=True: the exact-fp32 route (gta_plain32)
    with pytest.raises(native.GtaError, match="return_lse.*gta_plain32"):
        gta_amd.gta_attention(q, q, q, {"triv": 96}, {}, precise=True, return_lse=True)
    with pytest.raises(native.GtaError, match="return_lse.*key_views_backward"):
        gta_amd.gta_attention(q, q, q, {"triv": 96}, {}, key_views=[1], key_views_backward=True, return_lse=True)


def test_merge_refuses_bad_operand_lists():
    o, l = torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8)
    for outs, lses in (([], []), ([o] * 9, [l] * 9), ([o, o], [l])):
        with pytest.raises(native.GtaError, match="1 to 8"):
            gta_amd.gta_attention_merge(outs, lses)
    with pytest.raises(native.GtaError):                  # host tensors: there is no CPU path
        gta_amd.gta_attention_merge([o], [l])


def test_by_view_groups_refusals():
    q = torch.randn(1, 2, 8, 64)
    call = lambda **kw: gta_amd.gta_attention_by_view_groups(q, q, q, {"triv": 64}, {}, **kw)
    for v in (17, 0, True, (4, 17), ()):
        with pytest.raises(native.GtaError, match="views_per_call"):
            call(views_per_call=v, num_key_views=4)
    with pytest.raises(native.GtaError, match="kv_cache"):
        call(views_per_call=4, num_key_views=4, kv_cache={})
    with pytest.raises(native.GtaError, match="key_views"):
        call(views_per_call=4, num_key_views=4, key_views=[1])
    with pytest.raises(native.GtaError, match="return_attmap"):
        call(views_per_call=4, num_key_views=4, return_attmap=True)
    with pytest.raises(native.GtaError, match="num_key_views"):
        call(views_per_call=4)
    with pytest.raises(native.GtaError, match="add up"):
        call(views_per_call=(1, 2), num_key_views=4)
    with pytest.raises(native.GtaError, match="split evenly"):
        call(views_per_call=2, num_key_views=3)

"""Per-call times of the merge kernels and of an attention run by view groups.
  'merge':  gta_attn_merge / gta_attn_merge_bwd at B = 32, H = 8, Tq = 1280, dh = 96, bf16, n = 2 partials -- the native binding, no autograd
            and no allocation inside the timed call -- against `copy_` of the same bytes (forward: 2 out-sized reads + 1 write = 1.5 copies
            of one tensor's read + write; backward: 3 reads + 2 writes = 2.5), the yardstick DESIGN.md section 5.2 uses for a re-layout pass.
            The lse-sized operands (1 / 96 of the bytes at bf16) are left out of the byte count.
  'groups': gta_attention_by_view_groups with 2 groups (views_per_call = 3 of 5 views) against the whole gta_attention call at the MSN
            encoder shape (B = 32, bf16), forward under no_grad.
Sustained-clock timing as in tools/time_key_views.py: every figure is the median of `--blocks` blocks of `--iters` calls, each block after
a warm second of the same work.

    python tools/time_lse_merge.py               # one JSON line per part
Needs an MI355X.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gta_amd  # noqa: E402
from gta_amd import native  # noqa: E402
from tools.time_key_views import time_it  # noqa: E402


def merge_runs():
    B, H, Tq, dh, dt, n = 32, 8, 1280, 96, torch.bfloat16, 2
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, Tq, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    ml = lambda: torch.randn(B, H, Tq, device="cuda", generator=g)
    outs, lses, out, lse = [mk() for _ in range(n)], [ml() for _ in range(n)], mk(), ml()
    dout, dlse, douts, dlses = mk(), ml(), [mk() for _ in range(n)], [ml() for _ in range(n)]
    src, dst = mk(), mk()
    runs = {"merge_fwd": lambda: native.attn_merge(outs, lses, out, lse),
            "merge_bwd": lambda: native.attn_merge_bwd(outs, lses, dout, dlse, douts, dlses),
            "copy": lambda: dst.copy_(src)}
    return runs, {"part": "merge", "B": B, "H": H, "Tq": Tq, "dh": dh, "dtype": str(dt), "n": n, "tensor_MiB": round(src.numel() * 2 / 2 ** 20, 1)}


def group_runs():
    B, H, Nk, Pk, dt, f, L = 32, 8, 5, 256, torch.bfloat16, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}, 2
    T, dh = Nk * Pk, sum(f.values())
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    q, k, v = mk(), mk(), mk()
    from gta_amd import synth
    vrep = native.build_view_reps(synth.random_extrinsics(B, Nk, torch.Generator().manual_seed(Nk)).cuda().contiguous(), L)
    a = torch.rand(B, T, f["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = torch.stack([a.cos(), a.sin()], -1).contiguous()
    packed = {"vrep_q": vrep, "vrep_k": vrep, "cs_q": cs, "cs_k": cs}
    tc = torch.tensor([0.37], device="cuda")
    runs = {"whole": lambda: gta_amd.gta_attention(q, k, v, f, packed, so3_degree=L, trans_coeff=tc),
            "two_groups": lambda: gta_amd.gta_attention_by_view_groups(q, k, v, f, packed, views_per_call=3, so3_degree=L, trans_coeff=tc)}
    return runs, {"part": "groups", "shape": "msn-enc", "B": B, "Tq": T, "Tk": T, "dh": dh, "dtype": str(dt), "groups": [3, 2]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lse_merge.py needs an MI355X")
    for build in (merge_runs, group_runs):
        runs, rec = build()
        for name, run in runs.items():
            rec[name + "_us"], rec[name + "_blocks_us"] = time_it(run, a.blocks, a.iters)
        if rec["part"] == "merge":
            rec["merge_fwd_over_copy"] = round(rec["merge_fwd_us"] / rec["copy_us"], 3)          # same bytes: 1.5
            rec["merge_bwd_over_copy"] = round(rec["merge_bwd_us"] / rec["copy_us"], 3)          # same bytes: 2.5
        else:
            rec["two_groups_over_whole"] = round(rec["two_groups_us"] / rec["whole_us"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

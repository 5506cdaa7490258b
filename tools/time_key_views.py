"""Per-call time of a batch whose scenes have different numbers of input views, B = 32, at the CLEVR-TR decoder shape (fp32) and the MSN
encoder shape (bf16); view counts drawn uniformly from 1..Nk with a fixed seed.  Four ways to run it:
  (a) 'varlen'  = one call with key_views (gta_attn_fwd_varlen: the VARLEN pre-pass and gta_fwd2_kernel; padded tiles skipped);
  (b) 'grouped' = one call per distinct view count on the route such a call takes without key_views, on pre-gathered scene groups with the
                  key side (self-attention: the query side too) cut to the group's views -- what a user does without the feature;
  (c) 'padded'  = one call over the full Tk without a mask, on the route such a call takes (kv_mode='prepass': at the MSN encoder shape that is
                  the 64-rows-per-wave kernel, another family than (a)'s).  Its results are wrong; it is here for its time only.
  (d) 'padded_fwd2' = (c) on the kernel family of (a) (kv_mode='prepass_fwd2': the pre-pass and gta_fwd2_kernel without the mask) -- the leg
                  that 'prefix_tiles_over_full' is read against: (a) / (d) is what skipping the padded tiles saves, nothing else differs.
Sustained-clock timing: every figure is the median of `--blocks` blocks of `--iters` calls, each block after a warm second of the same work.

    python tools/time_key_views.py               # one JSON line per shape
Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gta_amd  # noqa: E402
from gta_amd import native  # noqa: E402

B = 32
SHAPES = {   # name: (H, Nk, Pk, Nq, Pq (None: self-attention), dtype, f_dims, so3 degree)      
    "clevrtr-dec": (6, 2, 300, 3, 853, torch.float32, {"se3": 32, "so2": 32}, 0),
    "msn-enc": (8, 5, 256, None, None, torch.bfloat16, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}, 2),
}


def setup(name, seed):
    H, Nk, Pk, Nq, Pq, dt, f, L = SHAPES[name]
    self_attn = Nq is None
    if self_attn:
        Nq, Pq = Nk, Pk
    Tq, Tk, dh = Nq * Pq, Nk * Pk, sum(f.values())
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda T: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    q, k, v = mk(Tq), mk(Tk), mk(Tk)

    def views(N):
        from gta_amd import synth
        return native.build_view_reps(synth.random_extrinsics(B, N, torch.Generator().manual_seed(N)).cuda().contiguous(), L)
    ang = lambda T: torch.rand(B, T, f["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = lambda a: torch.stack([a.cos(), a.sin()], -1).contiguous()
    packed = {"vrep_q": views(Nq), "vrep_k": views(Nk), "cs_q": cs(ang(Tq)), "cs_k": cs(ang(Tk))}
    tc = torch.tensor([0.37], device="cuda")
    kv = torch.randint(1, Nk + 1, (B,), generator=torch.Generator().manual_seed(seed)).tolist()
    call = lambda q_, k_, v_, pk, **kw: gta_amd.gta_attention(q_, k_, v_, f, pk, so3_degree=L, trans_coeff=tc, **kw)
    groups = []
    for n in sorted(set(kv)):
        idx = torch.tensor([b for b in range(B) if kv[b] == n], device="cuda")
        nq = n if self_attn else Nq
        pk = {"vrep_q": packed["vrep_q"][idx][:, :nq].contiguous(), "vrep_k": packed["vrep_k"][idx][:, :n].contiguous(),
              "cs_q": packed["cs_q"][idx][:, :nq * Pq].contiguous(), "cs_k": packed["cs_k"][idx][:, :n * Pk].contiguous()}
        groups.append((q[idx][:, :, :nq * Pq], k[idx][:, :, :n * Pk], v[idx][:, :, :n * Pk], pk))
    runs = {"varlen": lambda: call(q, k, v, packed, key_views=kv),
            "grouped": lambda: [call(*gr) for gr in groups],
            "padded": lambda: call(q, k, v, packed, kv_mode="prepass"),
            "padded_fwd2": lambda: call(q, k, v, packed, kv_mode="prepass_fwd2")}
    tiles = lambda t: (t + 63) // 64
    return runs, {"shape": name, "Tq": Tq, "Tk": Tk, "dh": dh, "dtype": str(dt), "key_views": kv, "distinct_counts": len(groups),
                  "prefix_tiles_over_full": round(sum(tiles(n * Pk) for n in kv) / (B * tiles(Tk)), 3)}


def time_it(run, blocks, iters):
    res = []
    with torch.no_grad():
        for _ in range(blocks):
            t0 = time.time()
            while time.time() - t0 < 1.0:              # sustained regime: the clock settles after ~1 s of load
                run()
                torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            res.append(e0.elapsed_time(e1) / iters * 1e3)
    return round(statistics.median(res), 1), [round(x, 1) for x in res]      # us per call, launches and allocations included


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_key_views.py needs an MI355X")
    for name in a.shapes.split(","):
        runs, rec = setup(name, a.seed)
        for route, run in runs.items():
            rec[route + "_us"], rec[route + "_blocks_us"] = time_it(run, a.blocks, a.iters)
        rec["varlen_over_padded"] = round(rec["varlen_us"] / rec["padded_us"], 3)
        rec["varlen_over_padded_fwd2"] = round(rec["varlen_us"] / rec["padded_fwd2_us"], 3)
        rec["varlen_over_grouped"] = round(rec["varlen_us"] / rec["grouped_us"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

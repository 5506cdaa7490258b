"""Forward + backward time of a batch whose scenes have different numbers of input views, B = 32, bf16, at the MSN encoder shape and the
CLEVR-TR encoder shape (self-attention: query_views = key_views); view counts drawn uniformly from 2..Nk with a fixed seed.  Three legs:
  (a) 'varlen'        = key_views with key_views_backward=True (gta_attn_fwd_varlen + gta_attn_bwd_varlen: padded tiles skipped both ways);
  (b) 'padded_keys32' = the same padded batch without a mask, forward on gta_fwd2_kernel and backward on the compiled pair
                        (kv_mode flags ROWS32 | FWD2_GENERIC | BWD_KEYS32) -- the kernels of (a) without the prefixes: (a) / (b) is what
                        the prefixes save, to be read against 'prefix_tiles_over_full';
  (c) 'padded'        = the padded batch on the default unmasked route (kv_mode='prepass': at the MSN shape the generated 64-row streams).
(b) and (c) compute wrong results for such a batch; they are here for their time only.
Sustained-clock timing: every figure is the median of `--blocks` blocks of `--iters` steps, each block after a warm second of the same work.

    python tools/time_key_views_bwd.py               # one JSON line per shape
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
from gta_amd import gta as G2  # noqa: E402
from gta_amd import native  # noqa: E402

B = 32
SHAPES = {   # name: (H, Nk, Pk, f_dims, so3 degree)      (self-attention)
    "msn-enc": (8, 5, 256, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}, 2),
    "clevrtr-enc": (6, 2, 300, {"se3": 32, "so2": 32}, 0),
}


def setup(name, seed):
    H, Nk, Pk, f, L = SHAPES[name]
    T, dh, dt = Nk * Pk, sum(f.values()), torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3).requires_grad_()
    q, k, v = mk(), mk(), mk()
    dout = torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    from gta_amd import synth
    vrep = native.build_view_reps(synth.random_extrinsics(B, Nk, torch.Generator().manual_seed(Nk)).cuda().contiguous(), L)
    ang = torch.rand(B, T, f["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    packed = {"vrep_q": vrep, "vrep_k": vrep, "cs_q": cs, "cs_k": cs}
    tc = torch.tensor([0.37], device="cuda", requires_grad=True)
    kv = torch.randint(2, Nk + 1, (B,), generator=torch.Generator().manual_seed(seed)).tolist()

    def step(**kw):
        out = gta_amd.gta_attention(q, k, v, f, packed, so3_degree=L, trans_coeff=tc, **kw)
        out.backward(dout)
        q.grad = k.grad = v.grad = tc.grad = None

    G2.KV_MODES.setdefault("prepass_fwd2_bwd_keys32", native.FLAG_ROWS32 | native.FLAG_FWD2_GENERIC | native.FLAG_BWD_KEYS32)
    runs = {"varlen": lambda: step(key_views=kv, key_views_backward=True, query_views=kv),
            "padded_keys32": lambda: step(kv_mode="prepass_fwd2_bwd_keys32"),
            "padded": lambda: step(kv_mode="prepass")}
    tiles = lambda t: (t + 63) // 64
    return runs, {"shape": name, "T": T, "dh": dh, "dtype": str(dt), "key_views": kv,
                  "prefix_tokens_over_full": round(sum(n * Pk for n in kv) / (B * T), 3),
                  "prefix_tiles_over_full": round(sum(tiles(n * Pk) for n in kv) / (B * tiles(T)), 3)}


def time_it(run, blocks, iters):
    res = []
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
    return round(statistics.median(res), 1), [round(x, 1) for x in res]      # us per step, launches and allocations included


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_key_views_bwd.py needs an MI355X")
    for name in a.shapes.split(","):
        runs, rec = setup(name, a.seed)
        for route, run in runs.items():
            rec[route + "_us"], rec[route + "_blocks_us"] = time_it(run, a.blocks, a.iters)
        rec["varlen_over_padded_keys32"] = round(rec["varlen_us"] / rec["padded_keys32_us"], 3)
        rec["varlen_over_padded"] = round(rec["varlen_us"] / rec["padded_us"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

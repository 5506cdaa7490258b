"""Forward + backward time under a key mask, B = 32, bf16, at the MSN encoder shape (self-attention, H = 8, 5 views x 256 tokens, dh = 96); view
counts drawn uniformly from 2..Nk with a fixed seed.  Three legs:
  (a) 'mask_views'     = key_mask of whole leading views with key_mask_backward=True (gta_attn_fwd_gather + gta_attn_bwd_gather);
  (b) 'key_views'      = the same view counts through key_views with key_views_backward=True and no query_views (gta_attn_fwd_varlen +
                         gta_attn_bwd_varlen): the same images, the same walks, consecutive rows -- (a) / (b) is what the index hop costs, in
                         the forward's pre-pass and in the dK/dV epilogue together;
  (c) 'mask_bernoulli' = a Bernoulli mask at the same valid share of every scene: the same tile counts with scattered rows.
The index tensors of (a) and (c) are built per call, as `gta_attention` builds them (a stable sort and a sum on the device).
Sustained-clock timing: every figure is the median of `--blocks` blocks of `--iters` steps, each block after a warm second of the same work;
the legs alternate inside a block round so that none of them owns the warmest clock.

    python tools/time_key_mask_bwd.py               # one JSON line
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
    views = torch.zeros(B, T, dtype=torch.bool)
    bern = torch.zeros(B, T, dtype=torch.bool)
    gm = torch.Generator().manual_seed(seed + 1)
    for b, n in enumerate(kv):
        views[b, :n * Pk] = True
        bern[b, torch.randperm(T, generator=gm)[:n * Pk]] = True        # exactly the same number of valid keys, anywhere
    views, bern = views.cuda(), bern.cuda()

    def step(**kw):
        out = gta_amd.gta_attention(q, k, v, f, packed, so3_degree=L, trans_coeff=tc, **kw)
        out.backward(dout)
        q.grad = k.grad = v.grad = tc.grad = None

    runs = {"mask_views": lambda: step(key_mask=views, key_mask_backward=True),
            "key_views": lambda: step(key_views=kv, key_views_backward=True),
            "mask_bernoulli": lambda: step(key_mask=bern, key_mask_backward=True)}
    return runs, {"shape": name, "B": B, "H": H, "T": T, "dh": dh, "dtype": str(dt), "key_views": kv,
                  "valid_share": round(sum(n * Pk for n in kv) / (B * T), 3)}


def time_once(run, iters):
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
    return e0.elapsed_time(e1) / iters * 1e3       # us per step, launches and allocations included


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="msn-enc")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_key_mask_bwd.py needs an MI355X")
    for name in a.shapes.split(","):
        runs, rec = setup(name, a.seed)
        res = {route: [] for route in runs}
        for _ in range(a.blocks):
            for route, run in runs.items():
                res[route].append(time_once(run, a.iters))
        for route, xs in res.items():
            rec[route + "_us"], rec[route + "_blocks_us"] = round(statistics.median(xs), 1), [round(x, 1) for x in xs]
        rec["mask_views_over_key_views"] = round(rec["mask_views_us"] / rec["key_views_us"], 3)
        rec["mask_bernoulli_over_key_views"] = round(rec["mask_bernoulli_us"] / rec["key_views_us"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

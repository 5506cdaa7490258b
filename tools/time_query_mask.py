"""What a query-side mask buys and costs, B = 32, bf16, at the MSN encoder shape (self-attention, H = 8, 5 views x 256 tokens, dh = 96).
For each mask two calls on the same box in the same run, forward (under no_grad) and forward + backward:
  'key'    = key_mask alone (key_mask_backward=True under grad): every query row live -- the call as it was before query_mask;
  'query'  = the same key_mask with query_mask = key_mask (gta_attn_fwd_qmask / gta_attn_bwd_qmask).
Masks: whole leading views at valid shares 1.0 / 0.6 / 0.2 (5 / 3 / 1 of 5 views in every scene: 0 / 40 / 80 % of the 128-row work items
dead), and a Bernoulli 0.5 mask, where no item is dead and every dead row is computed as a zero row.  `attn_us` is the attention kernel alone
(gta_fwd2_kernel, from the dispatch's own events).  Sustained-clock timing as tools/time_key_mask.py: every figure is the median of `--blocks`
blocks of `--iters` steps, each block after a warm second of the same work; the legs alternate inside a block round.

    python tools/time_query_mask.py               # one JSON line per mask
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

B, H, NK, PK, L = 32, 8, 5, 256, 2
F = {"triv": 0, "se3": 48, "so3": 24, "so2": 24}


def setup():
    T, dh, dt = NK * PK, sum(F.values()), torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3).requires_grad_()
    q, k, v = mk(), mk(), mk()
    dout = torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    from gta_amd import synth
    vrep = native.build_view_reps(synth.random_extrinsics(B, NK, torch.Generator().manual_seed(NK)).cuda().contiguous(), L)
    ang = torch.rand(B, T, F["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    packed = {"vrep_q": vrep, "vrep_k": vrep, "cs_q": cs, "cs_k": cs}
    tc = torch.tensor([0.37], device="cuda", requires_grad=True)

    def fwd(**kw):
        with torch.no_grad():
            gta_amd.gta_attention(q, k, v, F, packed, so3_degree=L, trans_coeff=tc, **kw)

    def step(**kw):
        gta_amd.gta_attention(q, k, v, F, packed, so3_degree=L, trans_coeff=tc, key_mask_backward=True, **kw).backward(dout)
        q.grad = k.grad = v.grad = tc.grad = None

    return fwd, step, T


def masks(T):
    out = {}
    for n in (5, 3, 1):
        m = torch.zeros(B, T, dtype=torch.bool)
        m[:, :n * PK] = True
        out[f"views_{n / NK:.1f}"] = m.cuda()
    out["bernoulli_0.5"] = (torch.rand(B, T, generator=torch.Generator().manual_seed(1)) < 0.5).cuda()
    return out


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


def kernel_us(run, n=20):
    """the attention kernel alone: the median of n launches timed by the dispatch's own start / stop events"""
    lib = native.lib()
    a, b = lib.gta_debug_event_create(), lib.gta_debug_event_create()
    xs = []
    for _ in range(n):
        lib.gta_debug_time_next_attention_kernel(a, b)
        run()
        torch.cuda.synchronize()
        xs.append(lib.gta_debug_event_elapsed_ms(a, b) * 1e3)
    lib.gta_debug_event_destroy(a)
    lib.gta_debug_event_destroy(b)
    return round(statistics.median(xs), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_query_mask.py needs an MI355X")
    fwd, step, T = setup()
    for name, m in masks(T).items():
        dead_items = 1.0 - m.view(B, -1, 128).any(-1).float().mean().item()
        rec = {"shape": "msn-enc", "B": B, "H": H, "T": T, "dtype": "bfloat16", "mask": name, "valid_share": round(m.float().mean().item(), 3),
               "dead_items_share": round(dead_items, 3)}
        legs = {"fwd_key": lambda: fwd(key_mask=m), "fwd_query": lambda: fwd(key_mask=m, query_mask=m),
                "fwdbwd_key": lambda: step(key_mask=m), "fwdbwd_query": lambda: step(key_mask=m, query_mask=m)}
        res = {leg: [] for leg in legs}
        for _ in range(a.blocks):
            for leg, run in legs.items():
                res[leg].append(time_once(run, a.iters))
        for leg, xs in res.items():
            rec[leg + "_us"] = round(statistics.median(xs), 1)
        rec["attn_key_us"], rec["attn_query_us"] = kernel_us(legs["fwd_key"]), kernel_us(legs["fwd_query"])
        rec["fwd_query_over_key"] = round(rec["fwd_query_us"] / rec["fwd_key_us"], 3)
        rec["fwdbwd_query_over_key"] = round(rec["fwdbwd_query_us"] / rec["fwdbwd_key_us"], 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

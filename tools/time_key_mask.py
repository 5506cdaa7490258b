"""What the key mask costs and saves at the MSN encoder shape (B = 32, bf16, 5 views of 256 tokens, self-attention).

  pre-pass   GTA_FLAG_PREP_ONLY calls through the ABI: 'prep_gather_all' = gta_attn_fwd_gather under an all-true mask against 'prep_varlen_full' =
             gta_attn_fwd_varlen under full prefixes.  Both move the same bytes and write the same images; the gap is the price of the index
             hop (one dependent 4-byte load per row in front of the DMA addresses, one cross-lane read per piece).
  call       gta_attention(key_mask=) with a Bernoulli(`--share`) mask on the device -- index build (a stable sort and a sum), gather pre-pass
             over the valid keys, VARLEN gta_fwd2_kernel -- as 'call_mask'; the same through a ForwardPlan (indices built once) as
             'plan_mask'; against the call over all keys on the same kernel family ('call_full_fwd2', kv_mode='prepass_fwd2') and on the route
             such a call takes by default ('call_full', kv_mode='prepass': the 64-rows-per-wave kernel).

Sustained-clock timing: every figure is the median of `--blocks` blocks; a block warms the device for a second with the legs it is about to
time, then times `--iters` calls of each leg in turn (the legs alternate inside a block, so a drift of the clock meets all of them).

    python tools/time_key_mask.py                # one JSON line
Needs an MI355X."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gta_amd  # noqa: E402
from gta_amd import native, plan  # noqa: E402

B, H, NK, PK = 32, 8, 5, 256
F = {"triv": 0, "se3": 48, "so3": 24, "so2": 24}
L = 2


def setup(share, seed):
    T, dh, dt = NK * PK, sum(F.values()), torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    q, k, v = mk(), mk(), mk()
    from gta_amd import synth
    vrep = native.build_view_reps(synth.random_extrinsics(B, NK, torch.Generator().manual_seed(NK)).cuda().contiguous(), L)
    ang = torch.rand(B, T, F["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    packed = {"vrep_q": vrep, "vrep_k": vrep, "cs_q": cs, "cs_k": cs}
    tc = torch.tensor([0.37], device="cuda")
    mask = (torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) < share)
    mask[:, 0] |= ~mask.any(1)
    mask = mask.cuda()
    everything = torch.ones(B, T, dtype=torch.bool, device="cuda")

    # the pre-pass alone, through the ABI
    out = torch.empty(B, T, H, dh, device="cuda", dtype=dt).permute(0, 2, 1, 3)
    desc = native.make_desc(q, k, v, out, F, L, NK, NK, dh ** -0.5, native.FLAG_V_TRANSFORM | native.FLAG_PREP_ONLY)
    ws = torch.empty(native.attn_fwd_workspace_bytes(desc), device="cuda", dtype=torch.uint8)
    idx_all, lens_all = gta_amd.key_index_tensors(everything, q.device)
    idx_half, lens_half = gta_amd.key_index_tensors(mask, q.device)
    tabs = (vrep, vrep, cs, cs, tc, None)
    call = lambda **kw: gta_amd.gta_attention(q, k, v, F, packed, so3_degree=L, trans_coeff=tc, **kw)
    fp = plan.ForwardPlan(q, k, v, F, so3_degree=L, Nq=NK, Nk=NK, key_mask=mask)
    prep = {"prep_gather_all": lambda: native.attn_fwd_gather(desc, None, k, v, *tabs, idx_all, lens_all, None, None, ws),
            "prep_varlen_full": lambda: native.attn_fwd_varlen(desc, None, k, v, *tabs, lens_all, None, None, ws),
            "prep_gather_mask": lambda: native.attn_fwd_gather(desc, None, k, v, *tabs, idx_half, lens_half, None, None, ws)}
    calls = {"call_mask": lambda: call(key_mask=mask),
             "plan_mask": lambda: fp(q, k, v, vrep, vrep, cs, cs, tc),
             "call_full_fwd2": lambda: call(kv_mode="prepass_fwd2"),
             "call_full": lambda: call(kv_mode="prepass")}
    tiles = lambda t: (t + 63) // 64
    rec = {"shape": "msn-enc", "B": B, "H": H, "Tq": T, "Tk": T, "dh": dh, "dtype": str(dt), "valid_share": round(mask.float().mean().item(), 3),
           "valid_tiles_over_full": round(sum(tiles(int(n)) for n in lens_half.tolist()) / (B * tiles(T)), 3)}
    return prep, calls, rec


def time_legs(legs, blocks, iters):
    res = {name: [] for name in legs}
    with torch.no_grad():
        for _ in range(blocks):
            t0 = time.time()
            while time.time() - t0 < 1.0:              # sustained regime: the clock settles after ~1 s of load
                for run in legs.values():
                    run()
                torch.cuda.synchronize()
            for name, run in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    run()
                e1.record()
                torch.cuda.synchronize()
                res[name].append(e0.elapsed_time(e1) / iters * 1e3)
    return {name: (round(statistics.median(x), 1), [round(y, 1) for y in x]) for name, x in res.items()}      # us per call, launches included


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_key_mask.py needs an MI355X")
    prep, calls, rec = setup(a.share, a.seed)
    for legs in (prep, calls):
        for name, (med, all_) in time_legs(legs, a.blocks, a.iters).items():
            rec[name + "_us"], rec[name + "_blocks_us"] = med, all_
    rec["prep_gather_over_varlen"] = round(rec["prep_gather_all_us"] / rec["prep_varlen_full_us"], 3)
    rec["call_mask_over_full_fwd2"] = round(rec["call_mask_us"] / rec["call_full_fwd2_us"], 3)
    rec["plan_mask_over_full_fwd2"] = round(rec["plan_mask_us"] / rec["call_full_fwd2_us"], 3)
    rec["call_mask_over_full"] = round(rec["call_mask_us"] / rec["call_full_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

"""What the gather costs in the staged generic pre-pass, at the `clevrtr/gta_euclid` encoder shape (bench.py's cl-enc workload: B = 32, H = 6,
2 views of 300 tokens, self-attention, dh 64 as `triv 2 | se3 30 | so2 32` under euclid, bf16).

  pre-pass   GTA_FLAG_PREP_ONLY calls through the ABI.  'prep_gather_views' = gta_attn_fwd_staged_gather under a mask of whole leading views
             (scenes alternate between 1 and 2 views) against 'prep_varlen_views' = gta_attn_fwd_staged_varlen under the same view counts: the
             same rows read, the same images and bias written; the gap is the price of the index hop (64 token numbers staged in LDS per tile,
             one LDS read per 16-byte unit in front of the row address).  'prep_gather_half' = a Bernoulli(`--share`) mask against
             'prep_gather_all' / 'prep_varlen_full', the full key side.
  call       gta_attention(key_mask=, key_mask_generic=True) with the Bernoulli mask on the device ('call_mask': index build, gather pre-pass,
             VARLEN gta_gen_attn_kernel) and through a ForwardPlan ('plan_mask': indices built once), against the call over all keys
             ('call_full': gta_attn_fwd_staged).

Sustained-clock timing: every figure is the median of `--blocks` blocks; a block warms the device for a second with the legs it is about to
time, then times `--iters` calls of each leg in turn (the legs alternate inside a block, so a drift of the clock meets all of them).

    python tools/time_key_mask_generic.py                # one JSON line
Needs an MI355X."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gta_amd  # noqa: E402
from gta_amd import native, plan  # noqa: E402
from tools.time_key_mask import time_legs  # noqa: E402

B, H, NK, PK = 32, 6, 2, 300
F = {"triv": 2, "se3": 30, "so2": 32}


def setup(share, seed):
    T, dh, dt = NK * PK, sum(F.values()), torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    q, k, v = mk(), mk(), mk()
    from gta_amd import synth
    vrep = native.build_view_reps(synth.random_extrinsics(B, NK, torch.Generator().manual_seed(NK)).cuda().contiguous(), 0)
    ang = torch.rand(B, T, F["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    packed = {"vrep_q": vrep, "vrep_k": vrep, "cs_q": cs, "cs_k": cs}
    tc = torch.tensor([0.37], device="cuda")
    mask = (torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) < share)
    mask[:, 0] |= ~mask.any(1)
    mask = mask.cuda()
    everything = torch.ones(B, T, dtype=torch.bool, device="cuda")
    views = [1 + b % 2 for b in range(B)]
    leading = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(views):
        leading[b, :n * PK] = True
    leading = leading.cuda()

    out = torch.empty(B, T, H, dh, device="cuda", dtype=dt).permute(0, 2, 1, 3)
    flags = native.FLAG_V_TRANSFORM | native.FLAG_EUCLID
    desc = native.make_desc(q, k, v, out, F, 0, NK, NK, dh ** -0.5, flags | native.FLAG_PREP_ONLY)
    ws = torch.empty(native.attn_fwd_staged_workspace_bytes(desc), device="cuda", dtype=torch.uint8)
    idx_all, lens_all = gta_amd.key_index_tensors(everything, q.device)
    idx_half, lens_half = gta_amd.key_index_tensors(mask, q.device)
    idx_views, lens_views = gta_amd.key_index_tensors(leading, q.device)
    tabs = (vrep, vrep, cs, cs, None, None, tc, None)
    call = lambda **kw: gta_amd.gta_attention(q, k, v, F, packed, trans_coeff=tc, euclid=True, **kw)
    fp = plan.ForwardPlan(q, k, v, F, Nq=NK, Nk=NK, euclid=True, key_mask=mask)
    gather = lambda idx, lens: (lambda: native.attn_fwd_staged_gather(desc, None, k, v, *tabs, idx, lens, None, None, ws))
    varlen = lambda lens: (lambda: native.attn_fwd_staged_varlen(desc, None, k, v, *tabs, lens, None, None, ws))
    prep = {"prep_gather_views": gather(idx_views, lens_views), "prep_varlen_views": varlen(lens_views),
            "prep_gather_all": gather(idx_all, lens_all), "prep_varlen_full": varlen(lens_all), "prep_gather_half": gather(idx_half, lens_half)}
    calls = {"call_mask": lambda: call(key_mask=mask, key_mask_generic=True),
             "plan_mask": lambda: fp(q, k, v, vrep, vrep, cs, cs, tc),
             "call_full": lambda: call()}
    tiles = lambda t: (t + 63) // 64
    rec = {"shape": "cl-enc gta_euclid", "B": B, "H": H, "Tq": T, "Tk": T, "dh": dh, "dtype": str(dt), "views": f"{views[0]},{views[1]},... of {NK}",
           "valid_share": round(mask.float().mean().item(), 3),
           "valid_tiles_over_full": round(sum(tiles(int(n)) for n in lens_half.tolist()) / (B * tiles(T)), 3)}
    return prep, calls, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--share", type=float, default=0.5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_key_mask_generic.py needs an MI355X")
    prep, calls, rec = setup(a.share, a.seed)
    for legs in (prep, calls):
        for name, (med, all_) in time_legs(legs, a.blocks, a.iters).items():
            rec[name + "_us"], rec[name + "_blocks_us"] = med, all_
    rec["prep_gather_over_varlen_views"] = round(rec["prep_gather_views_us"] / rec["prep_varlen_views_us"], 3)
    rec["prep_gather_over_varlen_full"] = round(rec["prep_gather_all_us"] / rec["prep_varlen_full_us"], 3)
    rec["prep_half_over_full"] = round(rec["prep_gather_half_us"] / rec["prep_gather_all_us"], 3)
    rec["call_mask_over_full"] = round(rec["call_mask_us"] / rec["call_full_us"], 3)
    rec["plan_mask_over_full"] = round(rec["plan_mask_us"] / rec["call_full_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

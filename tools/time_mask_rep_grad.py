"""Cost of pose / coordinate gradients under a key and query mask (`key_mask_rep_grad`, gta_rep_grad_sums_masked) at the MSN encoder shape
(self-attention, B = 32, H = 8, 5 views x 256 tokens, dh = 96, bf16).

The sums pass (both sides: (q, dq), (dout, out) and (dk, k), (dv, v); view and so2 sums), six legs on the same buffers:
  'plain'         gta_rep_grad_sums, no mask
  'masked_full'   gta_rep_grad_sums_masked under an all-True mask          -- over 'plain': what the mask byte and the workgroup-wide OR cost
  'varlen_full'   gta_rep_grad_sums_varlen under full prefixes
  'masked_views'  ... under a mask of whole leading views (counts drawn uniformly from 2..Nk, fixed seed)
  'varlen_views'  gta_rep_grad_sums_varlen with the same counts             -- 'masked_views' over it: the same rows live, byte against prefix
  'masked_bern'   ... under a Bernoulli 0.5 mask: rows are not compacted and no workgroup of 32 tokens is wholly dead -- what is saved is the
                  dead rows' memory traffic (they are never loaded), not launches or reductions
The training step (forward + backward through gta_attention with key_mask = query_mask = the leading-views mask, key_mask_backward=True):
  'step_detached' tables without grad (all a call could do before key_mask_rep_grad)
  'step_rep_grad' vrep and cs tables requiring grad, key_mask_rep_grad=True: the sums pass, the fp64 algebra and the mask upload on top
and, for scale, the same pair without any mask ('nomask_detached', 'nomask_rep_grad': the unmasked route's sums pass and the same algebra).
Sustained-clock timing: every figure is the median of `--blocks` blocks of `--iters` runs, each block after a warm second of the same work;
the legs alternate inside a block round so that none of them owns the warmest clock.

    python tools/time_mask_rep_grad.py               # one JSON line
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


def setup(seed):
    T, dh, dt = NK * PK, sum(F.values()), torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    q, dq, dout, out, k, dk, v, dv = (mk() for _ in range(8))
    desc = native.make_desc(q, k, v, out, F, L, NK, NK, dh ** -0.5, native.FLAG_V_TRANSFORM)
    kv = torch.randint(2, NK + 1, (B,), generator=torch.Generator().manual_seed(seed)).tolist()
    views = torch.zeros(B, T, dtype=torch.bool)
    for b, n in enumerate(kv):
        views[b, :n * PK] = True
    bern = torch.rand(B, T, generator=torch.Generator().manual_seed(seed + 1)) < 0.5
    full = torch.ones(B, T, dtype=torch.bool)
    views, bern, full = views.cuda(), bern.cuda(), full.cuda()
    lens_views = torch.tensor([n * PK for n in kv], dtype=torch.int32, device="cuda")
    lens_full = torch.full((B,), T, dtype=torch.int32, device="cuda")

    def sums(**kw):
        native.rep_grad_sums(desc, 0, ((q, dq), (dout, out)), view=True, so2=True, **kw)
        native.rep_grad_sums(desc, 1, ((dk, k), (dv, v)), view=True, so2=True, **kw)

    from gta_amd import synth
    vrep = native.build_view_reps(synth.random_extrinsics(B, NK, torch.Generator().manual_seed(NK)).cuda().contiguous(), L)
    ang = torch.rand(B, T, F["so2"] // 2, device="cuda", generator=g) * 6.28
    cs = torch.stack([ang.cos(), ang.sin()], -1).contiguous()
    tc = torch.tensor([0.37], device="cuda", requires_grad=True)
    qg, kg, vg = (t.detach().clone().requires_grad_() for t in (q, k, v))

    def step(rep_grad, masked=True):
        vr, c = (vrep.detach().requires_grad_(rep_grad), cs.detach().requires_grad_(rep_grad))
        kw = dict(key_mask=views, query_mask=views, key_mask_backward=True, **({"key_mask_rep_grad": True} if rep_grad else {})) if masked else {}
        o = gta_amd.gta_attention(qg, kg, vg, F, {"vrep_q": vr, "vrep_k": vr, "cs_q": c, "cs_k": c}, so3_degree=L, trans_coeff=tc, **kw)
        o.backward(dout)
        qg.grad = kg.grad = vg.grad = tc.grad = None

    runs = {"plain": lambda: sums(), "masked_full": lambda: sums(live=full), "varlen_full": lambda: sums(lens=lens_full),
            "masked_views": lambda: sums(live=views), "varlen_views": lambda: sums(lens=lens_views), "masked_bern": lambda: sums(live=bern),
            "step_detached": lambda: step(False), "step_rep_grad": lambda: step(True),
            "nomask_detached": lambda: step(False, False), "nomask_rep_grad": lambda: step(True, False)}
    return runs, {"shape": "msn-enc", "B": B, "H": H, "T": T, "dh": dh, "dtype": str(dt), "key_views": kv,
                  "valid_share_views": round(sum(kv) / (B * NK), 3), "valid_share_bern": round(bern.float().mean().item(), 3)}


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
    return e0.elapsed_time(e1) / iters * 1e3       # us per run, launches and allocations included


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mask_rep_grad.py needs an MI355X")
    runs, rec = setup(a.seed)
    res = {leg: [] for leg in runs}
    for _ in range(a.blocks):
        for leg, run in runs.items():
            res[leg].append(time_once(run, a.iters))
    for leg, xs in res.items():
        rec[leg + "_us"], rec[leg + "_blocks_us"] = round(statistics.median(xs), 1), [round(x, 1) for x in xs]
    for num, den in (("masked_full", "plain"), ("masked_full", "varlen_full"), ("masked_views", "varlen_views"), ("masked_bern", "varlen_full"),
                     ("masked_bern", "plain"), ("step_rep_grad", "step_detached"), ("nomask_rep_grad", "nomask_detached")):
        rec[f"{num}_over_{den}"] = round(rec[num + "_us"] / rec[den + "_us"], 3)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

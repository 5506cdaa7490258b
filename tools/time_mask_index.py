"""What the single-launch mask index (gta_mask_index, `gta_amd.mask_index`) costs against the torch chain it replaces, and what one shared
record does to a masked training step.

  (a) index build alone, on a CUDA Bernoulli(`--share`) mask, at B = 32, Tk = 1280 (MSN encoder) and B = 32, Tk = 600 (CLEVR-TR), the mask on
      both sides as in a padded self-attention layer:
        'chain'  key_index_tensors + query_mask_tensors + effective_key_mask  (what every masked `gta_attention` call under grad with
                 carriers runs; 'chain_keys' = key_index_tensors alone, what a key_mask-only call runs; 'chain_kq' = key_index_tensors +
                 query_mask_tensors, what a call with both masks runs without carriers -- an encoder layer of (b))
        'kernel' one `mask_index(mask, mask)` call (its four output allocations included; 'kernel_keys' = `mask_index(mask)`)
  (b) a masked `TransformingSRT` forward + backward at the MSN gta_so3 configuration (5 + 2 layers, 5 views of 256 tokens, `--model-batch`
      scenes, bf16 autocast, `input_mask_backward`, `input_mask_queries`): `input_mask_index=False` ('step_per_layer') against True
      ('step_shared').

Sustained-clock timing as in tools/time_key_mask.py: every figure is the median of `--blocks` blocks; a block warms the device for a second
with the legs it is about to time, then times `--iters` calls of each leg in turn (the legs alternate inside a block, so a drift of the clock
meets all of them).

    python tools/time_mask_index.py                # one JSON line
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
from gta_amd import gta as G2  # noqa: E402

SHAPES = {"msn": (32, 1280), "clevrtr": (32, 600)}


def index_legs(B, T, share, seed):
    mask = torch.rand(B, T, generator=torch.Generator().manual_seed(seed)) < share
    mask[:, 0] |= ~mask.any(1)
    mask = mask.cuda()
    dev = mask.device

    def chain():
        return G2.key_index_tensors(mask, dev), G2.query_mask_tensors(mask, dev), G2.effective_key_mask(mask, dev)

    return {"chain": chain, "kernel": lambda: gta_amd.mask_index(mask, mask, device=dev),
            "chain_keys": lambda: G2.key_index_tensors(mask, dev), "kernel_keys": lambda: gta_amd.mask_index(mask, device=dev),
            "chain_kq": lambda: (G2.key_index_tensors(mask, dev), G2.query_mask_tensors(mask, dev))}


def model_legs(batch, share, seed):
    from gta_amd import srt
    torch.manual_seed(1234)
    model = srt.TransformingSRT(srt.msn_gta_so3_cfg(dropout=0.0)).cuda()
    data = srt.synthetic_batch(batch, device="cuda", seed=99)
    B, N, P = data["input_coord"].shape[:3]
    mask = torch.rand(B, N, P, generator=torch.Generator().manual_seed(seed)) < share
    mask[:, :, 0] = True                       # (every view keeps a token: no image is selected away, both legs run the same rows)
    mask = mask.cuda()
    target = data["target_pixels"].flatten(1, 2)

    def step(shared):
        extras = {k: data[k] for k in ("input_transforms", "target_transforms", "input_coord", "target_coord")}
        with torch.autocast("cuda", dtype=torch.bfloat16):
            pred, _ = model(data["input_images"], data["input_camera_pos"], data["input_rays"], data["target_camera_pos"], data["target_rays"],
                            extras, input_mask=mask, input_mask_backward=True, input_mask_queries=True, input_mask_index=shared)
        ((pred.reshape(target.shape).float() - target) ** 2).mean().backward()
        for p in model.parameters():
            p.grad = None

    return {"step_per_layer": lambda: step(False), "step_shared": lambda: step(True)}, {"model_batch": B, "scene_tokens": N * P}


def time_legs(legs, blocks, iters, grad):
    res = {name: [] for name in legs}
    with torch.set_grad_enabled(grad):
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
    ap.add_argument("--share", type=float, default=0.7)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--model-iters", type=int, default=10)
    ap.add_argument("--model-batch", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_mask_index.py needs an MI355X")
    rec = {"share": a.share, "blocks": a.blocks, "iters": a.iters, "model_iters": a.model_iters}
    for shape, (B, T) in SHAPES.items():
        for name, (med, all_) in time_legs(index_legs(B, T, a.share, a.seed), a.blocks, a.iters, False).items():
            rec[f"{shape}_{name}_us"], rec[f"{shape}_{name}_blocks_us"] = med, all_
        rec[f"{shape}_kernel_over_chain"] = round(rec[f"{shape}_kernel_us"] / rec[f"{shape}_chain_us"], 3)
        rec[f"{shape}_kernel_keys_over_chain_keys"] = round(rec[f"{shape}_kernel_keys_us"] / rec[f"{shape}_chain_keys_us"], 3)
    if a.model_iters > 0:
        legs, what = model_legs(a.model_batch, a.share, a.seed)
        rec.update(what)
        for name, (med, all_) in time_legs(legs, a.blocks, a.model_iters, True).items():
            rec[name + "_us"], rec[name + "_blocks_us"] = med, all_
        rec["step_shared_over_per_layer"] = round(rec["step_shared_us"] / rec["step_per_layer_us"], 4)
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

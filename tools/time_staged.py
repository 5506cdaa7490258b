"""Per-call time of the generic path's two forward routes at the four run configs without a fused kernel, B = 32, encoder and decoder shapes:
'apply' = gta_rep_apply x 3-4 around gta_attn_fwd_plain (five launches, what a call under grad still runs), 'staged' = gta_attn_fwd_staged
(K/V pre-pass + attention kernel), 'cached' = the attention kernel alone on the images of an earlier call (kv_cache).  MSN configs in bf16,
the CLEVR-TR pair in fp32 (as their configs train).

    python tools/time_staged.py                  # sustained-regime event timing, one JSON line per (config, side)
    python tools/time_staged.py --rocprof DIR    # + the three loops under `rocprofv3 --kernel-trace --stats` (child processes): kernel times
    python tools/time_staged.py --render         # full-image decode of one 128 x 128 view, gta_so3_euclid settings, with / without the cache
Needs an MI355X.
"""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gta_amd import gta as G  # noqa: E402
from gta_amd import native  # noqa: E402

_MS = (8, 5, 256, 5, 512)      # H, views, tokens per input view, target views, tokens per target view  
_CL = (6, 2, 300, 3, 853)
CONFIGS = {   # name: (geometry, dtype, f_dims, so3 degree, euclid)
    "clevrtr/gta_euclid": (_CL, torch.float32, {"triv": 2, "se3": 30, "so2": 32}, 0, True),
    "clevrtr/gta_t2": (_CL, torch.float32, {"triv": 2, "se3": 32, "t2": 30}, 0, False),
    "msn/gta_so3_euclid": (_MS, torch.bfloat16, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}, 2, True),
    "msn/gta_t2": (_MS, torch.bfloat16, {"triv": 0, "se3": 48, "t2": 48}, 0, False),
}
B = 32


def setup(name, side):
    (H, Nk, Pk, Nq, Pq), dt, f, L, euclid = CONFIGS[name]
    if side == "enc":
        Nq, Pq = Nk, Pk
    Tq, Tk, dh = Nq * Pq, Nk * Pk, sum(f.values())
    g = torch.Generator(device="cuda").manual_seed(0)
    mk = lambda T: torch.randn(B, T, H, dh, device="cuda", dtype=dt, generator=g).permute(0, 2, 1, 3)
    q, k, v = mk(Tq), mk(Tk), mk(Tk)

    def views(N):                      # rigid poses in both slots of the record, identity Wigner blocks: the kernels' cost does not depend on the values
        from gta_amd import synth
        E = synth.random_extrinsics(B, N, torch.Generator().manual_seed(N)).cuda()
        return native.build_view_reps(E.contiguous(), L)
    packed = {"vrep_q": views(Nq), "vrep_k": views(Nk)}
    if f.get("so2"):
        ang = lambda T: torch.rand(B, T, f["so2"] // 2, device="cuda", generator=g) * 6.28
        packed["cs_q"], packed["cs_k"] = (torch.stack([a.cos(), a.sin()], -1).contiguous() for a in (ang(Tq), ang(Tk)))
    if f.get("t2"):
        packed["coord_q"], packed["coord_k"] = (torch.rand(B, T, 2, device="cuda", generator=g) for T in (Tq, Tk))
    tc = torch.tensor([0.37], device="cuda")
    args = (q, k, v, f, packed, L, tc, None, dh ** -0.5, True, euclid)
    cache = {}
    runs = {"apply": lambda: G._generic_forward(*args), "staged": lambda: G._staged_forward(*args),
            "cached": lambda: G._staged_forward(*args, kv_cache=cache)}
    esz = q.element_size()
    operands = (2 * B * H * Tq * dh + 2 * B * H * Tk * dh) * esz
    return runs, {"Tq": Tq, "Tk": Tk, "dh": dh, "dtype": str(dt), "operand_bytes": operands}


def time_it(run, seconds=1.0, iters=100):
    with torch.no_grad():
        t0 = time.time()
        while time.time() - t0 < seconds:              # sustained regime: the clock settles after ~1 s of load
            run()
            torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            run()
        e1.record()
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3           # us per call, launches and allocations included


def kernel_stats(outdir, calls):
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {outdir}")
    rows = [r for r in csv.DictReader(open(files[0])) if int(r["Calls"]) >= calls]      # (the setup's one-off kernels drop out)
    short = lambda n: re.sub(r"<.*", "", re.sub(r"\(anonymous namespace\)::|^void ", "", n)).split("(")[0].split("::")[-1]
    out = {}
    for r in rows:                                     # microseconds per call, template instances of one kernel summed
        out[short(r["Name"])] = round(out.get(short(r["Name"]), 0.0) + float(r["AverageNs"]) / 1e3 * int(r["Calls"]) / calls, 2)
    return out


def render(chunk=8192, Bv=4):
    from gta_amd import srt
    cfg = srt.msn_gta_so3_cfg(dropout=0.0)
    for part in ("encoder_kwargs", "decoder_kwargs"):
        cfg[part]["attn_args"]["method"]["args"]["euclid_sim"] = True
    torch.manual_seed(0)
    model = srt.TransformingSRT(cfg).cuda().eval()
    data = srt.synthetic_batch(Bv, n_in=5, n_tgt=1, image=128, points_per_view=512, device="cuda", seed=1)
    extras = {"input_transforms": data["input_transforms"], "input_coord": data["input_coord"], "target_transforms": data["target_transforms"][:, :1]}
    rays, cam = torch.randn(Bv, 128, 128, 3, device="cuda"), torch.randn(Bv, 3, device="cuda")
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        z, extras = model.encoder(data["input_images"], data["input_camera_pos"], data["input_rays"], extras)
        for reuse in (False, True, False, True):
            for _ in range(4):
                srt.render_image(model, z, cam, rays, extras, max_num_rays=chunk, reuse_kv=reuse)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                img, _ = srt.render_image(model, z, cam, rays, extras, max_num_rays=chunk, reuse_kv=reuse)
            torch.cuda.synchronize()
            print(json.dumps({"render": "msn gta_so3_euclid, 128x128 view", "B": Bv, "chunk": chunk, "reuse_kv": reuse,
                              "ms_per_image_batch": round((time.perf_counter() - t0) / 5 * 1e3, 2), "finite": bool(torch.isfinite(img).all())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--sides", default="enc,dec")
    ap.add_argument("--rocprof", metavar="DIR")
    ap.add_argument("--render", action="store_true")
    ap.add_argument("--loop", metavar="ROUTE", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_staged.py needs an MI355X")
    if a.render:
        return render()
    for name in a.configs.split(","):
        for side in a.sides.split(","):
            runs, rec = setup(name, side)
            if a.loop:                                 # the profiled child: 30 calls of one route ('cached': + the call that fills the cache)
                with torch.no_grad():
                    if a.loop == "cached":
                        runs["cached"]()
                    for _ in range(30):
                        runs[a.loop]()
                torch.cuda.synchronize()
                return
            rec = {"config": name, "side": side, **rec}
            for route, run in runs.items():
                rec[route + "_us"] = round(time_it(run), 1)
            rec["apply_over_staged"] = round(rec["apply_us"] / rec["staged_us"], 2)
            if a.rocprof:
                for route in runs:
                    out = os.path.join(a.rocprof, f"{name.replace('/', '_')}_{side}_{route}")
                    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "st", "--", sys.executable,
                                    os.path.abspath(__file__), "--loop", route, "--configs", name, "--sides", side], check=True, timeout=300,
                                   stdout=subprocess.DEVNULL)
                    rec[route + "_kernels_us"] = kernel_stats(out, 31 if route == "cached" else 30)     # (the cached child's priming call)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

"""Cost of the pose / coordinate gradient pass (gta_rep_grad_sums, gta_repgrad.hip) at the BASELINE shapes, bf16, B = 32.

What a backward adds when the extrinsics and coordinates require grad on the fused path: one launch per side, the query side over
(q, dq), (dout, out), the key side over (dk, k), (dv, v), reading the se3 and so2 channels of each row once (+ the per-view finish).

    python tools/time_rep_grad.py                 # sustained-regime event timing + bytes computed from shapes
    python tools/time_rep_grad.py --rocprof DIR   # the same loop under `rocprofv3 --kernel-trace --stats` (a child process),
                                                  # kernel microseconds and TB/s against the 6.3 TB/s measured HBM ceiling
    python tools/time_rep_grad.py --shapes ms-enc --key-views 2,5,3      # batches that mix view counts: the masked entry
                                                  # (gta_rep_grad_sums_varlen) beside the unmasked one on the same buffers
Needs an MI355X; prints one JSON line per shape.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gta_amd import native  # noqa: E402

HBM_TBS = 6.3
SHAPES = {   # B, H, Tq, Tk, Nq, Nk, f_dims  
    "ms-enc": (32, 8, 1280, 1280, 5, 5, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}),
    "ms-dec": (32, 8, 2560, 1280, 5, 5, {"triv": 0, "se3": 48, "so3": 24, "so2": 24}),
    "cl-enc": (32, 6, 600, 600, 2, 2, {"se3": 32, "so2": 32}),
    "cl-dec": (32, 6, 2559, 600, 3, 2, {"se3": 32, "so2": 32}),
    "dit": (32, 16, 1024, 1024, 1, 1, {"so2": 64}),
}


def setup(name, key_views=None):
    """-> (run, bytes) of the shape's pass; with ``key_views`` (view counts, cycled over the B scenes) -> (run, bytes, masked run, valid-token
    share): the masked entry (gta_rep_grad_sums_varlen) on the same buffers -- the key side under the counts, and the query side too where it
    has the key side's views (self-attention: query_views = key_views)"""
    B, H, Tq, Tk, Nq, Nk, f = SHAPES[name]
    dh = sum(f.values())
    mk = lambda T: torch.randn(B, T, H, dh, device="cuda", dtype=torch.bfloat16).permute(0, 2, 1, 3)
    q, dq, dout, out = mk(Tq), mk(Tq), mk(Tq), mk(Tq)
    k, dk, v, dv = mk(Tk), mk(Tk), mk(Tk), mk(Tk)
    desc = native.make_desc(q, k, v, out, f, 2 if f.get("so3") else 0, Nq, Nk, dh ** -0.5, native.FLAG_V_TRANSFORM)
    view, so2 = f.get("se3", 0) > 0, f.get("so2", 0) > 0

    def run(q_lens=None, k_lens=None):
        native.rep_grad_sums(desc, 0, ((q, dq), (dout, out)), view=view, so2=so2, lens=q_lens)
        native.rep_grad_sums(desc, 1, ((dk, k), (dv, v)), view=view, so2=so2, lens=k_lens)
    read = 4 * B * H * (Tq + Tk) * (f.get("se3", 0) + f.get("so2", 0)) * 2             # four tensors per side, the two slabs, bf16
    written = 4 * (B * (Nq + Nk) * 16 * (2 if view else 0) + B * (Tq + Tk) * f.get("so2", 0) * 2)   # view sums (+ partials) and so2 sums
    if key_views is None:
        return run, read + written
    if not view or any(n < 1 or n > Nk for n in key_views):
        raise SystemExit(f"--key-views: {name} has {Nk} key views" if view else f"--key-views: {name} has no view structure")
    counts = [key_views[b % len(key_views)] for b in range(B)]
    k_lens = torch.tensor([n * (Tk // Nk) for n in counts], dtype=torch.int32, device="cuda")
    self_attn = (Tq, Nq) == (Tk, Nk)
    q_lens = k_lens if self_attn else None
    share = (sum(counts) * (Tk // Nk) + (sum(counts) * (Tq // Nq) if self_attn else B * Tq)) / (B * (Tq + Tk))
    return run, read + written, lambda: run(q_lens, k_lens), share


def time_it(run, seconds=1.0, iters=200):
    t0 = time.time()
    while time.time() - t0 < seconds:                  # sustained regime: the clock settles after ~1 s of load
        run()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3           # us per pass (both sides, launches included)


def kernel_stats(outdir):
    """sum of the average kernel times of the pass's kernels per shape, from the rocprofv3 stats CSV"""
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_stats.csv under {outdir}")
    rows = list(csv.DictReader(open(files[0])))
    return {r["Name"]: (int(r["Calls"]), float(r["AverageNs"]) / 1e3) for r in rows if "repgrad" in r["Name"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--rocprof", metavar="DIR", help="profile the loop in a child process under rocprofv3 into DIR")
    ap.add_argument("--key-views", metavar="N,N,...", help="per-scene view counts (cycled over the batch): time the masked entry "
                    "(gta_rep_grad_sums_varlen) beside the unmasked one on the same buffers")
    ap.add_argument("--loop", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_rep_grad.py needs an MI355X")
    names = a.shapes.split(",")
    key_views = [int(x) for x in a.key_views.split(",")] if a.key_views else None
    if a.loop:                                         # the profiled child: one shape per call so the stats are per shape
        run = setup(names[0], key_views)[2 if key_views else 0]          # (with --key-views: the masked pass)
        for _ in range(50):
            run()
        torch.cuda.synchronize()
        return

    def profiled(out, name, extra=()):
        """kernel microseconds of one pass from a child under rocprofv3 (50 passes: each kernel's average time x its launches per pass)"""
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "rg", "--", sys.executable,
                        os.path.abspath(__file__), "--loop", "--shapes", name, *extra], check=True, timeout=300, stdout=subprocess.DEVNULL)
        st = kernel_stats(out)
        return st, sum(avg * (calls / 50) for calls, avg in st.values())

    for name in names:
        run, nbytes, *masked = setup(name, key_views)
        rec = {"shape": name, "bytes": nbytes, "us_per_pass_events": round(time_it(run), 2)}
        if masked:
            rec.update({"key_views": key_views, "valid_token_share": round(masked[1], 4), "us_per_pass_events_masked": round(time_it(masked[0]), 2)})
            rec["masked_over_unmasked_events"] = round(rec["us_per_pass_events_masked"] / rec["us_per_pass_events"], 4)
        if a.rocprof:
            st, us = profiled(os.path.join(a.rocprof, name), name)
            rec.update({"kernels": {k: round(v[1], 2) for k, v in st.items()}, "kernel_us_per_pass": round(us, 2),
                        "TB_s": round(nbytes / (us * 1e-6) / 1e12, 2), "of_hbm_ceiling": round(nbytes / (us * 1e-6) / 1e12 / HBM_TBS, 3)})
            if masked:
                st, us_m = profiled(os.path.join(a.rocprof, name + "-masked"), name, ("--key-views", a.key_views))
                rec.update({"kernels_masked": {k: round(v[1], 2) for k, v in st.items()}, "kernel_us_per_pass_masked": round(us_m, 2),
                            "masked_over_unmasked_kernels": round(us_m / us, 4)})
        else:
            rec["TB_s_events"] = round(nbytes / (rec["us_per_pass_events"] * 1e-6) / 1e12, 2)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

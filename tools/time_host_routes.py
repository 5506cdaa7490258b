"""Host time of ``gta_attention`` forward + backward on the fused layout, per route, with every native entry a no-op (the spies of
tests/_call_routes.py): what is left is the Python between the public call and the C ABI.  No GPU.

    python tools/time_host_routes.py [--against CHECKOUT] [--calls 200] [--warmup 20] [--repeats 5]

Per route and per repeat: the median microseconds of one forward + backward.  With ``--against`` the package of another checkout (the
parent commit) is loaded beside this one under another name and the two are called ALTERNATELY, call by call, in this one process, so that
both see the same machine; the line then holds both lists of medians, the other checkout's spread (max - min of its repeated medians) and
this checkout's median of medians minus the other's.  Prints one JSON line."""
import argparse
import contextlib
import importlib.util
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--against", default=None)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()

import gta_amd  # noqa: E402
from gta_amd import native  # noqa: E402
from tests import _call_routes as R  # noqa: E402


def load_copy(root, name):
    """the package of another checkout under ``name`` (its imports are relative); it runs on this checkout's library"""
    os.environ.setdefault("GTA_HIP_LIB", native.LIB_PATH)
    pkg = os.path.join(os.path.abspath(root), "gta_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


copies = {"this": gta_amd}
if args.against:
    copies["other"] = load_copy(args.against, "gta_amd_other")
F_DIMS = R.LAYOUTS["fused"]["f_dims"]
ROUTES = {
    "unmasked": ({}, False),
    "key_views_backward": (dict(key_views=[1, R.NK], key_views_backward=True), False),
    "key_mask_backward": (dict(key_mask=R.key_mask(), key_mask_backward=True), False),
    "both masks, carriers": (dict(key_mask=R.key_mask(), query_mask=R.query_mask(), key_mask_backward=True, key_mask_rep_grad=True), True),
}


def medians(kw, tables_grad):
    leaves, packed = R.inputs(F_DIMS, tables_grad=tables_grad)
    times = {name: [] for name in copies}
    order = list(copies.items())
    for i in range(args.warmup + args.calls):
        for name, pkg in order[::1 - 2 * (i % 2)]:          # (the one called first pays for the cold caches: take turns)
            t0 = time.perf_counter()
            out = pkg.gta_attention(leaves["q"], leaves["k"], leaves["v"], F_DIMS, packed, trans_coeff=leaves["trans_coeff"], tau=leaves["tau"], **kw)
            out.sum().backward()
            times[name].append(time.perf_counter() - t0)
    return {name: statistics.median(ts[args.warmup:]) * 1e6 for name, ts in times.items()}


result = {}
for route, (kw, tables_grad) in ROUTES.items():
    with contextlib.ExitStack() as stack:
        for name, pkg in copies.items():
            stack.enter_context(R.spies(None, cuda_carriers=tables_grad and name == "this", native=sys.modules[pkg.__name__ + ".native"],
                                        repgrad=sys.modules[pkg.__name__ + ".repgrad"]))
        runs = [medians(kw, tables_grad) for _ in range(args.repeats)]
    result[route] = {name: [round(r[name], 1) for r in runs] for name in copies}
    if args.against:
        other = result[route]["other"]
        result[route]["other_spread"] = round(max(other) - min(other), 1)
        result[route]["this_minus_other"] = round(statistics.median(result[route]["this"]) - statistics.median(other), 1)
print(json.dumps(result))

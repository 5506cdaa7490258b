"""Do the kernels of two checkouts compile to the same instructions?

    python tools/compare_disasm.py OLD_TREE [NEW_TREE]        # NEW_TREE: this checkout

Compiles every kernel source of gta_amd/csrc in both trees to gfx950 assembly with the Makefile's flags and compares, function by function,
the instruction streams (comments, directives and the numbering of local labels dropped; other symbols replaced by a placeholder).  A
function is matched by its demangled name; against an OLD_TREE from before the templates gained their defaulted VARLEN argument, a trailing
`false` of those is ignored and their `true` instances are counted as new (so are the instances with a trailing argument type: the GATHER
instances of gta_kv_prep_kernel and of gta_gen_prep_kernel, the q_lens / dlse / (q_lens, q_live) instances of gta_bwd_prep_kernel, the QMASK instances
`gta_fwd2_kernel<..., true, unsigned char const*>`; a kernel with a name of its own, as gta_bwd_dkv_gather_kernel or gta_bwd_dq_qmask_kernel, is new anyway).  Exit status 1 when a function of OLD_TREE is missing from NEW_TREE or differs.  Needs hipcc and c++filt."""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = ["gta_reps", "gta_fwd", "gta_prep", "gta_fwd2", "gta_fwd_gen", "gta_fwd_cl", "gta_fwd64", "gta_bwd", "gta_apply", "gta_plain32", "gta_repgrad", "gta_merge", "gta_maskidx",
           "gta_block", "gta_wgrad"]                                                             # (the block library's kernels)
NO_SLP = {"gta_fwd2", "gta_fwd64", "gta_fwd_gen", "gta_fwd_cl", "gta_bwd", "gta_prep"}          # (FLAGS_* of the Makefile)
VARLEN = ("gta_fwd2_kernel", "gta_kv_prep_kernel", "gta_gen_prep_kernel", "gta_gen_attn_kernel", "gta_bwd_prep_kernel")


def assembly(tree, name, out):
    if not os.path.exists(os.path.join(tree, "gta_amd", "csrc", name + ".hip")):      # a source the tree does not have yet: no functions
        return ""
    cmd = [HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", *(["-fno-slp-vectorize"] if name in NO_SLP else []),
           "-S", "--cuda-device-only", "-o", out, os.path.join(tree, "gta_amd", "csrc", name + ".hip")]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return open(out).read()


def functions(text):
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*(?:;.*)?$", text, re.M):
        end = text.find(".Lfunc_end", m.start())
        if end < 0:
            continue
        lines = []
        for line in text[m.end():end].split("\n"):
            line = line.split(";")[0].strip()
            if not line or (line.startswith(".") and not line.startswith(".LBB")):
                continue
            lines.append(re.sub(r"_Z\w+", "SYM", re.sub(r"\.LBB\d+_", ".LBB_", line)))
        out[m.group(1)] = lines
    names = list(out)
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"\(anonymous namespace\)::", "", d): out[n] for n, d in zip(names, plain)}


def canonical(name):
    """None for a VARLEN = true instance, else the name without a trailing defaulted `false`"""
    if not any(k + "<" in name for k in VARLEN):
        return name
    m = re.match(r"(.*?<)(.*)(>\(.*)$", name)
    args = m.group(2).split(", ")
    if args[-1] == "true":
        return None
    return name if args[-1] != "false" else m.group(1) + ", ".join(args[:-1]) + m.group(3)


def main():
    old_tree = sys.argv[1]
    new_tree = sys.argv[2] if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    total = same = new = 0
    bad = []
    with tempfile.TemporaryDirectory() as td, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        jobs = {(t, s): pool.submit(assembly, tree, s, os.path.join(td, f"{t}_{s}.s")) for t, tree in (("old", old_tree), ("new", new_tree)) for s in SOURCES}
        for s in SOURCES:
            old = functions(jobs[("old", s)].result())
            new_all = functions(jobs[("new", s)].result())
            # (the old tree's names are taken as they are; a name of the new tree that the old tree has too -- it has the extra argument as well -- is its own key)
            new_fns = {(k if k in old else canonical(k)): v for k, v in new_all.items() if k in old or canonical(k) is not None}
            new += len(new_all) - len(new_fns) + sum(1 for k in new_fns if k not in old)
            for name, body in old.items():
                total += 1
                key = name
                if key not in new_fns:
                    bad.append(f"{s}: {name}: not in the new tree")
                elif new_fns[key] != body:
                    n = sum(1 for a, b in zip(body, new_fns[key]) if a != b) + abs(len(body) - len(new_fns[key]))
                    bad.append(f"{s}: {name}: {n} of {len(body)} lines differ")
                else:
                    same += 1
    for line in bad:
        print(line)
    print(f"{same}/{total} functions of the old tree compile to the same instructions; {new} new functions")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()

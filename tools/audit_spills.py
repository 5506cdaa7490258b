"""Audit of the persistent attention kernel's register allocation (gta_fwd2_kernel).

The kernel is an item loop around a tile loop that needs the whole 256-register budget of a wave.  Three things make
hipcc spill there (gta_fwd2.hip says where each is handled): kernel arguments kept live across the loop nest, lane-derived
address arithmetic hoisted out of the item loop, and loop-body arrays that are assigned only conditionally (they become
loop-carried).  A spill of a freshly loaded value sits behind an s_waitcnt vmcnt(0) and serialises the prologue's loads,
so the shipped layouts must stay at ZERO scratch accesses.  This script compiles gta_fwd2.hip to assembly with the
Makefile's flags and reports, per instantiation, registers, scratch accesses and SGPR spill traffic."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (dhp, esz, layout) of the shipped configs: MSN gta_so3 (96, MS = 1), CLEVR-TR gta (64, CL = 2), pure so2 (64, SO2 = 3)
SHIPPED = {(96, 2, 1), (96, 4, 1), (64, 2, 2), (64, 4, 2), (64, 2, 3), (64, 4, 3)}


def audit():
    src = os.path.join(ROOT, "gta_amd", "csrc", "gta_fwd2.hip")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "fwd2.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-fno-slp-vectorize", "-S",
                        "--cuda-device-only", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
        text = open(out).read()
    report, problems = [], []
    for m in re.finditer(r"^(_ZN\w*gta_fwd2_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELb(\d)E\w+):", text, re.M):
        x3 = m.group(5) == "1"          # the fp32-faithful instances (split-bf16 operands): two workgroups per CU, 256 registers
        varlen = m.group(6) == "1"      # the instances with per-scene key prefixes (gta_attn_fwd_varlen): held to the rules of their twins
        qmask = "ELb1EJPKhEE" in m.group(1)    # the VARLEN instances with the trailing q_live argument (gta_attn_fwd_qmask): held to their VARLEN twins
        name, key = m.group(1), ((int(m.group(2)), int(m.group(3)), int(m.group(4))) + (("x3",) if x3 else ()) + (("varlen",) if varlen else ())
                                 + (("qmask",) if qmask else ()))
        body = text[m.start():text.index(".Lfunc_end", m.start())]
        meta = text[text.index(".amdhsa_kernel " + name):][:4000]
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        row = {"instance": key, "vgpr": vgpr, "scratch": body.count("scratch_"), "sgpr_spill_writes": body.count("v_writelane"),
               "sgpr_spill_reads": body.count("v_readlane")}
        report.append(row)
        if (key in SHIPPED or ((x3 or varlen) and key[:3] in SHIPPED)) and row["scratch"]:
            problems.append(f"perf: gta_fwd2_kernel<{key}> has {row['scratch']} scratch accesses")
        elif varlen and key[0] <= 64 and row["scratch"]:          # (every layout of the new instances at dh <= 64, not the shipped ones alone)
            problems.append(f"perf: gta_fwd2_kernel<{key}> has {row['scratch']} scratch accesses")
        if key[0] <= 64 and vgpr > (256 if x3 else 168):
            problems.append(f"perf: gta_fwd2_kernel<{key}> needs {vgpr} VGPRs: the dh <= 64 instances must allow three waves per SIMD")
    # a VARLEN instance never has more scratch accesses than its twin without the key prefix (a comparison inside one compiler run, so a hard
    # criterion, not a "perf:" one: it needs no headroom)
    scratch = {r["instance"]: r["scratch"] for r in report}
    for key, n in scratch.items():
        if key[-1] == "varlen" and key[:-1] in scratch and n > scratch[key[:-1]]:
            problems.append(f"gta_fwd2_kernel<{key}> has {n} scratch accesses, its twin without VARLEN {scratch[key[:-1]]}")
    # a QMASK instance by the same rule against its VARLEN twin, and it keeps the twin's occupancy (waves per SIMD the registers allow: the mask
    # must not live through the tile loop); one QMASK instance per VARLEN one
    vgprs = {r["instance"]: r["vgpr"] for r in report}
    waves = lambda v: min(8, 512 // ((v + 7) // 8 * 8))
    for key, n in scratch.items():
        if key[-1] == "qmask":
            twin = key[:-1]
            if twin not in scratch or n > scratch[twin]:
                problems.append(f"gta_fwd2_kernel<{key}> has {n} scratch accesses, its VARLEN twin {scratch.get(twin)}")
            elif waves(vgprs[key]) < waves(vgprs[twin]):
                problems.append(f"gta_fwd2_kernel<{key}> needs {vgprs[key]} VGPRs, its VARLEN twin {vgprs[twin]}: fewer waves per SIMD")
    n_qmask, n_varlen = sum(1 for k in scratch if k[-1] == "qmask"), sum(1 for k in scratch if k[-1] == "varlen")
    if n_qmask != n_varlen:
        problems.append(f"{n_qmask} QMASK instances of gta_fwd2_kernel for {n_varlen} VARLEN ones")
    # the dh = 64 bf16 instance (gta_fwd_cl.hip, r06): three workgroups per CU, no scratch anywhere
    text = _asm("gta_fwd_cl.hip", ("-fno-slp-vectorize",))
    for name, (layout,), body, vgpr in _kernels(text, r"gta_fwdc_kernelILi(\d+)E"):
        row = {"kernel": f"gta_fwdc_kernel<{layout}>", "vgpr": vgpr, "scratch": body.count("scratch_"), "sgpr_spill_writes": body.count("v_writelane")}
        report.append(row)
        if row["scratch"] and int(layout) == 2:
            problems.append(f"perf: {row['kernel']}: {row['scratch']} scratch accesses")
        if vgpr > 168:
            problems.append(f"perf: {row['kernel']}: {vgpr} VGPRs (three waves per SIMD need <= 168)")
    return report, problems


def _asm(src_name, extra=()):
    src = os.path.join(ROOT, "gta_amd", "csrc", src_name)
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", *extra, "-S",
                        "--cuda-device-only", "-o", out, src], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def _kernels(text, pattern):
    for m in re.finditer(r"^(_ZN\w*" + pattern + r"\w*):", text, re.M):
        name = m.group(1)
        body = text[m.start():text.index(".Lfunc_end", m.start())]
        meta = text[text.index(".amdhsa_kernel " + name):][:4000]
        yield name, m.groups()[1:], body, int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))


def audit_others():
    """The kernels beside the attention forward that were tuned by instruction counts and occupancy (DESIGN.md sections 4.1,
    4.3, 8): the K/V pre-pass must stay scratch-free and within the registers of five workgroups per CU at the shipped head
    sizes (it is at 89 VGPRs at dh = 96: the LDS would allow six), the backward kernels scratch-free (dK/dV at dh = 128 runs one workgroup per CU for that), and the weight-gradient kernel's steady-state loop (the loops with
    one step's 32 MFMAs) free of scratch accesses."""
    report, problems = [], []
    text = _asm("gta_prep.hip", ("-fno-slp-vectorize",))
    # template arguments <DHP, ESZ, X3, VARLEN, GATHER>; the GATHER instances (gta_attn_fwd_gather) are held to every rule of the others
    for name, (dhp, esz, x3, varlen, gather), body, vgpr in _kernels(text, r"gta_kv_prep_kernelILi(\d+)ELi(\d+)ELb(\d)ELb(\d)ELb(\d)E"):
        row = {"kernel": f"gta_kv_prep_kernel<{dhp},{esz}{', x3' if x3 == '1' else ''}{', varlen' if varlen == '1' else ''}{', gather' if gather == '1' else ''}>",
               "vgpr": vgpr, "scratch": body.count("scratch_")}
        report.append(row)
        if row["scratch"]:
            problems.append(f"perf: {row['kernel']}: {row['scratch']} scratch accesses")
        if int(dhp) <= 96 and int(esz) == 2 and vgpr > 96:
            problems.append(f"perf: {row['kernel']}: {vgpr} VGPRs (five 4-wave workgroups per CU need <= 96; six would need <= 80)")
    text = _asm("gta_bwd.hip", ("-fno-slp-vectorize",))
    bwd_scratch = {}
    for kern in ("gta_bwd_prep_kernel", "gta_bwd_dq_kernel", "gta_bwd_dkv_kernel"):
        for name, (dhp, esz), body, vgpr in _kernels(text, kern + r"ILi(\d+)ELi(\d+)E"):
            row = {"kernel": f"{kern}<{dhp},{esz}>", "vgpr": vgpr, "scratch": body.count("scratch_")}
            report.append(row)
            if kern == "gta_bwd_prep_kernel" and "ELb0ELb1E" in name:      # its VARLEN instances <dhp, esz, false, true, q_lens>: below
                report.pop()
                continue
            if kern == "gta_bwd_prep_kernel" and "JPKfE" in name:         # its DLSE instances <dhp, esz, x3, false, dlse>: below
                report.pop()
                continue
            if "ELb1E" not in name:                     # (not the prep kernel's X3 instances, which share <dhp, 4>)
                bwd_scratch[(kern, dhp, esz)] = row["scratch"]
            if row["scratch"]:
                problems.append(f"perf: {row['kernel']}: {row['scratch']} scratch accesses")
    # the VARLEN instances (gta_attn_bwd_varlen) are held to the rule of the forward's: never more scratch accesses than the twin without
    # the prefixes (a comparison inside one compiler run: a hard criterion)
    for kern in ("gta_bwd_prep", "gta_bwd_dq", "gta_bwd_dkv"):
        pattern = r"_kernelILi(\d+)ELi(\d+)ELb0ELb1E" if kern == "gta_bwd_prep" else r"_varlen_kernelILi(\d+)ELi(\d+)E"
        for name, (dhp, esz), body, vgpr in _kernels(text, kern + pattern):
            if "JPKiPKhEE" in name:                     # the pre-pass's QMASK instances <dhp, esz, false, true, q_lens, q_live>: below
                continue
            if "PKfEE" in name:                         # its masked DLSE twins <.., q_lens[, q_live], dlse>: below
                continue
            row = {"kernel": f"{kern}_varlen_kernel<{dhp},{esz}>", "vgpr": vgpr, "scratch": body.count("scratch_")}
            report.append(row)
            twin = bwd_scratch.get((kern + "_kernel", dhp, esz))
            if twin is None or row["scratch"] > twin:
                problems.append(f"{row['kernel']} has {row['scratch']} scratch accesses, its twin without VARLEN {twin}")
    # the GATHER instances of the dK/dV walk (gta_attn_bwd_gather) by the same rule against their VARLEN twins: eight of them, one per twin
    varlen_scratch = {r["kernel"]: r["scratch"] for r in report if r["kernel"].startswith("gta_bwd_dkv_varlen_kernel<")}
    n_gather = 0
    for name, (dhp, esz), body, vgpr in _kernels(text, r"gta_bwd_dkv_gather_kernelILi(\d+)ELi(\d+)E"):
        row = {"kernel": f"gta_bwd_dkv_gather_kernel<{dhp},{esz}>", "vgpr": vgpr, "scratch": body.count("scratch_")}
        report.append(row)
        n_gather += 1
        twin = varlen_scratch.get(f"gta_bwd_dkv_varlen_kernel<{dhp},{esz}>")
        if twin is None or row["scratch"] > twin:
            problems.append(f"{row['kernel']} has {row['scratch']} scratch accesses, its VARLEN twin {twin}")
    if n_gather != len(varlen_scratch):
        problems.append(f"{n_gather} GATHER instances of the dK/dV walk for {len(varlen_scratch)} VARLEN ones")
    # the QMASK instances of the pre-pass and of the dQ walk (gta_attn_bwd_qmask) by the same rule against their VARLEN twins, one per twin
    for kern, pattern in (("gta_bwd_prep", r"gta_bwd_prep_kernelILi(\d+)ELi(\d+)ELb0ELb1EJPKiPKhEE"), ("gta_bwd_dq", r"gta_bwd_dq_qmask_kernelILi(\d+)ELi(\d+)E")):
        twins = {r["kernel"]: r["scratch"] for r in report if r["kernel"].startswith(kern + "_varlen_kernel<")}
        n_qmask = 0
        for name, (dhp, esz), body, vgpr in _kernels(text, pattern):
            row = {"kernel": f"{kern}_qmask_kernel<{dhp},{esz}>", "vgpr": vgpr, "scratch": body.count("scratch_")}
            report.append(row)
            n_qmask += 1
            twin = twins.get(f"{kern}_varlen_kernel<{dhp},{esz}>")
            if twin is None or row["scratch"] > twin:
                problems.append(f"{row['kernel']} has {row['scratch']} scratch accesses, its VARLEN twin {twin}")
        if n_qmask != len(twins):
            problems.append(f"{n_qmask} QMASK instances of {kern} for {len(twins)} VARLEN ones")
    # the DLSE instances of the pre-pass (gta_attn_bwd_dlse) by the same rule against the twin without dlse, X3 ones against the X3 twin
    prep = {}
    for name, (dhp, esz, x3), body, vgpr in _kernels(text, r"gta_bwd_prep_kernelILi(\d+)ELi(\d+)ELb(\d)ELb0EJ"):
        prep[(dhp, esz, x3, "JPKfE" in name)] = (body.count("scratch_"), vgpr)
    for (dhp, esz, x3, dlse), (n, vgpr) in sorted(prep.items()):
        if not dlse:
            continue
        row = {"kernel": f"gta_bwd_prep_kernel<{dhp},{esz}{', x3' if x3 == '1' else ''}, dlse>", "vgpr": vgpr, "scratch": n}
        report.append(row)
        twin = prep.get((dhp, esz, x3, False))
        if twin is None or n > twin[0]:
            problems.append(f"{row['kernel']} has {n} scratch accesses, its twin without dlse {twin and twin[0]}")
    # the DLSE twins of the masked pre-pass instances (gta_attn_bwd_varlen_dlse / _gather_dlse: <.., q_lens, dlse>; gta_attn_bwd_qmask_dlse:
    # <.., q_lens, q_live, dlse>) by the same rule against the masked instance without dlse, one per twin
    for kind, tail in (("varlen", "JPKiPKfEE"), ("qmask", "JPKiPKhPKfEE")):
        twins = {r["kernel"]: r["scratch"] for r in report if r["kernel"].startswith(f"gta_bwd_prep_{kind}_kernel<")}
        n_dlse = 0
        for name, (dhp, esz), body, vgpr in _kernels(text, r"gta_bwd_prep_kernelILi(\d+)ELi(\d+)ELb0ELb1E" + tail):
            row = {"kernel": f"gta_bwd_prep_{kind}_dlse_kernel<{dhp},{esz}>", "vgpr": vgpr, "scratch": body.count("scratch_")}
            report.append(row)
            n_dlse += 1
            twin = twins.get(f"gta_bwd_prep_{kind}_kernel<{dhp},{esz}>")
            if twin is None or row["scratch"] > twin:
                problems.append(f"{row['kernel']} has {row['scratch']} scratch accesses, its twin without dlse {twin}")
        if n_dlse != len(twins):
            problems.append(f"{n_dlse} DLSE twins of gta_bwd_prep_{kind}_kernel for {len(twins)} instances without dlse")
    # the merge kernels (gta_merge.hip): the partials' pointers and strides are indexed by unrolled constants -- no scratch at all (hard)
    mtext = _asm("gta_merge.hip")
    n_merge = 0
    for name, (esz,), body, vgpr in _kernels(mtext, r"gta_merge_(?:bwd_)?kernelILi(\d+)E"):
        kind = "gta_merge_bwd_kernel" if "merge_bwd" in name else "gta_merge_kernel"
        row = {"kernel": f"{kind}<{esz}>", "vgpr": vgpr, "scratch": body.count("scratch_")}
        report.append(row)
        n_merge += 1
        if row["scratch"]:
            problems.append(f"{row['kernel']}: {row['scratch']} scratch accesses")
    if n_merge != 4:
        problems.append(f"gta_merge.hip: {n_merge} kernel instances found (expected 4)")
    # the mask-index kernel (gta_maskidx.hip): one instance, a handful of registers, no scratch of either kind (hard)
    xtext = _asm("gta_maskidx.hip")
    n_maskidx = 0
    for name, _, body, vgpr in _kernels(xtext, r"gta_mask_index_kernel()"):
        meta = xtext[xtext.index(".amdhsa_kernel " + name):][:4000]
        private = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        row = {"kernel": "gta_mask_index_kernel", "vgpr": vgpr, "scratch": body.count("scratch_") + private}
        report.append(row)
        n_maskidx += 1
        if row["scratch"]:
            problems.append(f"{row['kernel']}: scratch in use ({row['scratch']})")
    if n_maskidx != 1:
        problems.append(f"gta_maskidx.hip: {n_maskidx} kernel instances found (expected 1)")
    text = _asm("gta_wgrad.hip")
    for name, _, body, vgpr in _kernels(text, r"wgrad_kernelILb(\d)E"):
        lines = body.split("\n")
        labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
        steady = 0
        for i, l in enumerate(lines):
            m = re.search(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", l)
            if m and m.group(1) in labels and labels[m.group(1)] < i:
                loop = lines[labels[m.group(1)]:i]
                if sum("v_mfma" in x for x in loop) == 32 and len(loop) < 400:
                    steady += 1
                    if any("scratch_" in x for x in loop):
                        problems.append(f"perf: {name}: scratch access inside a steady-state loop")
        report.append({"kernel": name, "vgpr": vgpr, "steady_loops": steady})
        if not steady:
            problems.append(f"perf: {name}: no loop with one step's 32 MFMAs found")
    return report, problems


def audit_dkv64():
    """gta_bwd_dkv64_kernel (gta_bwd.hip): ONE generated statement (gen_bwd64.py) owns v24..v255 and every accumulator register; it leaves
    dK'^T / dV'^T in a[0:191] (the dQ kernel: a[0:95]) and names them as its OUTPUTS (GTA_BWD64_*_RESULTS, r05), so hipcc reads them out
    itself.  What it may do with the accumulator file: v_accvgpr_read of those result registers, nothing else (no writes, no copies, no
    other register); and at most a handful of scratch accesses (the epilogue holds 192 accumulator values beside its own)."""
    text = _asm("gta_bwd.hip", ("-fno-slp-vectorize",))
    report, problems = [], []
    for m in re.finditer(r"^(_ZN\w*gta_bwd_(?:dkv|dq|dqkv)64_kernel\w+):", text, re.M):
        name = m.group(1)
        want_stmts = 2 if "dqkv64" in name else 1            # (the joint launch holds both bodies)
        body = text[m.start():text.index(".Lfunc_end", m.start())]
        meta = text[text.index(".amdhsa_kernel " + name):][:4000]
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        accum = int(re.search(r"\.amdhsa_accum_offset\s+(\d+)", meta).group(1))
        n_results = 288 if "dqkv64" in name else 192 if "dkv64" in name else 96        # (the joint kernel: either body's registers)
        n_results = min(n_results, 192)
        inasm, compiler_acc, scratch, long_stmts, cur_len, result_reads = False, 0, 0, 0, 0, 0
        for line in body.split("\n"):
            if "#ASMSTART" in line:
                inasm, cur_len = True, 0
                continue
            if "#ASMEND" in line:
                inasm = False
                long_stmts += cur_len > 1000
                continue
            if inasm:
                cur_len += 1
                continue
            code = line.split(";")[0]
            n_acc = len(re.findall(r"\ba\[?\d+", code))
            mr = re.match(r"\s*v_accvgpr_read_b32\s+v\d+,\s*a(\d+)\s*$", code)
            if mr and int(mr.group(1)) < n_results:
                result_reads += 1
            else:
                compiler_acc += n_acc
            scratch += "scratch_" in line
        report.append({"kernel": name, "vgpr": vgpr, "accum_offset": accum, "result_reads": result_reads, "compiler_agpr_uses": compiler_acc,
                       "scratch": scratch, "loop_statements": long_stmts})
        if compiler_acc:
            problems.append(f"{name}: hipcc uses accumulator registers beyond reading the statements' results ({compiler_acc} operands)")
        want_reads = {"dqkv64": 288, "dkv64": 192}.get("dqkv64" if "dqkv64" in name else "dkv64" if "dkv64" in name else "", 96)
        if result_reads != want_reads:
            problems.append(f"{name}: {result_reads} reads of result registers (expected {want_reads}: every result once)")
        if long_stmts != want_stmts:
            problems.append(f"{name}: {long_stmts} generated statements (expected {want_stmts})")
        if vgpr != 512 or accum != 256:
            problems.append(f"{name}: register file split {accum} / {vgpr} (expected 256 / 512)")
        if scratch > 12 * want_stmts:
            problems.append(f"perf: {name}: {scratch} scratch accesses")
    return report, problems


def audit_attn64():
    """gta_attn64_kernel (gta_fwd64.hip): the tile loop statement owns v32-v255 and the accumulator file from a28 up by literal register
    number.  Since r05 what crosses its boundary in the accumulator file is in its operand list -- the Q' fragments it takes ("+{a[..]}"), the O
    accumulators it leaves ("={a[..]}"; gen_attn64.py) -- so hipcc moves those values itself and may park others in a[0:27] or anywhere the
    statement does not name; the audit counts that traffic for the record.  Checked: the loop statement is the single long one, the register
    file split, and (nearly) no scratch access (a reload sits behind a vmcnt(0))."""
    text = _asm("gta_fwd64.hip", ("-fno-slp-vectorize",))
    report, problems = [], []
    for m in re.finditer(r"^(_ZN\w*gta_attn64_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E\w+):", text, re.M):
        name, key = m.group(1), tuple(int(m.group(i)) for i in range(2, 7))       # (dh, element size, layout, variant, coalesced I/O)
        body = text[m.start():text.index(".Lfunc_end", m.start())]
        meta = text[text.index(".amdhsa_kernel " + name):][:4000]
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        accum = int(re.search(r"\.amdhsa_accum_offset\s+(\d+)", meta).group(1))
        inasm, compiler_acc, n_stmt_lines, scratch_lines, long_stmts, cur_len = False, 0, 0, [], 0, 0
        for i, line in enumerate(body.split("\n")):
            if "#ASMSTART" in line:
                inasm, cur_len = True, 0
                continue
            if "#ASMEND" in line:
                inasm = False
                long_stmts += cur_len > 1000
                continue
            if inasm:
                cur_len += 1
                continue
            for m2 in re.finditer(r"\ba\[?(\d+)(?::(\d+))?", line.split(";")[0]):
                compiler_acc += int(m2.group(2) or m2.group(1)) >= 28          # (a[0:27] are left to hipcc: gen_attn64.py)
            if "scratch_" in line:
                scratch_lines.append(i)
        row = {"instance": key, "vgpr": vgpr, "accum_offset": accum, "compiler_agpr_uses": compiler_acc, "scratch": len(scratch_lines),
               "loop_statements": long_stmts}
        report.append(row)
        if long_stmts != 1:
            problems.append(f"gta_attn64_kernel<{key}>: {long_stmts} loop statements (expected one)")
        if vgpr != 512 or accum != 256:
            problems.append(f"gta_attn64_kernel<{key}>: register file split {accum} / {vgpr} (expected 256 / 512)")
        if len(scratch_lines) > 16:
            problems.append(f"perf: gta_attn64_kernel<{key}>: {len(scratch_lines)} scratch accesses")
    # gta_attn64_items_kernel: the whole item loop is ONE statement that names v8..v255, every accumulator register and s20..s99; what
    # hipcc keeps across it lives in v0..v7 (SGPR spills go to lanes of those) -- no scratch, nothing of hipcc's in the accumulator file
    for m in re.finditer(r"^(_ZN\w*gta_attn64_items_kernel\w+):", text, re.M):
        name = m.group(1)
        body = text[m.start():text.index(".Lfunc_end", m.start())]
        meta = text[text.index(".amdhsa_kernel " + name):][:4000]
        vgpr = int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", meta).group(1))
        accum = int(re.search(r"\.amdhsa_accum_offset\s+(\d+)", meta).group(1))
        inasm, compiler_acc, long_stmts, cur_len, hi_vgpr = False, 0, 0, 0, 0
        for line in body.split("\n"):
            if "#ASMSTART" in line:
                inasm, cur_len = True, 0
                continue
            if "#ASMEND" in line:
                inasm = False
                long_stmts += cur_len > 1000
                continue
            if inasm:
                cur_len += 1
                continue
            code = line.split(";")[0]
            compiler_acc += len(re.findall(r"\ba\[?\d+", code))
        row = {"instance": "items", "vgpr": vgpr, "accum_offset": accum, "compiler_agpr_uses": compiler_acc, "scratch": body.count("scratch_"),
               "loop_statements": long_stmts}
        report.append(row)
        if compiler_acc or row["scratch"] or long_stmts != 1 or vgpr != 512 or accum != 256:
            problems.append(f"gta_attn64_items_kernel: {row}")
    return report, problems


def audit_gen():
    """The staged generic forward (gta_fwd_gen.hip): the pre-pass and both attention instances (with / without the euclid key bias) of every
    head size must stay scratch-free -- the row transform walks a row's slabs with run-time trip counts, the one construct here that could
    push a register array into scratch; the registers and the LDS of each instance are reported.  The LDS is dynamic (not in the assembly):
    the figures restate GenPrepSmem / Smem2 + the bias slots, and gta_fwd_gen.hip pins every one of them with a static_assert, so a layout
    change that this table misses does not compile."""
    text = _asm("gta_fwd_gen.hip", ("-fno-slp-vectorize",))
    report, problems = [], []
    for name, groups, body, vgpr in _kernels(text, r"gta_gen_(prep|attn)_kernelILi(\d+)E(?:Lb(\d)E)(?:Lb(\d)E)?"):
        # template arguments: prep <DHP, VARLEN[, key_idx]>, attn <DHP, BIAS, VARLEN>
        kind, dhp, b1, b2 = re.search(r"gta_gen_(prep|attn)_kernelILi(\d+)E(?:Lb(\d)E)(?:Lb(\d)E)?", name).groups()
        bias, varlen = (b1, b2) if kind == "attn" else ("0", b1)
        dhp = int(dhp)
        gather = kind == "prep" and "JPKiEE" in name      # the VARLEN pre-pass with the trailing key_idx argument (gta_attn_fwd_staged_gather): + its 256-byte row of token numbers
        lds = (2 * 64 * (dhp + 1) * 4 + 2 * 64 * dhp * 2 + (256 if gather else 0)) if kind == "prep" else 3 * 2 * 64 * dhp * 2 + (3 * 4 * 256 if bias == "1" else 0)
        row = {"kernel": f"gta_gen_{kind}_kernel<{dhp}{', bias' if bias == '1' else ''}{', varlen' if varlen == '1' else ''}{', gather' if gather else ''}>", "vgpr": vgpr, "scratch": body.count("scratch_"),
               "lds_bytes": lds, "sgpr_spill_writes": body.count("v_writelane")}
        report.append(row)
        if row["scratch"]:                                # (a hard failure, not a "perf:" warning: these kernels have no spill to tolerate)
            problems.append(f"{row['kernel']}: {row['scratch']} scratch accesses")
        if kind == "attn" and vgpr > (256 if dhp <= 96 else 512):
            problems.append(f"perf: {row['kernel']}: {vgpr} VGPRs (two workgroups per CU at dh <= 96 need <= 256)")
    return report, problems


def audit_repgrad():
    """The rep-gradient sums (gta_repgrad.hip): the six <ESZ, EUCLID, VEC> instances, their VARLEN twins (gta_rep_grad_sums_varlen) and
    their MASKED twins (gta_rep_grad_sums_masked: the trailing `const uint8_t*`).  Registers as the code object's metadata counts them
    (.vgpr_count), the static LDS and scratch; DESIGN.md 4.8 / 4.8c / 4.8d: no scratch, the 32 KiB reduction array, 44-64 VGPRs.  Hard:
    eighteen instances, no scratch, a VARLEN or MASKED twin with the LDS of its instance, and a MASKED twin with no more VGPRs than its
    VARLEN twin (the mask byte and the workgroup-wide OR die before the sums begin).  A MASKED twin above its unmasked instance's count is
    reported ("perf:"): hipcc gives every instance with a run-time row predicate 4 more than the one whose predicate is `tl < ntok`, the
    VARLEN twins included, and the LDS bounds the occupancy (five workgroups per CU) well below either count."""
    text = _asm("gta_repgrad.hip")
    report, problems, seen = [], [], {}
    for name, (esz, euclid, vec, varlen), body, _ in _kernels(text, r"gta_repgrad_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)E"):
        meta = text[text.index(".amdhsa_kernel " + name):][:4000]
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", meta).group(1))
        private = int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", meta).group(1))
        vgpr = int(re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text).group(1))
        masked = "JPKhEE" in name
        key = (int(esz), euclid == "1", vec == "1", "masked" if masked else varlen == "1")
        row = {"kernel": f"gta_repgrad_kernel<{esz}, {'euclid' if key[1] else 'se3'}, {'vec' if key[2] else 'scalar'}{', masked' if masked else ', varlen' if key[3] else ''}>",
               "vgpr": vgpr, "lds_bytes": lds, "scratch": body.count("scratch_") + private}
        seen[key] = row
        report.append(row)
        if row["scratch"]:
            problems.append(f"{row['kernel']}: scratch in use ({row['scratch']})")
        if vgpr > 64:
            problems.append(f"perf: {row['kernel']}: {vgpr} VGPRs (DESIGN.md 4.8: 44-64)")
    if len(seen) != 18:
        problems.append(f"gta_repgrad.hip: {len(seen)} kernel instances found (expected 18)")
    for key, row in seen.items():
        if key[3] == "masked":
            twin = seen.get(key[:3] + (False,))
            if twin is None or row["lds_bytes"] != twin["lds_bytes"]:
                problems.append(f"{row['kernel']}: no unmasked twin, or another LDS size")
            elif row["vgpr"] > twin["vgpr"]:
                problems.append(f"perf: {row['kernel']}: {row['vgpr']} VGPRs, its unmasked twin {twin['vgpr']}")
            varlen_twin = seen.get(key[:3] + (True,))
            if varlen_twin is None or row["vgpr"] > varlen_twin["vgpr"]:
                problems.append(f"{row['kernel']}: {row['vgpr']} VGPRs, its VARLEN twin {varlen_twin and varlen_twin['vgpr']}")
        elif key[3] and (key[:3] + (False,) not in seen or row["lds_bytes"] != seen[key[:3] + (False,)]["lds_bytes"]):
            problems.append(f"{row['kernel']}: no twin without VARLEN, or another LDS size")
    return report, problems


if __name__ == "__main__":
    rep, prob = audit()
    rep2, prob2 = audit_others()
    rep3, prob3 = audit_attn64()
    rep4, prob4 = audit_dkv64()
    rep5, prob5 = audit_gen()
    rep6, prob6 = audit_repgrad()
    rep5, prob5 = rep5 + rep6, prob5 + prob6
    for r in rep + rep2 + rep3 + rep4 + rep5:
        print(r)
    #  the build fails on the CORRECTNESS criteria only -- what hipcc does to the accumulator file around the generated statements, the
    # register-file split, statement and result-read counts; scratch and register counts are performance criteria sitting close to today's
    # compiler output: reported as warnings ("perf:"), with headroom
    allp = prob + prob2 + prob3 + prob4 + prob5
    hard = [x for x in allp if not x.startswith("perf:")]
    print("warnings:", [x for x in allp if x.startswith("perf:")] or "none")
    print("problems:", hard or "none")
    sys.exit(1 if hard else 0)

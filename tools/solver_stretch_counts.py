"""Static instruction counts of the solver stretch of a wave-kernel instance's .s file (tools/asm_variant.sh): what lies
between the two s_setprio that bracket wave 0's phase 2 in the kernel body, plus -- listed apart -- the out-of-line
functions it can call.  Copies (v_mov), selects (v_cndmask) and branches are bookkeeping, not arithmetic:
    python tools/solver_stretch_counts.py /tmp/asm/w8_2_occ4.s
The stretch holds the straight-line full-order solver AND the inlined generic one (a launch runs one of them).  With a
second listing -- the same instance built with -DFLACENC_SOLVER_FULL_ORDER=0, which holds the generic one alone -- the
difference, i.e. the straight-line path by itself, is printed as well:
    python tools/solver_stretch_counts.py default.s generic_only.s"""
import collections
import re
import sys


def classify(op):
    if op in ("v_mov_b64", "v_mov_b32", "v_accvgpr_write_b32", "v_accvgpr_read_b32", "v_accvgpr_mov_b32"):
        return "copy:" + op
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith(("s_swappc", "s_setpc")):
        return "call"
    if op.startswith("scratch_"):
        return "scratch"
    return None


def count(lines):
    c = collections.Counter()
    for l in lines:
        m = re.match(r"\s+([a-z_0-9]+)", l)
        if not m or l.lstrip().startswith((".", ";")):
            continue
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1))
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        k = classify(op)
        if k:
            c[k] += 1
        if op in ("v_max_f64", "v_div_scale_f64", "v_div_fmas_f64", "v_div_fixup_f64", "v_fma_f64", "v_mul_f64", "v_add_f64"):
            c["op:" + op] += 1
    return c


def show(tag, c):
    copies = sum(v for k, v in c.items() if k.startswith("copy:"))
    print("%-44s VALU %5d  copies %4d (%s)  selects %3d  branches %3d  calls %2d  scratch %3d" % (
        tag, c["valu"], copies, ", ".join("%s %d" % (k[5:], v) for k, v in sorted(c.items()) if k.startswith("copy:")),
        c["select"], c["branch"], c["call"], c["scratch"]))
    print("%-44s %s" % ("", "  ".join("%s %d" % (k[3:], v) for k, v in sorted(c.items()) if k.startswith("op:"))))


def report(path):
    lines = open(path).read().split("\n")
    start = [i for i, l in enumerate(lines) if re.match(r"_ZN\S*qlpc_wave4096_kernel\S*:", l)][0]
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    prio = [i for i in range(start, end) if re.match(r"\s+s_setprio\s", lines[i])]
    assert len(prio) >= 2, "no s_setprio pair in the kernel body"
    print(path)
    stretch = count(lines[prio[0]:prio[-1]])
    show("kernel: between the s_setprio (%d lines)" % (prio[-1] - prio[0]), stretch)
    # the device functions emitted out of line in the same unit
    for i, l in enumerate(lines):
        m = re.match(r"(_ZN\S*(levinson_phase\S*|quant_certified\S*)):", l)
        if m and "qlpc_wave4096_kernel" not in m.group(1):
            j = next(k for k in range(i + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
            show("out of line: %s" % re.sub(r"^_ZN\d+flacenc_hip\d+_GLOBAL__N_1\d+", "", m.group(1))[:30], count(lines[i:j]))
    text = "\n".join(lines[end:])
    m = {k: re.search(r"\.%s:\s+(\d+)" % k, text) for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count")}
    print("kernel resources: " + "  ".join("%s %s" % (k, v.group(1)) for k, v in m.items() if v))
    return stretch


first = report(sys.argv[1])
if len(sys.argv) > 2:
    second = report(sys.argv[2])
    delta = collections.Counter({k: first[k] - second[k] for k in set(first) | set(second)})
    show("first - second: the straight-line path alone", delta)

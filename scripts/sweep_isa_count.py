"""VALU instructions of the marching loops of a sweep kernel, role by role, from the assembly of a sweep unit
(hipcc ... --cuda-device-only -S with ramses_amd/build.py's flags of that unit):
scripts/sweep_isa_count.py FILE.s [KERNEL-SUBSTRING]
A marching loop is an innermost backward branch whose body holds the plane's barrier; the roles come out in code order
with their instruction counts (the full rows' loop is the longest), quarter-rate v_rcp/rsq_f64 apart, the scalar side beside
them (SALU by kind, branches, s_waitcnt), plus the kernel's registers, scratch and static LDS.
A loop is counted from its header to the instruction before its closing backward branch: that branch is one more (the full
rows' loop of the fast minmod kernel, 605 instructions with it, prints as 604)."""
import re
import sys


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "godunov_sweep_kernelILi1ELi0ELi12ELb0ELi0ELi5ELb0E"
    lines = open(path).read().splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and want in l and l.split(":")[0].endswith("E"))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith("\t.section") or lines[i].strip().startswith(".amdhsa_kernel"))
    body = lines[start:end]
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", l) or re.match(r"^\s+s_branch\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            if any("s_barrier" in s for s in body[labels[m.group(1)]:i]):
                loops.append((labels[m.group(1)], i))
    # the marching loops themselves: those that hold no other loop with a barrier (the box and chunk loops around them do)
    loops = [body[a:b] for a, b in loops if not any((a2, b2) != (a, b) and a <= a2 and b2 <= b for a2, b2 in loops)]
    print("%s: %d marching loops" % (want, len(loops)))
    for seg in loops:
        ins = [s.split()[0] for s in seg if s.startswith("\t") and not s.strip().startswith((".", ";"))]
        valu = [x for x in ins if x.startswith("v_")]
        kinds = {}
        for x in valu:
            k = ("rcp/rsq_f64" if x in ("v_rcp_f64_e32", "v_rsq_f64_e32") else "max/min_f64" if x.startswith(("v_max_f64", "v_min_f64"))
                 else "dpp" if "dpp" in x else "mov" if x.startswith("v_mov") or x.startswith("v_accvgpr") else "cndmask/cmp" if x.startswith(("v_cndmask", "v_cmp"))
                 else "f64" if "f64" in x else "other")
            kinds[k] = kinds.get(k, 0) + 1
        # scalar side: branches, waits and the barrier apart, the rest is SALU (s_mov, s_add, s_cmp, s_cselect, s_mul, ...)
        # (s_nop, s_setprio, s_sleep and the like compute nothing either: not SALU)
        branch = [x for x in ins if x.startswith(("s_cbranch", "s_branch"))]
        waits = [x for x in ins if x.startswith("s_waitcnt")]
        salu = [x for x in ins if x.startswith("s_") and not x.startswith(
            ("s_cbranch", "s_branch", "s_waitcnt", "s_barrier", "s_nop", "s_setprio", "s_sleep", "s_endpgm"))]
        skinds = {}
        for x in salu:
            k = x.split("_")[1]
            skinds[k] = skinds.get(k, 0) + 1
        print("  loop of %4d instructions: VALU %4d  %s  ds %d  buffer %d  barriers %d" % (
            len(ins), len(valu), " ".join("%s %d" % kv for kv in sorted(kinds.items())),
            sum(1 for x in ins if x.startswith("ds_")), sum(1 for x in ins if x.startswith("buffer_")),
            sum(1 for x in ins if x == "s_barrier")))
        print("       SALU %3d (%s)  branches %d  s_waitcnt %d" % (
            len(salu), " ".join("%s %d" % kv for kv in sorted(skinds.items())), len(branch), len(waits)))
    meta = "\n".join(lines)
    m = re.search(r"\.amdhsa_kernel [^\n]*" + re.escape(want) + r".*?\.end_amdhsa_kernel", meta, re.S)
    if m:
        for key in ("next_free_vgpr", "next_free_sgpr", "accum_offset", "private_segment_fixed_size", "group_segment_fixed_size"):
            mm = re.search(r"\.amdhsa_%s (\d+)" % key, m.group(0))
            if mm:
                print("  %s %s" % (key, mm.group(1)))


if __name__ == "__main__":
    main()

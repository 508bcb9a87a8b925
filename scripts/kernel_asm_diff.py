"""Compare the device assembly of two builds of one unit, function by function:  python scripts/kernel_asm_diff.py OLD.s NEW.s [label]
(hipcc --offload-arch=gfx950 ... --cuda-device-only -S, without --offload-compress).  Function bodies are compared with local
labels normalised and comments stripped, kernel descriptors (.amdhsa_kernel ... .end_amdhsa_kernel: registers, LDS, scratch,
kernarg size) field by field.  Prints one line: functions old / new, common, code differs, descriptor differs, new only, old only.
With --f64 as the last argument one more line follows for every function whose code differs, and for every function that kept its
name but not its parameter list: the instructions of parent and branch, the descriptor fields that differ, and whether the two
bodies hold the same f64 instructions the same number of times (the arithmetic did not change, only the indexing around it)."""
import collections
import re
import subprocess
import sys


def parse(path):
    funcs, descs = {}, {}
    name, body, dname, dbody = None, [], None, []
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        m = re.match(r"^(_Z\w+|\w+):\s*$", line)
        if m and not line.startswith(".L") and name is None and re.match(r"^_Z", m.group(1)):
            name, body = m.group(1), []
            continue
        # (the descriptor of a kernel stands before its .Lfunc_end or after it, by compiler version: never part of the body)
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            dname, dbody = m.group(1), []
            continue
        if dname is not None:
            if ".end_amdhsa_kernel" in line:
                descs[dname] = dbody
                dname = None
            elif line.strip():
                dbody.append(line.strip())
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                funcs[name] = body
                name = None
            elif line.strip():
                body.append(re.sub(r"\.L(BB|tmp|func_begin|func_end|post_getpc)?\d+(_\d+)?", ".L", line.strip()))
    return funcs, descs


def short(n):
    m = re.match(r"_ZN\d+ramses_amd\d+\w+?mode(\d+)", n)
    if m:
        rest = n[m.end():]
        return rest[:int(m.group(1))]
    return n[:40]


def instructions(body):
    return [l.split()[0] for l in body if not l.endswith(":") and not l.startswith(".")]


def base_names(names):
    """mangled name -> demangled name without its parameter list (template arguments kept)"""
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):
        out = list(names)
    return {n: re.sub(r"^void |\(anonymous namespace\)::|\(.*$", "", d) for n, d in zip(names, out)}


def f64_report(old_f, old_d, new_f, new_d, code, desc):
    ob, nb = base_names(sorted(old_f)), base_names(sorted(new_f))
    pairs = [(n, n) for n in code]
    for n in sorted(set(new_f) - set(old_f)):            # the same kernel with another parameter list
        pairs += [(o, n) for o in sorted(set(old_f) - set(new_f)) if ob[o] == nb[n]]
    for o, n in pairs:
        io, inn = instructions(old_f[o]), instructions(new_f[n])
        ho, hn = (collections.Counter(m for m in i if "_f64" in m) for i in (io, inn))
        fields = [a.replace(".amdhsa_", "") + " -> " + b.split()[-1] for a, b in zip(old_d.get(o, []), new_d.get(n, [])) if a != b]
        print("  %-44s instructions %5d -> %5d  f64 %4d in %2d mnemonics: %s  descriptor: %s" % (
            nb[n], len(io), len(inn), sum(hn.values()), len(hn), "same" if ho == hn else "DIFFER %s" % dict((hn - ho) + (ho - hn)),
            ", ".join(fields) or "same"))
    for n in desc:
        if n not in code:                                  # (an extern "C" kernel: its body is not among the _Z functions)
            print("  %-44s descriptor: %s" % (n, ", ".join(a.replace(".amdhsa_", "") + " -> " + b.split()[-1] for a, b in zip(old_d[n], new_d[n]) if a != b)))


if __name__ == "__main__":
    f64 = sys.argv[-1] == "--f64"
    if f64:
        sys.argv.pop()
    old_f, old_d = parse(sys.argv[1])
    new_f, new_d = parse(sys.argv[2])
    label = sys.argv[3] if len(sys.argv) > 3 else sys.argv[2]
    common = sorted(set(old_f) & set(new_f))
    code = [n for n in common if old_f[n] != new_f[n]]
    desc = [n for n in sorted(set(old_d) & set(new_d)) if old_d[n] != new_d[n]]
    new_only = sorted(set(new_f) - set(old_f))
    old_only = sorted(set(old_f) - set(new_f))
    print("%-26s %4d / %4d  common %4d  code differs %d %s  descriptor differs %d %s  new only %d %s  parent only %d %s" % (
        label, len(old_f), len(new_f), len(common), len(code), sorted({short(n) for n in code}), len(desc), sorted({short(n) for n in desc}),
        len(new_only), sorted({short(n) for n in new_only}), len(old_only), sorted({short(n) for n in old_only})))
    if f64:
        f64_report(old_f, old_d, new_f, new_d, code, desc)
    sys.exit(1 if code or desc or old_only else 0)

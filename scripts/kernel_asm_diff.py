"""Compare the device assembly of two builds of one unit, function by function:  python scripts/kernel_asm_diff.py OLD.s NEW.s [label]
(hipcc --offload-arch=gfx950 ... --cuda-device-only -S, without --offload-compress).  Function bodies are compared with local
labels normalised and comments stripped, kernel descriptors (.amdhsa_kernel ... .end_amdhsa_kernel: registers, LDS, scratch,
kernarg size) field by field.  Prints one line: functions old / new, common, code differs, descriptor differs, new only, old only."""
import re
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
        if name is not None:
            if line.startswith(".Lfunc_end"):
                funcs[name] = body
                name = None
            elif line.strip():
                body.append(re.sub(r"\.L(BB|tmp|func_begin|func_end|post_getpc)?\d+(_\d+)?", ".L", line.strip()))
            continue
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
    return funcs, descs


def short(n):
    m = re.match(r"_ZN\d+ramses_amd\d+\w+?mode(\d+)", n)
    if m:
        rest = n[m.end():]
        return rest[:int(m.group(1))]
    return n[:40]


if __name__ == "__main__":
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
    sys.exit(1 if code or desc or old_only else 0)

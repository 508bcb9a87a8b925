#!/usr/bin/env python3
"""Which data-dependent branches of the product's MHD headers does a test input reach?  (host code only; no GPU, no reference)

tests/native/mhd_host_check.cpp -- ramses_amd/csrc/mhd_core.hpp and mhd_assemble.hpp compiled for the host -- is built with
`g++ -O0 --coverage` into a temporary directory, a child process drives it over batches of 6^3 stencils for every pair of 1-D and
2-D solver and every slope type of tests/test_mhd_core_host.py, plus that test's gravity case (ctoprim_cell's `if (g)`), and
`gcov -b` says which branches were never taken.  Printed: every never-taken branch of the two headers, with its function and its
source line.

    python scripts/mhd_branch_coverage.py --state tests    # the stencils of tests/test_mhd_core_host.py ("smooth" and "jump")
    python scripts/mhd_branch_coverage.py --state harsh    # the 6^3 stencils around the octs of tests/helpers.py harsh_mhd_brick
    python scripts/mhd_branch_coverage.py --state both     # one after the other (profiles/mhd_harsh_state_branches.txt)

The harsh input runs with the density floor at 1e-10 and at 0.6, the tests' stencils with 1e-10 as in the test.  A template is
counted over all its instances: a branch is open when no instance took it.  -O0 keeps every `if` of the slopes, the trace and the
solvers as a branch of its own; fmax / fmin are builtins without one, so "this max(., smallr) never binds" is not visible here.

tests/test_mhd_harsh_state_branches.py imports never_taken() and the allow-list below."""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]
# the cases are the host test's own: its solver pairs, slope types, gravity cases, seeds, steps and its harsh brick
from test_mhd_core_host import (GRAVITY, HARSH_DT, HARSH_DX, HARSH_SEED as SEED, HARSH_SHAPE as SHAPE, PAIRS, SLOPES, TESTS_DT,  # noqa: E402
                                TESTS_DX, case_seed, gravity_case, slope_pair, stencils)

NVEC = 32                           # stencils per batch of the tests' kind
SOURCE = os.path.join(ROOT, "tests", "native", "mhd_host_check.cpp")
HEADERS = ("mhd_core.hpp", "mhd_assemble.hpp")

# the functions whose branches an input has to reach: slopes, trace, the 1-D and 2-D solvers
PHYSICS = ("ctoprim_cell", "slope", "trace_predict", "trace_state", "trace3d_cell", "trace_inputs", "efield", "find_mhd_flux",
           "find_speed_fast", "find_speed_info", "find_speed_alfven", "lax_friedrich", "upwind", "hll", "hlld", "roe_eigenvalues",
           "roe_eigen_cons", "athena_roe", "hydro_acoustic", "cmpflxm_face", "cmp_mag_flx_edge")

# never-taken branches that no input of the host driver can reach, matched by the text of their source line
ALLOWED = (
    (r"return st == 0 \|\| st == 1|slope_mag_type_supported\(st\) \|\| st == 3|return r >= RIEMANN",
     "a *_supported argument check: the driver passes supported values only"),
    (r"\(cfsq - cssq\) == 0\.0",
     "needs sqrt(q*^4 - 4 a^2 vax^2) == 0 exactly: no transverse field AND a Roe-averaged sound speed equal to the Alfven speed "
     "to the last bit, an exact coincidence of two independent roundings"),
    (r"RS >= 0 \? RS|RS != -2|R2 >= 0 \? R2|R2 != -2|S3 && st == 3",
     "tests a template argument: the host driver instantiates the run-time switch only (RS = R2 = -1, S3 = true)"),
    (r"\bdefault:", "llf and upwind share the default label of the switch; no other value passes riemann_supported"),
)


def allowed(text):
    for pat, why in ALLOWED:
        if re.search(pat, text):
            return why
    return None


def child(libpath, state, part=0, nparts=1):
    """runs in a process of its own: the counters are written (merged into the .gcda files) when it exits; child `part` of
    `nparts` takes every nparts-th case"""
    import ctypes as C
    import numpy as np
    from helpers import harsh_mhd_brick, oct_stencils
    host = C.CDLL(libpath)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    dbl = C.c_double
    gamma, smallc, theta = 5.0 / 3.0, 1e-10, 1.5

    ncase = [0]

    def run(uin, dx, dt, smallr, st, sm, r1, r2, grav=None):
        ncase[0] += 1
        if ncase[0] % nparts != part:
            return
        if callable(uin):
            uin = uin()
        nv = uin.shape[-1]
        flux = np.full((3, 8, 3, 3, 3, nv), np.nan)
        emf = [np.full((3, 3, 3, nv), np.nan) for _ in range(3)]
        host.mhd_host_set_gravin(vp(grav) if grav is not None else None)
        rc = host.mhd_host_unsplit(vp(uin), nv, nv, dbl(dx), dbl(dt), dbl(gamma), dbl(smallr), dbl(smallc), st, sm, dbl(theta), r1, r2,
                                   vp(flux), vp(emf[0]), vp(emf[1]), vp(emf[2]))
        host.mhd_host_set_gravin(None)
        assert rc == 0

    if part == 0:      # cmpdt_cell (no data-dependent branch; its loops are executed)
        host.mhd_host_cmpdt.restype = C.c_double
        host.mhd_host_cmpdt.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
        cells = np.ascontiguousarray(harsh_mhd_brick(*SHAPE, seed=SEED, gamma=gamma).reshape(11, -1)[:, :NVEC])
        assert np.isfinite(host.mhd_host_cmpdt(vp(cells), NVEC, NVEC, 1.0 / 32, 0.8, gamma, 0.6, smallc))
    if state == "harsh":
        uin = oct_stencils(harsh_mhd_brick(*SHAPE, seed=SEED, gamma=gamma))
        grav = np.ascontiguousarray(np.random.default_rng(7).normal(0.0, 2.0, (3,) + uin.shape[1:]))
        for smallr in (1e-10, 0.6):
            for r1, r2 in PAIRS:
                for st, sm in map(slope_pair, SLOPES):
                    run(uin, HARSH_DX, HARSH_DT, smallr, st, sm, r1, r2)
            for r1, r2, st in GRAVITY:
                run(uin, HARSH_DX, HARSH_DT, smallr, st, st, r1, r2, grav)
    else:
        dx, dt = TESTS_DX, TESTS_DT
        for kind in ("smooth", "jump"):
            for r1, r2 in PAIRS:
                for slope in SLOPES:
                    st, sm = slope_pair(slope)
                    run(lambda: stencils(NVEC, case_seed(slope, r1, r2), kind), dx, dt, 1e-10, st, sm, r1, r2)
        for r1, r2, st in GRAVITY:
            uin, grav = gravity_case(NVEC, r1)
            run(uin, dx, dt, 1e-10, st, st, r1, r2, grav)


def base_name(demangled):
    """ramses_amd::mhd::trace_state<1, 0, TracePred>(...) -> trace_state"""
    head = demangled.split("(")[0]
    head = re.sub(r"<.*", "", head)
    return head.split("::")[-1].split(" ")[-1]


def never_taken(state, keep=None):
    """compile, run (child process), gcov: {header: [(function, line, text, 'never taken' | 'never executed', reason it is allowed
    or None)]}, one entry per source line and kind"""
    work = tempfile.mkdtemp(prefix="mhd_cov_")
    try:
        lib = os.path.join(work, "libmhd_host_cov.so")
        subprocess.check_call(["g++", "-O0", "--coverage", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", lib, SOURCE],
                              cwd=work)
        nparts = max(1, min(8, len(os.sched_getaffinity(0))))
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", lib, "--state", state, "--part", "%d/%d" % (n, nparts)], cwd=work)
                 for n in range(nparts)]
        assert [p.wait() for p in procs] == [0] * nparts
        gcda = [f for f in os.listdir(work) if f.endswith(".gcda")]
        assert gcda, "the child left no counters"
        out = subprocess.check_output(["gcov", "-b", "-m", "--json-format", "--stdout"] + gcda, cwd=work, stderr=subprocess.DEVNULL)
        data = json.loads(out)
        result = {}
        for f in data["files"]:
            name = os.path.basename(f["file"])
            if name not in HEADERS:
                continue
            with open(os.path.join(ROOT, "ramses_amd", "csrc", name)) as fh:
                src = fh.read().split("\n")
            # a template's instances come as separate line records: add up branch by branch
            names = {fn["name"]: fn["demangled_name"] for fn in f["functions"]}
            counts, executed = {}, {}
            for ln in f["lines"]:
                br = [b for b in ln.get("branches", []) if not b.get("throw")]
                if not br:
                    continue
                key = (base_name(names.get(ln.get("function_name"), "?")), ln["line_number"])
                c = counts.setdefault(key, [0] * len(br))
                if len(c) != len(br):                       # instances of unlike shape: keep them apart
                    key = key + (ln.get("function_name"),)
                    c = counts.setdefault(key, [0] * len(br))
                for n, b in enumerate(br):
                    c[n] += b["count"]
                executed[key] = executed.get(key, 0) + ln["count"]
            rows = []
            for key in sorted(counts, key=lambda k: k[1]):
                func, lineno = key[0], key[1]
                nopen = sum(1 for c in counts[key] if c == 0)
                if not nopen:
                    continue
                text = src[lineno - 1].strip()
                what = "never taken" if executed[key] else "never executed"
                rows.append((func, lineno, text, what, allowed(text)))
            result[name] = rows
        return result
    finally:
        if keep:
            shutil.copytree(work, keep, dirs_exist_ok=True)
        shutil.rmtree(work, ignore_errors=True)


def report(state, out):
    res = never_taken(state)
    what = ("the stencils of tests/test_mhd_core_host.py (smooth, jump), floor 1e-10" if state == "tests" else
            "6^3 stencils around the octs of harsh_mhd_brick(%d, %d, %d, seed=%d), floors 1e-10 and 0.6" % (SHAPE + (SEED,)))
    print("== %s input: %s; %d solver pairs x %d slope types + %d gravity cases ==" % (state, what, len(PAIRS), len(SLOPES), len(GRAVITY)), file=out)
    nopen = 0
    for name, rows in res.items():
        for func, ln, text, kind, why in rows:
            nopen += why is None
            print("%-17s %-18s %4d  %-14s %-9s %s" % (name, func, ln, kind, "allowed" if why else "OPEN", text), file=out)
    physics = sum(1 for rows in res.values() for r in rows if r[4] is None and r[0] in PHYSICS)
    print("-- %s: %d never-taken branches outside the allow-list, %d of them in the slope / trace / solver functions" % (state, nopen, physics), file=out)
    return physics


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--state", choices=("tests", "harsh", "both"), default="both")
    ap.add_argument("--child", metavar="LIB", help=argparse.SUPPRESS)
    ap.add_argument("--part", default="0/1", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.state, *map(int, a.part.split("/")))
        return 0
    if shutil.which("gcov") is None or shutil.which("g++") is None:
        sys.exit("g++ and gcov are needed")
    for state in (("tests", "harsh") if a.state == "both" else (a.state,)):
        report(state, sys.stdout)
    if a.state == "both":
        print("-- allowed: " + "; ".join("%s -- %s" % (pat, why) for pat, why in ALLOWED))
    return 0


if __name__ == "__main__":
    sys.exit(main())

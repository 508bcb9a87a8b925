#!/usr/bin/env python3
"""Which data-dependent branches of the C oracle does a test state reach?  (host code only; no GPU)

The oracle's sources (oracle/hydro_oracle.c, hydro_oracle_plmde.c, amr_oracle.c, amr_godfine_oracle.c) are compiled with
`gcc -O0 --coverage` into a temporary directory (oracle/Makefile and oracle/liboracle.so are not touched), a child process runs
godunov_fine of an AMR level on them -- a level-L box with level L+1 in the tile tests' spherical shell, the five Riemann
solvers, slope types 0/1/2/3/7/8, both schemes, the density floor at 1e-10 and at 0.6, NVAR 5 and 7, pressure_fix and difmag
on -- and `gcov -b` says which branches were never taken.  Printed: every never-taken branch of hydro_oracle.c,
hydro_oracle_plmde.c and of ora_interpol_hydro (amr_oracle.c), with its function and its source line.

    python scripts/oracle_branch_coverage.py --state mild     # the state of the tile tests (subsonic, above every floor)
    python scripts/oracle_branch_coverage.py --state harsh    # tests/helpers.py harsh_tree_state
    python scripts/oracle_branch_coverage.py --state both     # one after the other (profiles/harsh_state_branches.txt)

-O0 keeps dmax/dmin as functions of their own: gcov counts their two outcomes over all callers, so "this max(., smallr) never
binds" is not visible per call site; what is visible is every `if` of the slopes, the trace and the solvers.

tests/test_harsh_state_branches.py imports never_taken() and the allow-list below."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 12
SOURCES = ("hydro_oracle.c", "hydro_oracle_plmde.c", "amr_oracle.c", "amr_godfine_oracle.c")
REPORTED = {"hydro_oracle.c": None, "hydro_oracle_plmde.c": None, "amr_oracle.c": ("ora_interpol_hydro",)}     # None: every function

# the functions whose branches a state has to reach: slopes, trace, Riemann solvers, cmpdivu / consup (and their small helpers)
PHYSICS = ("slope_mm", "slope_minmod3", "slope_vanleer", "slope_theta", "ora_uslope", "ora_trace", "ora_trace_plmde",
           "riemann_llf", "riemann_hll", "riemann_hllc", "riemann_acoustic", "riemann_approx", "gdnv_to_flux", "ora_riemann",
           "ora_cmpdivu", "ora_consup", "dmax", "dmin", "dmax_", "imin", "imax", "fsign")

# never-taken branches that no 3-D state can reach, matched by the text of their source line
ALLOWED = (
    (r"\bndim\b", "tests the number of dimensions (3 in every AMR sweep)"),
    (r"\bnt > [01]\b", "tests nt = ndim - 1, the number of transverse dimensions"),
    (r"niter_riemann", "the bound of the Newton loop (the iteration converges before it)"),
    (r"abort\(\)|default:|switch \(p->riemann\)", "the abort() of an unknown solver or slope type"),
    (r"else if \(st == 8\)", "its else leads to the 1-D slope types 4-6 and their abort()"),
)
# ... and the bodies of the 1-D slope types 4-6 (superbee, ultrabee, unstable): from the first line to the abort() after them
SPAN_1D_SLOPES = (r"ndim == 1 && st == 4", r"unknown slope type")


def allowed(text, what, count):
    """the reason a line's never-taken branches are allowed, or None.  A test of the kind the pattern names has ONE outcome that
    cannot occur, so a line may have as many never-taken branches as it has such tests and no more (`if (st == 3 && ndim >= 2)`
    with st == 3 never true would have two); branches that were never executed (the rest of a short-circuit behind such a test,
    code of another dimension) go with the line."""
    for pat, why in ALLOWED:
        n = len(re.findall(pat, text))
        if n and (what == "never executed" or count <= n):
            return why
    return None


# riemann, slope_type, scheme, smallr, nvar, difmag, pressure_fix, gravity, (interpol_var, interpol_type)
CASES = [
    ("llf", 1, "muscl", 1e-10, 5, 0.0, False, False, (0, 1)),
    ("llf", 3, "muscl", 0.6, 7, 0.0, True, True, (1, 2)),
    ("hllc", 2, "muscl", 1e-10, 7, 0.0, False, True, (2, 4)),
    ("hllc", 1, "muscl", 0.6, 5, 0.1, True, False, (0, 3)),
    ("hll", 7, "muscl", 0.6, 5, 0.0, False, False, (1, 0)),
    ("hll", 8, "muscl", 1e-10, 7, 0.05, False, True, (0, 1)),
    ("acoustic", 8, "muscl", 0.6, 5, 0.0, True, False, (1, 2)),
    ("acoustic", 3, "muscl", 1e-10, 5, 0.0, False, False, (0, 1)),
    ("exact", 1, "muscl", 0.6, 7, 0.0, False, True, (2, 4)),
    ("exact", 2, "muscl", 1e-10, 5, 0.1, True, False, (0, 3)),
    ("llf", 0, "muscl", 1e-10, 5, 0.0, False, False, (0, 1)),
    ("llf", 1, "plmde", 0.6, 7, 0.0, False, False, (1, 0)),
    ("hllc", 2, "plmde", 1e-10, 5, 0.0, True, True, (0, 1)),
    ("exact", 7, "plmde", 0.6, 5, 0.1, False, False, (1, 2)),
]


def child(libpath, state, level):
    """runs in a process of its own: the counters are written when it exits"""
    import numpy as np
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    from helpers import harsh_tree_state, mild_tree_state, shell_mask
    from oracle import pyoracle
    from ramses_amd import ic
    L = level
    T = ic.uniform_tree(L, order="scrambled", refine_mask=shell_mask(2 ** L), slack=7)
    lists = {L: T["igrid"], L + 1: T["igrid_fine"]}
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([lists[L], lists[L + 1]]).astype(np.int64) - 1 for ind in range(8)])
    grav = np.random.default_rng(5).normal(size=(3, T["ncell"]))
    for riemann, slope, scheme, smallr, nvar, difmag, pfix, withgrav, interp in CASES:
        uold = harsh_tree_state(T, L, SEED, nvar=nvar) if state == "harsh" else mild_tree_state(T, SEED, nvar)
        p = pyoracle.make_params(riemann=riemann, slope_type=slope, scheme=scheme, smallr=smallr, nvar=nvar, difmag=difmag)
        unew = uold.copy()
        divu, enew = (np.zeros(T["ncell"]), np.zeros(T["ncell"])) if pfix else (None, None)
        f = grav if withgrav else None
        for lev in (L + 1, L):
            dx = 1.0 / 2 ** lev
            pyoracle.godunov_fine_amr(p, lists[lev], T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew, dx, 0.02 * dx, 32,
                                      interp[0], interp[1], f=f, divu=divu, enew=enew, library=libpath)
        assert np.isfinite(unew[:, cells]).all(), (state, riemann, slope, scheme, smallr)


def parse_gcov(path, functions):
    """[(function, line number, source text, 'never taken' | 'never executed', how many such branches the line has)] of one
    .gcov file written by gcov -b: one entry per source line and kind (a line's short-circuit tests come as several branches)"""
    func, lineno, text = None, 0, ""
    seen = {}
    with open(path, errors="replace") as fh:
        for raw in fh:
            m = re.match(r"function (\S+) called", raw)
            if m:
                func = m.group(1)
                continue
            m = re.match(r"\s*([0-9#=\-*]+)\*?:\s*(\d+):(.*)$", raw)
            if m:
                lineno, text = int(m.group(2)), m.group(3).strip()
                continue
            m = re.match(r"branch\s+(\d+) (never executed|taken 0\b)", raw)
            if m and (functions is None or func in functions):
                what = "never executed" if m.group(2) == "never executed" else "never taken"
                key = (func, lineno, text, what)
                seen[key] = seen.get(key, 0) + 1
    return [key + (n,) for key, n in seen.items()]


def never_taken(state, level=4, keep=None):
    """compile, run (child process), gcov: {source file: [(function, line, text, what, reason it is allowed or None)]}"""
    work = tempfile.mkdtemp(prefix="oracle_cov_")
    try:
        for name in SOURCES + ("hydro_oracle.h",):
            shutil.copy(os.path.join(ROOT, "oracle", name), work)
        lib = os.path.join(work, "liboracle_cov.so")
        subprocess.check_call(["gcc", "-O0", "--coverage", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", lib]
                              + list(SOURCES) + ["-lm"], cwd=work)
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", lib, "--state", state, "--level", str(level)], cwd=work)
        gcda = [f for f in os.listdir(work) if f.endswith(".gcda")]
        subprocess.check_call(["gcov", "-b"] + gcda, cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        result = {}
        for name, functions in REPORTED.items():
            rows = parse_gcov(os.path.join(work, name + ".gcov"), functions)
            full = []
            span = None
            if name == "hydro_oracle.c":
                with open(os.path.join(work, name)) as fh:
                    src = fh.read().split("\n")
                first = next(i + 1 for i, s in enumerate(src) if re.search(SPAN_1D_SLOPES[0], s))
                last = next(i + 1 for i, s in enumerate(src) if re.search(SPAN_1D_SLOPES[1], s))
                span = (first, last + 1)
            for func, ln, text, what, count in rows:
                why = allowed(text, what, count)
                if why is None and span and span[0] <= ln <= span[1]:
                    why = "the 1-D slope types 4-6"
                full.append((func, ln, text, what, why))
            result[name] = full
        return result
    finally:
        if keep:
            shutil.copytree(work, keep, dirs_exist_ok=True)
        shutil.rmtree(work, ignore_errors=True)


def report(state, level, out):
    res = never_taken(state, level)
    print("== %s state, level %d + shell of level %d, %d solver/slope/scheme/floor cases ==" % (state, level, level + 1, len(CASES)), file=out)
    nopen = 0
    for name, rows in res.items():
        for func, ln, text, what, why in rows:
            nopen += why is None
            print("%-22s %-18s %4d  %-14s %-9s %s" % (name, func, ln, what, "allowed" if why else "OPEN", text), file=out)
    physics = sum(1 for rows in res.values() for r in rows if r[4] is None and r[0] in PHYSICS)
    print("-- %s: %d never-taken branches outside the allow-list, %d of them in the slope / trace / Riemann / cmpdivu / consup functions" %
          (state, nopen, physics), file=out)
    return physics


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--state", choices=("mild", "harsh", "both"), default="both")
    ap.add_argument("--level", type=int, default=4)
    ap.add_argument("--child", metavar="LIB", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.state, a.level)
        return 0
    if shutil.which("gcov") is None or shutil.which("gcc") is None:
        sys.exit("gcc and gcov are needed")
    for state in (("mild", "harsh") if a.state == "both" else (a.state,)):
        report(state, a.level, sys.stdout)
    return 0


if __name__ == "__main__":
    sys.exit(main())

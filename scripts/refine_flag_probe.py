#!/usr/bin/env python
"""The refinement-criteria kernels of a resident level, for a kernel trace:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python scripts/refine_flag_probe.py [L] [REPEATS] [ONLY]

Level L (default 7: 128^3 cells) complete, a mild random state with NVAR=7; each entry point is called REPEATS times on the
level: ramses_amd_amrres_hydro_flag (three gradients), ramses_amd_amrres_refine_flag with the same gradients, with the Jeans
criterion alone (no neighbour gathers), with everything at once, and ramses_amd_amrres_mass_map with ivar_refine 0 and 6.
hydro_flag and refine_flag run the same kernel, lvl_refine_kernel<true>: ONLY (a prefix of the names below, e.g. hydro_flag)
keeps a trace to the dispatches of one entry.
Prints the number of cells each flags and the wall time per call (launch, count and list back to the host included)."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ramses_amd  # noqa: E402
from ramses_amd import ic  # noqa: E402
from ramses_amd._capi import check, make_refine_crit  # noqa: E402
from helpers import mild_tree_state  # noqa: E402


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    rep = int(sys.argv[2]) if len(sys.argv) > 2 else 10
    only = sys.argv[3] if len(sys.argv) > 3 else ""
    lib = ramses_amd.lib()
    T = ic.uniform_tree(L, order="morton")
    u = mild_tree_state(T, 3, nvar=7)
    p = ramses_amd.make_params(nvar=7)
    check(lib.ramses_amd_amrres_invalidate())
    check(lib.ramses_amd_amrres_load(7, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
    ig = np.ascontiguousarray(T["igrid"]).astype(np.int32)
    cells = np.zeros(8 * len(ig), np.int32)
    n = C.c_int(0)
    rho = np.ascontiguousarray(u[0])
    grad = dict(err_grad_d=0.25, err_grad_p=0.25, err_grad_u=0.4)
    jeans = dict(n_jeans=4.0, tail_pix=0.5 / 2 ** L, factG=1.0)
    jeans["n_jeans"] = 1.45 / jeans["tail_pix"]      # lambda = sqrt(T pi / rho) with T, rho in [1, 2): about half of the cells

    def flag(**kw):
        crit = make_refine_crit(**kw)
        return lambda: lib.ramses_amd_amrres_refine_flag(C.byref(p), len(ig), vp(ig), C.byref(crit), vp(cells), C.byref(n))

    runs = [
        ("hydro_flag  (lvl_refine_kernel<true>, three gradients, the others off)",
         lambda: lib.ramses_amd_amrres_hydro_flag(C.byref(p), len(ig), vp(ig), 0.25, 0.25, 0.4, 1e-10, 1e-10, 1e-10, vp(cells), C.byref(n))),
        ("refine_flag (lvl_refine_kernel<true>, the same gradients)", flag(**grad)),
        ("refine_flag (lvl_refine_kernel<false>, Jeans alone)", flag(**jeans)),
        ("refine_flag (lvl_refine_kernel<true>, gradients + Jeans + density threshold)", flag(thr_mode=1, thr=1.5, **grad, **jeans)),
        ("mass_map    (lvl_mass_map_kernel<false>, host rho sent)",
         lambda: lib.ramses_amd_amrres_mass_map(C.byref(p), len(ig), vp(ig), 0.37, 4.0, 0, 0.5, vp(rho), vp(cells), C.byref(n))),
        ("mass_map    (lvl_mass_map_kernel<true>, ivar_refine=6, device rho)",
         lambda: lib.ramses_amd_amrres_mass_map(C.byref(p), len(ig), vp(ig), 0.37, 4.0, 6, 0.5, None, vp(cells), C.byref(n))),
    ]
    print("level %d: %d octs, %d cells, %d calls each" % (L, len(ig), 8 * len(ig), rep))
    for name, call in runs:
        if not name.startswith(only):
            continue
        check(call())
        t0 = time.perf_counter()
        for _ in range(rep):
            check(call())
        dt = (time.perf_counter() - t0) / rep
        print("%-80s %9d cells flagged  %8.3f ms per call (host wall, list included)" % (name, n.value, dt * 1e3))
    lib.ramses_amd_amrres_invalidate()


if __name__ == "__main__":
    main()

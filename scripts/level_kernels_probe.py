#!/usr/bin/env python
"""Every service kernel of a resident AMR level (csrc/capi_amr.hip lvl_*), for a kernel trace:

    rocprofv3 --kernel-trace --stats -f csv -d DIR -o t -- python scripts/level_kernels_probe.py [L] [REPEATS]

The tree of the level-kernel tests (tests/helpers.level_case: level L complete, default 6 = 64^3 cells in tiles, level L+1 in a
shell), harsh state with NVAR=7, an acceleration, pressure_fix on.  REPEATS times on both levels: set_unew_pfix, set_uold_pfix
(gravity source, pdv, set_uold, energy switch), set_unew, set_uold_grav, synchro, upload_fine, courant.  The refinement kernels
are scripts/refine_flag_probe.py's.  Prints the wall time of one round."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ramses_amd  # noqa: E402
from ramses_amd._capi import check  # noqa: E402
from helpers import level_case  # noqa: E402


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 else 6
    rep = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    os.environ.setdefault("RAMSES_AMD_TILE_MIN_OCTS", "0")
    lib = ramses_amd.lib()
    T, u, f = level_case(L, "morton")
    u = u.copy()
    p = ramses_amd.make_params(nvar=7, smallr=1e-10, courant_factor=0.8)
    check(lib.ramses_amd_amrres_invalidate())
    check(lib.ramses_amd_amrres_load(7, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
    lists = [(lev, T["lists"][lev]["sorted"]) for lev in (L, L + 1)]
    for _, ig in lists:
        check(lib.ramses_amd_amrres_load_f(len(ig), vp(ig), vp(f)))
    check(lib.ramses_amd_amrres_enable_pfix())
    out4 = np.zeros(4)

    def one_round():
        for lev, ig in lists:
            n, dx = len(ig), 0.5 ** lev
            check(lib.ramses_amd_amrres_set_unew_pfix(C.byref(p), n, vp(ig)))
            check(lib.ramses_amd_amrres_set_uold_pfix(C.byref(p), n, vp(ig), 1e-6, dx, 0.5, 0.0))
            check(lib.ramses_amd_amrres_set_unew(n, vp(ig)))
            check(lib.ramses_amd_amrres_set_uold_grav(C.byref(p), n, vp(ig), 1e-6))
            check(lib.ramses_amd_amrres_synchro(C.byref(p), n, vp(ig), 1e-6))
            check(lib.ramses_amd_amrres_upload_fine(C.byref(p), n, vp(ig), 1))
            check(lib.ramses_amd_amrres_courant(C.byref(p), n, vp(ig), dx, 1.0, vp(out4)))

    one_round()
    t0 = time.perf_counter()
    for _ in range(rep):
        one_round()
    dt = (time.perf_counter() - t0) / rep
    print("levels %d and %d: %d + %d octs, %d rounds, %.3f ms per round (host wall; courant_fine synchronises)" % (
        L, L + 1, len(lists[0][1]), len(lists[1][1]), rep, dt * 1e3))
    lib.ramses_amd_amrres_invalidate()


if __name__ == "__main__":
    main()

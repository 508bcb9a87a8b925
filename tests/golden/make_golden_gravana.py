#!/usr/bin/env python
"""Golden vectors of the analytic acceleration (gravity_type = 2; reference run HERE, vectors committed).

Runs the UNMODIFIED reference program with poisson=.true. and a point mass and stores, per case, a seeded sample of at most
3000 leaf cells of the last snapshot: level, centre x (user units), the three components of the grav_* file.

    oracle/build_ref.sh ramses 3 serial                        # -> oracle/_ref/ramses3d
    python tests/golden/make_golden_gravana.py                 # -> tests/golden/gravana_ref.npz

Cases (tests/test_gravana_checker.py holds the numpy restatement of poisson/gravana.f90 to them, bit for bit):
  point0     levels 3-5, sub-cycled, periodic, boxlen = 3, softening 0 (the mass sits on no cell centre)
  pointwall  levels 3-5, sub-cycled, two reflexive z walls (nz = 3, kcoarse_min = 1), boxlen = 3, softening 0.02
  uniform    one level of 16^3 cells, periodic, boxlen = 3
A cell that make_grid_fine created in the last regrid holds the value at its FATHER cell's centre (amr/refine_utils.f90:918-927)
until the next force_fine of its level: the checker accepts either, and counts.
"""
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ramses_snapshot as rs  # noqa: E402

NSAMPLE = 3000
NSTEP = 4
REFINE = """&REFINE_PARAMS
interpol_var=0
interpol_type=1
err_grad_p=0.1
/
"""
ZWALLS = """&BOUNDARY_PARAMS
nboundary=2
ibound_min= 0, 0
ibound_max= 0, 0
jbound_min= 0, 0
jbound_max= 0, 0
kbound_min=-1,+1
kbound_max=-1,+1
bound_type= 1, 1
/
"""
# tag -> (gravity_params, boxlen, levelmin, levelmax, walls)
CASES = {
    "point0": ((3.0, 0.0, 0.21, 0.13, 0.37), 3.0, 3, 5, False),
    "pointwall": ((3.0, 0.02, 0.2, 0.3, 0.1), 3.0, 3, 5, True),
    "uniform": ((3.0, 0.02, 0.2, 0.3, 0.1), 3.0, 4, 4, False),
}


def gravity_block(gtype, params):
    return "&POISSON_PARAMS\ngravity_type=%d\ngravity_params=%s\n/\n" % (gtype, ",".join(repr(float(p)) for p in params))


def namelist(tag, nstep=NSTEP):
    params, boxlen, lmin, lmax, walls = CASES[tag]
    extra = REFINE + (ZWALLS if walls else "") + gravity_block(2, params)
    nml = rs.sedov3d_namelist(level=lmin, nstepmax=nstep, foutput=nstep, riemann="hll", slope_type=1, boxlen=boxlen, extra=extra,
                              mem_factor=1.0, poisson=True)
    nml = nml.replace("levelmax=%d" % lmin, "levelmax=%d" % lmax)
    if lmax > lmin:
        nml = nml.replace("nsubcycle=10*1", "nsubcycle=1,1,2,2")
    return nml.replace("ngridtot=", "ngridtot=20000 !")


def main():
    out = {}
    for k, tag in enumerate(CASES):
        work, _ = rs.run_reference(namelist(tag))
        try:
            snap = rs.load_leaf_cells(os.path.join(work, "output_00002"), with_grav=True)
        finally:
            shutil.rmtree(work, ignore_errors=True)
        grav = np.asarray(snap["grav"])
        f = grav[-3:]                     # (backup_poisson writes the potential first, then the three components)
        n = snap["level"].size
        pick = np.sort(np.random.default_rng(1000 + k).choice(n, min(n, NSAMPLE), replace=False))
        out[tag + "_level"] = snap["level"][pick].astype(np.int8)
        out[tag + "_x"] = np.ascontiguousarray(snap["x"][pick].T)
        out[tag + "_f"] = np.ascontiguousarray(f[:, pick])
        out[tag + "_params"] = np.array(CASES[tag][0])
        out[tag + "_boxlen"] = np.array(CASES[tag][1])
        out[tag + "_walls"] = np.array(int(CASES[tag][4]))
        print("%s: %d leaf cells, levels %s, %d kept" % (tag, n, sorted(set(int(l) for l in snap["level"])), pick.size))
    dst = os.path.join(ROOT, "tests", "golden", "gravana_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()

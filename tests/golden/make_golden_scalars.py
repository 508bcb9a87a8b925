#!/usr/bin/env python
"""Golden vectors of passive scalars beyond NVAR=7 on a uniform level.

Builds the UNMODIFIED reference program with -DNENER=0 -DNVAR=10|16, -DNENER=1 -DNVAR=9 and -DNENER=2 -DNVAR=8,
wrapped by oracle/dump_patch, from a temporary copy of oracle/build_ref.sh exactly as make_golden_nener.py does (its
build / read_dump / oct_positions / to_brick are reused; oracle/ and oracle/_ref/ are never written).  Each case runs
a 16^3 periodic level (levelmin = levelmax = 4) for 5 coarse steps and keeps, per godunov_fine call k of the first
KEEP = 3, the level's conserved state as dense bricks [nvar, z, y, x]:

    uold[k]   uold on entry of call k
    unew[k]   unew after call k (the sweep of uold[k])
    dt[k]     dtnew of the level on call k (courant_fine of uold[k])

so that uold[k] -> unew[k] pins the sweep and unew[k] -> uold[k+1] pins set_uold: its near-floor scalar fix, and with
NENER the pdV term.  Every scalar has its own value in each of three regions (the background and two off-centre boxes; a
point blast off-centre); in the cases marked `floor` the box's density is below smallr, so the fix fires.

    python tests/golden/make_golden_scalars.py      # -> tests/golden/scalars_ref.npz
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_nener as mgn  # noqa: E402
from make_golden_nener import rs  # noqa: E402

LEVEL = 4
NSTEP = 5
KEEP = 3      # calls kept: uold of the first KEEP, unew of the first KEEP-1 (the later states of the NVAR=16 runs do not
              # compress: all five kept come to 2.6 MB, three to 0.42 MB)
# (tag, nener, nvar, riemann, slope_type, floor)
CASES = [
    ("v10_llf_s1", 0, 10, "llf", 1, True),
    ("v10_exact_s7", 0, 10, "exact", 7, False),
    ("v10_acoustic_s8", 0, 10, "acoustic", 8, True),
    ("v16_hllc_s2", 0, 16, "hllc", 2, True),
    ("v16_hll_s0", 0, 16, "hll", 0, False),
    ("e1v9_hllc_s3", 1, 9, "hllc", 3, False),
    ("e2v8_hll_s1", 2, 8, "hll", 1, False),
]
RIEMANN = {"llf": 0, "hllc": 1, "hll": 2, "acoustic": 3, "exact": 4}

# (region_condinit, hydro/init_flow_fine.f90:530-600: a 'point' region sets the passive scalars of EVERY cell to its
#  var_region, so it comes right after the background and the two off-centre boxes give the scalars their shape)
INIT = """nregion=4
region_type(1)='square'
region_type(2)='point'
region_type(3)='square'
region_type(4)='square'
x_center=0.5,0.31,0.30,0.72
y_center=0.5,0.62,0.65,0.28
z_center=0.5,0.44,0.40,0.60
length_x=10.0,1.0,0.30,0.25
length_y=10.0,1.0,0.20,0.35
length_z=10.0,1.0,0.25,0.20
exp_region=10.0,10.0,10.0,10.0
d_region=1.0,0.0,{dbox},2.0
u_region=0.3,0.0,0.1,-0.1
v_region=-0.2,0.0,0.05,0.2
w_region=0.1,0.0,-0.15,0.05
p_region=1e-3,0.4,2e-3,3e-3
{prad}{var}"""


def namelist(nener, nvar, riemann, slope, floor):
    prad = "".join("prad_region(1,%d)=%g\nprad_region(2,%d)=%g\nprad_region(3,%d)=%g\nprad_region(4,%d)=%g\n"
                   % (i + 1, 2e-3 * (i + 1), i + 1, 0.2 / (i + 1), i + 1, 1e-3, i + 1, 3e-3) for i in range(nener))
    var = "".join("var_region(1,%d)=%g\nvar_region(2,%d)=%g\nvar_region(3,%d)=%g\nvar_region(4,%d)=%g\n"
                  % (k + 1, 0.0, k + 1, 0.1 + 0.05 * k, k + 1, 0.9 - 0.07 * k, k + 1, 0.3 + 0.11 * (k % 4))
                  for k in range(nvar - 5 - nener))
    init = INIT.format(dbox="1e-11" if floor else "0.5", prad=prad, var=var).rstrip("\n")
    return rs.sedov3d_namelist(level=LEVEL, nstepmax=NSTEP, foutput=1000, riemann=riemann, slope_type=slope,
                               boxlen=1.0, init=init, mem_factor=1.5)


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="scalars_ref_")
    try:
        bins = {}
        for tag, nener, nvar, riemann, slope, floor in CASES:
            if (nener, nvar) not in bins:
                bins[(nener, nvar)] = mgn.build(tmp, nener, nvar)
            os.environ["RAMSES_DUMP_CALLS"] = ",".join(str(k) for k in range(1, NSTEP + 1))
            work, log = rs.run_reference(namelist(nener, nvar, riemann, slope, floor), binary=bins[(nener, nvar)])
            try:
                ds = [mgn.read_dump(work, k) for k in range(1, NSTEP + 1)]
            finally:
                shutil.rmtree(work, ignore_errors=True)
            pos = mgn.oct_positions(ds[0])
            out[tag + "_uold"] = np.stack([mgn.to_brick(d["uold"], d, pos) for d in ds[:KEEP]])
            out[tag + "_unew"] = np.stack([mgn.to_brick(d["unew"], d, pos) for d in ds[:KEEP - 1]])
            out[tag + "_dt"] = np.array([d["dt"] for d in ds[:KEEP]])
            out[tag + "_meta"] = np.array([nener, nvar, slope, RIEMANN[riemann], int(floor)], np.int64)
            out[tag + "_dx"] = np.array(ds[0]["dx"])
            u, un = out[tag + "_uold"], out[tag + "_unew"]
            print(tag, "dt", out[tag + "_dt"], "cells changed by set_uold",
                  [int((u[k + 1] != un[k]).any(0).sum()) for k in range(KEEP - 1)])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(HERE, "scalars_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

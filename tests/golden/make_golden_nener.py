#!/usr/bin/env python
"""Golden vectors of the non-thermal energies (NENER = 1, 2) on a uniform level.

Builds the UNMODIFIED reference program with -DNENER=1|2 -DNVAR=6|7, wrapped by
oracle/dump_patch (used read-only: it dumps uold / unew around every godunov_fine
call), in a temporary directory: oracle/build_ref.sh hard-codes NENER=0, so a
temporary copy of it is driven there with the define changed; oracle/ and
oracle/_ref/ are never written.  Each case runs a 16^3 periodic level
(levelmin = levelmax = 4) for 5 coarse steps and keeps, per godunov_fine call k,
the level's conserved state as dense bricks [nvar, z, y, x]:

    uold[k]   uold on entry of call k
    unew[k]   unew after call k (the sweep of uold[k])
    dt[k]     dtnew of the level on call k (courant_fine of uold[k])

so that uold[k] -> unew[k] pins the sweep and unew[k] -> uold[k+1] pins set_uold
with the pdV term of the non-thermal energies (add_pdv_source_terms).

    python tests/golden/make_golden_nener.py      # -> tests/golden/nener_ref.npz
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ramses_snapshot as rs  # noqa: E402

LEVEL = 4
NSTEP = 5
# (tag, nener, nvar, riemann, slope_type, gamma_rad or None)
CASES = [
    ("e1_llf_s1", 1, 6, "llf", 1, None),
    ("e1_hllc_s2", 1, 6, "hllc", 2, None),
    ("e1_hll_s7", 1, 6, "hll", 7, None),
    ("e1_hllc_s8", 1, 6, "hllc", 8, None),
    ("e1_llf_s3", 1, 6, "llf", 3, None),
    ("e1_llf_s0", 1, 6, "llf", 0, None),
    ("e2_hllc_s1", 2, 7, "hllc", 1, (1.4, 1.6)),
    ("e1v7_llf_s1", 1, 7, "llf", 1, None),
]

# Uniform background with a bulk velocity that differs along x, y and z, an off-centre point blast;
# non-thermal pressure in both.  Nothing is symmetric under a permutation of the axes.
INIT = """nregion=2
region_type(1)='square'
region_type(2)='point'
x_center=0.5,0.31
y_center=0.5,0.62
z_center=0.5,0.44
length_x=10.0,1.0
length_y=10.0,1.0
length_z=10.0,1.0
exp_region=10.0,10.0
d_region=1.0,0.0
u_region=0.3,0.0
v_region=-0.2,0.0
w_region=0.1,0.0
p_region=1e-3,0.4
{prad}{var}"""


def namelist(nener, nvar, riemann, slope, gamma_rad):
    prad = "".join("prad_region(1,%d)=%g\nprad_region(2,%d)=%g\n" % (i + 1, 2e-3 * (i + 1), i + 1, 0.2 / (i + 1))
                   for i in range(nener))
    var = ""
    if nvar > 5 + nener:
        var = "var_region(1,1)=0.25\nvar_region(2,1)=0.0\n"
    init = INIT.format(prad=prad, var=var).rstrip("\n")
    nml = rs.sedov3d_namelist(level=LEVEL, nstepmax=NSTEP, foutput=1000, riemann=riemann, slope_type=slope,
                              boxlen=1.0, init=init, mem_factor=1.5)
    if gamma_rad is not None:
        nml = nml.replace("riemann='%s'" % riemann,
                          "riemann='%s'\ngamma_rad=%s" % (riemann, ",".join("%r" % g for g in gamma_rad)))
    return nml


def build(tmp, nener, nvar):
    """The reference program with -DNENER=nener -DNVAR=nvar and the dump patch -> path of the binary."""
    orc = os.path.join(tmp, "oracle")
    if not os.path.isdir(orc):
        shutil.copytree(os.path.join(ROOT, "oracle"), orc, ignore=shutil.ignore_patterns("_ref", "__pycache__"))
        script = os.path.join(orc, "build_ref.sh")
        with open(script) as fh:
            text = fh.read()
        old = "-DNENER=0 -DNVAR=$nvar -DSOLVERhydro"
        assert old in text
        with open(script, "w") as fh:
            fh.write(text.replace(old, "-DNENER=${REF_NENER:-0} -DNVAR=$nvar -DSOLVERhydro"))
    tag = "e%dv%d" % (nener, nvar)
    env = dict(os.environ, REF_NENER=str(nener), REF_NVAR=str(nvar), REF_TAG=tag)
    subprocess.run(["bash", os.path.join(orc, "build_ref.sh"), "ramses", "3", "serial",
                    os.path.join(ROOT, "oracle", "dump_patch")], env=env, check=True)
    return os.path.join(orc, "_ref", "ramses3d_dump_patch_" + tag)


def read_dump(work, k):
    with open(os.path.join(work, "godunov_%04d_in.bin" % k), "rb") as fh:
        hdr = [int(x) for x in np.fromfile(fh, np.int32, 11)]
        ilevel, ngrid, ngridmax, ncoarse, nvar = hdr[:5]
        assert hdr[9] == 0 and hdr[10] == 0          # no gravity, no pressure_fix
        dx, dt = np.fromfile(fh, np.float64, 5)[:2]
        igrid = np.fromfile(fh, np.int32, ngrid)
        ncell = ncoarse + 8 * ngridmax
        son = np.fromfile(fh, np.int32, ncell)
        nbor = np.fromfile(fh, np.int32, ngridmax * 6).reshape(6, ngridmax)
        np.fromfile(fh, np.int32, ngridmax)                                   # father
        uold = np.fromfile(fh, np.float64, ncell * nvar).reshape(nvar, ncell)
        np.fromfile(fh, np.float64, ncell * nvar)                             # unew on entry (= uold)
        assert fh.read() == b""
    with open(os.path.join(work, "godunov_%04d_out.bin" % k), "rb") as fh:
        unew = np.fromfile(fh, np.float64, ncell * nvar).reshape(nvar, ncell)
        assert fh.read() == b""
    return dict(ilevel=ilevel, ngridmax=ngridmax, ncoarse=ncoarse, dx=dx, dt=dt, igrid=igrid, son=son, nbor=nbor,
                uold=uold, unew=unew)


def oct_positions(d):
    """Oct coordinates of the level's octs from the neighbour links (nbor(igrid, face) = the father cell of the
    neighbouring oct, son(cell) = that oct): positions relative to the first oct, wrapped periodically."""
    n = 2 ** (d["ilevel"] - 1)
    son, nbor = d["son"], d["nbor"]
    pos = {int(d["igrid"][0]): (0, 0, 0)}
    todo = [int(d["igrid"][0])]
    while todo:
        ig = todo.pop()
        p = pos[ig]
        for f in range(6):
            q = int(son[nbor[f, ig - 1] - 1])
            if q > 0 and q not in pos:
                s = list(p)
                s[f // 2] = (s[f // 2] + (1 if f % 2 else -1)) % n
                pos[q] = tuple(s)
                todo.append(q)
    assert len(pos) == len(d["igrid"]) == n ** 3
    return pos


def to_brick(u, d, pos):
    n = 2 ** d["ilevel"]
    out = np.full((u.shape[0], n, n, n), np.nan)
    for ig, (ox, oy, oz) in pos.items():
        for ind in range(8):
            cell = d["ncoarse"] + ind * d["ngridmax"] + ig - 1
            out[:, 2 * oz + (ind >> 2), 2 * oy + ((ind >> 1) & 1), 2 * ox + (ind & 1)] = u[:, cell]
    assert not np.isnan(out).any()
    return out


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="nener_ref_")
    try:
        bins = {}
        for tag, nener, nvar, riemann, slope, grad in CASES:
            if (nener, nvar) not in bins:
                bins[(nener, nvar)] = build(tmp, nener, nvar)
            os.environ["RAMSES_DUMP_CALLS"] = ",".join(str(k) for k in range(1, NSTEP + 1))
            work, log = rs.run_reference(namelist(nener, nvar, riemann, slope, grad), binary=bins[(nener, nvar)])
            try:
                ds = [read_dump(work, k) for k in range(1, NSTEP + 1)]
            finally:
                shutil.rmtree(work, ignore_errors=True)
            pos = oct_positions(ds[0])
            out[tag + "_uold"] = np.stack([to_brick(d["uold"], d, pos) for d in ds])
            out[tag + "_unew"] = np.stack([to_brick(d["unew"], d, pos) for d in ds])
            out[tag + "_dt"] = np.array([d["dt"] for d in ds])
            out[tag + "_meta"] = np.array([nener, nvar, slope, {"llf": 0, "hllc": 1, "hll": 2}[riemann]], np.int64)
            out[tag + "_gamma_rad"] = np.array(grad if grad else (1.33333333334, 1.33333333334))
            out[tag + "_dx"] = np.array(ds[0]["dx"])
            print(tag, "dt", out[tag + "_dt"], "cells changed by pdV",
                  [int((out[tag + "_uold"][k + 1] != out[tag + "_unew"][k]).any(0).sum()) for k in range(NSTEP - 1)])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "nener_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

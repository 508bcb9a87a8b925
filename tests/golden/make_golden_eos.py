#!/usr/bin/env python
"""Golden vectors of cooling_fine in a barotropic run without cooling (reference run HERE, vectors committed).

Builds the UNMODIFIED reference program wrapped by tests/golden/eos_dump_patch (which only dumps uold and son of the active
octs' cells around its cooling_fine), runs it on three namelists and stores two calls of each:

    python tests/golden/make_golden_eos.py                     # -> tests/golden/eos_ref.npz

Cases, all 16^3 coarse cells (levelmin = 4), boxlen = 1, smallr = 0.3, &UNITS_PARAMS with a scale_nH that is no power of two:
  iso_uniform   one level; barotropic_eos_form = 'isothermal'
  iso_amr       levels 4-5 (gradient criteria); 'isothermal'; a cube of density 0.1 < smallr; one call of the partially refined
                level 4 (its split cells must come back unchanged), one of level 5
  legacy        levels 4-5; isothermal=.true., g_star = 1, T2_star = 4.8: the old idiom ('legacy' is the default form)
Per call <tag><k>_: meta (ilevel, ngrid, nvar), par (gamma, smallr, scale_nH, scale_T2, T2_eos, T2_star, g_star, jeans_ncells),
uin / uout [nvar][8*ngrid] and sin / sout [8*ngrid] (uold and son of the cells of the active octs before and after the call).
tests/test_eos_checker.py holds tests/eos_checker.py and the library's host evaluation to them, bit for bit.
"""
import os
import shutil
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ramses_snapshot as rs  # noqa: E402

DUMP_PATCH = os.path.join(ROOT, "tests", "golden", "eos_dump_patch")
BINARY = os.path.join(ROOT, "oracle", "_ref", "ramses3d_eos_dump_patch")

# a background of density 1 drifting across the box, a cube of density 20, a cube of density 0.1 (below smallr = 0.3)
INIT = """nregion=3
region_type(1)='square'
region_type(2)='square'
region_type(3)='square'
x_center=0.5,0.3,0.7
y_center=0.5,0.4,0.7
z_center=0.5,0.45,0.6
length_x=10.0,0.2,0.26
length_y=10.0,0.2,0.26
length_z=10.0,0.2,0.26
exp_region=10.0,10.0,10.0
d_region=1.0,20.0,0.1
u_region=0.3,0.0,0.1
v_region=-0.2,0.1,0.0
w_region=0.1,0.0,-0.3
p_region=0.04,0.8,0.004"""
# scale_v = 1e5 cm/s, scale_T2 = mH/kB scale_v^2 = 120.2 K: T2c = 4.8 K is a sound speed squared of 0.04 in code units
UNITS = """&UNITS_PARAMS
units_density=1.3d-21
units_time=3.1d13
units_length=3.1d18
/
"""
ISOTHERMAL = """&COOLING_PARAMS
barotropic_eos=.true.
barotropic_eos_form='isothermal'
T_eos=4.8
mu_gas=1.0
/
"""
LEGACY = """&COOLING_PARAMS
isothermal=.true.
/
&SF_PARAMS
T2_star=4.8
g_star=1.0
n_star=0.1
/
"""
GRADIENTS = """&REFINE_PARAMS
interpol_var=0
interpol_type=1
err_grad_d=0.2
/
"""
SMALLR = "0.3"


def eos_block(form):
    """&COOLING_PARAMS (and &SF_PARAMS) of a form: 'isothermal', 'legacy', or any other barotropic_eos_form by name"""
    if form == "isothermal":
        return ISOTHERMAL
    if form == "legacy":
        return LEGACY
    return ISOTHERMAL.replace("'isothermal'", "'%s'\npolytrope_rho=2.6d-20\npolytrope_index=1.4" % form)


def namelist(form, lmin, lmax, nstep, refine=GRADIENTS, poisson=False, ngridtot=12000, nsubcycle="1,1,2,2", riemann="hllc", slope=1):
    extra = (refine if lmax > lmin else "") + UNITS + eos_block(form)
    if poisson:
        extra += "&POISSON_PARAMS\nepsilon=1e-5\n/\n"
    nml = rs.sedov3d_namelist(level=lmin, nstepmax=nstep, foutput=nstep, riemann=riemann, slope_type=slope, boxlen=1.0, extra=extra,
                              init=INIT, mem_factor=1.0, poisson=poisson)
    for old, new in (("levelmax=%d" % lmin, "levelmax=%d" % lmax), ("gamma=1.4", "gamma=1.4\nsmallr=" + SMALLR),
                     ("ngridtot=", "ngridtot=%d !" % ngridtot)):
        assert old in nml
        nml = nml.replace(old, new)
    if lmax > lmin:
        nml = nml.replace("nsubcycle=10*1", "nsubcycle=" + nsubcycle)
    return nml


# tag -> (form, levelmin, levelmax, steps)
CASES = {
    "iso_uniform": ("isothermal", 4, 4, 3),
    "iso_amr": ("isothermal", 4, 5, 3),
    "legacy": ("legacy", 4, 5, 3),
}


def read_dump(work, call):
    rec = {}
    for what in ("in", "out"):
        raw = open(os.path.join(work, "cooling_%04d_%s.bin" % (call, what)), "rb").read()
        ilevel, ngrid, nvar = np.frombuffer(raw, np.int32, 3)
        par = np.frombuffer(raw, np.float64, 8, 12)
        n = 8 * int(ngrid)
        u = np.frombuffer(raw, np.float64, nvar * n, 12 + 64).reshape(nvar, n)
        son = np.frombuffer(raw, np.int32, n, 12 + 64 + 8 * nvar * n)
        assert len(raw) == 12 + 64 + 8 * nvar * n + 4 * n
        rec["meta"], rec["par"] = np.array([ilevel, ngrid, nvar]), par.copy()
        rec["u" + what], rec["s" + what] = u.copy(), son.copy()
    return rec


def main():
    subprocess.check_call([os.path.join(ROOT, "oracle", "build_ref.sh"), "ramses", "3", "serial", DUMP_PATCH])
    out = {}
    ncall = 12
    for tag, (form, lmin, lmax, nstep) in CASES.items():
        os.environ["RAMSES_DUMP_CALLS"] = ",".join(str(c) for c in range(1, ncall + 1))
        work, log = rs.run_reference(namelist(form, lmin, lmax, nstep), binary=BINARY)
        try:
            calls = [c for c in range(1, ncall + 1) if os.path.exists(os.path.join(work, "cooling_%04d_out.bin" % c))]
            recs = {c: read_dump(work, c) for c in calls}
        finally:
            shutil.rmtree(work, ignore_errors=True)
        if lmax == lmin:
            keep = [calls[0], calls[-1]]
        else:
            # the last call of the partially refined coarse level (split cells among its leaves) and the last of the fine level
            coarse = [c for c in calls if recs[c]["meta"][0] == lmin and (recs[c]["sin"] > 0).any() and (recs[c]["sin"] == 0).any()]
            fine = [c for c in calls if recs[c]["meta"][0] == lmax]
            keep = [coarse[-1], fine[-1]]
        for k, c in enumerate(keep):
            r = recs[c]
            leaf = r["sin"] == 0
            print("%s call %d: level %d, %d octs, %d leaf cells, %d below smallr, %d energies changed" % (
                tag, c, r["meta"][0], r["meta"][1], leaf.sum(), (r["uin"][0] < r["par"][1]).sum(), (r["uin"][4] != r["uout"][4]).sum()))
            for name, v in r.items():
                out["%s%d_%s" % (tag, k, name)] = v
    dst = os.path.join(ROOT, "tests", "golden", "eos_ref.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()

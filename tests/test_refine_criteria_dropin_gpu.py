"""Live GPU test of the Jeans and mass refinement criteria on a resident AMR run: the patched program against the untouched
reference program (oracle/_ref), bit for bit.  The run is tests/golden/make_golden_amr.py selfgrav_namelist() -- hydro +
self-gravity, levels 3-5, a cube of density 20 in a background of density 1, a point explosion in the corner -- without its
gradient criteria and with the pressure p_region=0.1,0.4,0.1 (the Jeans length is 0.56 in the background and 0.028 in the cube;
boxlen 0.5, G = 1), refined instead by
  (a) jeans_refine=4.,4.                         one rank    (jeans_length_refine, hydro/hydro_flag.f90:185-258)
  (b) m_refine=4.,4. with mass_sph=1e-4          one rank    (rho_fine's quasi-Lagrangian map, pm/rho_fine.f90:96-118,201-214)
  (c) m_refine=2.49,0.3113 with mass_sph=1e-4,   one rank    (poisson_refine's density threshold, amr/flag_utils.f90:480-485: the
      no self-gravity                                        host's uold is stale at flag_fine time on a resident run.  The
                                                             threshold is a density of 1.02 on both levels, just above the
                                                             background, so the blast front moves the flags every step)
  (d) (a) and (b) together                       two ranks
  (e) (b) with ivar_refine=6, var_cut_refine=0.5 one rank    the NVAR=7 pair of programs; the scalar is 0.9 in the cube, 0.1 outside
(array entries count from levelmin: the values above belong to levels 3 and 4.)

The mesh of the reference alone at the last output, octs of the level / octs it could hold:
                 level 4          level 5
  (a)         512/512 = 100 %   294/4096 = 7.2 %
  (b), (e)    496/512 = 96.9 %  150/4096 = 3.7 %
  (c)         512/512 = 100 %   587/4096 = 14.3 %  (294 after the initial refinement, 579 after the first step)
  (d)         512/512 = 100 %   294/4096 = 7.2 %
  none         0                 0             (the same namelist without a criterion never leaves level 3)
Level 5 is partial in every case; level 4 cannot stay below 60 % of its 512 octs once level 5 exists: levelmin is 8 cells wide,
and a level-5 patch of 205 octs (5 %) is at least 6 level-4 cells wide, which ensure_ref_rules and the nexpand=1 smoothing of
flag_fine (amr/flag_utils.f90) widen to the whole box at level 3 -- an elongated cube (tried: 0.44 x 0.09 x 0.09) ends the same
way.  So level 4 is complete but built by the criterion, and the coarse-fine boundary the criterion draws lies between levels 4
and 5."""
import os
import shutil

import numpy as np
import pytest

import live

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
RESIDENT = "AMR levels stay resident on the GPU"

JEANS = "jeans_refine=4.,4.\n"
MASS = "m_refine=4.,4.\nmass_sph=1e-4\n"
FRONT = "m_refine=2.49,0.3113\nmass_sph=1e-4\n"
SCALARS = "\nvar_region(1,1)=0.1\nvar_region(1,2)=0.2\nvar_region(3,1)=0.9\nvar_region(3,2)=0.5\n/\n\n&OUTPUT_PARAMS"
CASES = {
    "a": dict(crit=JEANS, nproc=1, gravity=True, shims=("hydro_flag (shim",)),
    "b": dict(crit=MASS, nproc=1, gravity=True, shims=("rho_fine (shim: refinement map",)),
    "c": dict(crit=FRONT, nproc=1, gravity=False, shims=("poisson_refine (shim",)),
    "d": dict(crit=JEANS + MASS, nproc=2, gravity=True, shims=("hydro_flag (shim", "rho_fine (shim: refinement map")),
    "e": dict(crit=MASS + "ivar_refine=6\nvar_cut_refine=0.5\n", nproc=1, gravity=True, v7=True, shims=("rho_fine (shim: refinement map",)),
}


def _namelist(crit, gravity=True, nproc=1, v7=False):
    mka = live.golden_module("amr")
    nml = mka.selfgrav_namelist()
    for old, new in (("err_grad_p=0.1\n", ""), ("err_grad_d=0.2\n", ""), ("p_region=1e-5,0.4,1e-3", "p_region=0.1,0.4,0.1"),
                     ("&REFINE_PARAMS\n", "&REFINE_PARAMS\n" + crit)):
        assert old in nml
        nml = nml.replace(old, new)
    if not gravity:
        nml = nml.replace("poisson=.true.", "")
    if nproc > 1:
        nml = nml.replace("ngridtot=6000 !", "ngridtot=60000 !")
    if v7:
        assert "\n/\n\n&OUTPUT_PARAMS" in nml
        nml = nml.replace("\n/\n\n&OUTPUT_PARAMS", SCALARS)
    return nml


@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_run_with_refinement_criteria_equals_the_reference(gpu_lib, case):
    cfg = CASES[case]
    nproc, gravity = cfg["nproc"], cfg["gravity"]
    tag = "ramses3d" + ("_mpi" if nproc > 1 else "")
    ref, patched = (os.path.join(REF_DIR, tag + s + ("_v7" if cfg.get("v7") else "")) for s in ("", "_patch"))
    if not (os.path.exists(ref) and os.path.exists(patched)):
        pytest.skip("%s / %s not built" % (os.path.basename(ref), os.path.basename(patched)))
    live.enough_cores(nproc)
    nml = _namelist(cfg["crit"], gravity, nproc, cfg.get("v7", False))
    workp, outp = live.run(nml, patched, nproc, {"RAMSES_AMD": "1", "RAMSES_AMD_PROFILE": "1"})
    try:
        assert RESIDENT in outp, outp[-1500:]
        for row in cfg["shims"]:         # the criterion ran on the device: the shim's row in the wall-clock table
            assert row in outp, (row, outp[-3000:])
        sol_p = live.poisson_solves(outp)
        got = live.leaves(workp, with_grav=gravity)
    finally:
        shutil.rmtree(workp, ignore_errors=True)
    workr, outr = live.run(nml, ref, nproc, {})
    try:
        sol_r = live.poisson_solves(outr)
        want = live.leaves(workr, with_grav=gravity)
    finally:
        shutil.rmtree(workr, ignore_errors=True)
    assert {4, 5} <= set(int(l) for l in np.unique(want[0])), np.unique(want[0])      # the criterion built both levels
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (len(got[0]), len(want[0]))
    assert np.array_equal(got[2], want[2]), np.abs(got[2] - want[2]).max()     # hydro state
    if gravity:
        assert len(sol_r) > 0 and sol_p == sol_r
        assert np.array_equal(got.grav, want.grav), np.abs(got.grav - want.grav).max()     # phi, f


def test_the_old_gating_comes_back_with_the_switch(gpu_lib):
    """RAMSES_AMD_RESIDENT_REFINE=0: case (a) takes the staged path again (A/B runs) and still equals the reference"""
    ref, patched = os.path.join(REF_DIR, "ramses3d"), os.path.join(REF_DIR, "ramses3d_patch")
    if not (os.path.exists(ref) and os.path.exists(patched)):
        pytest.skip("ramses3d / ramses3d_patch not built")
    nml = _namelist(JEANS)
    workp, outp = live.run(nml, patched, 1, {"RAMSES_AMD": "1", "RAMSES_AMD_RESIDENT_REFINE": "0"})
    try:
        assert RESIDENT not in outp
        got = live.leaves(workp, with_grav=True)
    finally:
        shutil.rmtree(workp, ignore_errors=True)
    workr, _ = live.run(nml, ref, 1, {})
    try:
        want = live.leaves(workr, with_grav=True)
    finally:
        shutil.rmtree(workr, ignore_errors=True)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)

"""Live runs with analytic gravity (gravity_type 1, 2): the patched program with RAMSES_AMD_GRAVANA=1 against the unmodified
reference program.  With the switch the run keeps its device-resident path -- force_fine writes the resident acceleration from the
resident oct centres (patch/force_fine.f90: ramses_amd_force_fine_ana, csrc/capi_amr.hip: lvl_gravana_kernel; make_boundary_force
on the device between walls) -- and the last snapshot equals the reference's bit for bit: leaf level, x, the primitive variables AND
the three components of f of the grav_* files (cells created in the last regrid hold their father cell's f there).  Without the
switch the run stays staged as before, bit-identical too.

  (a) gravity_type 1, g = (0, 0, -1.7), corner blast between two reflexive z walls, periodic in x and y, levels 4-6, sub-cycled
  (b) gravity_type 2, periodic, levels 4-6, sub-cycled, on 1 and 2 ranks
  (c) one uniform level 5, gravity_type 2 (the brick path)
  (d) (b) without the switch: staged

Every program runs once per case (functools.lru_cache); the assertions on the exit statistics are tests of their own.

No acceleration goes to the device outside the loads of the whole device image: across a regrid the rebuilt levels get their f
device to device (patch/ramses_amd_iface.f90: ramses_amd_amr_stash_f / ramses_amd_amr_restore_f)."""
import functools
import os
import re
import shutil

import numpy as np
import pytest

import live
from test_walls_resident_gpu import CORNER

pytestmark = pytest.mark.gpu

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
NSTEP = 6


def _gravity(gtype, params):
    return "&POISSON_PARAMS\ngravity_type=%d\ngravity_params=%s\n/\n" % (gtype, ",".join(repr(float(p)) for p in params))


def _namelist(case):
    from oracle import ramses_snapshot as rs
    mka = live.golden_module("amr")
    if case == "a":
        extra = mka.REFINE.format(ivar=0, itype=1) + ZWALLS + _gravity(1, (0.0, 0.0, -1.7))
        nml = rs.sedov3d_namelist(level=4, nstepmax=NSTEP, foutput=NSTEP, riemann="hll", slope_type=1, extra=extra, init=CORNER,
                                  mem_factor=1.0, poisson=True)
    elif case == "b":
        extra = mka.REFINE.format(ivar=0, itype=1) + _gravity(2, (3.0, 0.02, 0.2, 0.3, 0.1))
        nml = rs.sedov3d_namelist(level=4, nstepmax=NSTEP, foutput=NSTEP, riemann="hll", slope_type=1, extra=extra, mem_factor=1.0,
                                  poisson=True)
    else:
        extra = _gravity(2, (3.0, 0.02, 0.2, 0.3, 0.1))
        nml = rs.sedov3d_namelist(level=5, nstepmax=NSTEP, foutput=NSTEP, riemann="hll", slope_type=1, extra=extra, poisson=True)
        return nml
    return live.replace_keys(nml, ("levelmax=4", "levelmax=6"), ("nsubcycle=10*1", "nsubcycle=1,1,1,2,2"), ("ngridtot=", "ngridtot=60000 !"))


def _snapshot(work):
    from oracle import ramses_snapshot as rs
    snap = rs.load_leaf_cells(os.path.join(work, "output_00002"), with_grav=True)
    order = np.lexsort((snap["x"][:, 0], snap["x"][:, 1], snap["x"][:, 2], snap["level"]))
    grav = np.asarray(snap["grav"])[-3:]
    return snap["level"][order], snap["x"][order], snap["prim"][:, order], grav[:, order], snap["info"]["t"]


@functools.lru_cache(maxsize=None)
def _pair(case, nproc, switch):
    """(patched program's output text, its snapshot, the reference program's snapshot)"""
    pat_bin, ref_bin = live.binaries(nproc > 1)
    nml = _namelist(case)
    env = {"RAMSES_AMD": "1", "RAMSES_AMD_PROFILE": "1", "RAMSES_AMD_STATS": "1", "RAMSES_AMD_GRAVANA": "1" if switch else "0"}
    workp, outp = live.run(nml, pat_bin, nproc, env)
    try:
        got = _snapshot(workp)
    finally:
        shutil.rmtree(workp, ignore_errors=True)
    workr, _ = live.run(nml, ref_bin, nproc, {})
    try:
        ref = _snapshot(workr)
    finally:
        shutil.rmtree(workr, ignore_errors=True)
    return outp, got, ref


def _same_snapshot(got, ref, min_levels):
    assert got[4] == ref[4]
    assert len(set(int(l) for l in ref[0])) >= min_levels, "the run must have refined"
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2].view(np.int64), ref[2].view(np.int64)), np.abs(got[2] - ref[2]).max()
    bad = (got[3].view(np.int64) != ref[3].view(np.int64)).any(axis=0)
    assert not bad.any(), "%d of %d leaf cells differ in f, max %g" % (bad.sum(), bad.size, np.abs(got[3] - ref[3]).max())
    assert np.abs(ref[3]).max() > 0


CASES = [("a", 1), ("b", 1), ("b", 2), ("c", 1)]
IDS = ["%s-%d" % c for c in CASES]


@pytest.mark.parametrize("case,nproc", CASES, ids=IDS)
def test_run_with_analytic_gravity_stays_resident_and_equals_the_reference(gpu_lib, case, nproc):
    outp, got, ref = _pair(case, nproc, True)
    assert "analytic gravity (gravity_type" in outp and "is evaluated on the GPU" in outp, outp[-3000:]
    if case == "c":
        assert "stays resident on the GPU" in outp, outp[-3000:]
    else:
        assert "AMR levels stay resident on the GPU" in outp, outp[-3000:]
        assert "force_fine (device, analytic)" in outp, outp[-3000:]
    if case == "a":
        assert "make_boundary_hydro (device)" in outp, outp[-3000:]
    _same_snapshot(got, ref, 1 if case == "c" else 3)


@pytest.mark.parametrize("case,nproc", CASES, ids=IDS)
def test_no_acceleration_goes_to_the_device_after_the_initial_load(gpu_lib, case, nproc):
    """RAMSES_AMD_STATS=1: the exit lines split ramses_amd_amrres_f_traffic's host -> device bytes into what went up with a load of
    the WHOLE device image and the rest.  The rest must be 0: force_fine writes f on the device, and across a regrid the rebuilt
    levels get their f device to device (octs that were there park it, new octs take their father cell's).  The image is loaded
    twice per rank in these runs: at the start, and once more after the reference's defrag before the snapshot, which renumbers the
    host's octs and drops the image of any resident run, state and tree included (patch/load_balance.f90).
    Case (c), the one-level brick, never has a resident AMR image: no f line at all may appear."""
    outp = _pair(case, nproc, True)[0]
    if case == "c":
        assert "acceleration f over PCIe" not in outp and "analytic gravity:" not in outp, outp[-3000:]
        return
    lines = re.findall(r"analytic gravity: (\d+) calls of force_fine wrote the resident acceleration on the device; f to the device: "
                       r"(\d+) bytes in (\d+) loads of the whole device image, (\d+) bytes otherwise", outp)
    totals = re.findall(r"acceleration f over PCIe: (\d+) bytes to the device", outp)
    assert len(lines) == nproc and len(totals) == nproc, outp[-3000:]
    for (calls, image, loads, rest), total in zip(lines, totals):
        print("case %s, %d ranks: %s calls, %s bytes in %s image loads, %s bytes otherwise, %s in all" % (case, nproc, calls, image, loads, rest, total))
        assert int(calls) > 0 and int(image) > 0 and int(loads) == 2
        assert int(rest) == 0 and int(total) == int(image)


def test_without_the_switch_the_run_stays_staged_and_equals_the_reference(gpu_lib):
    outp, got, ref = _pair("b", 1, False)
    assert "stay resident on the GPU" not in outp and "is evaluated on the GPU" not in outp, outp[-3000:]
    _same_snapshot(got, ref, 3)

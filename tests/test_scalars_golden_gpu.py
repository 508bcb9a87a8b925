"""Passive scalars beyond NVAR=7 against the reference program itself.

tests/golden/scalars_ref.npz (tests/golden/make_golden_scalars.py) holds, for seven runs of the unmodified reference
built with -DNENER=0 -DNVAR=10|16, -DNENER=1 -DNVAR=9 and -DNENER=2 -DNVAR=8 on a 16^3 periodic level, the conserved
state around every godunov_fine call: uold[k] -> unew[k] is the sweep, unew[k] -> uold[k+1] is set_uold (the near-floor
scalar fix; with NENER the pdV term), dt[k] is courant_fine's dtnew.  The device fuses set_uold's scalar fix into the
sweep, so its unew is compared where both agree: the hydro (and non-thermal) rows with unew[k], the scalar rows with
uold[k+1].  Strict build, bit for bit (the exact solver's pow() to 1e-12, as at NVAR <= 7).
"""
import ctypes as C
import os

import numpy as np
import pytest

from helpers import rel_linf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "scalars_ref.npz"))
CASES = sorted({k[:-len("_meta")] for k in GOLD.files if k.endswith("_meta")})
RIEMANN = {0: "llf", 1: "hllc", 2: "hll", 3: "acoustic", 4: "exact"}
NSTEP = 2      # calls kept in the goldens: uold of 3, unew of 2


def _meta(tag):
    nener, nvar, slope, riemann, floor = (int(x) for x in GOLD[tag + "_meta"])
    return nener, nvar, slope, RIEMANN[riemann], floor


def _params(tag, fast=False):
    from ramses_amd import _capi
    nener, nvar, slope, riemann, _ = _meta(tag)
    # the namelist of make_golden_scalars.py: gamma=1.4, courant_factor=0.8, the reference's other defaults
    return _capi.make_params(nvar=nvar, nener=nener, gamma=1.4, courant_factor=0.8, slope_type=slope, riemann=riemann,
                             fast_math=fast)


def _level(tag):
    from ramses_amd.hydro import HydroLevel
    return HydroLevel(16, 16, 16, float(GOLD[tag + "_dx"]), params=_params(tag))


def _same(tag, a, b):
    if _meta(tag)[3] == "exact":
        return rel_linf(np.asarray(a), np.asarray(b)) <= 1e-12
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def test_the_goldens_exercise_what_they_pin():
    assert len(CASES) == 7
    assert {(_meta(t)[0], _meta(t)[1]) for t in CASES} == {(0, 10), (0, 16), (1, 9), (2, 8)}
    assert {_meta(t)[3] for t in CASES} == set(RIEMANN.values())
    fired = 0
    for tag in CASES:
        nener, nvar, _, _, floor = _meta(tag)
        u, un = GOLD[tag + "_uold"], GOLD[tag + "_unew"]
        # every scalar its own field
        for a in range(5 + nener, nvar):
            for b in range(a + 1, nvar):
                assert not np.array_equal(u[0][a], u[0][b])
        if floor:
            fired += sum(int((u[k + 1][5:] != un[k][5:]).any(0).sum()) for k in range(NSTEP))
    assert fired > 0          # set_uold's near-floor scalar fix acts in the floor cases


@pytest.mark.parametrize("tag", CASES)
def test_courant_dt_equals_the_reference(tag):
    lv = _level(tag)
    for k in range(NSTEP):
        lv.upload(GOLD[tag + "_uold"][k])
        assert lv.courant_fine()[0] == GOLD[tag + "_dt"][k], "call %d" % (k + 1)


@pytest.mark.parametrize("tag", CASES)
def test_sweep_matches_the_reference(tag):
    nh = 5 + _meta(tag)[0]
    lv = _level(tag)
    for k in range(NSTEP):
        lv.upload(GOLD[tag + "_uold"][k])
        lv.godunov_fine(float(GOLD[tag + "_dt"][k]))
        got = lv.download(lv.unew)
        assert _same(tag, got[:nh], GOLD[tag + "_unew"][k][:nh]), "hydro rows of call %d" % (k + 1)
        assert _same(tag, got[nh:], GOLD[tag + "_uold"][k + 1][nh:]), "scalar rows of call %d" % (k + 1)


@pytest.mark.parametrize("tag", CASES)
def test_chained_steps_match_the_reference(tag):
    """courant -> godunov -> set_uold (with the pdV term when NENER > 0), the device's state carried from step to step"""
    lv = _level(tag)
    lv.upload(GOLD[tag + "_uold"][0])
    for k in range(NSTEP):
        dt = lv.courant_fine()[0]
        assert dt == GOLD[tag + "_dt"][k] or _meta(tag)[3] == "exact"
        lv.godunov_fine(float(GOLD[tag + "_dt"][k]))
        lv.set_uold()
        assert _same(tag, lv.download(), GOLD[tag + "_uold"][k + 1]), "after call %d" % (k + 1)


def _cellvec(brick, ngridmax, ncoarse):
    """[nvar, 16, 16, 16] brick -> the reference's uold(1:ncell, 1:nvar), oct ig = 1 + ox + 8 oy + 64 oz."""
    nvar, n = brick.shape[0], brick.shape[1]
    no = n // 2
    u = np.zeros((nvar, ncoarse + 8 * ngridmax))
    for ind in range(8):
        ix, iy, iz = ind & 1, (ind >> 1) & 1, ind >> 2
        u[:, ncoarse + ind * ngridmax: ncoarse + ind * ngridmax + no ** 3] = brick[:, iz::2, iy::2, ix::2].reshape(nvar, -1)
    return np.ascontiguousarray(u)


def _brick(u, n, ngridmax, ncoarse):
    nvar, no = u.shape[0], n // 2
    out = np.zeros((nvar, n, n, n))
    for ind in range(8):
        ix, iy, iz = ind & 1, (ind >> 1) & 1, ind >> 2
        out[:, iz::2, iy::2, ix::2] = u[:, ncoarse + ind * ngridmax: ncoarse + ind * ngridmax + no ** 3].reshape(nvar, no, no, no)
    return out


def _octs(n):
    no = n // 2
    io = np.arange(no ** 3)
    igrid = np.arange(1, no ** 3 + 1, dtype=np.int32)
    xg = np.concatenate([(io % no + 0.5) / no, ((io // no) % no + 0.5) / no, (io // no ** 2 + 0.5) / no])
    return igrid, xg


@pytest.mark.parametrize("tag", ["v16_hllc_s2", "e1v9_hllc_s3"])
def test_resident_f90_entry_points_on_the_cell_layout_match_the_reference(tag):
    """ramses_amd_resident_*_f90 on RAMSES's uold(1:ncell, 1:nvar): the gather / scatter of all NVAR columns"""
    from ramses_amd import _capi
    from ramses_amd._capi import check
    L = _capi.lib()
    p = _params(tag)
    nener = _meta(tag)[0]
    dx = float(GOLD[tag + "_dx"])
    level, n = 4, 16
    igrid, xg = _octs(n)
    ngrid = ngridmax = len(igrid)
    ncoarse = 1
    uold = _cellvec(GOLD[tag + "_uold"][0], ngridmax, ncoarse)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    L.ramses_amd_resident_invalidate()
    try:
        for k in range(NSTEP):
            out4 = np.zeros(4)
            check(L.ramses_amd_resident_courant_f90(C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1,
                                                    vp(uold), dx, 1e30, vp(out4)))
            assert out4[0] == GOLD[tag + "_dt"][k]
            dt = float(out4[0])
            check(L.ramses_amd_resident_godunov_f90(C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1,
                                                    vp(uold), dx, dt))
            if nener:
                check(L.ramses_amd_resident_set_uold_pdv_f90(C.byref(p), level, dx, dt))
            else:
                check(L.ramses_amd_resident_set_uold_f90(level))
            check(L.ramses_amd_resident_sync_host_f90(vp(uold)))
            got = _brick(uold, n, ngridmax, ncoarse)
            assert _same(tag, got, GOLD[tag + "_uold"][k + 1]), "after call %d" % (k + 1)
    finally:
        L.ramses_amd_resident_invalidate()


def test_mpi_resident_entry_points_match_the_reference():
    """ramses_amd_mpires_* at NVAR=10 on one rank: setup, courant, godunov, reverse, set_uold, the halo of all NVAR fields"""
    from ramses_amd import _capi
    from ramses_amd._capi import check
    tag = "v10_llf_s1"
    L = _capi.lib()
    p = _params(tag)
    dx = float(GOLD[tag + "_dx"])
    level, n = 4, 16
    igrid, xg = _octs(n)
    ngrid = ngridmax = len(igrid)
    ncoarse = 1
    uold = _cellvec(GOLD[tag + "_uold"][0], ngridmax, ncoarse)
    unew = uold.copy()
    zero = np.zeros(1, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    check(L.ramses_amd_mpires_setup(C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1, vp(uold), vp(unew),
                                    1, 1, vp(zero), vp(zero), vp(zero), vp(zero)))
    try:
        out4 = np.zeros(4)
        sp, sl, hp, hl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        for k in range(NSTEP):
            check(L.ramses_amd_mpires_courant(C.byref(p), dx, 1e30, vp(out4)))
            assert out4[0] == GOLD[tag + "_dt"][k]
            check(L.ramses_amd_mpires_godunov(C.byref(p), dx, float(out4[0])))
            check(L.ramses_amd_mpires_reverse_unew())
            check(L.ramses_amd_mpires_set_uold())
            check(L.ramses_amd_mpires_halo_stage_out(C.byref(sp), C.byref(sl), C.byref(hp), C.byref(hl)))
            check(L.ramses_amd_mpires_halo_stage_in())
        check(L.ramses_amd_mpires_sync_host(vp(uold)))
        assert _same(tag, _brick(uold, n, ngridmax, ncoarse), GOLD[tag + "_uold"][NSTEP])
    finally:
        L.ramses_amd_mpires_invalidate()

"""Non-thermal energies (NENER = 1, 2) on a uniform level, against the reference program itself.

tests/golden/nener_ref.npz (tests/golden/make_golden_nener.py) holds, for eight runs of the unmodified reference
built with -DNENER=1|2 on a 16^3 periodic level, the conserved state around every godunov_fine call: uold[k] ->
unew[k] is the sweep, unew[k] -> uold[k+1] is set_uold with the pdV term of the non-thermal energies, dt[k] is
courant_fine's dtnew.  Each part is checked on its own, bit for bit in the strict build, so that a failure names
the part that is wrong; then the whole chain, the fast build against the strict one, and the MPI-resident entry
points against HydroLevel.
"""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "nener_ref.npz"))
CASES = sorted({k[:-len("_meta")] for k in GOLD.files if k.endswith("_meta")})
RIEMANN = {0: "llf", 1: "hllc", 2: "hll"}
NSTEP = 4


def _params(tag, fast=False):
    from ramses_amd import _capi
    nener, nvar, slope, riemann = (int(x) for x in GOLD[tag + "_meta"])
    # the namelist of make_golden_nener.py: gamma=1.4, courant_factor=0.8, the reference's other defaults
    return _capi.make_params(nvar=nvar, nener=nener, gamma=1.4, courant_factor=0.8, slope_type=slope,
                             riemann=RIEMANN[riemann], gamma_rad=tuple(GOLD[tag + "_gamma_rad"]), fast_math=fast)


def _level(tag, fast=False):
    from ramses_amd.hydro import HydroLevel
    return HydroLevel(16, 16, 16, float(GOLD[tag + "_dx"]), params=_params(tag, fast))


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _where(a, b):
    d = np.nonzero(np.asarray(a).view(np.int64) != np.asarray(b).view(np.int64))
    return "%d values differ, first at (var,z,y,x)=%s" % (d[0].size, tuple(int(x[0]) for x in d)) if d[0].size else ""


def test_the_goldens_exercise_what_they_pin():
    assert len(CASES) == 8
    for tag in CASES:
        u, un = GOLD[tag + "_uold"], GOLD[tag + "_unew"]
        nener = int(GOLD[tag + "_meta"][0])
        # the pdV term moves the non-thermal energies between the sweep and the next step ...
        assert any((u[k + 1][5:5 + nener] != un[k][5:5 + nener]).any() for k in range(NSTEP))
        # ... and nothing else (no passive-scalar fix, no floor in these runs)
        for k in range(NSTEP):
            rest = [v for v in range(u.shape[1]) if not 5 <= v < 5 + nener]
            assert _bits_equal(u[k + 1][rest], un[k][rest])
        # not symmetric under a permutation of the axes
        assert not np.array_equal(u[2][1], u[2][2].transpose(0, 2, 1))


@pytest.mark.parametrize("tag", CASES)
def test_courant_dt_equals_the_reference(tag):
    lv = _level(tag)
    for k in range(NSTEP + 1):
        lv.upload(GOLD[tag + "_uold"][k])
        dt, mass, etot, eint = lv.courant_fine()
        assert dt == GOLD[tag + "_dt"][k], (k, dt, GOLD[tag + "_dt"][k])
    # eint of courant_fine (courant_fine.f90:105-118): E - kinetic - non-thermal energies
    u = GOLD[tag + "_uold"][NSTEP]
    nener = lv.params.nener
    vol = lv.dx ** 3
    ei = u[4] * vol
    for d in range(3):
        ei = ei - 0.5 * u[1 + d] ** 2 / np.maximum(u[0], 1e-10) * vol
    for n in range(nener):
        ei = ei - u[5 + n] * vol
    assert abs(eint - ei.sum()) <= 1e-12 * abs(ei).sum()


@pytest.mark.parametrize("tag", CASES)
def test_sweep_matches_the_reference_bit_for_bit(tag):
    lv = _level(tag)
    for k in range(NSTEP):
        lv.upload(GOLD[tag + "_uold"][k])
        lv.godunov_fine(float(GOLD[tag + "_dt"][k]))
        got = lv.download(lv.unew)
        assert _bits_equal(got, GOLD[tag + "_unew"][k]), "sweep of call %d: %s" % (k + 1, _where(got, GOLD[tag + "_unew"][k]))


@pytest.mark.parametrize("tag", CASES)
def test_set_uold_pdv_matches_the_reference_bit_for_bit(tag):
    import torch
    lv = _level(tag)
    for k in range(NSTEP):
        lv.upload(GOLD[tag + "_uold"][k])
        lv.unew.copy_(torch.as_tensor(GOLD[tag + "_unew"][k]).to(lv.device))
        lv._dt_swept = float(GOLD[tag + "_dt"][k])
        lv.set_uold()
        got = lv.download()
        assert _bits_equal(got, GOLD[tag + "_uold"][k + 1]), "set_uold after call %d: %s" % (k + 1, _where(got, GOLD[tag + "_uold"][k + 1]))


@pytest.mark.parametrize("tag", ["e1_hllc_s2", "e2_hllc_s1"])
def test_chained_steps_with_ghost_layers(tag):
    """courant -> godunov -> set_uold (pdV) -> make_virtual_fine_dp on a brick with ghost layers (ng = 2)."""
    from ramses_amd.hydro import HydroLevel
    lv = HydroLevel(16, 16, 16, float(GOLD[tag + "_dx"]), params=_params(tag), ng=2)
    lv.upload(GOLD[tag + "_uold"][0])
    lv.make_virtual_fine_dp()
    for k in range(NSTEP):
        dt = lv.courant_fine()[0]
        assert dt == GOLD[tag + "_dt"][k]
        lv.godunov_fine()
        lv.set_uold()
        lv.make_virtual_fine_dp()
        assert _bits_equal(lv.download(), GOLD[tag + "_uold"][k + 1]), "step %d" % (k + 1)


def test_set_uold_with_nener_needs_a_sweep_first():
    from ramses_amd import _capi
    lv = _level("e1_llf_s1")
    with pytest.raises(_capi.RamsesAmdError):
        lv.set_uold()


@pytest.mark.parametrize("tag", ["e2_hllc_s1", "e1_llf_s1", "e1_hll_s7"])
def test_fast_build_stays_within_1e12_of_strict_over_20_steps(tag):
    s, f = _level(tag), _level(tag, fast=True)
    s.upload(GOLD[tag + "_uold"][0])
    f.upload(GOLD[tag + "_uold"][0])
    worst = 0.0
    for _ in range(20):
        dt = s.courant_fine()[0]
        s.godunov_fine(dt)
        f.godunov_fine(dt)
        s.set_uold()
        f.set_uold()
        a, b = s.download(), f.download()
        for v in range(a.shape[0]):
            worst = max(worst, float(np.abs(a[v] - b[v]).max() / np.abs(a[v]).max()))
    assert worst <= 1e-12, worst
    assert worst > 0.0       # the fast kernels did run


# ---- the MPI-resident entry points on one rank ----------------------------------------------------------------


def _cellvec(brick, ngridmax, ncoarse):
    """[nvar, 16, 16, 16] brick -> the reference's uold(1:ncell, 1:nvar), oct ig = 1 + ox + 8 oy + 64 oz."""
    nvar, n = brick.shape[0], brick.shape[1]
    no = n // 2
    ncell = ncoarse + 8 * ngridmax
    u = np.zeros((nvar, ncell))
    for ind in range(8):
        ix, iy, iz = ind & 1, (ind >> 1) & 1, ind >> 2
        cells = brick[:, iz::2, iy::2, ix::2].reshape(nvar, no ** 3)      # [oz, oy, ox] -> ig - 1
        u[:, ncoarse + ind * ngridmax: ncoarse + ind * ngridmax + no ** 3] = cells
    return np.ascontiguousarray(u)


def _brick(u, n, ngridmax, ncoarse):
    nvar, no = u.shape[0], n // 2
    out = np.zeros((nvar, n, n, n))
    for ind in range(8):
        ix, iy, iz = ind & 1, (ind >> 1) & 1, ind >> 2
        out[:, iz::2, iy::2, ix::2] = u[:, ncoarse + ind * ngridmax: ncoarse + ind * ngridmax + no ** 3].reshape(nvar, no, no, no)
    return out


def test_mpi_resident_entry_points_give_the_bits_of_hydro_level():
    from ramses_amd import _capi
    from ramses_amd._capi import check
    tag = "e1_hllc_s8"
    L = _capi.lib()
    p = _params(tag)
    dx = float(GOLD[tag + "_dx"])
    level, n = 4, 16
    no = n // 2
    ngrid = ngridmax = no ** 3
    ncoarse = 1
    igrid = np.arange(1, ngrid + 1, dtype=np.int32)
    io = np.arange(ngrid)
    xg = np.concatenate([((io >> (3 * 0)) % no + 0.5) / no, ((io // no) % no + 0.5) / no, (io // no ** 2 + 0.5) / no])
    uold = _cellvec(GOLD[tag + "_uold"][0], ngridmax, ncoarse)
    unew = uold.copy()
    zero = np.zeros(1, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    check(L.ramses_amd_mpires_setup(C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1, vp(uold), vp(unew),
                                    1, 1, vp(zero), vp(zero), vp(zero), vp(zero)))
    try:
        lv = _level(tag)
        lv.upload(GOLD[tag + "_uold"][0])
        out4 = np.zeros(4)
        sp, sl, hp, hl = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        for k in range(NSTEP):
            check(L.ramses_amd_mpires_courant(C.byref(p), dx, 1e30, vp(out4)))
            dt = lv.courant_fine()[0]
            assert out4[0] == dt == GOLD[tag + "_dt"][k]
            check(L.ramses_amd_mpires_godunov(C.byref(p), dx, dt))
            check(L.ramses_amd_mpires_reverse_unew())
            assert L.ramses_amd_mpires_set_uold() == -1          # the plain swap would drop the pdV term
            check(L.ramses_amd_mpires_set_uold_pdv(C.byref(p), dx, dt))
            check(L.ramses_amd_mpires_halo_stage_out(C.byref(sp), C.byref(sl), C.byref(hp), C.byref(hl)))
            check(L.ramses_amd_mpires_halo_stage_in())
            lv.godunov_fine(dt)
            lv.set_uold()
        check(L.ramses_amd_mpires_sync_host(vp(uold)))
        got = _brick(uold, n, ngridmax, ncoarse)
        assert _bits_equal(got, lv.download()), _where(got, lv.download())
        assert _bits_equal(got, GOLD[tag + "_uold"][NSTEP])
    finally:
        L.ramses_amd_mpires_invalidate()


# ---- the overlapped step of a decomposed level ------------------------------------------------------------------


def _rolled(tag, what, k):
    """The goldens moved periodically by 4 cells along -x: the blast then sits in the first cells of the box, next to a
    brick face, so the ghosts a sweep reads carry the pdV term (a periodic level does not care where its origin is)."""
    return np.roll(GOLD[tag + "_" + what][k], -4, axis=3)


def test_overlapped_step_with_nener_takes_the_pdv_term_into_the_ghosts():
    """BrickDecomposition.step_overlapped on one rank (the exchange is the periodic self-fill): with NENER the ghosts of
    the new state must carry set_uold's pdV term."""
    import ramses_amd  # noqa: F401
    from ramses_amd.parallel import BrickDecomposition
    tag = "e1_hllc_s2"
    dec = BrickDecomposition((1, 1, 1), 0, 16, boxlen=1.0)
    assert dec.dx == float(GOLD[tag + "_dx"])
    lev = dec.make_level(_params(tag))
    lev.upload(_rolled(tag, "uold", 0))
    dec.make_virtual_fine_dp(lev)
    for k in range(NSTEP):
        dec.step_overlapped(lev, float(GOLD[tag + "_dt"][k]))
        got = lev.download()
        assert _bits_equal(got, _rolled(tag, "uold", k + 1)), "step %d: %s" % (k + 1, _where(got, _rolled(tag, "uold", k + 1)))


def test_overlapped_step_with_nener_on_two_ranks():
    """Two virtual ranks, each a 8 x 16 x 16 half of the level, exchanging over the in-process transport."""
    import torch
    from ramses_amd.parallel import BrickDecomposition, rank_coords
    from ramses_amd.transport import LocalWorld
    tag = "e2_hllc_s1"

    def body(tr):
        dec = BrickDecomposition((2, 1, 1), tr.rank, (8, 16, 16), boxlen=1.0, transport=tr)
        lev = dec.make_level(_params(tag))
        x0 = 8 * rank_coords(tr.rank, (2, 1, 1))[0]
        lev.upload(np.ascontiguousarray(_rolled(tag, "uold", 0)[..., x0:x0 + 8]))
        dec.make_virtual_fine_dp(lev)
        ok = []
        for k in range(NSTEP):
            dec.step_overlapped(lev, float(GOLD[tag + "_dt"][k]))
            torch.cuda.synchronize()
            ok.append(_bits_equal(lev.download(), _rolled(tag, "uold", k + 1)[..., x0:x0 + 8]))
        return ok

    res = LocalWorld(2).run(body)
    assert res == [[True] * NSTEP] * 2, res


# ---- the plain swap of a level with non-thermal energies is refused ------------------------------------------


def test_resident_level_with_nener_refuses_the_plain_swap():
    from ramses_amd import _capi
    from ramses_amd._capi import check
    tag = "e1_llf_s1"
    L = _capi.lib()
    p = _params(tag)
    dx = float(GOLD[tag + "_dx"])
    level, n, no, ncoarse = 4, 16, 8, 1
    ngrid = ngridmax = no ** 3
    igrid = np.arange(1, ngrid + 1, dtype=np.int32)
    io = np.arange(ngrid)
    xg = np.concatenate([(io % no + 0.5) / no, ((io // no) % no + 0.5) / no, (io // no ** 2 + 0.5) / no])
    uold = _cellvec(GOLD[tag + "_uold"][0], ngridmax, ncoarse)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    out4 = np.zeros(4)
    try:
        for k in range(2):
            check(L.ramses_amd_resident_courant_f90(C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1, vp(uold),
                                                    dx, 1e30, vp(out4)))
            assert out4[0] == GOLD[tag + "_dt"][k]
            check(L.ramses_amd_resident_godunov_f90(C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1, vp(uold),
                                                    dx, out4[0]))
            assert L.ramses_amd_resident_set_uold_f90(level) == -1
            assert b"ramses_amd_resident_set_uold_pdv_f90" in L.ramses_amd_last_error()
            check(L.ramses_amd_resident_set_uold_pdv_f90(C.byref(p), level, dx, out4[0]))
        check(L.ramses_amd_resident_sync_host_f90(vp(uold)))
        assert _bits_equal(_brick(uold, n, ngridmax, ncoarse), GOLD[tag + "_uold"][2])
    finally:
        L.ramses_amd_resident_invalidate()

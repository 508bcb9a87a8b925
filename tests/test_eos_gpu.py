"""cooling_fine of a barotropic run of constant temperature on the device, through the C ABI, against the numpy checker
(tests/eos_checker.py, itself held to the reference program by tests/test_eos_checker.py) BIT FOR BIT:

  ramses_amd_amrres_cooling_fine         lvl_eos_kernel on the resident AMR state: the leaf cells of the listed octs
  ramses_amd_resident_cooling_fine_f90   eos_brick_kernel on the one-level resident brick
  ramses_amd_mpires_cooling_fine         eos_brick_kernel on a rank's brick with ghost layers

AMR levels: the trees and the harsh state of helpers.level_case (NVAR = 7; with smallr = 0.6 about half of the densities lie below
the floor): L = 4 in both oct orders (the host's numbering), L = 6 in the device's Z-order without tiles, L = 6 in tiles, L = 6 with
RAMSES_AMD_DEVICE_ORDER=0; every entry with a level's full list, a ragged list of 37 octs and ngrid = 0.  After EVERY call the
whole state comes back and every variable of every cell must carry the bits of the checker: the cells outside the listed octs,
the split cells inside them, the density, the momenta and the scalars unchanged.

Bricks: the resident brick is a whole level, so a cube: 8^3 and 16^3.  The MPI-resident brick: 8^3 (one rank, periodic self-fill)
and 38 x 10 x 6 (19 x 5 x 3 octs somewhere in a level of 32^3 octs, its one-oct shell received from a second rank): the host gets
the ghost octs back with the level, and they must be what was loaded."""
import ctypes as C
import itertools

import numpy as np
import pytest

import eos_checker as EC
import helpers as H
import resident as R
from resident import vp

pytestmark = pytest.mark.gpu

SMALLR, GAMMA = 0.6, 1.4
# (T2c, scale_nH, scale_T2): the units of the golden runs and a second set
EOS = [(4.8, 0.76 / 1.66e-24 * 1.3e-21, 1.66e-24 / 1.3806200e-16 * 1.0e10), (37.5, 1.2345e3, 7.7)]
# (L, order, environment)
CASES = [(4, "scrambled", {}), (4, "morton", {}), (6, "scrambled", {"RAMSES_AMD_TILES": "0"}), (6, "scrambled", {}),
         (6, "scrambled", {"RAMSES_AMD_DEVICE_ORDER": "0"})]
IDS = ["L4-scrambled-hostnumbers", "L4-morton-hostnumbers", "L6-zorder", "L6-tiles", "L6-hostorder"]


@pytest.fixture(autouse=True)
def _tiles_on_small_levels_too(monkeypatch):
    R.force_tiles(monkeypatch, clear=R.ALL_LAYOUT_VARS)
    yield
    R.reset_library()


def _set(Lb, eos):
    from ramses_amd._capi import check
    check(Lb.ramses_amd_eos_set(*eos))


def _tree_levels(T):
    """the octs of every level of the tree, walking son() down from the coarse cells"""
    out, cells = {}, np.arange(T["ncoarse"])
    lev = 0
    while True:
        g = T["son"][cells]
        g = g[g > 0].astype(np.int64)
        if g.size == 0:
            return out
        lev += 1
        out[lev] = np.ascontiguousarray(np.sort(g), dtype=np.int32)
        cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + g - 1 for ind in range(8)])


@pytest.mark.parametrize("L,order,env", CASES, ids=IDS)
def test_cooling_fine_on_resident_levels(gpu_lib, monkeypatch, L, order, env):
    from ramses_amd import _capi
    from ramses_amd._capi import check
    T, u0, _ = H.level_case(L, order)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    levels = _tree_levels(T)
    p = _capi.make_params(nvar=7, gamma=GAMMA, smallr=SMALLR)
    u = np.array(u0)
    R.load(gpu_lib, T, u)
    tiled = gpu_lib.ramses_amd_amrres_tiled_levels()
    assert tiled == (2 if IDS[CASES.index((L, order, env))] == "L6-tiles" else 0), tiled
    try:
        for eos in EOS:
            _set(gpu_lib, eos)
            for lev, kind in itertools.product((L + 1, L), ("full", "sub", "none")):
                octs = T["lists"][lev][kind]
                what = "T2c %g, level %d, %s list" % (eos[0], lev, kind)
                before = u.copy()
                want = before.copy()
                cells = H.oct_cells(T, octs) if len(octs) else np.zeros(0, np.int64)
                want[:, cells] = EC.cooling_fine(before[:, cells], T["son"][cells], *eos, SMALLR, GAMMA)
                check(gpu_lib.ramses_amd_amrres_cooling_fine(C.byref(p), len(octs), vp(octs)))
                for ig in levels.values():
                    check(gpu_lib.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(u)))
                other = np.ones(T["ncell"], bool)
                other[cells] = False
                moved = other & (EC.bits(u) != EC.bits(before)).any(axis=0)
                assert not moved.any(), "%s: %d cells outside the listed octs changed" % (what, moved.sum())
                split = cells[T["son"][cells] != 0]
                assert np.array_equal(EC.bits(u[:, split]), EC.bits(before[:, split])), "%s: split cells changed" % what
                bad = (EC.bits(u[:, cells]) != EC.bits(want[:, cells])).any(axis=0)
                assert not bad.any(), "%s: %d of %d listed cells differ from the checker, first got %r want %r" % (
                    what, bad.sum(), len(cells), u[:, cells[bad][:1]], want[:, cells[bad][:1]])
                assert np.array_equal(EC.bits(u), EC.bits(want)), what
                if kind == "full":
                    leaf = cells[T["son"][cells] == 0]
                    assert (before[0, leaf] < SMALLR).sum() > 100, "densities below the floor"
                    assert (EC.bits(u[4, leaf]) != EC.bits(before[4, leaf])).sum() > 100, "the call must do something"
                    if lev == L:
                        assert 0 < len(split) < len(cells)
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


def test_cooling_fine_needs_its_state(gpu_lib):
    from ramses_amd import _capi
    T, u0, _ = H.level_case(4, "scrambled")
    p = _capi.make_params(nvar=7, gamma=GAMMA, smallr=SMALLR)
    octs = T["lists"][4]["full"]
    gpu_lib.ramses_amd_amrres_invalidate()
    _set(gpu_lib, EOS[0])
    assert gpu_lib.ramses_amd_amrres_cooling_fine(C.byref(p), len(octs), vp(octs)) == -1
    assert b"no resident AMR state" in gpu_lib.ramses_amd_last_error()


def _harsh_cells(nvar, n, seed):
    """cell vectors [nvar][n]: about half of the densities below SMALLR, momenta of both signs, some cells at rest"""
    rng = np.random.default_rng(seed)
    u = np.zeros((nvar, n))
    u[0] = SMALLR * 10.0 ** rng.uniform(-1.5, 1.5, n)
    u[1:4] = u[0] * rng.normal(0.0, 0.7, (3, n))
    u[1:4, rng.random(n) < 0.05] = 0.0
    u[4] = rng.uniform(0.05, 2.0, n) / (GAMMA - 1.0) + 0.5 * (u[1:4] ** 2).sum(0) / u[0]
    for v in range(5, nvar):
        u[v] = u[0] * rng.uniform(0, 1, n)
    return u


def _uniform_octs(n):
    no = n // 2
    io = np.arange(no ** 3)
    igrid = np.arange(1, no ** 3 + 1, dtype=np.int32)
    xg = np.concatenate([(io % no + 0.5) / no, ((io // no) % no + 0.5) / no, (io // no ** 2 + 0.5) / no])
    return igrid, xg


@pytest.mark.parametrize("level,nvar", [(3, 5), (4, 7)], ids=["8cube", "16cube-nvar7"])
def test_cooling_fine_on_the_resident_brick(gpu_lib, level, nvar):
    from ramses_amd import _capi
    from ramses_amd._capi import check
    n = 2 ** level
    igrid, xg = _uniform_octs(n)
    ngrid = len(igrid)
    ngridmax, ncoarse = ngrid + 5, 1
    xgp = np.zeros((3, ngridmax))
    xgp[:, :ngrid] = xg.reshape(3, ngrid)
    p = _capi.make_params(nvar=nvar, gamma=GAMMA, smallr=SMALLR)
    u = _harsh_cells(nvar, ncoarse + 8 * ngridmax, 5 + level)
    before = u.copy()
    cells = np.concatenate([ncoarse + ind * ngridmax + igrid.astype(np.int64) - 1 for ind in range(8)])
    gpu_lib.ramses_amd_resident_invalidate()
    try:
        out4 = np.zeros(4)
        check(gpu_lib.ramses_amd_resident_courant_f90(C.byref(p), level, ngrid, vp(igrid), vp(xgp), ngridmax, ncoarse, 1, vp(u), 1.0 / n, 1e30, vp(out4)))
        for eos in EOS:
            _set(gpu_lib, eos)
            want = before.copy()
            want[:, cells] = EC.cooling_fine(before[:, cells], np.zeros(len(cells), np.int32), *eos, SMALLR, GAMMA)
            check(gpu_lib.ramses_amd_resident_cooling_fine_f90(C.byref(p), level))
            check(gpu_lib.ramses_amd_resident_sync_host_f90(vp(u)))
            assert (before[0, cells] < SMALLR).sum() > 100 and (EC.bits(u[4, cells]) != EC.bits(before[4, cells])).sum() > 100
            assert np.array_equal(EC.bits(u), EC.bits(want)), "T2c %g: %d cells differ" % (eos[0], (EC.bits(u) != EC.bits(want)).any(axis=0).sum())
            before = u.copy()
        assert gpu_lib.ramses_amd_resident_cooling_fine_f90(C.byref(p), level + 1) == -1
        assert b"is not resident" in gpu_lib.ramses_amd_last_error()
    finally:
        gpu_lib.ramses_amd_resident_sync_host_f90(vp(u))
        gpu_lib.ramses_amd_resident_invalidate()


def _box_rank(level, lo, dim, seed):
    """one rank of a level whose octs fill the box (lo, dim) of octs, its one-oct shell received from a second rank: igrid, xg,
    ngridmax, the ghost octs' slots"""
    rng = np.random.default_rng(seed)
    no = 2 ** (level - 1)
    own = [(lo[0] + i, lo[1] + j, lo[2] + k) for k in range(dim[2]) for j in range(dim[1]) for i in range(dim[0])]
    mine = set(own)
    ghosts = sorted({((lo[0] + i) % no, (lo[1] + j) % no, (lo[2] + k) % no) for k in range(-1, dim[2] + 1) for j in range(-1, dim[1] + 1)
                     for i in range(-1, dim[0] + 1)} - mine)
    ngridmax = len(own) + len(ghosts) + 11
    slots = rng.permutation(ngridmax)[:len(own) + len(ghosts)] + 1
    xg = np.zeros((3, ngridmax))
    for o, sl in zip(own + ghosts, slots):
        xg[:, sl - 1] = [(o[d] + 0.5) / no for d in range(3)]
    igrid = np.ascontiguousarray(slots[:len(own)][rng.permutation(len(own))], dtype=np.int32)
    ghost_slots = np.ascontiguousarray(slots[len(own):][rng.permutation(len(ghosts))], dtype=np.int32)
    return igrid, xg, ngridmax, ghost_slots


@pytest.mark.parametrize("shape", ["8cube", "38x10x6"])
def test_cooling_fine_on_the_mpi_resident_brick(gpu_lib, shape):
    from ramses_amd import _capi
    from ramses_amd._capi import check
    nvar, ncoarse = 6, 1
    if shape == "8cube":
        level = 3
        igrid, xg = _uniform_octs(8)
        ngridmax = len(igrid)
        xg = xg.reshape(3, ngridmax)
        ghost = np.zeros(0, np.int32)
        ncpu, em_n, rc_n, rc_ig = 1, np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    else:
        level = 6
        igrid, xg, ngridmax, ghost = _box_rank(level, (3, 20, 9), (19, 5, 3), 3)
        ncpu, em_n, rc_n, rc_ig = 2, np.zeros(2, np.int32), np.array([0, len(ghost)], np.int32), ghost
        assert len(igrid) * 8 == 38 * 10 * 6
    p = _capi.make_params(nvar=nvar, gamma=GAMMA, smallr=SMALLR)
    u = _harsh_cells(nvar, ncoarse + 8 * ngridmax, 11 + level)
    unew = u.copy()
    before = u.copy()
    cells = np.concatenate([ncoarse + ind * ngridmax + igrid.astype(np.int64) - 1 for ind in range(8)])
    gcells = np.concatenate([ncoarse + ind * ngridmax + ghost.astype(np.int64) - 1 for ind in range(8)])
    zero = np.zeros(1, np.int32)
    check(gpu_lib.ramses_amd_mpires_setup(C.byref(p), level, len(igrid), vp(igrid), vp(np.ascontiguousarray(xg)), ngridmax, ncoarse, 1, vp(u), vp(unew),
                                          ncpu, 1, vp(em_n), vp(zero), vp(rc_n), vp(rc_ig)))
    try:
        for eos in EOS:
            _set(gpu_lib, eos)
            want = before.copy()
            want[:, cells] = EC.cooling_fine(before[:, cells], np.zeros(len(cells), np.int32), *eos, SMALLR, GAMMA)
            check(gpu_lib.ramses_amd_mpires_cooling_fine(C.byref(p)))
            check(gpu_lib.ramses_amd_mpires_sync_host(vp(u)))
            assert (before[0, cells] < SMALLR).sum() > 100 and (EC.bits(u[4, cells]) != EC.bits(before[4, cells])).sum() > 100
            assert np.array_equal(EC.bits(u[:, gcells]), EC.bits(before[:, gcells])), "T2c %g: ghost octs changed" % eos[0]
            assert np.array_equal(EC.bits(u), EC.bits(want)), "T2c %g: %d cells differ" % (eos[0], (EC.bits(u) != EC.bits(want)).any(axis=0).sum())
            before = u.copy()
    finally:
        gpu_lib.ramses_amd_mpires_sync_host(vp(u))
        gpu_lib.ramses_amd_mpires_invalidate()

"""The device's own oct numbering and the dense sweep on levels in tiles (csrc/amr_layout.hpp, csrc/capi_amr.hip
tile_level_sweep) for a coarse grid of SEVERAL cells (ramses_amd_amrres_coarse_grid): boxes between walls -- one more coarse
cell per wall, whose octs are boundary octs: part of the tree, read as neighbours, never listed -- and elongated periodic boxes.
The lattice of a level is then neither cubic nor a power of two (96 x 32 x 32 octs at level 6 of a (3, 1, 1) grid).  Modelled
on tests/test_amr_tiles_gpu.py: host oct numbers in, one amr_step's worth of calls (set_unew, godunov_fine of level L+1 then L,
set_uold, sync), the C oracle of godfine1 (oracle/amr_godfine_oracle.c, which moves through nbor only) bit for bit out --
whatever the device did with the numbering: tiles, Z-order (RAMSES_AMD_TILES=0) or none (RAMSES_AMD_DEVICE_ORDER=0).

set_unew / set_uold run over the ACTIVE octs only, as in the reference (hydro/godunov_fine.f90:40-130, 135-232 loop over
active(ilevel)): the boundary octs' uold is make_boundary_hydro's business and must come back as it was loaded."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import oct_cells
from resident import force_tiles, reset_library, vp

pytestmark = pytest.mark.gpu

L = 6
N = 2 ** L
MODES = ["tiles", "z_order", "host_order"]


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    """the dense sweep on small levels too; the grid back to one cell afterwards (the setting holds for every later load of the
    process)"""
    force_tiles(monkeypatch, clear=("RAMSES_AMD_COARSE_GRID_TILES", "RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE",
                                    "RAMSES_AMD_COVERED_DENSE", "RAMSES_AMD_DEVICE_OCTS"))
    yield
    reset_library()


def _mode(monkeypatch, mode):
    if mode == "z_order":
        monkeypatch.setenv("RAMSES_AMD_TILES", "0")
    if mode == "host_order":
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", "0")


def _box(mask, xr, yr, zr):
    mask[zr[0]:zr[1], yr[0]:yr[1], xr[0]:xr[1]] = True


def _mask_x_walls(shift=0):
    """(3, 1, 1): level-6 cells [z, y, x] of 64 x 64 x 192, the active coarse cell at x in [64, 128)"""
    m = np.zeros((N, N, 3 * N), bool)
    _box(m, (64, 67), (10, 20), (10, 20))            # touches the low wall: the ghost octs beyond it come from boundary cells of level 6
    _box(m, (125, 128), (30, 40), (30, 40))          # touches the high wall
    _box(m, (60, 68), (40, 48), (8, 16))             # refined on the boundary side too: the neighbour exists at level 7
    _box(m, (90, 100), (0, 3), (20, 26))             # the periodic y seam
    _box(m, (90, 100), (61, 64), (20, 26))
    _box(m, (70, 80), (20, 26), (0, 2))              # the periodic z seam
    _box(m, (70, 80), (20, 26), (62, 64))
    _box(m, (80 + shift, 110 + shift), (24, 40), (24, 40))
    return m


def _mask_yz_walls():
    """(1, 3, 2): cells [z, y, x] of 128 x 192 x 64, the active coarse cell at y in [64, 128), z in [0, 64); walls at both ends in
    y, one coarse cell of boundary octs in z (it is the neighbour on both z sides of the active cell)"""
    m = np.zeros((2 * N, 3 * N, N), bool)
    _box(m, (10, 20), (64, 67), (10, 20))            # low y wall
    _box(m, (30, 40), (125, 128), (30, 40))          # high y wall
    _box(m, (40, 48), (60, 68), (8, 16))             # across the low y wall
    _box(m, (20, 30), (80, 90), (61, 64))            # the z wall (high side)
    _box(m, (20, 30), (100, 110), (0, 3))            # the z wall again, through the wrap of the tile rows in z
    _box(m, (44, 52), (100, 108), (60, 68))          # across the z wall
    _box(m, (0, 3), (90, 100), (20, 26))             # the periodic x seam
    _box(m, (61, 64), (90, 100), (20, 26))
    _box(m, (24, 40), (80, 110), (24, 40))
    return m


def _mask_elongated():
    """(2, 1, 1): a shell around the seam between the two coarse cells"""
    z, y, x = np.meshgrid(np.arange(N), np.arange(N), np.arange(2 * N), indexing="ij")
    r = np.sqrt((x - N + 0.5) ** 2 + (y - N / 2 + 0.5) ** 2 + (z - N / 2 + 0.5) ** 2)
    m = (r >= 0.25 * N) & (r <= 0.33 * N)
    m[0, 0, :5] = True                               # and the periodic ends
    m[N - 1, N - 1, 2 * N - 3:] = True
    return m


def _case(grid, active_cell, mask, order, slack=300000):
    """the tree, the octs of the active coarse cell per level (the others are boundary octs), every oct per level"""
    from ramses_amd import ic
    nx, ny, nz = grid
    T = ic.coarse_grid_tree(grid, L, order=order, refine_mask=mask, slack=slack)
    no = 2 ** (L - 1)
    if active_cell is None:
        act6 = np.ones((nz * no, ny * no, nx * no), bool)
        actf = np.ones(len(T["fine_ids"]), bool)
    else:
        i, j, k = active_cell
        act6 = np.zeros((nz * no, ny * no, nx * no), bool)
        act6[k * no:(k + 1) * no, j * no:(j + 1) * no, i * no:(i + 1) * no] = True
        cz, cy, cx = T["fine_pos"]
        actf = (cx // N == i) & (cy // N == j) & (cz // N == k)
    ids6 = T["oct_ids"][L]
    in_list6 = np.zeros(T["ngridmax"] + 1, bool)
    in_list6[ids6[act6]] = True
    in_listf = np.zeros(T["ngridmax"] + 1, bool)
    in_listf[T["fine_ids"][actf]] = True
    # (the lists keep the builder's order: scrambled or Z-order)
    T["active"] = {L: np.ascontiguousarray(T["igrid"][in_list6[T["igrid"]]]), L + 1: np.ascontiguousarray(T["igrid_fine"][in_listf[T["igrid_fine"]]])}
    T["everything"] = {L: np.ascontiguousarray(np.sort(T["igrid"])), L + 1: np.ascontiguousarray(np.sort(T["igrid_fine"]))}
    bnd = np.concatenate([T["igrid"][~in_list6[T["igrid"]]], T["igrid_fine"][~in_listf[T["igrid_fine"]]]])
    T["boundary_octs"] = bnd
    T["is_boundary"] = np.zeros(T["ngridmax"] + 1, bool)
    T["is_boundary"][bnd] = True
    return T


def _random_state(T, seed, nvar=5):
    """(not helpers.mild_tree_state: this one draws a value for cell 0 as well, which shifts every later draw; the cases of this file
    were validated on these states)"""
    rng = np.random.default_rng(seed)
    ncell = T["ncell"]
    u = np.zeros((nvar, ncell))
    u[0] = 1.0 + rng.random(ncell)
    for d in (1, 2, 3):
        u[d] = u[0] * (rng.random(ncell) - 0.5)
    u[4] = 1.0 + rng.random(ncell) + 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0]
    return u


def _oracle_step(oracle, po, T, uold, f, lists, ivar=0, itype=1):
    unew = uold.copy()
    for level in (L + 1, L):
        dx = 1.0 / 2 ** level
        oracle.godunov_fine_amr(po, lists[level], T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew, dx, 0.02 * dx, 32,
                                ivar, itype, f=f)
    return unew


def _device_step(Lb, p, T, u, f, lists, ivar=0, itype=1, load=True):
    from ramses_amd._capi import check
    if load:
        check(Lb.ramses_amd_amrres_invalidate())
        check(Lb.ramses_amd_amrres_coarse_grid(*T["grid"]))
        check(Lb.ramses_amd_amrres_load(u.shape[0], T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
        if f is not None:
            for lev in (L, L + 1):           # (the boundary octs' too: a ghost oct beyond a wall takes its father cell's)
                ig = T["everything"][lev]
                check(Lb.ramses_amd_amrres_load_f(len(ig), vp(ig), vp(f)))
    for lev in (L, L + 1):
        ig = T["active"][lev]
        check(Lb.ramses_amd_amrres_set_unew(len(ig), vp(ig)))
    for lev in (L + 1, L):
        ig = np.ascontiguousarray(lists[lev])
        dx = 1.0 / 2 ** lev
        check(Lb.ramses_amd_amrres_godunov(C.byref(p), lev, len(ig), vp(ig), dx, 0.02 * dx, 32, ivar, itype))
    for lev in (L, L + 1):
        ig = T["active"][lev]
        check(Lb.ramses_amd_amrres_set_uold(C.byref(p), len(ig), vp(ig)))
    for lev in (L, L + 1):
        ig = T["everything"][lev]
        check(Lb.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(u)))
    return u


def _wall_side_ghosts(T, listed_fine, dirs):
    """listed level-7 octs with a neighbour position beyond a wall (its father cell belongs to a boundary oct) that holds no oct"""
    count = 0
    for d in dirs:
        c = T["nbor"][d, listed_fine - 1].astype(np.int64)
        assert (c > T["ncoarse"]).all()
        g = (c - T["ncoarse"] - 1) % T["ngridmax"] + 1
        count += int((T["is_boundary"][g] & (T["son"][c - 1] == 0)).sum())
    return count


CASES = {
    # name: (grid, active coarse cell, mask, order, solver keywords, gravity, interpolation, wall directions)
    "x_walls_llf": ((3, 1, 1), (1, 0, 0), _mask_x_walls, "morton", dict(riemann="llf", slope_type=1), False, (0, 1), (0, 1)),
    "x_walls_hllc_grav": ((3, 1, 1), (1, 0, 0), _mask_x_walls, "scrambled", dict(riemann="hllc", slope_type=2), True, (1, 2), (0, 1)),
    "yz_walls": ((1, 3, 2), (0, 1, 0), _mask_yz_walls, "scrambled", dict(riemann="hll", slope_type=1), False, (0, 1), (2, 3, 4, 5)),
    "elongated": ((2, 1, 1), None, _mask_elongated, "scrambled", dict(riemann="llf", slope_type=1), False, (0, 1), ()),
    "part_of_the_list": ((3, 1, 1), (1, 0, 0), _mask_x_walls, "scrambled", dict(riemann="hllc", slope_type=1), False, (0, 1), (0, 1)),
}


@functools.lru_cache(maxsize=1)
def _prepared(name):
    """tree, state, lists and the oracle's result of a case: once for its three numberings (nothing here is written afterwards)"""
    from oracle import pyoracle
    pyoracle.build_oracle()
    grid, active, mask, order, kw, grav, interp, walls = CASES[name]
    T = _case(grid, active, mask(), order)
    uold = _random_state(T, 11)
    f = np.random.default_rng(5).normal(size=(3, T["ncell"])) if grav else None
    lists = dict(T["active"])
    if name == "part_of_the_list":
        # several ranks: the call's list holds the rank's own octs, the other active octs are there but are not updated
        for lev, mod, keep in ((L, 3, lambda r: r != 0), (L + 1, 5, lambda r: r < 3)):
            fc = T["father"][lists[lev] - 1].astype(np.int64)
            lists[lev] = np.ascontiguousarray(lists[lev][keep(fc % mod)])
            assert 0 < len(lists[lev]) < len(T["active"][lev])
    ref = _oracle_step(pyoracle, pyoracle.make_params(**kw), T, uold, f, lists, *interp)
    for a in (uold, ref) + ((f,) if grav else ()):
        a.setflags(write=False)
    return T, uold, f, lists, ref


@pytest.mark.parametrize("mode", MODES)        # (the numbering varies fastest: _prepared holds one case)
@pytest.mark.parametrize("name", list(CASES))
def test_levels_of_a_multi_cell_coarse_grid_equal_the_oracle(gpu_lib, monkeypatch, name, mode):
    import ramses_amd
    grid, active, mask, order, kw, grav, interp, walls = CASES[name]
    T, uold, f, lists, ref = _prepared(name)
    _mode(monkeypatch, mode)
    if walls:
        assert len(T["boundary_octs"]) > 0
        assert _wall_side_ghosts(T, lists[L + 1], walls) > 0          # the ghost path at the wall is really taken
    p = ramses_amd.make_params(**kw)
    t0, w0, c0 = gpu_lib.ramses_amd_amrres_tile_sweeps(), gpu_lib.ramses_amd_amrres_tree_sweeps(), gpu_lib.ramses_amd_amrres_covered_sweeps()
    got = _device_step(gpu_lib, p, T, uold.copy(), f, lists, *interp)
    dt, dw = gpu_lib.ramses_amd_amrres_tile_sweeps() - t0, gpu_lib.ramses_amd_amrres_tree_sweeps() - w0
    if mode == "tiles":
        assert gpu_lib.ramses_amd_amrres_tiled_levels() == 2
        assert (dt, dw) == (2, 0)
        # (a level between walls is never "covered"; the complete level of the elongated box, listed whole, is)
        assert gpu_lib.ramses_amd_amrres_covered_sweeps() - c0 == (1 if name == "elongated" else 0)
    else:
        assert gpu_lib.ramses_amd_amrres_tiled_levels() == 0 and (dt, dw) == (0, 2)
    assert gpu_lib.ramses_amd_amrres_first_changed() == (0 if mode == "host_order" else 1)
    cells = oct_cells(T, np.concatenate([lists[L], lists[L + 1]]))
    assert np.array_equal(got[:, cells].view(np.int64), ref[:, cells].view(np.int64)), np.abs(got[:, cells] - ref[:, cells]).max()
    assert (ref[:, cells] != uold[:, cells]).any(0).mean() > 0.9
    if len(T["boundary_octs"]):
        b = oct_cells(T, T["boundary_octs"])
        assert np.array_equal(got[:, b].view(np.int64), uold[:, b].view(np.int64))
    # (active octs that are not in the call's list: set_unew / set_uold leave them as they were)
    rest = np.setdiff1d(np.concatenate([T["active"][L], T["active"][L + 1]]), np.concatenate([lists[L], lists[L + 1]]))
    if len(rest):
        # ... except for what a listed level-7 oct owes to a leaf cell of level 6 (hydro/godunov_fine.f90:798-908): the oracle's unew
        r = oct_cells(T, rest)
        assert np.array_equal(got[:, r].view(np.int64), ref[:, r].view(np.int64))


def test_load_refuses_an_ncoarse_that_is_not_the_grid(gpu_lib):
    from ramses_amd import ic
    from ramses_amd._capi import check
    T = ic.coarse_grid_tree((3, 1, 1), 2)
    uold = _random_state(T, 3)
    check(gpu_lib.ramses_amd_amrres_invalidate())
    check(gpu_lib.ramses_amd_amrres_coarse_grid(2, 1, 1))
    rc = gpu_lib.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(uold), vp(T["son"]), vp(T["nbor"]), vp(T["father"]))
    assert rc != 0 and b"coarse grid 2 x 1 x 1" in gpu_lib.ramses_amd_last_error()
    assert gpu_lib.ramses_amd_amrres_coarse_grid(0, 1, 1) != 0 and b"coarse_grid" in gpu_lib.ramses_amd_last_error()
    # the right grid: the device's own numbering is in force (levels 1 and 2: Z-order, nothing to store in tiles)
    check(gpu_lib.ramses_amd_amrres_coarse_grid(3, 1, 1))
    check(gpu_lib.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(uold), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
    assert gpu_lib.ramses_amd_amrres_first_changed() == 1 and gpu_lib.ramses_amd_amrres_tiled_levels() == 0
    back = np.zeros_like(uold)
    back[:] = uold
    check(gpu_lib.ramses_amd_amrres_sync_all(vp(uold)))
    assert np.array_equal(uold, back)


def test_a_regrid_of_level_7_keeps_the_layout_of_level_6(gpu_lib, oracle, monkeypatch):
    """refine_fine's hook between walls: after a step level 7 is rebuilt on the host, the tree goes down again and ONLY level 7 is
    reloaded (ramses_amd_amrres_first_changed() == 7); level 6 -- active and boundary octs -- stays where it was on the device with
    the state the first step left there.  Two steps on the device == two steps of the oracle."""
    import ramses_amd
    from ramses_amd._capi import check
    m1, m2 = _mask_x_walls(0), _mask_x_walls(-9)
    n1, n2 = int(m1.sum()), int(m2.sum())
    T1 = _case((3, 1, 1), (1, 0, 0), m1, "morton", slack=300000 + max(n1, n2) - n1)
    T2 = _case((3, 1, 1), (1, 0, 0), m2, "morton", slack=300000 + max(n1, n2) - n2)
    assert T1["ngridmax"] == T2["ngridmax"] and np.array_equal(T1["igrid"], T2["igrid"]) and not np.array_equal(m1, m2)
    kw = dict(riemann="llf", slope_type=2)
    p, po = ramses_amd.make_params(**kw), oracle.make_params(**kw)
    u0 = _random_state(T1, 19)
    h1 = _oracle_step(oracle, po, T1, u0, None, T1["active"])
    # (the oracle's unew -> uold on the active octs only, as set_uold does: boundary octs keep their uold)
    a1 = oct_cells(T1, np.concatenate([T1["active"][L], T1["active"][L + 1]]))
    s1 = u0.copy()
    s1[:, a1] = h1[:, a1]

    def refill(u):
        # what refine_fine leaves on the host for the rebuilt level: from the (synced) coarser level, a factor per octant
        v = u.copy()
        igf = T2["everything"][L + 1]
        for ind in range(8):
            c = T2["ncoarse"] + ind * T2["ngridmax"] + igf - 1
            v[:, c] = u[:, T2["father"][igf - 1] - 1] * (1.0 + 0.01 * (ind - 3.5))
        return v
    s1r = refill(s1)
    h2 = _oracle_step(oracle, po, T2, s1r, None, T2["active"])
    u = _device_step(gpu_lib, p, T1, u0.copy(), None, T1["active"])
    assert gpu_lib.ramses_amd_amrres_tiled_levels() == 2
    u[:] = refill(u)
    c6 = oct_cells(T2, T2["everything"][L])
    u[:, c6] = -7.0                      # if the device read level 6 from the host again, the result would show it
    check(gpu_lib.ramses_amd_amrres_tree(vp(T2["son"]), vp(T2["nbor"]), vp(T2["father"])))
    assert gpu_lib.ramses_amd_amrres_first_changed() == L + 1
    igf = T2["everything"][L + 1]
    check(gpu_lib.ramses_amd_amrres_load_level(len(igf), vp(igf), vp(u)))
    t0, w0 = gpu_lib.ramses_amd_amrres_tile_sweeps(), gpu_lib.ramses_amd_amrres_tree_sweeps()
    got = _device_step(gpu_lib, p, T2, u, None, T2["active"], load=False)
    assert gpu_lib.ramses_amd_amrres_tile_sweeps() - t0 == 2 and gpu_lib.ramses_amd_amrres_tree_sweeps() == w0
    cells = oct_cells(T2, np.concatenate([T2["active"][L], T2["active"][L + 1]]))
    assert np.array_equal(got[:, cells].view(np.int64), h2[:, cells].view(np.int64)), np.abs(got[:, cells] - h2[:, cells]).max()
    assert (h2[:, cells] != s1r[:, cells]).any(0).mean() > 0.9
    b6 = oct_cells(T2, T2["igrid"][T2["is_boundary"][T2["igrid"]]])
    assert np.array_equal(got[:, b6].view(np.int64), u0[:, b6].view(np.int64))        # level 6's boundary octs: as loaded, through both steps

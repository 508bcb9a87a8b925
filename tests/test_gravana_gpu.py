"""Analytic gravity (gravity_type 1, 2) on the device, through the C ABI, against the numpy checker (tests/gravana_checker.py,
itself held to the reference program by tests/test_gravana_checker.py) BIT FOR BIT:

  ramses_amd_amrres_force_ana        lvl_gravana_kernel on the resident f, from the resident oct centres
  ramses_amd_amrres_boundary_force   bnd_mark / bndf_compute / bnd_store: make_boundary_force's in-place, chunked loop
  ramses_amd_gravana_eval            the device function on positions the caller gives
  ramses_amd_resident_force_ana_f90  gravana_brick_kernel on the one-level resident brick
  ramses_amd_gravana_set             refuses gravity_type 3 by name

Modelled on tests/test_amr_level_kernels_gpu.py: the trees of helpers.level_case (L = 4 in both oct orders: the host's numbering;
L = 6 in tiles; L = 6 with RAMSES_AMD_DEVICE_ORDER=0), every entry with a level's full list, a ragged list of 37 octs and
ngrid = 0.  f starts as N(0, 1) in every cell of every level; after EVERY call the whole f comes back (ramses_amd_amrres_sync_f
over every level) and every cell outside the listed octs must be bit-identical to what was loaded.  The only tolerance is on the
potential-energy sum, n 2^-53 sum |terms|, which bounds any order of summation."""
import ctypes as C
import itertools

import numpy as np
import pytest

import gravana_checker as GC
import helpers as H
import resident as R
from resident import vp

pytestmark = pytest.mark.gpu

# (gravity_type, gravity_params, boxlen)
GRAVITY = [(1, (0.3, -0.2, -1.7), 0.5),
           (2, (3.0, 0.02, 0.2, 0.3, 0.1), 0.5),
           (2, (3.0, 0.02, 0.2, 0.3, 0.1), 3.0),
           (2, (3.0, 0.0, 0.21, 0.13, 0.37), 3.0),
           (2, (3.0, 0.0, 0.21, 0.13, 0.37), 0.5)]
CASES = [(4, "scrambled", None), (4, "morton", None), (6, "scrambled", None), (6, "scrambled", "0")]
IDS = ["L%d-%s%s" % (c[0], c[1], "-hostorder" if c[2] == "0" else "") for c in CASES]


@pytest.fixture(autouse=True)
def _tiles_on_small_levels_too(monkeypatch):
    R.force_tiles(monkeypatch, clear=R.ALL_LAYOUT_VARS)
    yield
    R.reset_library()


def _params10(params):
    return np.array(list(params) + [0.0] * (10 - len(params)))


def _set(Lb, gtype, params, skip, scale):
    from ramses_amd._capi import check
    check(Lb.ramses_amd_gravana_set(gtype, vp(_params10(params)), vp(np.array(skip, dtype=np.float64)), float(scale)))


def tree_levels(T):
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


def _load(Lb, T, levels, xg, f, grid=(1, 1, 1)):
    """the tree (any state), the oct centres and f of every level onto the device"""
    u = np.ones((5, T["ncell"]))
    R.load(Lb, T, u, f, levels=levels.values(), grid=grid, xg=xg)
    return u


def _fetch_f(Lb, levels, into):
    from ramses_amd._capi import check
    for ig in levels.values():
        check(Lb.ramses_amd_amrres_sync_f(len(ig), vp(ig), vp(into)))


def _same_bits(a, b):
    return np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("L,order,device_order", CASES, ids=IDS)
def test_force_ana_on_resident_levels(gpu_lib, monkeypatch, L, order, device_order):
    from ramses_amd._capi import check
    T, _, f0 = H.level_case(L, order)
    if device_order is not None:
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", device_order)
    levels = tree_levels(T)
    assert sorted(levels) == list(range(1, L + 2))
    xg = GC.tree_xg(T)
    f = np.array(f0)
    _load(gpu_lib, T, levels, xg, f)
    assert gpu_lib.ramses_amd_amrres_tiled_levels() == (2 if L >= 6 and device_order != "0" else 0)
    try:
        for gtype, params, boxlen in GRAVITY:
            _set(gpu_lib, gtype, params, (0.0, 0.0, 0.0), boxlen)
            for lev, kind in itertools.product((L + 1, L), ("full", "sub", "none")):
                octs = T["lists"][lev][kind]
                dx = 0.5 ** lev
                what = "gravity_type %d %r boxlen %g, level %d, %s list" % (gtype, params, boxlen, lev, kind)
                before = f.copy()
                want = GC.force_ana(T, xg, before, octs, gtype, params, dx, (0.0, 0.0, 0.0), boxlen)
                if gtype == 2 and len(octs):
                    g = octs.astype(np.int64)
                    rr = np.concatenate([GC.gravana(2, params, GC.cell_centres(xg[:, g - 1], ind, dx, (0, 0, 0), boxlen))[1] for ind in range(8)])
                    assert (rr > 0).all() and np.isfinite(want).all(), what
                diag = np.full(2, np.nan)
                fact = -0.37
                check(gpu_lib.ramses_amd_amrres_force_ana(lev, len(octs), vp(octs), dx, fact, vp(diag)))
                _fetch_f(gpu_lib, levels, f)
                cells = H.oct_cells(T, octs) if len(octs) else np.zeros(0, np.int64)
                other = np.ones(T["ncell"], bool)
                other[cells] = False
                moved = other & (f.view(np.int64) != before.view(np.int64)).any(axis=0)
                assert not moved.any(), "%s: %d cells outside the listed octs changed" % (what, moved.sum())
                bad = (f[:, cells].view(np.int64) != want[:, cells].view(np.int64)).any(axis=0)
                assert not bad.any(), "%s: %d of %d listed cells differ from the checker, first got %r want %r" % (
                    what, bad.sum(), len(cells), f[:, cells[bad][:1]], want[:, cells[bad][:1]])
                assert _same_bits(f, want), what
                # the diagnostics: fact * sum f**2 over the leaf cells of the list; no deposit on the device -> -1
                leaves = H.leaf_cells(T, octs) if len(octs) else np.zeros(0, np.int64)
                terms = (fact * (want[:, leaves] * want[:, leaves])).reshape(-1)
                s, bound = H.fsum_bound(terms) if terms.size else (0.0, 0.0)
                assert abs(diag[0] - s) <= bound, (what, diag[0], s, bound)
                assert diag[1] == -1.0, (what, diag)
                if lev == L and kind == "full":
                    assert 0 < len(leaves) < len(cells)          # (split cells are left out of the sum)
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("mode", ["tiles", "host_order"])
def test_force_ana_between_walls_uses_the_coarse_grid_offset(gpu_lib, monkeypatch, mode):
    """coarse_grid_tree((1, 1, 3), 5): nz = 3, skip = (0, 0, 1); the octs of the middle coarse cell are the level's list"""
    from ramses_amd import ic
    from ramses_amd._capi import check
    if mode == "host_order":
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", "0")
    grid, L = (1, 1, 3), 5
    T = ic.coarse_grid_tree(grid, L)
    levels = tree_levels(T)
    xg = GC.tree_xg(T, grid)
    no = 2 ** (L - 1)
    rng = np.random.default_rng(5)
    active = np.ascontiguousarray(rng.permutation(T["oct_ids"][L][no:2 * no].reshape(-1)), dtype=np.int32)
    f = rng.normal(size=(3, T["ncell"]))
    _load(gpu_lib, T, levels, xg, f, grid)
    skip = (0.0, 0.0, 1.0)
    try:
        for gtype, params, boxlen in GRAVITY[1:4]:
            _set(gpu_lib, gtype, params, skip, boxlen)
            for octs in (np.ascontiguousarray(active[5:42]), active):          # (the ragged list first: both calls change something)
                before = f.copy()
                want = GC.force_ana(T, xg, before, octs, gtype, params, 0.5 ** L, skip, boxlen)
                # the centres lie in [0, boxlen]: the offset is in force
                z = GC.cell_centres(xg[:, octs.astype(np.int64) - 1], 0, 0.5 ** L, skip, boxlen)[2]
                assert z.min() > 0 and z.max() < boxlen
                diag = np.zeros(2)
                check(gpu_lib.ramses_amd_amrres_force_ana(L, len(octs), vp(octs), 0.5 ** L, 1.0, vp(diag)))
                _fetch_f(gpu_lib, levels, f)
                assert _same_bits(f, want), (gtype, params, boxlen, len(octs))
                assert (f != before).any()
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


def test_gravana_eval_on_given_positions(gpu_lib):
    from ramses_amd._capi import check
    rng = np.random.default_rng(11)
    x = np.ascontiguousarray(rng.uniform(0.0, 3.0, (3, 100)))
    for gtype, params, boxlen in GRAVITY:
        _set(gpu_lib, gtype, params, (0.0, 0.0, 0.0), boxlen)
        f = np.full((3, 100), np.nan)
        check(gpu_lib.ramses_amd_gravana_eval(100, vp(x), vp(f)))
        assert _same_bits(f, GC.gravana(gtype, params, x)[0]), (gtype, params)
    check(gpu_lib.ramses_amd_gravana_eval(0, None, None))


def test_gravity_type_3_is_refused_by_name(gpu_lib):
    p, s = np.zeros(10), np.zeros(3)
    for gtype in (3, 0, -1, 4):
        rc = gpu_lib.ramses_amd_gravana_set(gtype, vp(p), vp(s), 1.0)
        assert rc == -2 and b"gravity_type" in gpu_lib.ramses_amd_last_error() and b"ramses_amd_gravana_set" in gpu_lib.ramses_amd_last_error()
    assert gpu_lib.ramses_amd_gravana_set(2, None, vp(s), 1.0) == -1


def test_entries_fail_loudly_without_their_state(gpu_lib):
    from ramses_amd._capi import check
    check(gpu_lib.ramses_amd_amrres_invalidate())
    _set(gpu_lib, 1, (0.0, 0.0, -1.0), (0, 0, 0), 1.0)
    ig, d = np.array([1], np.int32), np.zeros(2)
    assert gpu_lib.ramses_amd_amrres_force_ana(1, 1, vp(ig), 0.5, 1.0, vp(d)) == -1
    assert b"no resident AMR state" in gpu_lib.ramses_amd_last_error()
    one = np.array([1], np.int32)
    assert gpu_lib.ramses_amd_amrres_boundary_force(1, vp(one), vp(one), vp(ig), 32, 0.5) == -1
    assert b"no resident AMR state" in gpu_lib.ramses_amd_last_error()
    assert gpu_lib.ramses_amd_resident_invalidate() == 0
    assert gpu_lib.ramses_amd_resident_force_ana_f90(4, 1.0, vp(d)) == -1
    assert b"is not resident" in gpu_lib.ramses_amd_last_error()


def test_force_ana_on_the_resident_brick(gpu_lib):
    """a 16^3 level resident as a brick (rho_fine has left its deposit): f of every cell of the level == the checker at (i + 0.5) dx
    boxlen; cells off the level keep their host values; diag2 = {fact sum f**2 within the summation bound, max |rho| exactly}"""
    import ramses_amd
    from test_capi_host_levels_gpu import Level, _rho_brick
    level, n = 4, 16
    u = H.random_brick(n, n, n, seed=54)
    u[0] = _rho_brick(n, 7)
    L = Level(level, 404, u=u)
    uold = L.vec["u"]
    p = ramses_amd.make_params()
    rng = np.random.default_rng(3)
    kz, ky, kx = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    try:
        for gtype, params, boxlen in GRAVITY:
            phi, f, rho = rng.normal(size=(1, L.ncell)), rng.normal(size=(3, L.ncell)), rng.normal(size=(1, L.ncell))
            before = f.copy()
            mp, diag = np.zeros(4), np.zeros(2)
            assert gpu_lib.ramses_amd_resident_invalidate() == 0
            assert gpu_lib.ramses_amd_resident_rho_fine_f90(C.byref(p), *L.head(), vp(uold), boxlen, 32, vp(mp)) == 0, gpu_lib.ramses_amd_last_error()
            _set(gpu_lib, gtype, params, (0.0, 0.0, 0.0), boxlen)
            fact = -0.11
            assert gpu_lib.ramses_amd_resident_force_ana_f90(level, fact, vp(diag)) == 0, gpu_lib.ramses_amd_last_error()
            assert gpu_lib.ramses_amd_resident_sync_poisson_f90(vp(phi), vp(f), vp(rho)) == 0, gpu_lib.ramses_amd_last_error()
            dx = 0.5 ** level
            x = np.stack([((k + 0.5) * dx - 0.0) * boxlen for k in (kx, ky, kz)]).reshape(3, -1)
            want = GC.gravana(gtype, params, x)[0].reshape(3, n, n, n)
            got = L.to_brick(f)
            assert _same_bits(got, want), (gtype, params, boxlen)
            assert L.off_level_kept(f, before)
            s, bound = H.fsum_bound((fact * (want * want)).reshape(-1))
            assert abs(diag[0] - s) <= bound, (diag, s, bound)
            assert diag[1] == np.abs(L.to_brick(rho)).max()
    finally:
        gpu_lib.ramses_amd_resident_invalidate()


# ---- make_boundary_force -----------------------------------------------------------------------------------------------------------

def _row_tree(nocts=7):
    """a row of octs along every axis at once (tests/test_walls_resident_gpu.py): coarse cell c holds oct c, the neighbour of oct g
    towards the low end of any axis is coarse cell g - 1, towards the high end g + 1"""
    ncoarse = ngridmax = nocts
    ncell = ncoarse + 8 * ngridmax
    son = np.zeros(ncell, dtype=np.int32)
    son[:ncoarse] = np.arange(1, nocts + 1)
    nbor = np.zeros((6, ngridmax), dtype=np.int32)
    for g in range(1, nocts + 1):
        for axis in range(3):
            nbor[2 * axis, g - 1] = g - 1
            nbor[2 * axis + 1, g - 1] = g + 1 if g < nocts else 0
    father = np.arange(1, nocts + 1, dtype=np.int32)
    return dict(son=son, nbor=nbor, father=father, ncoarse=ncoarse, ngridmax=ngridmax, ncell=ncell)


@pytest.mark.parametrize("nvector", [1, 2, 32])
@pytest.mark.parametrize("btype", [1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16, 21, 24, 25])
def test_deep_boundary_regions_of_f_follow_the_references_in_place_loop(gpu_lib, btype, nvector):
    """a row of 7 octs along the wall's normal, the outer three of them boundary octs of one region, in every list order: what an
    oct reads from an oct of its own region (new or old) must be what the reference's chunked loop reads.  Imposed regions take
    gravana at their own centres (the row's oct centres are made up: any numbers do)."""
    from ramses_amd._capi import check
    T = _row_tree()
    high = (btype % 10) % 2 == 0
    region = [7, 6, 5] if high else [1, 2, 3]
    rng = np.random.default_rng(200 + btype)
    xg = np.ascontiguousarray(rng.uniform(0.1, 0.9, (3, T["ngridmax"])))
    grav = (2, (3.0, 0.02, 0.2, 0.3, 0.1), (0.0, 0.0, 0.0), 3.0)
    _set(gpu_lib, grav[0], grav[1], grav[2], grav[3])
    dx = 0.125
    u = np.ones((5, T["ncell"]))
    everything = np.arange(1, 8, dtype=np.int32)
    differ = 0
    try:
        for order in itertools.permutations(region):
            f0 = rng.normal(size=(3, T["ncell"]))
            want = f0.copy()
            GC.boundary_force(want, T["son"], T["nbor"], T["ncoarse"], T["ngridmax"], btype, list(order), nvector, grav, xg, dx)
            alt = f0.copy()
            GC.boundary_force(alt, T["son"], T["nbor"], T["ncoarse"], T["ngridmax"], btype, list(order), 3 if nvector == 1 else 1, grav, xg, dx)
            differ += int(not _same_bits(alt, want))
            got = f0.copy()
            check(gpu_lib.ramses_amd_amrres_invalidate())
            check(gpu_lib.ramses_amd_amrres_coarse_grid(1, 1, 1))
            check(gpu_lib.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
            check(gpu_lib.ramses_amd_amrres_xg(vp(xg)))
            check(gpu_lib.ramses_amd_amrres_load_f(7, vp(everything), vp(got)))
            bt, ng, ig = np.array([btype], np.int32), np.array([3], np.int32), np.array(order, np.int32)
            check(gpu_lib.ramses_amd_amrres_boundary_force(1, vp(bt), vp(ng), vp(ig), nvector, dx))
            got[:] = np.nan
            check(gpu_lib.ramses_amd_amrres_sync_f(7, vp(everything), vp(got)))
            assert _same_bits(got[:, T["ncoarse"]:], want[:, T["ncoarse"]:]), (btype, nvector, order)
        if btype < 20:
            assert differ > 0          # (the chunking matters in this input: the case tests something)
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("nvector", [1, 32])
@pytest.mark.parametrize("types", [(5, 6), (15, 16), (25, 26), (5, 16), (25, 6)], ids=lambda t: "z%d-%d" % t)
@pytest.mark.parametrize("mode", ["device_order", "host_order"])
def test_boundary_force_between_z_walls(gpu_lib, monkeypatch, mode, types, nvector):
    """coarse_grid_tree((1, 1, 3), 4): the z walls are regions one oct deep at level 1 and two octs deep at level 2 ... eight at
    level 4; reflexive, free and imposed regions, region after region, against the numpy loop; the rest of f does not move"""
    from ramses_amd import ic
    from ramses_amd._capi import check
    from test_gravana_checker import wall_regions
    if mode == "host_order":
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", "0")
    grid, L = (1, 1, 3), 4
    T = ic.coarse_grid_tree(grid, L)
    levels = tree_levels(T)
    xg = GC.tree_xg(T, grid)
    f = np.random.default_rng(7).normal(size=(3, T["ncell"]))
    grav = (2, (3.0, 0.02, 0.2, 0.3, 0.1), (0.0, 0.0, 1.0), 3.0)
    _load(gpu_lib, T, levels, xg, f, grid)
    _set(gpu_lib, *grav)
    try:
        for level in (1, 2, 4):
            regions = wall_regions(T, grid, level)
            before = f.copy()
            want = before.copy()
            for bt, octs in zip(types, regions):
                GC.boundary_force(want, T["son"], T["nbor"], T["ncoarse"], T["ngridmax"], bt, octs, nvector, grav, xg, 0.5 ** level)
            bt = np.array(types, np.int32)
            ng = np.array([len(r) for r in regions], np.int32)
            ig = np.ascontiguousarray(np.concatenate(regions), dtype=np.int32)
            check(gpu_lib.ramses_amd_amrres_boundary_force(2, vp(bt), vp(ng), vp(ig), nvector, 0.5 ** level))
            _fetch_f(gpu_lib, levels, f)
            assert _same_bits(f, want), (level, types, nvector)
            assert (f != before).any()
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


def test_a_corner_region_reads_what_an_earlier_region_wrote(gpu_lib):
    """two regions that share an edge: the octs of the second (a y wall) have their reference octs in the first (an x wall), so the
    second region must see the first one's NEW values -- a 2 x 2 block of octs in the x-y plane, oct 1 the corner"""
    from ramses_amd._capi import check
    # octs: 1 = corner (x wall AND y wall side), 2 = beyond the x wall only (region 1), 3 = beyond the y wall only, 4 = the box
    ncoarse = ngridmax = 4
    ncell = ncoarse + 8 * ngridmax
    son = np.zeros(ncell, np.int32)
    son[:4] = [1, 2, 3, 4]
    nbor = np.zeros((6, ngridmax), np.int32)
    # +x neighbour (index 1) and +y neighbour (index 3) as coarse cells; oct 1 -> +x is oct 3's cell?  layout: x: (1,3),(2,4); y: (1,2),(3,4)
    nbor[1] = [3, 4, 3, 4]
    nbor[0] = [1, 2, 1, 2]
    nbor[3] = [2, 2, 4, 4]
    nbor[2] = [1, 1, 3, 3]
    nbor[4] = nbor[5] = [1, 2, 3, 4]
    father = np.array([1, 2, 3, 4], np.int32)
    rng = np.random.default_rng(9)
    xg = np.ascontiguousarray(rng.uniform(0.1, 0.9, (3, ngridmax)))
    u = np.ones((5, ncell))
    everything = np.arange(1, 5, dtype=np.int32)
    _set(gpu_lib, 1, (0.3, -0.2, -1.7), (0, 0, 0), 1.0)
    try:
        for t1, t2 in ((1, 3), (11, 3), (1, 13)):
            f0 = rng.normal(size=(3, ncell))
            # region 1 (x low wall, reads towards +x): octs 1 and 2 read octs 3 and 4; region 2 (y low wall, towards +y): octs 1, 3 read 2, 4
            regions = [np.array([1, 2], np.int32), np.array([3, 1], np.int32)]
            want = f0.copy()
            GC.boundary_force(want, son, nbor, ncoarse, ngridmax, t1, regions[0], 32)
            mid = want.copy()
            GC.boundary_force(want, son, nbor, ncoarse, ngridmax, t2, regions[1], 32)
            stale = f0.copy()
            GC.boundary_force(stale, son, nbor, ncoarse, ngridmax, t2, regions[1], 32)
            c1 = np.concatenate([ncoarse + ind * ngridmax + np.array([0]) for ind in range(8)])          # the corner oct's cells
            assert not _same_bits(want[:, c1], stale[:, c1]) and not _same_bits(want[:, c1], mid[:, c1])
            got = f0.copy()
            check(gpu_lib.ramses_amd_amrres_invalidate())
            check(gpu_lib.ramses_amd_amrres_coarse_grid(1, 1, 1))
            check(gpu_lib.ramses_amd_amrres_load(5, ngridmax, ncoarse, vp(u), vp(son), vp(nbor), vp(father)))
            check(gpu_lib.ramses_amd_amrres_xg(vp(xg)))
            check(gpu_lib.ramses_amd_amrres_load_f(4, vp(everything), vp(got)))
            bt, ng = np.array([t1, t2], np.int32), np.array([2, 2], np.int32)
            ig = np.ascontiguousarray(np.concatenate(regions), dtype=np.int32)
            check(gpu_lib.ramses_amd_amrres_boundary_force(2, vp(bt), vp(ng), vp(ig), 32, 0.25))
            got[:] = np.nan
            check(gpu_lib.ramses_amd_amrres_sync_f(4, vp(everything), vp(got)))
            assert _same_bits(got[:, ncoarse:], want[:, ncoarse:]), (t1, t2)
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


# ---- f across a regrid: parked in the host's numbering, taken back or inherited from the father cell ---------------------------------

@pytest.mark.parametrize("L,order,device_order", CASES, ids=IDS)
def test_stash_and_restore_of_f(gpu_lib, monkeypatch, L, order, device_order):
    """ramses_amd_amrres_stash_f parks f of both levels; the device's copy is then overwritten (load_f of another array);
    ramses_amd_amrres_restore_f of level L, then of level L+1, with every third oct flagged to inherit: a flagged oct's eight cells
    hold its father cell's f as it is on the device at that moment (level L's fathers were never parked: the overwritten values;
    level L+1's fathers: level L after its own restore), every other oct what it parked; nothing else moves."""
    from ramses_amd._capi import check
    T, _, f0 = H.level_case(L, order)
    if device_order is not None:
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", device_order)
    levels = tree_levels(T)
    f = np.array(f0)
    _load(gpu_lib, T, levels, GC.tree_xg(T), f)
    try:
        for lev in (L, L + 1):
            ig = T["lists"][lev]["full"]
            check(gpu_lib.ramses_amd_amrres_stash_f(len(ig), vp(ig)))
        other = np.random.default_rng(21).normal(size=f.shape)
        for ig in levels.values():
            check(gpu_lib.ramses_amd_amrres_load_f(len(ig), vp(ig), vp(other)))
        want = other.copy()
        in_tree = np.zeros(T["ncell"], bool)
        for ig in levels.values():
            in_tree[H.oct_cells(T, ig)] = True
        want[:, ~in_tree] = f[:, ~in_tree]                       # (the fetch below writes the tree's cells only)
        for lev in (L, L + 1):
            ig = T["lists"][lev]["full"]
            inherit = np.ascontiguousarray((np.arange(len(ig)) % 3 == 0).astype(np.int32))
            g = ig.astype(np.int64)
            fc = T["father"][g - 1].astype(np.int64) - 1
            for ind in range(8):
                cells = T["ncoarse"] + ind * T["ngridmax"] + g - 1
                want[:, cells] = np.where(inherit[None, :] != 0, want[:, fc], f0[:, cells])
            check(gpu_lib.ramses_amd_amrres_restore_f(len(ig), vp(ig), vp(inherit)))
            got = f.copy()
            _fetch_f(gpu_lib, levels, got)
            assert _same_bits(got, want), "level %d" % lev
        check(gpu_lib.ramses_amd_amrres_stash_f(0, None))
        check(gpu_lib.ramses_amd_amrres_restore_f(0, None, None))
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()

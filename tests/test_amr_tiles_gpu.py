"""The device's own oct numbering (csrc/amr_layout.hpp: levels in tiles of 32 x 4 x 4 octs) and the dense sweep of AMR levels on
it (csrc/capi_amr.hip tile_level_sweep, csrc/hydro_sweep.hip MASK) against the C ORACLE of godfine1
(oracle/amr_godfine_oracle.c, itself pinned on the reference's dumps): hydro/godunov_fine.f90:486-911 -- interpolated ghost octs
(:563-626), fluxes reset at refined faces (:720-747), the update of unew (:752-790), the fluxes owed to the coarser level
(:798-908).  Everything goes through the C ABI with the HOST's oct numbers; what comes back must be the oracle's result bit for
bit whatever the device did with the numbering -- tiles, Z-order (tiles that do not fit), or none (RAMSES_AMD_DEVICE_ORDER=0)."""
import ctypes as C

import numpy as np
import pytest

import live
import resident as R
from helpers import mild_tree_state, shell_mask
from resident import vp

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _dense_sweep_on_small_levels_too(monkeypatch):
    R.force_tiles(monkeypatch, clear=())


def _oracle_step(oracle, po, T, L, uold, f, lists, ivar=0, itype=1):
    """set_unew on both levels, godunov_fine of level L+1 then L (the order of amr_step), set_uold"""
    unew = uold.copy()
    for level, igrid in ((L + 1, lists[L + 1]), (L, lists[L])):
        dx = 1.0 / 2 ** level
        oracle.godunov_fine_amr(po, igrid, T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew, dx, 0.02 * dx, 32,
                                ivar, itype, f=f)
    return unew


def _device_step(Lb, p, T, L, u, f, lists, ivar=0, itype=1, load=True):
    from ramses_amd._capi import check
    if load:
        R.load(Lb, T, u, f)
    for lev in (L, L + 1):
        ig = np.ascontiguousarray(T["all_octs"][lev])
        check(Lb.ramses_amd_amrres_set_unew(len(ig), vp(ig)))
    for lev in (L + 1, L):
        ig = np.ascontiguousarray(lists[lev])
        dx = 1.0 / 2 ** lev
        check(Lb.ramses_amd_amrres_godunov(C.byref(p), lev, len(ig), vp(ig), dx, 0.02 * dx, 32, ivar, itype))
    for lev in (L, L + 1):
        ig = np.ascontiguousarray(T["all_octs"][lev])
        check(Lb.ramses_amd_amrres_set_uold(C.byref(p), len(ig), vp(ig)))
        check(Lb.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(u)))
    return u


@pytest.mark.parametrize("order,riemann,slope,grav,interp", [("morton", "llf", 1, False, (0, 1)), ("scrambled", "hllc", 2, True, (1, 2)),
                                                             ("scrambled", "hll", 7, False, (2, 4)), ("morton", "acoustic", 8, True, (0, 3))])
def test_levels_in_tiles_equal_the_oracle(gpu_lib, oracle, monkeypatch, order, riemann, slope, grav, interp):
    """level 6 complete (64^3: 64 full tiles), level 7 in a spherical shell with refined cells on the periodic seam (tiles with free
    slots: ghost octs on both surfaces, fluxes owed to level-6 leaf cells): one amr_step's worth of calls == the oracle"""
    import ramses_amd
    L = 6
    mask = shell_mask(2 ** L)
    T = R.two_level_tree(L, order, mask, slack=260000)
    uold = mild_tree_state(T, 11)
    rng = np.random.default_rng(5)
    f = rng.normal(size=(3, T["ncell"])) if grav else None
    kw = dict(riemann=riemann, slope_type=slope)
    p, po = ramses_amd.make_params(**kw), oracle.make_params(**kw)
    lists = {L: T["igrid"], L + 1: T["igrid_fine"]}
    ref = _oracle_step(oracle, po, T, L, uold, f, lists, *interp)
    for var in ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE"):
        monkeypatch.delenv(var, raising=False)
    t0, w0 = gpu_lib.ramses_amd_amrres_tile_sweeps(), gpu_lib.ramses_amd_amrres_tree_sweeps()
    got = _device_step(gpu_lib, p, T, L, uold.copy(), f, lists, *interp)
    assert gpu_lib.ramses_amd_amrres_tiled_levels() == 2
    assert gpu_lib.ramses_amd_amrres_tile_sweeps() - t0 == 2 and gpu_lib.ramses_amd_amrres_tree_sweeps() == w0
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([T["igrid"], T["igrid_fine"]]) - 1 for ind in range(8)])
    assert np.array_equal(got[:, cells], ref[:, cells]), np.abs(got[:, cells] - ref[:, cells]).max()
    assert (ref[:, cells] != uold[:, cells]).any(0).mean() > 0.9
    gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("nvar,riemann,slope,grav,fast", [(7, "hllc", 1, False, False), (6, "llf", 2, True, False), (5, "exact", 1, False, False),
                                                          (7, "hll", 8, True, True), (5, "exact", 2, True, True),
                                                          (5, "hllc", 3, False, False), (7, "llf", 3, True, False), (5, "acoustic", 3, True, True),
                                                          (5, "plmde:llf", 1, False, False), (5, "plmde:hllc", 2, True, False),
                                                          (5, "plmde:hll", 3, False, False), (5, "plmde:llf", 7, True, True),
                                                          (5, "hllc", 1, False, True), (5, "hllc", 2, True, True)])     # (fast HLLC on tiles: round 6)
def test_passive_scalars_and_the_newton_solver_on_tiles(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, grav, fast):
    """Round 6 (missing #3): NVAR = 6 / 7 (passive scalars: interpolated in the ghost octs, in the flux records,
    in the replay), riemann = 'exact', slope_type = 3 (the 27-point slope: the surface pass gathers the 3 x 3 x 3 neighbourhoods
    of the two cells of an interface) and scheme = 'plmde' take the levels in tiles as well -- the kernels of 8 rows (256
    registers), the plan cut into work items of 4 rows.  Strict arithmetic: the oracle bit for bit (the Newton solver: <= 1e-12, its pow() is the device's), no sweep through the
    tree; fast arithmetic: <= 1e-12."""
    import ramses_amd
    L = 6
    mask = shell_mask(2 ** L)
    T = R.two_level_tree(L, "scrambled", mask, slack=260000)
    uold = mild_tree_state(T, 17, nvar=nvar)
    rng = np.random.default_rng(23)
    for n in range(5, nvar):
        uold[n, 1:] = uold[0, 1:] * rng.random(T["ncell"] - 1)          # passive scalars: density x a fraction in [0, 1)
        uold[n, 0] = uold[n, 1]
    f = rng.normal(size=(3, T["ncell"])) if grav else None
    scheme = "plmde" if riemann.startswith("plmde:") else "muscl"
    riemann = riemann.split(":")[-1]
    kw = dict(riemann=riemann, slope_type=slope, nvar=nvar, scheme=scheme)
    p, po = ramses_amd.make_params(fast_math=fast, **kw), oracle.make_params(**kw)
    lists = {L: T["igrid"], L + 1: T["igrid_fine"]}
    ref = _oracle_step(oracle, po, T, L, uold, f, lists, 1, 2)
    for var in ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE"):
        monkeypatch.delenv(var, raising=False)
    t0, w0 = gpu_lib.ramses_amd_amrres_tile_sweeps(), gpu_lib.ramses_amd_amrres_tree_sweeps()
    got = _device_step(gpu_lib, p, T, L, uold.copy(), f, lists, 1, 2)
    assert gpu_lib.ramses_amd_amrres_tiled_levels() == 2
    assert gpu_lib.ramses_amd_amrres_tile_sweeps() - t0 == 2 and gpu_lib.ramses_amd_amrres_tree_sweeps() == w0
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([T["igrid"], T["igrid_fine"]]) - 1 for ind in range(8)])
    if fast or riemann == "exact":        # ('exact' calls pow(): the device's libm differs from the host's in the last ulp, as on bricks)
        scale = np.abs(ref[:, cells]).max(axis=1, keepdims=True)
        assert (np.abs(got[:, cells] - ref[:, cells]) / scale).max() <= 1e-12
    else:
        assert np.array_equal(got[:, cells], ref[:, cells]), np.abs(got[:, cells] - ref[:, cells]).max()
    assert (ref[:, cells] != uold[:, cells]).any(0).mean() > 0.9
    gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("mode", ["host_order", "z_order", "no_room", "tree_walk_on_tiles"])
def test_every_numbering_gives_the_same_result(gpu_lib, oracle, monkeypatch, mode):
    """the switches of the layout: the host's numbering, Z-order without tiles, tiles that do not fit (ngridmax without slack: the
    partial level falls back to Z-order and the tree-walking sweep), tiles with the tree-walking sweep -- all == the oracle"""
    import ramses_amd
    L = 6
    mask = shell_mask(2 ** L, seam=False)
    T = R.two_level_tree(L, "scrambled", mask, slack=7 if mode == "no_room" else 260000)
    uold = mild_tree_state(T, 13)
    p, po = ramses_amd.make_params(riemann="llf", slope_type=1), oracle.make_params(riemann="llf", slope_type=1)
    lists = {L: T["igrid"], L + 1: T["igrid_fine"]}
    ref = _oracle_step(oracle, po, T, L, uold, None, lists)
    for var in ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE"):
        monkeypatch.delenv(var, raising=False)
    if mode == "host_order":
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", "0")
    if mode == "z_order":
        monkeypatch.setenv("RAMSES_AMD_TILES", "0")
    if mode == "tree_walk_on_tiles":
        monkeypatch.setenv("RAMSES_AMD_TILE_DENSE", "0")
        monkeypatch.setenv("RAMSES_AMD_COVERED_DENSE", "0")
    t0, w0 = gpu_lib.ramses_amd_amrres_tile_sweeps(), gpu_lib.ramses_amd_amrres_tree_sweeps()
    got = _device_step(gpu_lib, p, T, L, uold.copy(), None, lists)
    tiled = gpu_lib.ramses_amd_amrres_tiled_levels()
    dt, dw = gpu_lib.ramses_amd_amrres_tile_sweeps() - t0, gpu_lib.ramses_amd_amrres_tree_sweeps() - w0
    assert (tiled, dt, dw) == {"host_order": (0, 0, 2), "z_order": (0, 0, 2), "no_room": (1, 1, 1), "tree_walk_on_tiles": (2, 0, 2)}[mode]
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([T["igrid"], T["igrid_fine"]]) - 1 for ind in range(8)])
    assert np.array_equal(got[:, cells], ref[:, cells]), np.abs(got[:, cells] - ref[:, cells]).max()
    gpu_lib.ramses_amd_amrres_invalidate()


def test_a_list_that_is_part_of_the_level(gpu_lib, oracle, monkeypatch):
    """several ranks: the call's list holds the rank's own octs, the other octs of the level are there (virtual octs, filled by
    the exchange) but are not updated, and a face between an own and a virtual oct owes nothing to the coarser level"""
    import ramses_amd
    L = 6
    nc = 2 ** L
    mask = shell_mask(nc)
    T = R.two_level_tree(L, "scrambled", mask, slack=260000)
    uold = mild_tree_state(T, 17)
    p, po = ramses_amd.make_params(riemann="hllc", slope_type=1), oracle.make_params(riemann="hllc", slope_type=1)
    # own = a fixed subset of each level (by the index of the father cell): the oracle sees the same lists
    fcL, fcF = T["father"][T["igrid"] - 1].astype(np.int64), T["father"][T["igrid_fine"] - 1].astype(np.int64)
    own = {L: np.ascontiguousarray(T["igrid"][(fcL % 3) != 0]), L + 1: np.ascontiguousarray(T["igrid_fine"][(fcF % 5) < 3])}
    assert 0 < len(own[L]) < len(T["igrid"]) and 0 < len(own[L + 1]) < len(T["igrid_fine"])
    ref = _oracle_step(oracle, po, T, L, uold, None, own)
    for var in ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE"):
        monkeypatch.delenv(var, raising=False)
    t0 = gpu_lib.ramses_amd_amrres_tile_sweeps()
    got = _device_step(gpu_lib, p, T, L, uold.copy(), None, own)
    assert gpu_lib.ramses_amd_amrres_tile_sweeps() - t0 == 2
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([T["igrid"], T["igrid_fine"]]) - 1 for ind in range(8)])
    assert np.array_equal(got[:, cells], ref[:, cells]), np.abs(got[:, cells] - ref[:, cells]).max()
    gpu_lib.ramses_amd_amrres_invalidate()


def test_a_regrid_keeps_the_levels_that_did_not_change(gpu_lib, oracle, monkeypatch):
    """refine_fine's hook in small: after a step the finer level is rebuilt on the host (another set of octs, other host indices),
    the tree goes down again and ONLY the rebuilt level is reloaded; level L stays where it was on the device with the state the
    first step left there.  Two steps on the device == two steps of the oracle on the host arrays."""
    import ramses_amd
    from ramses_amd._capi import check
    L = 6
    nc = 2 ** L
    m1 = shell_mask(nc, 0.23, 0.36)
    m2 = shell_mask(nc, 0.15, 0.30, seam=False)
    n1, n2 = int(m1.sum()), int(m2.sum())
    T1 = R.two_level_tree(L, "morton", m1, slack=260000 + max(n1, n2) - n1)
    T2 = R.two_level_tree(L, "morton", m2, slack=260000 + max(n1, n2) - n2)
    assert T1["ngridmax"] == T2["ngridmax"] and np.array_equal(T1["igrid"], T2["igrid"])
    p, po = ramses_amd.make_params(riemann="llf", slope_type=2), oracle.make_params(riemann="llf", slope_type=2)
    for var in ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE"):
        monkeypatch.delenv(var, raising=False)
    u0 = mild_tree_state(T1, 19)
    # oracle: step 1 on tree 1; the new finer octs take their father cell's state (times a factor per octant); step 2 on tree 2
    l1 = {L: T1["igrid"], L + 1: T1["igrid_fine"]}
    l2 = {L: T2["igrid"], L + 1: T2["igrid_fine"]}
    h1 = _oracle_step(oracle, po, T1, L, u0, None, l1)

    def refill(u):
        # what refine_fine leaves on the host for the rebuilt level: interpolated from the (synced) coarser level
        v = u.copy()
        for ind in range(8):
            c = T2["ncoarse"] + ind * T2["ngridmax"] + T2["igrid_fine"] - 1
            v[:, c] = u[:, T2["father"][T2["igrid_fine"] - 1] - 1] * (1.0 + 0.01 * (ind - 3.5))
        return v
    h1r = refill(h1)
    h2 = _oracle_step(oracle, po, T2, L, h1r, None, l2)
    # device: step 1, level L back to the host (refine_fine reads it), new tree, ONLY level L+1 reloaded, step 2
    u = _device_step(gpu_lib, p, T1, L, u0.copy(), None, l1)
    u[:] = refill(u)                     # (the same host array all along: the one the state was loaded from)
    c_l = np.concatenate([T2["ncoarse"] + ind * T2["ngridmax"] + T2["igrid"] - 1 for ind in range(8)])
    u[:, c_l] = -7.0                     # if the device read level L from the host again, the result would show it
    check(gpu_lib.ramses_amd_amrres_tree(vp(T2["son"]), vp(T2["nbor"]), vp(T2["father"])))
    assert gpu_lib.ramses_amd_amrres_first_changed() == L + 1      # what the caller has to send again: level L + 1, nothing coarser
    igf = np.ascontiguousarray(np.sort(T2["igrid_fine"]))
    check(gpu_lib.ramses_amd_amrres_load_level(len(igf), vp(igf), vp(u)))
    t0 = gpu_lib.ramses_amd_amrres_tile_sweeps()
    got = _device_step(gpu_lib, p, T2, L, u, None, l2, load=False)
    assert gpu_lib.ramses_amd_amrres_tile_sweeps() - t0 == 2
    cells = np.concatenate([T2["ncoarse"] + ind * T2["ngridmax"] + np.concatenate([T2["igrid"], T2["igrid_fine"]]) - 1 for ind in range(8)])
    assert np.array_equal(got[:, cells], h2[:, cells]), np.abs(got[:, cells] - h2[:, cells]).max()
    gpu_lib.ramses_amd_amrres_invalidate()


def test_flagged_cells_come_back_in_host_numbers(gpu_lib, monkeypatch):
    """hydro_flag's compact list crosses the interface the other way: device cell indices -> the host's"""
    import ramses_amd
    from ramses_amd._capi import check
    L = 6
    T = R.two_level_tree(L, "scrambled", shell_mask(2 ** L, seam=False), slack=260000)
    u = mild_tree_state(T, 23)
    p = ramses_amd.make_params()
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", mode)
        check(gpu_lib.ramses_amd_amrres_invalidate())
        check(gpu_lib.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
        ig = np.ascontiguousarray(T["igrid_fine"])
        cells = np.zeros(8 * len(ig), np.int32)
        n = C.c_int(0)
        check(gpu_lib.ramses_amd_amrres_hydro_flag(C.byref(p), len(ig), vp(ig), 0.3, -1.0, -1.0, 1e-10, 1e-10, 1e-10, vp(cells), C.byref(n)))
        out[mode] = cells[:n.value].copy()
        v = np.zeros_like(u)
        v[:] = u
        check(gpu_lib.ramses_amd_amrres_sync_all(vp(u)))
        assert np.array_equal(u, v)
    assert len(out["0"]) > 100 and np.array_equal(out["0"], out["1"])
    gpu_lib.ramses_amd_amrres_invalidate()


def test_a_regrid_whose_finer_level_outgrows_the_room_the_kept_tiles_left(gpu_lib, oracle, monkeypatch):
    """a level in tiles keeps its layout -- free tile slots included -- across a regrid of the finer levels;
    its fit was checked against the finer levels of THAT moment.  Here level 8 grows sevenfold between two steps: the tree still
    fits into ngridmax, but not behind the 97 000 free slots of level 7's tiles.  ramses_amd_amrres_tree must not fail: it parks the
    kept levels' state (which lives on the device only), lays every level out again and puts the state back
    (ramses_amd_amrres_relayouts counts it); two steps on the device == two steps of the oracle, with level 6 and 7 never re-sent."""
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd._capi import check
    L = 6
    nc = 2 ** L

    def shell(n, lo, hi):
        z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
        r = np.sqrt((x - n / 2 + 0.5) ** 2 + (y - n / 2 + 0.5) ** 2 + (z - n / 2 + 0.5) ** 2)
        return (r >= lo * n) & (r <= hi * n)
    m1 = shell(nc, 0.23, 0.36)
    m2a, m2b = shell(2 * nc, 0.29, 0.30), shell(2 * nc, 0.26, 0.33)
    base = sum(8 ** (l - 1) for l in range(1, L + 1))
    ngm = base + int(m1.sum()) + int(m2b.sum()) + 10                    # the second tree fills ngridmax to ten octs
    T1 = ic.uniform_tree(L, order="morton", refine_mask=m1, refine_mask2=m2a, slack=ngm - base - int(m1.sum()) - int(m2a.sum()))
    T2 = ic.uniform_tree(L, order="morton", refine_mask=m1, refine_mask2=m2b, slack=10)
    assert T1["ngridmax"] == T2["ngridmax"] == ngm
    assert np.array_equal(T1["igrid"], T2["igrid"]) and np.array_equal(T1["igrid_fine"], T2["igrid_fine"])
    p, po = ramses_amd.make_params(riemann="hllc", slope_type=1), oracle.make_params(riemann="hllc", slope_type=1)
    for var in ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE", "RAMSES_AMD_DEVICE_OCTS"):
        monkeypatch.delenv(var, raising=False)
    levels = (L, L + 1, L + 2)

    def lists(T):
        return {L: np.ascontiguousarray(np.sort(T["igrid"])), L + 1: np.ascontiguousarray(np.sort(T["igrid_fine"])),
                L + 2: np.ascontiguousarray(np.sort(T["igrid_fine2"]))}

    def oracle_step(T, uold):
        unew = uold.copy()
        for lev in reversed(levels):
            dx = 1.0 / 2 ** lev
            oracle.godunov_fine_amr(po, lists(T)[lev], T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew, dx, 0.02 * dx, 32, 0, 1, f=None)
        return unew

    def device_step(T, u):
        ll = lists(T)
        for lev in levels:
            check(gpu_lib.ramses_amd_amrres_set_unew(len(ll[lev]), vp(ll[lev])))
        for lev in reversed(levels):
            dx = 1.0 / 2 ** lev
            check(gpu_lib.ramses_amd_amrres_godunov(C.byref(p), lev, len(ll[lev]), vp(ll[lev]), dx, 0.02 * dx, 32, 0, 1))
        for lev in levels:
            check(gpu_lib.ramses_amd_amrres_set_uold(C.byref(p), len(ll[lev]), vp(ll[lev])))
            check(gpu_lib.ramses_amd_amrres_sync_level(len(ll[lev]), vp(ll[lev]), vp(u)))
        return u

    def refill(T, u):
        v = u.copy()
        ig = T["igrid_fine2"]
        for ind in range(8):
            c = T["ncoarse"] + ind * T["ngridmax"] + ig - 1
            v[:, c] = u[:, T["father"][ig - 1] - 1] * (1.0 + 0.01 * (ind - 3.5))
        return v
    u0 = mild_tree_state(T1, 29)
    h1 = oracle_step(T1, u0)
    h2 = oracle_step(T2, refill(T2, h1))
    u = u0.copy()
    check(gpu_lib.ramses_amd_amrres_invalidate())
    check(gpu_lib.ramses_amd_amrres_load(5, T1["ngridmax"], T1["ncoarse"], vp(u), vp(T1["son"]), vp(T1["nbor"]), vp(T1["father"])))
    assert gpu_lib.ramses_amd_amrres_tiled_levels() >= 2          # level 6 and the shell of level 7 live in tiles
    u = device_step(T1, u)
    u[:] = refill(T2, u)
    for lev, ig in ((L, T2["igrid"]), (L + 1, T2["igrid_fine"])):
        c = np.concatenate([T2["ncoarse"] + ind * T2["ngridmax"] + ig - 1 for ind in range(8)])
        u[:, c] = -7.0                     # if the device read these levels from the host again, the result would show it
    before = gpu_lib.ramses_amd_amrres_relayouts()
    check(gpu_lib.ramses_amd_amrres_tree(vp(T2["son"]), vp(T2["nbor"]), vp(T2["father"])))
    assert gpu_lib.ramses_amd_amrres_relayouts() - before == 1
    ig8 = lists(T2)[L + 2]
    check(gpu_lib.ramses_amd_amrres_load_level(len(ig8), vp(ig8), vp(u)))
    got = device_step(T2, u)
    cells = np.concatenate([T2["ncoarse"] + ind * T2["ngridmax"] + np.concatenate([T2["igrid"], T2["igrid_fine"], T2["igrid_fine2"]]) - 1 for ind in range(8)])
    assert np.array_equal(got[:, cells], h2[:, cells]), np.abs(got[:, cells] - h2[:, cells]).max()
    gpu_lib.ramses_amd_amrres_invalidate()


def test_patched_program_with_passive_scalars_sweeps_its_levels_in_tiles(gpu_lib, monkeypatch):
    """Live A/B of the NVAR = 7 build: the patched program (oracle/_ref/ramses3d_patch_v7, strict arithmetic, tiles forced for the
    small levels of the test) against the untouched NVAR = 7 reference (oracle/_ref/ramses3d_v7) on a point explosion next to a
    dense block carrying two scalars, levels 6-7, sub-cycling, regrids -- leaf cell by leaf cell, all seven variables bit for
    bit, and no sweep of a level through the tree (the exit line of RAMSES_AMD_STATS=1)."""
    import os
    import shutil
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    patched, ref = (os.path.join(root, "oracle", "_ref", b) for b in ("ramses3d_patch_v7", "ramses3d_v7"))
    if not (os.path.exists(patched) and os.path.exists(ref)):
        pytest.skip("oracle/_ref/ramses3d[_patch]_v7 not built")
    from oracle import ramses_snapshot as rs
    nml = live.golden_module("amr").v7_namelist().replace("levelmin=3", "levelmin=6").replace("levelmax=5", "levelmax=7").replace("ngridtot=8000 !", "ngridtot=400000 !")
    nml = nml.replace("nsubcycle=1,1,2,2", "nsubcycle=1,1,1,1,1,2,2")
    assert "levelmin=6" in nml and "levelmax=7" in nml and "ngridtot=400000" in nml

    for k, v in (("RAMSES_AMD", "1"), ("RAMSES_AMD_STRICT", "1"), ("RAMSES_AMD_STATS", "1"), ("RAMSES_AMD_TILE_MIN_OCTS", "0")):
        monkeypatch.setenv(k, v)
    work, out = rs.run_reference(nml, binary=patched)
    try:
        got = live.leaves(work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    tiles, tree = live.sweep_counts(out)
    assert tiles >= 10 and tree == 0, (tiles, tree)
    monkeypatch.setenv("RAMSES_AMD", "0")
    work, _ = rs.run_reference(nml, binary=ref)
    try:
        want = live.leaves(work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert got.prim.shape[0] == 7 and (want.level == 7).sum() > 1000
    assert np.array_equal(got.level, want.level)
    assert np.array_equal(got.prim, want.prim), np.abs(got.prim - want.prim).max()

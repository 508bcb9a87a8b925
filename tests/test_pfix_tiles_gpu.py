"""pressure_fix on AMR levels in tiles: divu / enew through the dense sweep (csrc/hydro_sweep.hip godunov_sweep_pfix_kernel, the
surface pass surface_flux_pfix_kernel, the replay tile_coarse_update_kernel; csrc/capi_amr.hip tile_level_sweep) against the C
ORACLE of godfine1 (oracle/amr_godfine_oracle.c, itself pinned on the reference's dumps by tests/test_amr_oracle.py):
hydro/godunov_fine.f90:720-747 (the two face quantities reset at refined interfaces), :752-790 (divu / enew of the updated cells,
ADDED to what the vectors hold), :798-908 (what the level owes to the leaf cells of the coarser one).  Built like
tests/test_amr_tiles_gpu.py: level 6 complete, level 7 a spherical shell with refined cells on the periodic seam, both in tiles."""
import ctypes as C

import numpy as np
import pytest

import live
import resident as R
from helpers import mild_tree_state, oct_cells

pytestmark = pytest.mark.gpu
L = 6


@pytest.fixture(autouse=True)
def _dense_sweep_on_small_levels_too(monkeypatch):
    R.force_tiles(monkeypatch)


def _tree(order):
    return R.two_level_tree(L, order)


def _cells(T, lev):
    return oct_cells(T, T["lists"][lev])


def _load(Lb, p, T, u, f):
    """load, enable_pfix, set_unew_pfix on both levels; returns the device's divu / enew after it (host vectors)"""
    R.load(Lb, T, u, f, pfix=True)
    return R.set_unew(Lb, p, T, pfix=True)


CASES = [
    # nvar, riemann, slope, gravity, oct order, (interpol_var, interpol_type), fast_math
    (5, "hllc", 1, False, "scrambled", (0, 1), False),
    (6, "llf", 2, True, "morton", (1, 2), False),
    (7, "hll", 7, False, "scrambled", (2, 4), False),
    (5, "acoustic", 8, True, "morton", (0, 3), False),
    (5, "exact", 1, False, "scrambled", (1, 2), False),
    (5, "hllc", 3, False, "morton", (0, 1), False),
    (6, "hll", 3, True, "scrambled", (1, 0), False),
    (7, "llf", 3, True, "scrambled", (1, 2), False),           # (the 6-row kernel: NVAR = 7 with the 27-point slope)
    (7, "exact", 2, True, "morton", (0, 1), False),
    (5, "hllc", 2, True, "scrambled", (1, 2), True),            # fast_math: a pressure_fix level is swept in strict arithmetic
    (7, "acoustic", 1, False, "morton", (2, 3), True),
]


@pytest.mark.parametrize("nvar,riemann,slope,grav,order,interp,fast", CASES)
def test_pressure_fix_levels_in_tiles_equal_the_oracle(gpu_lib, oracle, nvar, riemann, slope, grav, order, interp, fast):
    """godunov_fine of level 7 and of level 6 with pressure_fix: unew, divu and enew of every cell of both levels == the oracle's,
    which starts from the vectors the device holds after set_unew; both calls through the dense kernel on tiles (on the parent
    commit both walked the tree: that assertion failed there)"""
    import ramses_amd
    T = _tree(order)
    uold = mild_tree_state(T, 11, nvar=nvar)
    f = np.random.default_rng(5).normal(size=(3, T["ncell"])) if grav else None
    kw = dict(riemann=riemann, slope_type=slope, nvar=nvar)
    p, po = ramses_amd.make_params(fast_math=fast, **kw), oracle.make_params(**kw)
    u = uold.copy()
    divu0, enew0 = _load(gpu_lib, p, T, u, f)
    assert gpu_lib.ramses_amd_amrres_tiled_levels() == 2
    divu, enew = divu0.copy(), enew0.copy()
    unew = R.oracle_step(oracle, po, T, uold, f, interp, divu, enew)
    counts = R.sweep_levels(gpu_lib, p, T, interp)
    got = R.read_back(gpu_lib, p, T, u, pfix=True)
    gpu_lib.ramses_amd_amrres_invalidate()
    assert counts == (2, 0), "sweeps through the tiles / through the tree: %d / %d" % counts
    c7, c6 = _cells(T, L + 1), _cells(T, L)
    # not vacuous (from the oracle alone): the vectors are populated; refined level-6 cells keep 0 (their interfaces are reset)
    assert (divu[c7] != 0).mean() > 0.9 and (divu[c6] != 0).mean() > 0.7
    assert (enew[c7] != enew0[c7]).mean() > 0.9
    R.compare(got, (unew, divu, enew), np.concatenate([c6, c7]), riemann == "exact")


def test_the_oracle_case_is_not_vacuous(gpu_lib, oracle):
    """From the oracle alone: the level-7 call by itself changes divu and enew of more than 1000 level-6 leaf cells (the coarse
    corrections), and level 6's vectors differ there between "level 7 then 6" and "level 6 alone" -- a kernel that overwrites
    instead of accumulating cannot equal the oracle.  Then the device, on the same case, cell by cell in those cells."""
    import ramses_amd
    T = _tree("scrambled")
    uold = mild_tree_state(T, 11)
    kw = dict(riemann="hllc", slope_type=1)
    p, po = ramses_amd.make_params(**kw), oracle.make_params(**kw)
    u = uold.copy()
    divu0, enew0 = _load(gpu_lib, p, T, u, None)
    c7, c6 = _cells(T, L + 1), _cells(T, L)
    leaf6 = c6[T["son"][c6] == 0]
    # level 7 alone
    u7, d7, e7 = uold.copy(), divu0.copy(), enew0.copy()
    R.oracle_sweep(oracle, po, T, L + 1, uold, u7, 0, 1, divu=d7, enew=e7)
    corrected = leaf6[(d7[leaf6] != divu0[leaf6]) & (e7[leaf6] != enew0[leaf6])]
    print("level-6 leaf cells corrected by the level-7 call:", len(corrected))
    assert len(corrected) > 1000
    # 7 then 6 against 6 alone
    u76, d76, e76 = u7.copy(), d7.copy(), e7.copy()
    R.oracle_sweep(oracle, po, T, L, uold, u76, 0, 1, divu=d76, enew=e76)
    u6, d6, e6 = uold.copy(), divu0.copy(), enew0.copy()
    R.oracle_sweep(oracle, po, T, L, uold, u6, 0, 1, divu=d6, enew=e6)
    differ = (d76[corrected] != d6[corrected]) & (e76[corrected] != e6[corrected])
    print("of them order-dependent:", int(differ.sum()))
    assert differ.sum() > 1000
    print("divu != 0: level 7 %.4f, level 6 %.4f" % ((d76[c7] != 0).mean(), (d76[c6] != 0).mean()))
    assert (d76[c7] != 0).mean() > 0.9 and (d76[c6] != 0).mean() > 0.7
    R.sweep_levels(gpu_lib, p, T, (0, 1))
    got = R.read_back(gpu_lib, p, T, u, pfix=True)
    gpu_lib.ramses_amd_amrres_invalidate()
    R.compare(got, (u76, d76, e76), corrected, False)
    R.compare(got, (u76, d76, e76), np.concatenate([c6, c7]), False)


def _cold_supersonic_state(T, seed):
    """the random state with a cold, supersonic region (thermal energy 1e-6 of the kinetic): where set_uold's energy switch fires"""
    u = mild_tree_state(T, seed)
    n = T["ncell"]
    cold = np.zeros(n, bool)
    cold[1:] = np.random.default_rng(seed + 1).random(n - 1) < 0.3
    ekin = 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0]
    u[1:4, cold] *= 20.0
    ekin = 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0]
    u[4, cold] = ekin[cold] * (1.0 + 1e-6)
    return u


def _two_steps(Lb, p, T, u0, beta_fix, tile_sweep, monkeypatch):
    from ramses_amd._capi import check
    if tile_sweep:
        monkeypatch.delenv("RAMSES_AMD_TILE_SWEEP", raising=False)
    else:
        monkeypatch.setenv("RAMSES_AMD_TILE_SWEEP", "0")
    u = u0.copy()
    _load(Lb, p, T, u, None)
    t0, w0 = Lb.ramses_amd_amrres_tile_sweeps(), Lb.ramses_amd_amrres_tree_sweeps()
    dtfac = 0.002
    for step in range(2):
        if step:
            R.set_unew(Lb, p, T, pfix=True)
        R.sweep_levels(Lb, p, T, (0, 1), dtfac)
        for lev in (L, L + 1):
            ig = T["all_octs"][lev]
            dx = 1.0 / 2 ** lev
            check(Lb.ramses_amd_amrres_set_uold_pfix(C.byref(p), len(ig), R.vp(ig), dtfac * dx, dx, beta_fix, 0.0))
    R.sync(Lb, T, u)
    counts = (Lb.ramses_amd_amrres_tile_sweeps() - t0, Lb.ramses_amd_amrres_tree_sweeps() - w0)
    Lb.ramses_amd_amrres_invalidate()
    monkeypatch.delenv("RAMSES_AMD_TILE_SWEEP", raising=False)
    return u, counts


def test_two_steps_with_the_energy_switch_equal_the_tree_walker(gpu_lib, monkeypatch):
    """set_unew_pfix, the sweeps of level 7 and 6, set_uold_pfix (pdV term and the energy switch, beta_fix = 0.5), twice, on a state
    with a cold supersonic region: the levels on tiles == the same calls with RAMSES_AMD_TILE_SWEEP=0 (the tree-walking sweep,
    pinned against the reference program by the live tests), bit for bit.  The switch fires: on the tree-walking path the energy
    differs from a run with beta_fix = 0 (where e_cons < 0 alone could trigger it)."""
    import ramses_amd
    T = _tree("scrambled")
    u0 = _cold_supersonic_state(T, 31)
    p = ramses_amd.make_params(riemann="hllc", slope_type=1)
    tree, ctree = _two_steps(gpu_lib, p, T, u0, 0.5, False, monkeypatch)
    assert ctree == (0, 4), ctree
    noswitch, _ = _two_steps(gpu_lib, p, T, u0, 0.0, False, monkeypatch)
    cells = np.concatenate([_cells(T, L), _cells(T, L + 1)])
    fired = int((tree[4, cells] != noswitch[4, cells]).sum())
    print("cells whose energy the switch changed (tree-walking path):", fired)
    assert fired > 0
    tiles, ctiles = _two_steps(gpu_lib, p, T, u0, 0.5, True, monkeypatch)
    assert ctiles == (4, 0), ctiles
    assert np.isfinite(tree[:, cells]).all()
    assert np.array_equal(tiles[:, cells], tree[:, cells]), np.abs(tiles[:, cells] - tree[:, cells]).max()


def test_sync_pfix_is_refused_before_pressure_fix_is_enabled(gpu_lib):
    import ramses_amd
    from ramses_amd._capi import check
    T = _tree("morton")
    u = mild_tree_state(T, 3)
    check(gpu_lib.ramses_amd_amrres_invalidate())
    check(gpu_lib.ramses_amd_amrres_load(5, T["ngridmax"], T["ncoarse"], R.vp(u), R.vp(T["son"]), R.vp(T["nbor"]), R.vp(T["father"])))
    ig = T["all_octs"][L]
    divu, enew = np.zeros(T["ncell"]), np.zeros(T["ncell"])
    rc = gpu_lib.ramses_amd_amrres_sync_pfix(len(ig), R.vp(ig), R.vp(divu), R.vp(enew))
    assert rc == -1 and b"pressure_fix not enabled" in gpu_lib.ramses_amd_last_error()
    gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("what", ["plmde", "difmag"])
def test_what_stays_on_the_tree_walker(gpu_lib, oracle, what):
    """scheme = 'plmde' with pressure_fix (the tree walker's single-oct kernel) and difmag > 0 with pressure_fix: swept through the
    tree, results equal the oracle"""
    import ramses_amd
    T = _tree("scrambled")
    uold = mild_tree_state(T, 11)
    kw = dict(riemann="llf", slope_type=1)
    kw.update({"scheme": "plmde"} if what == "plmde" else {"difmag": 0.05})
    p, po = ramses_amd.make_params(**kw), oracle.make_params(**kw)
    u = uold.copy()
    divu0, enew0 = _load(gpu_lib, p, T, u, None)
    divu, enew = divu0.copy(), enew0.copy()
    unew = R.oracle_step(oracle, po, T, uold, None, (0, 1), divu, enew)
    counts = R.sweep_levels(gpu_lib, p, T, (0, 1))
    got = R.read_back(gpu_lib, p, T, u, pfix=True)
    gpu_lib.ramses_amd_amrres_invalidate()
    assert counts == (0, 2), counts
    R.compare(got, (unew, divu, enew), np.concatenate([_cells(T, L), _cells(T, L + 1)]), False)


# ---- live, end to end: the patched program against the untouched one -------------------------------------------------------

def _namelist(lmin, lmax, riemann="hllc", nstep=4, poisson=False, ngridtot=400000):
    riemann = riemann + "'\npressure_fix=.true.\nbeta_fix=0.5\n!'"
    nml = live.amr_namelist(lmin, lmax, nstep, riemann, 1, "1,1,1,1,1,2,2", ngridtot, poisson=poisson)
    assert "pressure_fix=.true." in nml
    return nml


def _live(nml, nproc, env, min_octs="0"):
    return live.ab(nml, nproc, dict({"RAMSES_AMD_STRICT": "1", "RAMSES_AMD_STATS": "1"}, **env), ref_env={"RAMSES_AMD": "0"}, min_octs=min_octs)


@pytest.mark.parametrize("nproc,poisson", [(1, False), (2, False), (1, True)], ids=["1rank", "2ranks", "self-gravity"])
def test_patched_program_with_pressure_fix_sweeps_its_levels_in_tiles(gpu_lib, nproc, poisson):
    """sedov3d, levels 6-7, pressure_fix with beta_fix = 0.5, strict arithmetic, tiles forced for the small levels: the leaf cells
    of the last snapshot bit-identical to the unpatched program, every sweep of a level through the dense kernel on tiles"""
    out, want = _live(_namelist(6, 7, poisson=poisson), nproc, {})
    assert "AMR levels stay resident on the GPU" in out, out[-3000:]
    assert (want.level == 7).sum() >= 64, "the run must have refined (eight octs of level 7 at least)"
    tiles, tree = live.sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)


def test_a_uniform_64_cubed_level_with_pressure_fix_takes_the_tiles_at_the_production_threshold(gpu_lib):
    """no override of RAMSES_AMD_TILE_MIN_OCTS: a uniform 64^3 level (32768 octs, the production crossover) with pressure_fix"""
    out, _ = _live(_namelist(6, 6, nstep=3, ngridtot=80000), 1, {}, min_octs=None)
    tiles, tree = live.sweep_counts(out)
    assert tiles > 0, (tiles, tree)


def test_default_arithmetic_run_with_pressure_fix_is_bit_identical_and_says_so(gpu_lib):
    """no RAMSES_AMD_STRICT: the program's default (fast) arithmetic sweeps pressure_fix levels in strict arithmetic"""
    out, _ = _live(_namelist(6, 7), 1, {"RAMSES_AMD_STRICT": None})
    assert "dense sweep arithmetic = fast" in out, out[-3000:]
    assert "pressure_fix: AMR levels in tiles are swept in strict arithmetic" in out, out[-3000:]
    tiles, tree = live.sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)

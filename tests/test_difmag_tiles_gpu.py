"""difmag > 0 on AMR levels in tiles: cmpdivu / consup (hydro/uplmde.f90:702-866) through the dense sweep (csrc/difmag_core.hpp;
csrc/hydro_sweep.hip godunov_sweep_difmag_kernel, the surface pass surface_flux_difmag_kernel; csrc/capi_amr.hip tile_level_sweep)
against the C ORACLE of godfine1 with the same difmag (oracle/amr_godfine_oracle.c over oracle/hydro_oracle.c ora_cmpdivu /
ora_consup, pinned on the reference's dumps), against the tree-walking sweep (the second implementation on the device) and,
live, against the unpatched program.  Built like tests/test_pfix_tiles_gpu.py: level 6 complete, level 7 a spherical shell with
refined cells on the periodic seam, both in tiles; dt = 0.02 dx."""
import numpy as np
import pytest

import live
import resident as R
from helpers import mild_tree_state, oct_cells

pytestmark = pytest.mark.gpu
L = 6


@pytest.fixture(autouse=True)
def _dense_sweep_on_small_levels_too(monkeypatch):
    R.force_tiles(monkeypatch, RAMSES_AMD_DIFMAG_TILES="1")        # (difmag on tiles is opt-in until it is measured: the tests ask for it)


def _tree(order):
    return R.two_level_tree(L, order)


def _cells(T, lev):
    return oct_cells(T, T["lists"][lev])


def _amr_step(Lb, p, T, u, f, interp):
    """set_unew, godunov of level 7 then 6, set_uold, sync_level; returns the state and (tile sweeps, tree sweeps)"""
    R.load(Lb, T, u, f)
    R.set_unew(Lb, p, T)
    counts = R.sweep_levels(Lb, p, T, interp)
    R.set_uold(Lb, p, T)
    got = R.sync(Lb, T, u)
    Lb.ramses_amd_amrres_invalidate()
    return got, counts


CASES = [
    # nvar, riemann, slope, gravity, oct order, (interpol_var, interpol_type), fast_math, difmag
    (5, "llf", 1, False, "scrambled", (0, 1), False, 0.1),
    (5, "hllc", 2, True, "morton", (1, 2), False, 0.1),
    (6, "hll", 7, False, "scrambled", (2, 4), False, 0.05),
    (6, "acoustic", 8, True, "morton", (0, 3), False, 0.1),
    (7, "llf", 1, True, "scrambled", (1, 2), False, 0.05),
    (7, "hllc", 3, True, "morton", (1, 0), False, 0.1),          # NVAR = 7 with the 27-point slope
    (5, "exact", 1, False, "scrambled", (1, 2), False, 0.1),
    (6, "exact", 2, True, "morton", (0, 1), False, 0.1),
    (5, "hll", 3, False, "morton", (0, 1), False, 0.2),
    (7, "acoustic", 2, False, "scrambled", (2, 3), False, 0.1),
    (5, "hllc", 1, True, "scrambled", (1, 2), True, 0.1),        # fast_math: a difmag level is swept in strict arithmetic
    (7, "hll", 8, False, "morton", (0, 1), True, 0.1),
]


@pytest.mark.parametrize("nvar,riemann,slope,grav,order,interp,fast,difmag", CASES)
def test_difmag_levels_in_tiles_equal_the_oracle(gpu_lib, oracle, nvar, riemann, slope, grav, order, interp, fast, difmag):
    """One amr_step's worth of calls with difmag > 0: every cell of both levels == the oracle's with the same difmag; both sweeps
    through the dense kernel on tiles (on the parent commit both walked the tree: that assertion failed there)"""
    import ramses_amd
    T = _tree(order)
    uold = mild_tree_state(T, 11, nvar=nvar)
    f = np.random.default_rng(5).normal(size=(3, T["ncell"])) if grav else None
    kw = dict(riemann=riemann, slope_type=slope, nvar=nvar, difmag=difmag)
    p, po = ramses_amd.make_params(fast_math=fast, **kw), oracle.make_params(**kw)
    want = R.oracle_step(oracle, po, T, uold, f, interp)
    got, counts = _amr_step(gpu_lib, p, T, uold.copy(), f, interp)
    assert counts == (2, 0), "sweeps through the tiles / through the tree: %d / %d" % counts
    c7, c6 = _cells(T, L + 1), _cells(T, L)
    # (not vacuous: test_the_oracle_case_is_not_vacuous measures, on this very state, how many cells the term changes)
    R.compare(got, want, np.concatenate([c6, c7]), riemann == "exact")


@pytest.mark.parametrize("nvar,grav,difmag", [(5, False, 0.1), (7, True, 0.05)])
def test_the_oracle_case_is_not_vacuous(gpu_lib, oracle, nvar, grav, difmag):
    """From the oracle alone, before the device is looked at (LLF, minmod, seed 11): the update with difmag differs from the one
    without in more than 0.85 of the level-7 cells and 0.7 of the level-6 cells, and of the level-6 leaf cells that the level-7
    call corrects more than 6000 get a different correction (measured: 0.889, 0.766, 6784 of 7892; NVAR = 7 with gravity and
    difmag = 0.05: 0.889, 0.766, 6783).  Then the device, cell by cell in those corrected leaf cells and overall."""
    import ramses_amd
    T = _tree("scrambled")
    uold = mild_tree_state(T, 11, nvar=nvar)
    f = np.random.default_rng(5).normal(size=(3, T["ncell"])) if grav else None
    kw = dict(riemann="llf", slope_type=1, nvar=nvar)
    po, po0 = oracle.make_params(difmag=difmag, **kw), oracle.make_params(**kw)
    c7, c6 = _cells(T, L + 1), _cells(T, L)
    leaf6 = c6[T["son"][c6] == 0]
    with_d, without = R.oracle_step(oracle, po, T, uold, f, (0, 1)), R.oracle_step(oracle, po0, T, uold, f, (0, 1))
    d7, d6 = (with_d[:, c7] != without[:, c7]).any(axis=0).mean(), (with_d[:, c6] != without[:, c6]).any(axis=0).mean()
    # the level-7 call alone: what it leaves in the level-6 leaf cells
    u7d, u70 = uold.copy(), uold.copy()
    R.oracle_sweep(oracle, po, T, L + 1, uold, u7d, 0, 1, f=f)
    R.oracle_sweep(oracle, po0, T, L + 1, uold, u70, 0, 1, f=f)
    corrected = leaf6[(u7d[:, leaf6] != uold[:, leaf6]).any(axis=0)]
    differ = corrected[(u7d[:, corrected] != u70[:, corrected]).any(axis=0)]
    print("cells the term changes: level 7 %.3f, level 6 %.3f; corrected leaf cells %d, with another correction %d" % (d7, d6, len(corrected), len(differ)))
    assert d7 > 0.85 and d6 > 0.7 and len(differ) > 6000
    p = ramses_amd.make_params(difmag=difmag, **kw)
    got, counts = _amr_step(gpu_lib, p, T, uold.copy(), f, (0, 1))
    assert counts == (2, 0), counts
    R.compare(got, with_d, differ, False, names=("corrected leaf cells",))
    R.compare(got, with_d, np.concatenate([c6, c7]), False)


def _two_steps(Lb, p, T, u0, tile_sweep, monkeypatch):
    if tile_sweep:
        monkeypatch.delenv("RAMSES_AMD_TILE_SWEEP", raising=False)
    else:
        monkeypatch.setenv("RAMSES_AMD_TILE_SWEEP", "0")
    u = u0.copy()
    R.load(Lb, T, u, None)
    t0, w0 = Lb.ramses_amd_amrres_tile_sweeps(), Lb.ramses_amd_amrres_tree_sweeps()
    for step in range(2):
        R.set_unew(Lb, p, T)
        R.sweep_levels(Lb, p, T, (0, 1))
        R.set_uold(Lb, p, T)
    R.sync(Lb, T, u)
    counts = (Lb.ramses_amd_amrres_tile_sweeps() - t0, Lb.ramses_amd_amrres_tree_sweeps() - w0)
    Lb.ramses_amd_amrres_invalidate()
    monkeypatch.delenv("RAMSES_AMD_TILE_SWEEP", raising=False)
    return u, counts


def test_two_steps_equal_the_tree_walker(gpu_lib, monkeypatch):
    """set_unew, the sweeps of level 7 and 6, set_uold, twice (HLLC, minmod, difmag = 0.1): the levels on tiles == the same calls with
    RAMSES_AMD_TILE_SWEEP=0 (the tree-walking sweep with difmag, pinned against the reference program by the live tests), bit for bit"""
    import ramses_amd
    T = _tree("scrambled")
    u0 = mild_tree_state(T, 31)
    p = ramses_amd.make_params(riemann="hllc", slope_type=1, difmag=0.1)
    tree, ctree = _two_steps(gpu_lib, p, T, u0, False, monkeypatch)
    assert ctree == (0, 4), ctree
    tiles, ctiles = _two_steps(gpu_lib, p, T, u0, True, monkeypatch)
    assert ctiles == (4, 0), ctiles
    cells = np.concatenate([_cells(T, L), _cells(T, L + 1)])
    assert np.isfinite(tree[:, cells]).all()
    assert (tree[:, cells] != u0[:, cells]).any(axis=0).mean() > 0.9
    assert np.array_equal(tiles[:, cells], tree[:, cells]), np.abs(tiles[:, cells] - tree[:, cells]).max()


def test_difmag_with_plmde_stays_on_the_tree_walker(gpu_lib, oracle):
    """scheme = 'plmde' with difmag > 0: swept through the tree, result equal to the oracle"""
    import ramses_amd
    T = _tree("scrambled")
    uold = mild_tree_state(T, 11)
    kw = dict(riemann="llf", slope_type=1, scheme="plmde", difmag=0.1)
    p, po = ramses_amd.make_params(**kw), oracle.make_params(**kw)
    want = R.oracle_step(oracle, po, T, uold, None, (0, 1))
    got, counts = _amr_step(gpu_lib, p, T, uold.copy(), None, (0, 1))
    assert counts == (0, 2), counts
    R.compare(got, want, np.concatenate([_cells(T, L), _cells(T, L + 1)]), False)


# ---- live, end to end: the patched program against the untouched one -------------------------------------------------------

def _namelist(lmin, lmax, riemann="hllc", nstep=4, poisson=False, ngridtot=400000):
    nml = live.amr_namelist(lmin, lmax, nstep, riemann, 1, "1,1,1,1,1,2,2", ngridtot, poisson=poisson)
    solver = "riemann='%s'\n" % riemann
    assert nml.count(solver) == 1 and "difmag" not in nml
    return nml.replace(solver, solver + "difmag=0.1\n")          # (&HYDRO_PARAMS)


def _live(nml, nproc, env, min_octs="0"):
    e = {"RAMSES_AMD_STRICT": "1", "RAMSES_AMD_STATS": "1", "RAMSES_AMD_DIFMAG_TILES": "1"}
    return live.ab(nml, nproc, dict(e, **env), ref_env={"RAMSES_AMD": "0"}, min_octs=min_octs)


@pytest.mark.parametrize("nproc,poisson", [(1, False), (2, False), (1, True)], ids=["1rank", "2ranks", "self-gravity"])
def test_patched_program_with_difmag_sweeps_its_levels_in_tiles(gpu_lib, nproc, poisson):
    """sedov3d, levels 6-7, difmag = 0.1, HLLC, strict arithmetic, tiles forced for the small levels: the leaf cells of the last
    snapshot bit-identical to the unpatched program, every sweep of a level through the dense kernel on tiles"""
    out, want = _live(_namelist(6, 7, poisson=poisson), nproc, {})
    assert "AMR levels stay resident on the GPU" in out, out[-3000:]
    assert (want.level == 7).sum() >= 64, "the run must have refined (eight octs of level 7 at least)"
    tiles, tree = live.sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)


def test_a_uniform_64_cubed_level_with_difmag_takes_the_tiles_at_the_production_threshold(gpu_lib):
    """no override of RAMSES_AMD_TILE_MIN_OCTS: a uniform 64^3 level (32768 octs, the production crossover) with difmag"""
    out, _ = _live(_namelist(6, 6, nstep=3, ngridtot=80000), 1, {}, min_octs=None)
    tiles, tree = live.sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)


def test_default_arithmetic_run_with_difmag_is_bit_identical_and_says_so(gpu_lib):
    """no RAMSES_AMD_STRICT: the program's default (fast) arithmetic sweeps difmag levels in strict arithmetic"""
    out, _ = _live(_namelist(6, 7), 1, {"RAMSES_AMD_STRICT": None})
    assert "dense sweep arithmetic = fast" in out, out[-3000:]
    assert "difmag: AMR levels in tiles are swept in strict arithmetic" in out, out[-3000:]
    tiles, tree = live.sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)

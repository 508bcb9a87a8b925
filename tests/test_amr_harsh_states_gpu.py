"""The sweeps of AMR levels against the C ORACLE of godfine1 on a SUPERSONIC state with densities on both sides of the floor.

Every other kernel-level test of the AMR paths (tests/test_amr_tiles_gpu.py, test_pfix_tiles_gpu.py, test_difmag_tiles_gpu.py, the
synthetic trees of test_amr_godunov_gpu.py) uses one mild state -- density in [1, 2), momenta rho (U - 1/2), internal energy in
[1, 2), smallr = 1e-10 -- on which the oracle never takes the supersonic outcomes of HLLC, of the acoustic and of the Newton
solver, never resets a traced density, and no floor ever binds (profiles/harsh_state_branches.txt, written by
scripts/oracle_branch_coverage.py; tests/test_harsh_state_branches.py keeps it true).  The tile kernels
(csrc/hydro_sweep.hip godunov_sweep_kernel<MASK>, godunov_sweep_pfix_kernel, godunov_sweep_difmag_kernel, the three surface-flux
kernels, tile_coarse_update_kernel) and the father-oct kernel of the tree walker (csrc/amr_sweep.hip) are kernels of their own, with
their own register budgets and, in fast arithmetic, their own trimmed LLF stream: a wrong upwind choice, a missing floor or a flux
record filed from the wrong star state on a supersonic face shows here and nowhere else.

The state is tests/helpers.py harsh_tree_state; the tree is the tile tests': level 6 complete, level 7 in a spherical shell with
refined cells on the periodic seam (tiles do not exist below level 6).  A case is one amr_step's worth of calls through the C ABI
-- set_unew on both levels, godunov_fine of level 7 then 6, set_uold, sync -- compared in all cells of both levels: strict
arithmetic bit for bit, riemann = 'exact' to 1e-12 of each variable's maximum (the device's pow()), fast arithmetic to the same
1e-12.  With NVAR > 5 the expectation is the oracle's unew through set_uold's passive-scalar floor fix (numpy, helpers.py)."""
import functools

import numpy as np
import pytest

import resident as R
from helpers import _set_uold_scalar_fix, harsh_tree_state, oct_cells, tree_cell_kind, tree_state_shares

pytestmark = pytest.mark.gpu
L = 6
SEED = 12
FLOOR = 0.6           # the high density floor: about half of the cells lie below it
MAX_SHARE_BELOW_ZERO, LOWEST_DENSITY = 1e-4, -0.01   # what the ORACLE may leave with that floor (see _oracle_step); 0 cells with 1e-10
@pytest.fixture(autouse=True)
def _dense_sweep_on_small_levels_too(monkeypatch):
    R.force_tiles(monkeypatch, clear=R.LAYOUT_VARS + ("RAMSES_AMD_DIFMAG_TILES",))


@functools.lru_cache(maxsize=None)
def _tree(order):
    T = R.two_level_tree(L, order)
    T["cells"] = {lev: oct_cells(T, T["lists"][lev]) for lev in (L, L + 1)}
    T["both"] = np.concatenate([T["cells"][L], T["cells"][L + 1]])
    T["grav"] = np.random.default_rng(5).normal(size=(3, T["ncell"]))
    return T


@functools.lru_cache(maxsize=None)
def _state7(order):
    """the state of a tree with two passive scalars (its first 5 / 6 variables are the state for NVAR = 5 / 6), made once; what it
    is there for is asserted from the state alone: measured 0.573 of the cells above Mach 1 and 0.511 below the floor at L = 6,
    for both oct orders"""
    T = _tree(order)
    u = harsh_tree_state(T, L, SEED, nvar=7)
    mach, low = tree_state_shares(T, L, u, FLOOR)
    print("harsh state (%s): share of cells above Mach 1 %.3f, below the floor of %.1f: %.3f" % (order, mach, FLOOR, low))
    assert mach > 0.3, mach
    assert 0.3 < low < 0.7, low
    u.setflags(write=False)
    return u


def _inputs(order, nvar, grav):
    T = _tree(order)
    return T, np.ascontiguousarray(_state7(order)[:nvar]).copy(), (T["grav"] if grav else None)


def _oracle_step(oracle, po, T, uold, f, interp, pfix0=None):
    """godunov_fine of level L+1 then L (the order of amr_step): unew (and divu, enew from what the device holds after set_unew).
    Asserted from the oracle alone: a finite result that changes more than 0.9 of the cells and stays within twice the state's
    range in every variable (an unlimited interpolation of the ghost octs next to the floor of 1e-10 would not: velocities of
    1e17 make the 1e-12 of a variable's maximum meaningless), and positive densities: all of them with the floor at 1e-10.  With
    the floor at 0.6 a cell far below it loses mass at the floor's rate (fluxes are formed with max(rho, smallr)), so in the
    reference's own arithmetic a few of the 567 616 cells end below zero: over the floored cases of this file (CPU, oracle alone)
    1 to 3 cells, 11 with the acoustic solver and the 27-point slope, the lowest at -5.8e-3.  Bounded here at one cell in 10 000
    (56 cells) and -0.01 (a sixtieth of the floor); a state or an oracle that drove densities negative at large would not pass."""
    divu, enew = (pfix0[0].copy(), pfix0[1].copy()) if pfix0 else (None, None)
    unew = R.oracle_step(oracle, po, T, uold, f, interp, divu, enew)
    cells = T["both"]
    assert np.isfinite(unew[:, cells]).all()
    growth = (np.abs(unew[:, cells]).max(axis=1) / np.abs(uold[:, cells]).max(axis=1)).max()
    changed = (unew[:, cells] != uold[:, cells]).any(axis=0).mean()
    print("oracle: cells changed %.3f, smallest density %.3e (%d cells below zero), largest growth of a variable's maximum %.3f" %
          (changed, unew[0, cells].min(), int((unew[0, cells] <= 0).sum()), growth))
    assert changed > 0.9, changed
    assert growth <= 2.0, growth
    below = int((unew[0, cells] <= 0).sum())
    if po.smallr < 1e-3:
        assert below == 0, unew[0, cells].min()
    else:
        assert below <= MAX_SHARE_BELOW_ZERO * len(cells) and unew[0, cells].min() >= LOWEST_DENSITY, (below, unew[0, cells].min())
    return unew, divu, enew


def _compare(T, got, ref, tolerant, names=("unew", "divu", "enew")):
    """bit for bit; tolerant (riemann = 'exact': the device's pow(); fast arithmetic): 1e-12 of each variable's maximum.  Prints the
    figures before it asserts; a difference is reported with its first cell"""
    cells = T["both"]
    worst = 0.0
    for name, g, r in zip(names, got, ref):
        g, r = np.atleast_2d(g)[:, cells], np.atleast_2d(r)[:, cells]
        scale = np.abs(r).max(axis=1, keepdims=True)
        scale[scale == 0] = 1.0
        rel = np.abs(g - r) / scale
        ndiff = int((g != r).any(axis=0).sum())
        first = ""
        if ndiff:
            v, k = np.unravel_index(np.argmax(rel), rel.shape)
            first = "; largest in variable %d, %s (got %r, oracle %r); first differing %s" % (
                v, tree_cell_kind(T, L, cells[k]), g[v, k], r[v, k], tree_cell_kind(T, L, cells[np.nonzero((g != r).any(axis=0))[0][0]]))
        own = np.abs(r)
        own[own == 0] = 1.0
        print("%s: cells that differ %d of %d, max difference %.3e of the variable's maximum, %.3e of the cell's own value%s" %
              (name, ndiff, len(cells), rel.max(), (np.abs(g - r) / own).max(), first))
        if tolerant:
            assert rel.max() <= 1e-12, (name, rel.max(), first)
        else:
            assert ndiff == 0, (name, ndiff, rel.max(), first)
        worst = max(worst, rel.max())
    return worst


def _set_unew_pfix_numpy(T, uold, smallr):
    """what set_unew leaves in divu / enew under pressure_fix (hydro/godunov_fine.f90:71-81), in its operation order:
    divu = 0, enew = E - 0.5 d (u^2 + v^2 + w^2) with d = max(rho, smallr) and u, v, w = momenta / d; in the cells of both levels"""
    divu, enew = np.zeros(T["ncell"]), np.zeros(T["ncell"])
    c = T["both"]
    d = np.maximum(uold[0, c], smallr)
    u, v, w = uold[1, c] / d, uold[2, c] / d, uold[3, c] / d
    enew[c] = uold[4, c] - 0.5 * d * (u * u + v * v + w * w)
    return divu, enew


def _case(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, fast=False, scheme="muscl", difmag=0.0,
          pfix=False, walker=False):
    """one amr_step's worth of calls on the harsh state == the oracle's, through the path the case is about"""
    import ramses_amd
    T, uold, f = _inputs(order, nvar, grav)
    kw = dict(riemann=riemann, slope_type=slope, nvar=nvar, smallr=smallr, scheme=scheme, difmag=difmag)
    p, po = ramses_amd.make_params(fast_math=fast, **kw), oracle.make_params(**kw)
    if walker:
        monkeypatch.setenv("RAMSES_AMD_TILE_SWEEP", "0")
    if difmag > 0:
        monkeypatch.setenv("RAMSES_AMD_DIFMAG_TILES", "1")         # (difmag on tiles is opt-in; the tree walker does not read it)
    pfix0 = _set_unew_pfix_numpy(T, uold, smallr) if pfix else None
    ref = _oracle_step(oracle, po, T, uold, f, interp, pfix0)      # before the device is looked at
    u = uold.copy()
    try:
        R.load(gpu_lib, T, u, f, pfix=pfix)
        assert gpu_lib.ramses_amd_amrres_tiled_levels() == 2
        dev0 = R.set_unew(gpu_lib, p, T, pfix)
        counts = R.sweep_levels(gpu_lib, p, T, interp)
        got = R.read_back(gpu_lib, p, T, u, pfix)
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()
    assert counts == ((0, 2) if walker else (2, 0)), "sweeps through the tiles / through the tree: %d / %d" % counts
    if pfix:          # set_unew with pressure_fix (lvl_pfix_init_kernel: its max(rho, smallr) binds in half of the cells with the high floor)
        for name, a, b in zip(("divu", "enew"), dev0, pfix0):
            assert np.array_equal(a[T["both"]], b[T["both"]]), ("set_unew_pfix", name, np.abs(a[T["both"]] - b[T["both"]]).max())
    want = (_set_uold_scalar_fix(uold, ref[0], smallr),) + ((ref[1], ref[2]) if pfix else ())
    if nvar > 5 and smallr == FLOOR:
        fixed = int((want[0][5:, T["both"]] != ref[0][5:, T["both"]]).any(axis=0).sum())
        print("cells whose passive scalars set_uold's floor fix changes:", fixed)
        assert fixed > 1000          # (a third of the cells lie below the floor and gain or lose mass)
    if pfix:
        c7, c6 = T["cells"][L + 1], T["cells"][L]
        assert (ref[1][c7] != 0).mean() > 0.9 and (ref[1][c6] != 0).mean() > 0.7 and (ref[2][c7] != pfix0[1][c7]).mean() > 0.9
    return _compare(T, got, want, tolerant=(riemann == "exact" or (fast and not pfix and difmag == 0)))


# Every table: NVAR, solver, slope_type, smallr, gravity, oct order, (interpol_var, interpol_type) [, more].  The oct order, the
# interpolation of the ghost octs and the gravity are mixed over the cases, not crossed.
PLAIN = [
    (5, "llf", 1, 1e-10, False, "morton", (0, 1), "muscl"),
    (7, "llf", 3, FLOOR, True, "scrambled", (1, 2), "muscl"),
    (6, "hllc", 2, 1e-10, True, "scrambled", (2, 4), "muscl"),
    (7, "hllc", 7, FLOOR, False, "morton", (0, 3), "muscl"),
    (5, "hll", 8, 1e-10, True, "morton", (1, 0), "muscl"),
    (6, "hll", 2, FLOOR, False, "scrambled", (0, 1), "muscl"),
    (5, "acoustic", 7, 1e-10, False, "scrambled", (1, 2), "muscl"),
    (6, "acoustic", 1, FLOOR, True, "morton", (2, 4), "muscl"),
    (5, "exact", 3, 1e-10, True, "morton", (0, 1), "muscl"),
    (7, "exact", 8, FLOOR, False, "scrambled", (1, 0), "muscl"),
    (5, "llf", 1, FLOOR, True, "scrambled", (1, 2), "plmde"),
    (5, "hllc", 2, 1e-10, False, "morton", (0, 1), "plmde"),
]


@pytest.mark.parametrize("nvar,riemann,slope,smallr,grav,order,interp,scheme", PLAIN)
def test_plain_tiles_strict(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, scheme):
    """godunov_sweep_kernel<MASK>, surface_flux_kernel, tile_coarse_update_kernel in strict arithmetic: every solver below and above
    the floor, bit for bit ('exact': 1e-12)"""
    _case(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, scheme=scheme)


FAST = [
    (5, "llf", 1, 1e-10, False, "scrambled", (0, 1)),
    (5, "llf", 1, FLOOR, True, "morton", (1, 2)),
    (5, "hllc", 1, 1e-10, True, "morton", (2, 4)),
    (6, "hllc", 1, FLOOR, False, "scrambled", (0, 3)),
    (5, "hllc", 2, 1e-10, False, "morton", (1, 0)),
    (5, "hllc", 2, FLOOR, True, "scrambled", (0, 1)),
    (7, "hll", 8, 1e-10, True, "scrambled", (1, 2)),
    (5, "hll", 8, FLOOR, False, "morton", (2, 4)),
]


@pytest.mark.parametrize("nvar,riemann,slope,smallr,grav,order,interp", FAST)
def test_plain_tiles_fast(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp):
    """the fast build of the same kernels (reciprocals, the trimmed LLF stream that leaves the floor of the traced densities to
    the trace): <= 1e-12 of each variable's maximum, the bound of tests/test_amr_tiles_gpu.py"""
    _case(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, fast=True)


PFIX = [
    (5, "hllc", 2, 1e-10, True, "scrambled", (0, 1)),
    (5, "exact", 1, FLOOR, False, "morton", (1, 2)),
    (7, "acoustic", 3, FLOOR, True, "scrambled", (0, 3)),
    (6, "llf", 7, 1e-10, False, "morton", (2, 4)),
]


@pytest.mark.parametrize("nvar,riemann,slope,smallr,grav,order,interp", PFIX)
def test_pressure_fix_tiles(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp):
    """godunov_sweep_pfix_kernel, surface_flux_pfix_kernel: unew, divu (the face velocity through the upwind branch of the solver)
    and enew (the internal-energy flux) of every cell of both levels"""
    _case(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, pfix=True)


DIFMAG = [
    (5, "llf", 1, FLOOR, False, "scrambled", (1, 0), 0.1),
    (7, "hllc", 2, 1e-10, True, "morton", (0, 1), 0.05),
    (5, "hll", 8, 1e-10, False, "morton", (1, 2), 0.1),
    (6, "exact", 7, FLOOR, True, "scrambled", (2, 4), 0.05),
]


@pytest.mark.parametrize("nvar,riemann,slope,smallr,grav,order,interp,difmag", DIFMAG)
def test_difmag_tiles(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, difmag):
    """godunov_sweep_difmag_kernel, surface_flux_difmag_kernel (RAMSES_AMD_DIFMAG_TILES=1): cmpdivu / consup where the flow converges
    at more than the sound speed"""
    _case(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, difmag=difmag)


WALKER = [
    # ..., scheme, difmag, pressure_fix
    (5, "hllc", 1, 1e-10, False, "scrambled", (0, 1), "muscl", 0.0, False),
    (5, "exact", 2, 1e-10, True, "morton", (1, 2), "muscl", 0.0, False),
    (5, "hll", 7, 1e-10, True, "scrambled", (2, 4), "muscl", 0.1, True),
    (5, "hllc", 2, 1e-10, False, "morton", (1, 0), "plmde", 0.0, True),
    (7, "acoustic", 8, FLOOR, True, "scrambled", (0, 3), "muscl", 0.0, False),
]


@pytest.mark.parametrize("nvar,riemann,slope,smallr,grav,order,interp,scheme,difmag,pfix", WALKER)
def test_tree_walker_on_the_same_tree(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, scheme, difmag, pfix):
    """RAMSES_AMD_TILE_SWEEP=0: the father-oct kernel of csrc/amr_sweep.hip on the levels in tiles"""
    _case(gpu_lib, oracle, monkeypatch, nvar, riemann, slope, smallr, grav, order, interp, scheme=scheme, difmag=difmag, pfix=pfix, walker=True)

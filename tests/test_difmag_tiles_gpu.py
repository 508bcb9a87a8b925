"""difmag > 0 on AMR levels in tiles: cmpdivu / consup (hydro/uplmde.f90:702-866) through the dense sweep (csrc/difmag_core.hpp;
csrc/hydro_sweep.hip godunov_sweep_difmag_kernel, the surface pass surface_flux_difmag_kernel; csrc/capi_amr.hip tile_level_sweep)
against the C ORACLE of godfine1 with the same difmag (oracle/amr_godfine_oracle.c over oracle/hydro_oracle.c ora_cmpdivu /
ora_consup, pinned on the reference's dumps), against the tree-walking sweep (the second implementation on the device) and,
live, against the unpatched program.  Built like tests/test_pfix_tiles_gpu.py: level 6 complete, level 7 a spherical shell with
refined cells on the periodic seam, both in tiles; dt = 0.02 dx."""
import ctypes as C
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 6
LAYOUT_VARS = ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE", "RAMSES_AMD_TILE_SWEEP")


@pytest.fixture(autouse=True)
def _dense_sweep_on_small_levels_too(monkeypatch):
    """(levels below RAMSES_AMD_TILE_MIN_OCTS octs take the tree-walking sweep in production: the tests force the tiles)"""
    monkeypatch.setenv("RAMSES_AMD_TILE_MIN_OCTS", "0")
    monkeypatch.setenv("RAMSES_AMD_DIFMAG_TILES", "1")        # (difmag on tiles is opt-in until it is measured: the tests ask for it)
    for var in LAYOUT_VARS:
        monkeypatch.delenv(var, raising=False)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _shell_mask(nc, lo=0.23, hi=0.36):
    z, y, x = np.meshgrid(np.arange(nc), np.arange(nc), np.arange(nc), indexing="ij")
    r = np.sqrt((x - nc / 2 + 0.5) ** 2 + (y - nc / 2 + 0.5) ** 2 + (z - nc / 2 + 0.5) ** 2)
    mask = (r >= lo * nc) & (r <= hi * nc)
    mask[0, 0, :5] = True              # refined cells on the periodic seam too (tiles wrap)
    mask[nc - 1, nc - 1, nc - 3:] = True
    return mask


def _tree(order):
    from ramses_amd import ic
    T = ic.uniform_tree(L, order=order, refine_mask=_shell_mask(2 ** L), slack=260000)
    T["all_octs"] = {L: np.ascontiguousarray(np.sort(T["igrid"])), L + 1: np.ascontiguousarray(np.sort(T["igrid_fine"]))}
    T["lists"] = {L: np.ascontiguousarray(T["igrid"]), L + 1: np.ascontiguousarray(T["igrid_fine"])}
    return T


def _cells(T, lev):
    return np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + T["lists"][lev] - 1 for ind in range(8)])


def _random_state(T, seed, nvar=5):
    rng = np.random.default_rng(seed)
    ncell = T["ncell"]
    uold = np.zeros((nvar, ncell))
    n = ncell - 1
    uold[0, 1:] = 1.0 + rng.random(n)
    for d in (1, 2, 3):
        uold[d, 1:] = uold[0, 1:] * (rng.random(n) - 0.5)
    uold[4, 1:] = 1.0 + rng.random(n) + 0.5 * (uold[1, 1:] ** 2 + uold[2, 1:] ** 2 + uold[3, 1:] ** 2) / uold[0, 1:]
    for v in range(5, nvar):
        uold[v, 1:] = uold[0, 1:] * rng.random(n)          # passive scalars: density x a fraction in [0, 1)
    uold[:, 0] = uold[:, 1]
    return uold


def _load(Lb, T, u, f):
    from ramses_amd._capi import check
    check(Lb.ramses_amd_amrres_invalidate())
    check(Lb.ramses_amd_amrres_load(u.shape[0], T["ngridmax"], T["ncoarse"], _vp(u), _vp(T["son"]), _vp(T["nbor"]), _vp(T["father"])))
    if f is not None:
        for lev in (L, L + 1):
            check(Lb.ramses_amd_amrres_load_f(len(T["all_octs"][lev]), _vp(T["all_octs"][lev]), _vp(f)))
    T["host_u"] = u                       # (ramses_amd_amrres_sync_level writes into the array the state was loaded from)


def _set_unew(Lb, T):
    from ramses_amd._capi import check
    for lev in (L, L + 1):
        ig = T["all_octs"][lev]
        check(Lb.ramses_amd_amrres_set_unew(len(ig), _vp(ig)))


def _sweep(Lb, p, T, lev, ivar, itype):
    from ramses_amd._capi import check
    ig = T["lists"][lev]
    dx = 1.0 / 2 ** lev
    check(Lb.ramses_amd_amrres_godunov(C.byref(p), lev, len(ig), _vp(ig), dx, 0.02 * dx, 32, ivar, itype))


def _set_uold(Lb, p, T):
    from ramses_amd._capi import check
    for lev in (L, L + 1):
        ig = T["all_octs"][lev]
        check(Lb.ramses_amd_amrres_set_uold(C.byref(p), len(ig), _vp(ig)))


def _sync(Lb, T):
    from ramses_amd._capi import check
    u = T["host_u"]
    for lev in (L, L + 1):
        ig = T["all_octs"][lev]
        check(Lb.ramses_amd_amrres_sync_level(len(ig), _vp(ig), _vp(u)))
    return u


def _amr_step(Lb, p, T, u, f, interp):
    """set_unew, godunov of level 7 then 6, set_uold, sync_level; returns the state and (tile sweeps, tree sweeps)"""
    _load(Lb, T, u, f)
    _set_unew(Lb, T)
    t0, w0 = Lb.ramses_amd_amrres_tile_sweeps(), Lb.ramses_amd_amrres_tree_sweeps()
    for lev in (L + 1, L):
        _sweep(Lb, p, T, lev, *interp)
    counts = (Lb.ramses_amd_amrres_tile_sweeps() - t0, Lb.ramses_amd_amrres_tree_sweeps() - w0)
    _set_uold(Lb, p, T)
    got = _sync(Lb, T)
    Lb.ramses_amd_amrres_invalidate()
    return got, counts


def _oracle_sweep(oracle, po, T, lev, uold, unew, f, ivar, itype):
    dx = 1.0 / 2 ** lev
    oracle.godunov_fine_amr(po, T["lists"][lev], T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew, dx, 0.02 * dx, 32,
                            ivar, itype, f=f)


def _oracle_step(oracle, po, T, uold, f, interp):
    unew = uold.copy()
    for lev in (L + 1, L):
        _oracle_sweep(oracle, po, T, lev, uold, unew, f, *interp)
    return unew


def _compare(got, ref, cells, exact_solver, what="unew"):
    """bit for bit; riemann = 'exact' calls pow(), whose last ulp is the device's: relative 1e-12, as the other tile tests do"""
    g, r = got[:, cells], ref[:, cells]
    if exact_solver:
        scale = np.abs(r).max(axis=-1, keepdims=True)
        err = (np.abs(g - r) / scale).max()
        print(what, "max relative difference", err)
        assert err <= 1e-12, (what, err)
    else:
        print(what, "cells that differ", int((g != r).any(axis=0).sum()), "of", len(cells), "max abs difference", np.abs(g - r).max())
        assert np.array_equal(g, r), (what, np.abs(g - r).max())


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
    uold = _random_state(T, 11, nvar=nvar)
    f = np.random.default_rng(5).normal(size=(3, T["ncell"])) if grav else None
    kw = dict(riemann=riemann, slope_type=slope, nvar=nvar, difmag=difmag)
    p, po = ramses_amd.make_params(fast_math=fast, **kw), oracle.make_params(**kw)
    want = _oracle_step(oracle, po, T, uold, f, interp)
    got, counts = _amr_step(gpu_lib, p, T, uold.copy(), f, interp)
    assert counts == (2, 0), "sweeps through the tiles / through the tree: %d / %d" % counts
    c7, c6 = _cells(T, L + 1), _cells(T, L)
    # (not vacuous: test_the_oracle_case_is_not_vacuous measures, on this very state, how many cells the term changes)
    _compare(got, want, np.concatenate([c6, c7]), riemann == "exact")


@pytest.mark.parametrize("nvar,grav,difmag", [(5, False, 0.1), (7, True, 0.05)])
def test_the_oracle_case_is_not_vacuous(gpu_lib, oracle, nvar, grav, difmag):
    """From the oracle alone, before the device is looked at (LLF, minmod, seed 11): the update with difmag differs from the one
    without in more than 0.85 of the level-7 cells and 0.7 of the level-6 cells, and of the level-6 leaf cells that the level-7
    call corrects more than 6000 get a different correction (measured: 0.889, 0.766, 6784 of 7892; NVAR = 7 with gravity and
    difmag = 0.05: 0.889, 0.766, 6783).  Then the device, cell by cell in those corrected leaf cells and overall."""
    import ramses_amd
    T = _tree("scrambled")
    uold = _random_state(T, 11, nvar=nvar)
    f = np.random.default_rng(5).normal(size=(3, T["ncell"])) if grav else None
    kw = dict(riemann="llf", slope_type=1, nvar=nvar)
    po, po0 = oracle.make_params(difmag=difmag, **kw), oracle.make_params(**kw)
    c7, c6 = _cells(T, L + 1), _cells(T, L)
    leaf6 = c6[T["son"][c6] == 0]
    with_d, without = _oracle_step(oracle, po, T, uold, f, (0, 1)), _oracle_step(oracle, po0, T, uold, f, (0, 1))
    d7, d6 = (with_d[:, c7] != without[:, c7]).any(axis=0).mean(), (with_d[:, c6] != without[:, c6]).any(axis=0).mean()
    # the level-7 call alone: what it leaves in the level-6 leaf cells
    u7d, u70 = uold.copy(), uold.copy()
    _oracle_sweep(oracle, po, T, L + 1, uold, u7d, f, 0, 1)
    _oracle_sweep(oracle, po0, T, L + 1, uold, u70, f, 0, 1)
    corrected = leaf6[(u7d[:, leaf6] != uold[:, leaf6]).any(axis=0)]
    differ = corrected[(u7d[:, corrected] != u70[:, corrected]).any(axis=0)]
    print("cells the term changes: level 7 %.3f, level 6 %.3f; corrected leaf cells %d, with another correction %d" % (d7, d6, len(corrected), len(differ)))
    assert d7 > 0.85 and d6 > 0.7 and len(differ) > 6000
    p = ramses_amd.make_params(difmag=difmag, **kw)
    got, counts = _amr_step(gpu_lib, p, T, uold.copy(), f, (0, 1))
    assert counts == (2, 0), counts
    _compare(got, with_d, differ, False, "corrected leaf cells")
    _compare(got, with_d, np.concatenate([c6, c7]), False)


def _two_steps(Lb, p, T, u0, tile_sweep, monkeypatch):
    if tile_sweep:
        monkeypatch.delenv("RAMSES_AMD_TILE_SWEEP", raising=False)
    else:
        monkeypatch.setenv("RAMSES_AMD_TILE_SWEEP", "0")
    _load(Lb, T, u0.copy(), None)
    t0, w0 = Lb.ramses_amd_amrres_tile_sweeps(), Lb.ramses_amd_amrres_tree_sweeps()
    for step in range(2):
        _set_unew(Lb, T)
        for lev in (L + 1, L):
            _sweep(Lb, p, T, lev, 0, 1)
        _set_uold(Lb, p, T)
    u = _sync(Lb, T)
    counts = (Lb.ramses_amd_amrres_tile_sweeps() - t0, Lb.ramses_amd_amrres_tree_sweeps() - w0)
    Lb.ramses_amd_amrres_invalidate()
    monkeypatch.delenv("RAMSES_AMD_TILE_SWEEP", raising=False)
    return u, counts


def test_two_steps_equal_the_tree_walker(gpu_lib, monkeypatch):
    """set_unew, the sweeps of level 7 and 6, set_uold, twice (HLLC, minmod, difmag = 0.1): the levels on tiles == the same calls with
    RAMSES_AMD_TILE_SWEEP=0 (the tree-walking sweep with difmag, pinned against the reference program by the live tests), bit for bit"""
    import ramses_amd
    T = _tree("scrambled")
    u0 = _random_state(T, 31)
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
    uold = _random_state(T, 11)
    kw = dict(riemann="llf", slope_type=1, scheme="plmde", difmag=0.1)
    p, po = ramses_amd.make_params(**kw), oracle.make_params(**kw)
    want = _oracle_step(oracle, po, T, uold, None, (0, 1))
    got, counts = _amr_step(gpu_lib, p, T, uold.copy(), None, (0, 1))
    assert counts == (0, 2), counts
    _compare(got, want, np.concatenate([_cells(T, L), _cells(T, L + 1)]), False)


# ---- live, end to end: the patched program against the untouched one -------------------------------------------------------

def _mka():
    spec = importlib.util.spec_from_file_location("mka", os.path.join(ROOT, "tests", "golden", "make_golden_amr.py"))
    mka = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mka)
    return mka


def _namelist(lmin, lmax, riemann="hllc", nstep=4, poisson=False, ngridtot=400000):
    from oracle import ramses_snapshot as rs
    mka = _mka()
    extra = mka.REFINE.format(ivar=0, itype=2) if lmax > lmin else ""
    kw = {}
    if poisson:
        kw["init"] = mka.SELFGRAV_INIT
        extra += "&POISSON_PARAMS\nepsilon=1e-5\n/\n"
    nml = rs.sedov3d_namelist(level=lmin, nstepmax=nstep, foutput=nstep, riemann=riemann, slope_type=1, extra=extra, mem_factor=1.0, poisson=poisson, **kw)
    nml = nml.replace("levelmax=%d" % lmin, "levelmax=%d" % lmax).replace("nsubcycle=10*1", "nsubcycle=1,1,1,1,1,2,2")
    solver = "riemann='%s'\n" % riemann
    assert nml.count(solver) == 1 and "difmag" not in nml and "ngridtot=" in nml
    nml = nml.replace(solver, solver + "difmag=0.1\n")          # (&HYDRO_PARAMS)
    return nml.replace("ngridtot=", "ngridtot=%d !" % ngridtot)


def _run(nml, binary, nproc, env):
    from oracle import ramses_snapshot as rs
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        return rs.run_reference(nml, binary=binary, nproc=nproc)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _leaves(work):
    from oracle import ramses_snapshot as rs
    snap = rs.load_leaf_cells(os.path.join(work, "output_00002"))
    order = np.lexsort((snap["x"][:, 0], snap["x"][:, 1], snap["x"][:, 2], snap["level"]))
    return snap["level"][order], snap["prim"][:, order]


def _sweep_counts(out):
    m = re.search(r"godunov_fine of AMR levels:\s*(\d+) sweeps through the dense kernel on tiles.*?(\d+) through the tree-walking kernel", out)
    assert m, out[-2000:]
    return int(m.group(1)), int(m.group(2))


def _binaries(mpi):
    names = ("ramses3d_mpi_patch", "ramses3d_mpi") if mpi else ("ramses3d_patch", "ramses3d")
    patched, ref = (os.path.join(ROOT, "oracle", "_ref", b) for b in names)
    if not (os.path.exists(patched) and os.path.exists(ref)):
        pytest.skip("oracle/_ref/%s, %s not built" % names)
    return patched, ref


def _live(nml, nproc, env, min_octs="0"):
    patched, ref = _binaries(nproc > 1)
    e = {"RAMSES_AMD": "1", "RAMSES_AMD_STRICT": "1", "RAMSES_AMD_STATS": "1", "RAMSES_AMD_TILE_MIN_OCTS": min_octs, "RAMSES_AMD_DIFMAG_TILES": "1"}
    e.update(env)
    work, out = _run(nml, patched, nproc, e)
    try:
        got = _leaves(work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    work, _ = _run(nml, ref, nproc, {"RAMSES_AMD": "0"})
    try:
        want = _leaves(work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1]), np.abs(got[1] - want[1]).max()
    assert np.array_equal(got[1].view(np.int64), want[1].view(np.int64))
    return out, want


@pytest.mark.parametrize("nproc,poisson", [(1, False), (2, False), (1, True)], ids=["1rank", "2ranks", "self-gravity"])
def test_patched_program_with_difmag_sweeps_its_levels_in_tiles(gpu_lib, nproc, poisson):
    """sedov3d, levels 6-7, difmag = 0.1, HLLC, strict arithmetic, tiles forced for the small levels: the leaf cells of the last
    snapshot bit-identical to the unpatched program, every sweep of a level through the dense kernel on tiles"""
    out, want = _live(_namelist(6, 7, poisson=poisson), nproc, {})
    assert "AMR levels stay resident on the GPU" in out, out[-3000:]
    assert (want[0] == 7).sum() >= 64, "the run must have refined (eight octs of level 7 at least)"
    tiles, tree = _sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)


def test_a_uniform_64_cubed_level_with_difmag_takes_the_tiles_at_the_production_threshold(gpu_lib):
    """no override of RAMSES_AMD_TILE_MIN_OCTS: a uniform 64^3 level (32768 octs, the production crossover) with difmag"""
    out, _ = _live(_namelist(6, 6, nstep=3, ngridtot=80000), 1, {}, min_octs=None)
    tiles, tree = _sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)


def test_default_arithmetic_run_with_difmag_is_bit_identical_and_says_so(gpu_lib):
    """no RAMSES_AMD_STRICT: the program's default (fast) arithmetic sweeps difmag levels in strict arithmetic"""
    out, _ = _live(_namelist(6, 7), 1, {"RAMSES_AMD_STRICT": None})
    assert "dense sweep arithmetic = fast" in out, out[-3000:]
    assert "difmag: AMR levels in tiles are swept in strict arithmetic" in out, out[-3000:]
    tiles, tree = _sweep_counts(out)
    assert tiles > 0 and tree == 0, (tiles, tree)

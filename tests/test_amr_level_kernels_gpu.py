"""The small routines amr_step calls between sweeps on a RESIDENT AMR level (csrc/capi_amr.hip) against independent checkers:

  ramses_amd_amrres_courant        lvl_courant_kernel<GRAV>, its init / final kernels   the C oracle's cmpdt; math.fsum of the terms
  ramses_amd_amrres_synchro        lvl_synchro_kernel                                   the C oracle's synchro_hydro
  ramses_amd_amrres_set_uold_grav  lvl_gravity_source_kernel, lvl_set_uold_kernel       the C oracle's add_gravity_source + scalar fix
  ramses_amd_amrres_upload_fine    lvl_upload_kernel<5|6|7>                             the C oracle's upl
  ramses_amd_amrres_set_uold_pfix  lvl_pdv_kernel, lvl_pfix_switch_kernel               numpy restatements of the reference (helpers.py)

The live runs behind these kernels are Sedov and blob runs: smallr never binds, interpol_var and hexp are 0, the energy switch
rarely fires and the oct lists are whole levels.  Here the state is helpers.harsh_tree_state (two thirds of the cells above Mach 1
and below the high floor), smallr is 1e-10 and 0.6, and every routine is called with a level's full list, with a ragged list
of 37 octs (296 cells: one full workgroup and a partial one) and with ngrid = 0.  After EVERY call the whole state comes back
(sync_all; sync_pfix for divu / enew) and every cell that is not a cell of a listed oct must be bit-identical to what it was: a
wrong stride or a slip in the device's own oct numbering shows there.  The listed cells equal the checker bit for bit; the only
tolerance is on courant_fine's three sums, n 2^-53 sum |terms|, which bounds any order of summation and is not measured.

Trees: level L complete, level L+1 in a shell (helpers.level_case): L = 4 in both oct orders (the host's numbering), L = 6 in
tiles, and one L = 6 case per routine with RAMSES_AMD_DEVICE_ORDER=0.  tests/test_amr_level_checkers.py asserts, without a GPU,
that these inputs make the branches bind (split cells that would lower dt, a fired share of 0.4, 3888 faces at 1.5 dx, ...)."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers as H
from resident import ALL_LAYOUT_VARS, force_tiles, load, vp

pytestmark = pytest.mark.gpu

GAMMA, FLOOR, CF, BETA = 1.4, 0.6, 0.8, 0.5
KINDS = ("full", "sub", "none")
# (L, oct order, RAMSES_AMD_DEVICE_ORDER, smallr)
CASES = [(4, "scrambled", None, 1e-10), (4, "scrambled", None, FLOOR), (4, "morton", None, 1e-10), (4, "morton", None, FLOOR),
         (6, "scrambled", None, 1e-10), (6, "scrambled", None, FLOOR), (6, "scrambled", "0", FLOOR)]
IDS = ["L%d-%s%s-smallr%g" % (c[0], c[1], "-hostorder" if c[2] == "0" else "", c[3]) for c in CASES]


@pytest.fixture(autouse=True)
def _tiles_on_small_levels_too(monkeypatch):
    force_tiles(monkeypatch, clear=ALL_LAYOUT_VARS)


def _params(oracle, nvar, smallr, smallc=1e-10, **kw):
    import ramses_amd
    kw = dict(nvar=nvar, gamma=GAMMA, smallr=smallr, smallc=smallc, **kw)
    return ramses_amd.make_params(courant_factor=CF, **kw), oracle.make_params(**kw)


def _load(Lb, monkeypatch, T, u, f, device_order, pfix=False):
    """the state (and the acceleration, both levels) onto the device; u is the array every sync_all writes into"""
    if device_order is not None:
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", device_order)
    L = T["L"]
    load(Lb, T, u, f, levels=[T["lists"][lev]["sorted"] for lev in (L, L + 1)], pfix=pfix)
    assert Lb.ramses_amd_amrres_tiled_levels() == (2 if L >= 6 and device_order != "0" else 0)


def _set_unew(Lb, p, T, pfix=False):
    from ramses_amd._capi import check
    for lev in (T["L"], T["L"] + 1):
        ig = T["lists"][lev]["sorted"]
        if pfix:
            check(Lb.ramses_amd_amrres_set_unew_pfix(C.byref(p), len(ig), vp(ig)))
        else:
            check(Lb.ramses_amd_amrres_set_unew(len(ig), vp(ig)))


def _sync(Lb, T, u, pfix=False):
    """the whole state back into u; with pressure_fix also (divu, enew) of both levels (zero elsewhere)"""
    from ramses_amd._capi import check
    check(Lb.ramses_amd_amrres_sync_all(vp(u)))
    if not pfix:
        return None
    divu, enew = np.zeros(T["ncell"]), np.zeros(T["ncell"])
    for lev in (T["L"], T["L"] + 1):
        ig = T["lists"][lev]["sorted"]
        check(Lb.ramses_amd_amrres_sync_pfix(len(ig), vp(ig), vp(divu), vp(enew)))
    return divu, enew


def _check(T, got, want, before, octs, what):
    """every cell that is not a cell of a listed oct: bit-identical to what it was; the listed cells: the checker's, bit for bit"""
    got, want, before = np.atleast_2d(got), np.atleast_2d(want), np.atleast_2d(before)
    cells = H.oct_cells(T, octs)
    other = np.ones(T["ncell"], bool)
    other[cells] = False
    moved = other & (got != before).any(axis=0)
    assert not moved.any(), "%s: %d cells outside the %d listed octs changed, first cell %d" % (what, moved.sum(), len(octs), np.nonzero(moved)[0][0])
    diff = (got[:, cells] != want[:, cells]).any(axis=0)
    if diff.any():
        k = cells[np.nonzero(diff)[0][0]]
        raise AssertionError("%s: %d of %d listed cells differ from the checker, first %s: got %r, checker %r" %
                             (what, diff.sum(), len(cells), H.tree_cell_kind(T, T["L"], k), got[:, k], want[:, k]))
    assert np.array_equal(got, want), what          # (and nothing else: want is `before` outside the listed cells)


@functools.lru_cache(maxsize=None)
def _planted(L, order):
    T, u, f = H.level_case(L, order)
    up, cell = H.plant_fast_split_cell(T, u)
    up.setflags(write=False)
    return up, cell


# ---- courant_fine ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nvar,grav", [(7, True), (5, False)], ids=["nvar7-grav", "nvar5-nograv"])
@pytest.mark.parametrize("L,order,device_order,smallr", CASES, ids=IDS)
def test_courant(gpu_lib, oracle, monkeypatch, L, order, device_order, smallr, nvar, grav):
    """dt == cmpdt over the LEAF cells of the list bit for bit (one split cell of level L moves at 1e3 times the state's largest
    velocity: were it to enter the minimum, dt would drop -- asserted on the oracle first), with smallc at 1e-10 and on the 0.2
    quantile of the sound speeds, dt_in above and below the result.  Over the full and the ragged list a warm, fast cell sets dt,
    which no floor touches; the two 'cold' lists (helpers.level_case) are there for that: over them dt moves with smallc, with
    smallr and with the acceleration, at L = 4 and at L = 6 -- asserted on the oracle first.  Mass, total and internal energy
    within n 2^-53 sum |terms| of math.fsum of the reference's terms -- a bound on ANY order of adding them, not a measured one;
    ngrid = 0: min(dt_in, courant_factor dx / smallc) and zero sums; the state does not move."""
    from ramses_amd._capi import check
    T, _, f7 = H.level_case(L, order)
    up, cell = _planted(L, order)
    u0 = np.ascontiguousarray(up[:nvar])
    f = f7 if grav else None
    u = u0.copy()
    print("\n".join(H.courant_floors_bind(oracle, T, u0, f, smallr, CF, GAMMA)))
    try:
        _load(gpu_lib, monkeypatch, T, u, f, device_order)
        for smallc in (1e-10, T["smallc"][smallr]):
            p, po = _params(oracle, nvar, smallr, smallc)
            for lev in (L + 1, L):
                dx = 1.0 / 2 ** lev
                for kind in KINDS + ("cold1e-10", "cold0.6"):
                    octs = T["lists"][lev][kind]
                    leaves = H.leaf_cells(T, octs)
                    want = H.courant_dt_oracle(oracle, po, u0, f, leaves, dx, CF)
                    if lev == L and kind in ("full", "sub"):
                        assert H.courant_dt_oracle(oracle, po, u0, f, H.oct_cells(T, octs), dx, CF) < want      # the planted cell
                    out = np.full(4, np.nan)
                    check(gpu_lib.ramses_amd_amrres_courant(C.byref(p), len(octs), vp(octs), dx, 1e30, vp(out)))
                    what = "level %d, %s list, smallc %g" % (lev, kind, smallc)
                    assert out[0] == want, (what, out[0], want)
                    for k, (name, terms) in enumerate(zip(("mass", "total energy", "internal energy"), H.courant_sum_terms(u0, leaves, dx, smallr))):
                        s, bound = H.fsum_bound(terms)
                        print("%s: %s %.17g, fsum %.17g, difference %.3e, bound %.3e" % (what, name, out[1 + k], s, abs(out[1 + k] - s), bound))
                        assert abs(out[1 + k] - s) <= bound, (what, name, out[1 + k], s, bound)
                    if kind == "none":
                        assert out[0] == CF * dx / smallc and (out[1:] == 0).all(), out
                    # dt_in below the level's own time step comes back
                    out2 = np.full(4, np.nan)
                    check(gpu_lib.ramses_amd_amrres_courant(C.byref(p), len(octs), vp(octs), dx, 0.5 * want, vp(out2)))
                    assert out2[0] == 0.5 * want and np.array_equal(out2[1:], out[1:]), (what, out2, out)
        _sync(gpu_lib, T, u)
        assert np.array_equal(u, u0)
    finally:
        gpu_lib.ramses_amd_amrres_invalidate()


# ---- synchro_hydro_fine -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,order,device_order,smallr", CASES, ids=IDS)
def test_synchro(gpu_lib, oracle, monkeypatch, L, order, device_order, smallr):
    """the kick by +dt/2 and then by -dt/2 of level L+1, then of level L: after each call the listed cells == the oracle applied
    to the state before the call (the second comparison is with the oracle too, not with the initial state)"""
    from ramses_amd._capi import check
    T, u7, f = H.level_case(L, order)
    p, _ = _params(oracle, 7, smallr)
    for kind in KINDS:
        u = u7.copy()
        try:
            _load(gpu_lib, monkeypatch, T, u, f, device_order)
            for lev in (L + 1, L):
                octs = T["lists"][lev][kind]
                dt = 0.02 / 2 ** lev
                for dteff in (0.5 * dt, -0.5 * dt):
                    before = u.copy()
                    want = H.synchro_oracle(oracle, before, f, H.oct_cells(T, octs), dteff, smallr)
                    if kind != "none":
                        assert (want[1:5] != before[1:5]).any(axis=0).sum() == 8 * len(octs)
                    check(gpu_lib.ramses_amd_amrres_synchro(C.byref(p), len(octs), vp(octs), dteff))
                    _sync(gpu_lib, T, u)
                    _check(T, u, want, before, octs, "synchro of level %d, %s list, dteff %g" % (lev, kind, dteff))
        finally:
            gpu_lib.ramses_amd_amrres_invalidate()


# ---- the cases that come after a sweep share the oracle's sweep of both levels (helpers.oracle_sweeps) -----------------------------

def _device_sweeps(Lb, p, T, interp):
    from ramses_amd._capi import check
    L = T["L"]
    for lev in (L + 1, L):
        ig = T["lists"][lev]["full"]
        dx = 1.0 / 2 ** lev
        check(Lb.ramses_amd_amrres_godunov(C.byref(p), lev, len(ig), vp(ig), dx, 0.02 * dx, 32, interp[0], interp[1]))


SWEPT_CASES = [(4, "scrambled", None, "llf-floor"), (4, "morton", None, "llf-floor"), (6, "scrambled", None, "llf-floor"),
               (6, "scrambled", "0", "llf-floor"), (4, "scrambled", None, "hllc"), (4, "morton", None, "hllc")]
SWEPT_IDS = ["L%d-%s%s-%s" % (c[0], c[1], "-hostorder" if c[2] == "0" else "", c[3]) for c in SWEPT_CASES]


# ---- set_uold with poisson --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,order,device_order,smallr", CASES, ids=IDS)
def test_set_uold_grav_without_a_sweep(gpu_lib, oracle, monkeypatch, L, order, device_order, smallr):
    """set_unew, then set_uold of level L+1 and of level L: add_gravity_source(unew = uold, uold, f, dt) and the scalar fix"""
    from ramses_amd._capi import check
    T, u7, f = H.level_case(L, order)
    p, _ = _params(oracle, 7, smallr)
    for kind in KINDS:
        u = u7.copy()
        try:
            _load(gpu_lib, monkeypatch, T, u, f, device_order)
            _set_unew(gpu_lib, p, T)
            for lev in (L + 1, L):
                octs = T["lists"][lev][kind]
                dt = 0.02 / 2 ** lev
                before = u.copy()
                want = H.set_uold_grav_expected(oracle, before, u7, f, H.oct_cells(T, octs), dt, smallr)
                if kind != "none":
                    assert (want[1:5] != before[1:5]).any(axis=0).sum() == 8 * len(octs)
                check(gpu_lib.ramses_amd_amrres_set_uold_grav(C.byref(p), len(octs), vp(octs), dt))
                _sync(gpu_lib, T, u)
                _check(T, u, want, before, octs, "set_uold_grav of level %d, %s list" % (lev, kind))
        finally:
            gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("L,order,device_order,which", SWEPT_CASES, ids=SWEPT_IDS)
def test_set_uold_grav_after_a_sweep(gpu_lib, oracle, monkeypatch, L, order, device_order, which):
    """set_unew, godunov_fine of level L+1 then L (strict arithmetic), set_uold of level L+1 then L: the oracle's unew through
    add_gravity_source and the scalar fix.  With the high floor the fix changes the scalars of more than 1000 cells at L = 6."""
    from ramses_amd._capi import check
    nvar, riemann, slope, smallr, interp = H.SWEPT[which]
    T, u7, f = H.level_case(L, order)
    unew = H.oracle_sweeps(L, order, which)[0]
    p, _ = _params(oracle, nvar, smallr, riemann=riemann, slope_type=slope)
    for kind in KINDS:
        u = np.ascontiguousarray(u7[:nvar]).copy()
        try:
            _load(gpu_lib, monkeypatch, T, u, f, device_order)
            _set_unew(gpu_lib, p, T)
            _device_sweeps(gpu_lib, p, T, interp)
            for lev in (L + 1, L):
                octs = T["lists"][lev][kind]
                cells = H.oct_cells(T, octs)
                dt = 0.02 / 2 ** lev
                before = u.copy()
                want = H.set_uold_grav_expected(oracle, before, unew, f, cells, dt, smallr)
                if kind == "full" and nvar > 5 and smallr == FLOOR:
                    unfixed = H.gravity_source_oracle(oracle, unew, before, f, cells, dt, smallr)
                    fixed = int((want[5:, cells] != unfixed[5:]).any(axis=0).sum())
                    print("level %d: cells whose passive scalars set_uold's floor fix changes: %d of %d" % (lev, fixed, len(cells)))
                    assert fixed > (1000 if L >= 6 else 0)
                check(gpu_lib.ramses_amd_amrres_set_uold_grav(C.byref(p), len(octs), vp(octs), dt))
                _sync(gpu_lib, T, u)
                _check(T, u, want, before, octs, "set_uold_grav after a sweep, level %d, %s list" % (lev, kind))
        finally:
            gpu_lib.ramses_amd_amrres_invalidate()


# ---- upload_fine ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,order,device_order,smallr", CASES, ids=IDS)
def test_upload_fine(gpu_lib, oracle, monkeypatch, L, order, device_order, smallr):
    """every split cell of the listed octs of level L == upl of its eight children, for interpol_var 0, 1, 2 and NVAR 5, 6, 7 (L = 6:
    the three pairs (0, 5), (1, 6), (2, 7)); the leaf cells of the listed octs and every other cell stay as they were; level L+1
    has no split cell: nothing changes.  Every (interpol_var, NVAR) starts from a freshly loaded state -- interpol_var 1 and 2 restrict alike, so on a
    state that one of them had left a kernel doing nothing for the other would pass -- and every call must change more than half
    of the split cells it is given; within one pair the five calls follow each other (the children never change)."""
    from ramses_amd._capi import check
    T, u7, f = H.level_case(L, order)
    combos = [(iv, nv) for nv in (5, 6, 7) for iv in (0, 1, 2)] if L < 6 else [(0, 5), (1, 6), (2, 7)]
    for ivar, nvar in combos:
        p, _ = _params(oracle, nvar, smallr)
        u = np.ascontiguousarray(u7[:nvar]).copy()
        try:
            _load(gpu_lib, monkeypatch, T, u, None, device_order)       # a fresh state for every (interpol_var, NVAR)
            for lev, kind in ((L, "none"), (L, "sub"), (L, "full"), (L + 1, "full"), (L + 1, "sub")):
                octs = T["lists"][lev][kind]
                before = u.copy()
                want, split = H.upl_oracle(oracle, T, before, octs, ivar, smallr)
                check(gpu_lib.ramses_amd_amrres_upload_fine(C.byref(p), len(octs), vp(octs), ivar))
                _sync(gpu_lib, T, u)
                what = "upload_fine of level %d, %s list, interpol_var %d, NVAR %d" % (lev, kind, ivar, nvar)
                _check(T, u, want, before, octs, what)
                assert len(split) == (0 if lev == L + 1 or kind == "none" else (T["son"][H.oct_cells(T, octs)] > 0).sum())
                if len(split):
                    assert (want[:, split] != before[:, split]).any(axis=0).mean() > 0.5, what      # (the call had something to do)
                leaves = H.leaf_cells(T, octs)
                assert np.array_equal(u[:, leaves], before[:, leaves]), what
        finally:
            gpu_lib.ramses_amd_amrres_invalidate()


# ---- set_uold with pressure_fix ---------------------------------------------------------------------------------------------------

def _check_pfix(T, got, want, before, octs, what):
    for name, g, w, b in zip(("uold", "divu", "enew"), got, want, before):
        _check(T, g, w, b, octs, what + ": " + name)


@pytest.mark.parametrize("grav", [False, True], ids=["nograv", "grav"])
@pytest.mark.parametrize("L,order,device_order,smallr", CASES, ids=IDS)
def test_set_uold_pfix_without_a_sweep(gpu_lib, oracle, monkeypatch, L, order, device_order, smallr, grav):
    """enable_pfix, set_unew_pfix, then set_uold_pfix of level L+1 and of level L with beta_fix = 0.5 and hexp of each level such
    that beta_fix (3 hexp dx)^2 is the 0.4 quantile of the checker's e_cons / d: divu is zero, so this isolates the pdV term (its
    1.5 dx branch at the coarse-fine boundary) and the 3 hexp dx side of the switch's max.  uold, enew and divu == the numpy
    restatement of the reference (helpers.py), after each level."""
    from ramses_amd._capi import check
    T, u7, f7 = H.level_case(L, order)
    f = f7 if grav else None
    p, _ = _params(oracle, 7, smallr)
    for kind in KINDS:
        R = H.pfix_no_sweep_expected(oracle, T, u7, f, {lev: T["lists"][lev][kind] for lev in (L, L + 1)}, smallr, GAMMA, beta_fix=BETA)
        if kind != "none":
            for lev in (L + 1, L):
                r = R["levels"][lev]
                share = r["fired"].mean()
                print("level %d, %s list: hexp %.4f, fired share %.3f, faces at 1.5 dx %d" % (lev, kind, r["hexp"], share, H.coarser_faces(T, T["lists"][lev][kind])))
                assert 0.2 < share < 0.6 and (R["uold"][4, r["cells"][r["fired"]]] != r["before"][r["fired"]]).all()
            assert H.coarser_faces(T, T["lists"][L + 1][kind]) > 0
        u = u7.copy()
        try:
            _load(gpu_lib, monkeypatch, T, u, f, device_order, pfix=True)
            _set_unew(gpu_lib, p, T, pfix=True)
            divu, enew = _sync(gpu_lib, T, u, pfix=True)
            assert np.array_equal(u, u7) and np.array_equal(enew, R["enew0"]) and not divu.any()
            # the checker once more, level by level, for the state after each call
            uold_c, enew_c, divu_c = u7.copy(), R["enew0"].copy(), np.zeros(T["ncell"])
            for lev in (L + 1, L):
                octs = T["lists"][lev][kind]
                dx = 1.0 / 2 ** lev
                dt = 0.02 * dx
                hexp = R["levels"][lev]["hexp"] if kind != "none" else 1.0
                before = (uold_c.copy(), divu_c.copy(), enew_c.copy())
                if kind != "none":
                    H.set_uold_pfix_numpy(oracle, T, octs, uold_c, u7, divu_c, enew_c, f, dx, dt, BETA, hexp, GAMMA, smallr)
                check(gpu_lib.ramses_amd_amrres_set_uold_pfix(C.byref(p), len(octs), vp(octs), dt, dx, BETA, hexp))
                divu, enew = _sync(gpu_lib, T, u, pfix=True)
                _check_pfix(T, (u, divu, enew), (uold_c, divu_c, enew_c), before, octs, "set_uold_pfix of level %d, %s list" % (lev, kind))
            assert np.array_equal(uold_c, R["uold"]) and np.array_equal(enew_c, R["enew"])
        finally:
            gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("L,order,device_order,which", SWEPT_CASES, ids=SWEPT_IDS)
def test_set_uold_pfix_after_a_sweep(gpu_lib, oracle, monkeypatch, L, order, device_order, which):
    """set_unew_pfix, godunov_fine of level L+1 then L, set_uold_pfix of level L+1 then L with hexp = 0 and beta_fix = 0.5: the
    oracle's unew, divu and enew through the gravity source, the pdV term, the scalar fix and the switch on its |divu| dx / dt side"""
    from ramses_amd._capi import check
    nvar, riemann, slope, smallr, interp = H.SWEPT[which]
    T, u7, f = H.level_case(L, order)
    unew, divu_o, enew_o = H.oracle_sweeps(L, order, which)
    u0 = np.ascontiguousarray(u7[:nvar])
    p, _ = _params(oracle, nvar, smallr, riemann=riemann, slope_type=slope)
    for kind in KINDS:
        u = u0.copy()
        try:
            _load(gpu_lib, monkeypatch, T, u, f, device_order, pfix=True)
            _set_unew(gpu_lib, p, T, pfix=True)
            _device_sweeps(gpu_lib, p, T, interp)
            uold_c, divu_c, enew_c = u0.copy(), divu_o.copy(), enew_o.copy()
            fired = []
            for lev in (L + 1, L):
                octs = T["lists"][lev][kind]
                dx = 1.0 / 2 ** lev
                dt = 0.02 * dx
                before = (uold_c.copy(), divu_c.copy(), enew_c.copy())
                if kind != "none":
                    fired.append(H.set_uold_pfix_numpy(oracle, T, octs, uold_c, unew, divu_c, enew_c, f, dx, dt, BETA, 0.0, GAMMA, smallr)["fired"])
                check(gpu_lib.ramses_amd_amrres_set_uold_pfix(C.byref(p), len(octs), vp(octs), dt, dx, BETA, 0.0))
                divu, enew = _sync(gpu_lib, T, u, pfix=True)
                _check_pfix(T, (u, divu, enew), (uold_c, divu_c, enew_c), before, octs,
                            "set_uold_pfix after a sweep, level %d, %s list" % (lev, kind))
            if kind == "full":
                fired = np.concatenate(fired)
                print("after a sweep (%s): the switch fires in %.3f of the cells" % (which, fired.mean()))
                assert fired.any() and not fired.all()
        finally:
            gpu_lib.ramses_amd_amrres_invalidate()

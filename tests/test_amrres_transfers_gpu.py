"""The host <-> device transfers of one level of a resident AMR run (csrc/capi_amr.hip: sync_level, load_level, sync_all,
sync_density, load_f, sync_f, compare_f, sync_rho and the two traffic counters).  Every one of them is a COPY: gather the
8 x ngrid cells of the listed octs from a device vector, cross PCIe, scatter into the host vector through the HOST's list with the
HOST's strides (ncell_h, ngridmax of the host) -- or the reverse.  So every comparison is bit for bit, and every cell that is not
a cell of a listed oct must keep what it held.  Two layouts: the device's own numbering with both levels in tiles (device and
host index spaces differ), and the host's numbering (RAMSES_AMD_DEVICE_ORDER=0).  ngridmax has slack in both, so the host
vectors hold cells of oct indices that are in no list -- the cells a wrong stride or a wrong list would hit.  The lists go down
in the tree's own (scrambled) order."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from helpers import shell_mask
from resident import bits, load, vp

pytestmark = pytest.mark.gpu

POISON = -7.0e77
LAYOUT_VARS = ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_DEVICE_OCTS", "RAMSES_AMD_LIST_CACHE")
GOLD_AMR = os.path.join(os.path.dirname(__file__), "golden", "rho_fine_amr_ref.npz")


@functools.lru_cache(maxsize=None)
def _tree(layout):
    """tiles: level 6 complete, level 7 a shell with octs on the periodic seam (the tile tests' tree, the smallest on which a level
    is stored in tiles); host: levels 1-3 complete and a small box of level-4 octs.  Never modified by a test."""
    from ramses_amd import ic
    if layout == "tiles":
        T = ic.uniform_tree(6, order="scrambled", refine_mask=shell_mask(64), slack=260000)
    else:
        T = ic.uniform_tree(3, refine_box=((2, 5), (1, 4), (3, 6)))
    T["lists"] = (np.ascontiguousarray(T["igrid"]), np.ascontiguousarray(T["igrid_fine"]))
    T["tree_octs"] = np.flatnonzero(T["father"]) + 1                  # every oct of the tree, levels 1 .. L+1 (1-based)
    assert len(T["tree_octs"]) < T["ngridmax"] - 5                    # oct indices that are in no list
    for ig in T["lists"]:
        assert (np.diff(ig) < 0).any()                                # list order, not sorted
    return T


def _cells(T, octs):
    """0-based indices into a host cell vector of the 8 cells of every oct"""
    return np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.asarray(octs, np.int64) - 1 for ind in range(8)])


def _set_layout(monkeypatch, layout):
    for var in LAYOUT_VARS:
        monkeypatch.delenv(var, raising=False)
    if layout == "host":
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", "0")


def _load(L, T, u, layout):
    load(L, T, u)
    assert L.ramses_amd_amrres_tiled_levels() == (2 if layout == "tiles" else 0)


def _f_traffic(L):
    t = np.zeros(2, np.int64)
    assert L.ramses_amd_amrres_f_traffic(vp(t)) == 0
    return t


@pytest.mark.parametrize("layout", ["tiles", "host"])
def test_uold_of_a_level_goes_home_and_comes_back(gpu_lib, monkeypatch, layout):
    """sync_level, load_level, sync_all, sync_density"""
    from ramses_amd._capi import check
    L = gpu_lib
    T = _tree(layout)
    _set_layout(monkeypatch, layout)
    nvar, ncell = 5, T["ncell"]
    rng = np.random.default_rng(101)
    u0 = rng.normal(size=(nvar, ncell))
    u = u0.copy()
    _load(L, T, u, layout)
    try:
        # sync_level: the listed cells, all variables, nothing else
        for ig in T["lists"]:
            c = _cells(T, ig)
            u[:, c] = POISON
            want = u.copy()
            want[:, c] = u0[:, c]
            check(L.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(u)))
            assert np.array_equal(bits(u), bits(want))
        # ... refused for another array than the loaded one (the error it returns today)
        other = u.copy()
        ig = T["lists"][1]
        assert L.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(other)) == -1
        assert b"sync_level: not the array the state was loaded from" in L.ramses_amd_last_error()
        assert np.array_equal(bits(other), bits(u))
        # sync_density: variable 0 of the listed cells, nothing else
        for ig in T["lists"]:
            c = _cells(T, ig)
            u[:, c] = POISON
            want = u.copy()
            want[0, c] = u0[0, c]
            check(L.ramses_amd_amrres_sync_density(len(ig), vp(ig), vp(u)))
            assert np.array_equal(bits(u), bits(want))
        # load_level of new values for one level, then the whole state back
        ig = T["lists"][1]
        c = _cells(T, ig)
        u1 = u0.copy()
        u1[:, c] = rng.normal(size=(nvar, len(c)))
        u[:] = u1
        check(L.ramses_amd_amrres_load_level(len(ig), vp(ig), vp(u)))
        u[:] = POISON
        check(L.ramses_amd_amrres_sync_all(vp(u)))
        if layout == "tiles":
            # the coarse cell and the cells of the tree's octs; the cells of oct indices outside the tree keep what the host holds
            want = np.full((nvar, ncell), POISON)
            tc = np.concatenate([np.arange(T["ncoarse"]), _cells(T, T["tree_octs"])])
            want[:, tc] = u1[:, tc]
        else:
            want = u1            # (the host's numbering: the device vector IS the host's, it comes back whole)
        assert np.array_equal(bits(u), bits(want))
    finally:
        check(L.ramses_amd_amrres_invalidate())


@pytest.mark.parametrize("layout", ["tiles", "host"])
def test_the_acceleration_of_a_level_goes_down_and_comes_home(gpu_lib, monkeypatch, layout):
    """load_f, sync_f, compare_f, f_traffic"""
    from ramses_amd._capi import check
    L = gpu_lib
    T = _tree(layout)
    _set_layout(monkeypatch, layout)
    ncell = T["ncell"]
    rng = np.random.default_rng(103)
    u = rng.normal(size=(5, ncell))
    f = rng.normal(size=(3, ncell))
    _load(L, T, u, layout)
    try:
        listed = np.zeros(ncell, bool)
        for ig in T["lists"]:
            t0 = _f_traffic(L)
            check(L.ramses_amd_amrres_load_f(len(ig), vp(ig), vp(f)))
            assert np.array_equal(_f_traffic(L) - t0, [3 * 8 * 8 * len(ig), 0])
            listed[_cells(T, ig)] = True
        assert L.ramses_amd_amrres_has_gravity() == 1
        got = np.full((3, ncell), POISON)
        for ig in T["lists"]:
            t0 = _f_traffic(L)
            check(L.ramses_amd_amrres_sync_f(len(ig), vp(ig), vp(got)))
            assert np.array_equal(_f_traffic(L) - t0, [0, 3 * 8 * 8 * len(ig)])
        want = np.full((3, ncell), POISON)
        want[:, listed] = f[:, listed]
        assert np.array_equal(bits(got), bits(want))
        # compare_f: equal; then k cells of listed octs changed by known amounts
        maxdiff, ndiff = C.c_double(-1.0), C.c_int64(-1)
        t0 = _f_traffic(L)
        for ig in T["lists"]:
            check(L.ramses_amd_amrres_compare_f(len(ig), vp(ig), vp(f), C.byref(maxdiff), C.byref(ndiff)))
            assert (maxdiff.value, ndiff.value) == (0.0, 0)
        ig = T["lists"][1]
        c = _cells(T, ig)
        k = 7
        pick = rng.choice(c, size=k, replace=False)
        comp = rng.integers(0, 3, k)
        f2 = f.copy()
        f2[comp, pick] += 2.0 ** np.arange(-3, k - 3)
        amounts = np.abs(f[comp, pick] - f2[comp, pick])
        assert (amounts > 0).all()
        check(L.ramses_amd_amrres_compare_f(len(ig), vp(ig), vp(f2), C.byref(maxdiff), C.byref(ndiff)))
        assert ndiff.value == k and maxdiff.value == amounts.max()
        # ... and the other level's list sees none of them
        ig = T["lists"][0]
        check(L.ramses_amd_amrres_compare_f(len(ig), vp(ig), vp(f2), C.byref(maxdiff), C.byref(ndiff)))
        assert (maxdiff.value, ndiff.value) == (0.0, 0)
        assert np.array_equal(_f_traffic(L), t0)              # compare_f is not counted
    finally:
        check(L.ramses_amd_amrres_invalidate())


@pytest.mark.parametrize("layout", ["device", "host"])
def test_the_deposit_of_a_level_comes_home(gpu_lib, monkeypatch, layout):
    """sync_rho, rho_traffic: on the tree and density of the reference's rho_fine dump, in both numberings"""
    import ramses_amd
    from ramses_amd._capi import check
    L = gpu_lib
    _set_layout(monkeypatch, layout)
    z = np.load(GOLD_AMR)
    k = "c%d_" % int(z["calls"][0])
    ilevel, icount, ngrid, ngridmax, ncoarse, levelmin, nvector = [int(x) for x in z[k + "meta"]]
    boxlen, smallr = [float(x) for x in z[k + "real"]]
    nlevelmax = int(z[k + "nlevelmax"][0])
    first = np.ascontiguousarray(z[k + "first"], np.int32)
    igrid_all = np.ascontiguousarray(z[k + "igrid_all"], np.int32)
    son, nbor, father = (np.ascontiguousarray(z[k + n], np.int32) for n in ("son", "nbor", "father"))
    xg = np.ascontiguousarray(z[k + "xg"])
    ncell = ncoarse + 8 * ngridmax
    rng = np.random.default_rng(5)
    uold = rng.uniform(0.5, 1.5, (5, ncell))
    uold[0] = z[k + "dens"]
    p = ramses_amd.make_params(smallr=smallr)
    check(L.ramses_amd_amrres_invalidate())
    check(L.ramses_amd_amrres_load(5, ngridmax, ncoarse, vp(uold), vp(son), vp(nbor), vp(father)))
    try:
        rho = np.full(ncell, POISON)
        mp = np.zeros(4)
        check(L.ramses_amd_amrres_xg(vp(xg)))
        check(L.ramses_amd_amrres_rho_fine(C.byref(p), ilevel, nlevelmax, levelmin, nvector, vp(first), vp(igrid_all), boxlen, vp(rho), vp(mp)))
        nlev = 0
        for li in range(len(first) - 1):
            ig = np.ascontiguousarray(igrid_all[first[li]:first[li + 1]])
            if len(ig) == 0:
                continue
            lev = np.zeros(ncell, bool)
            for ind in range(8):
                lev[ncoarse + ind * ngridmax + ig - 1] = True
            assert (rho[lev] != POISON).all()
            got = np.full(ncell, POISON)
            t0 = L.ramses_amd_amrres_rho_traffic()
            check(L.ramses_amd_amrres_sync_rho(len(ig), vp(ig), vp(got)))
            assert L.ramses_amd_amrres_rho_traffic() - t0 == 8 * 8 * len(ig)
            want = np.full(ncell, POISON)
            want[lev] = rho[lev]
            assert np.array_equal(bits(got), bits(want))
            nlev += 1
        assert nlev >= 2
        # an empty list: nothing moves, nothing is counted
        got = np.full(ncell, POISON)
        t0 = L.ramses_amd_amrres_rho_traffic()
        assert L.ramses_amd_amrres_sync_rho(0, vp(igrid_all), vp(got)) == 0
        assert L.ramses_amd_amrres_rho_traffic() == t0 and (got == POISON).all()
    finally:
        check(L.ramses_amd_amrres_invalidate())


def test_an_empty_list_moves_nothing(gpu_lib, monkeypatch):
    """ngrid = 0: sync_f and sync_density return 0 and leave the host array alone (sync_rho: in the test above)"""
    from ramses_amd._capi import check
    L = gpu_lib
    T = _tree("host")
    _set_layout(monkeypatch, "host")
    ncell = T["ncell"]
    rng = np.random.default_rng(107)
    u = rng.normal(size=(5, ncell))
    f = rng.normal(size=(3, ncell))
    _load(L, T, u, "host")
    try:
        ig = T["lists"][1]
        check(L.ramses_amd_amrres_load_f(len(ig), vp(ig), vp(f)))
        t0 = _f_traffic(L)
        got = np.full((3, ncell), POISON)
        assert L.ramses_amd_amrres_sync_f(0, vp(ig), vp(got)) == 0
        assert (got == POISON).all() and np.array_equal(_f_traffic(L), t0)
        want = u.copy()
        assert L.ramses_amd_amrres_sync_density(0, vp(ig), vp(u)) == 0
        assert np.array_equal(bits(u), bits(want))
    finally:
        check(L.ramses_amd_amrres_invalidate())

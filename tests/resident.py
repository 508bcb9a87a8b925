"""Shared test helpers: a synthetic two-level tree in the resident AMR state of the library (the ramses_amd_amrres_* entries of the
C ABI), swept on the device and by the C oracle.  T is ic.uniform_tree's dict with, from two_level_tree, T["L"], T["all_octs"]
(per level, sorted) and T["lists"] (per level, the tree's own order)."""
import ctypes as C

import numpy as np

from helpers import shell_mask

LAYOUT_VARS = ("RAMSES_AMD_DEVICE_ORDER", "RAMSES_AMD_TILES", "RAMSES_AMD_TILE_DENSE", "RAMSES_AMD_COVERED_DENSE", "RAMSES_AMD_TILE_SWEEP")
ALL_LAYOUT_VARS = LAYOUT_VARS + ("RAMSES_AMD_DIFMAG_TILES", "RAMSES_AMD_SORTED_LISTS", "RAMSES_AMD_LIST_CACHE")


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def i32(*v):
    return (C.c_int * len(v))(*v)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def force_tiles(monkeypatch, clear=LAYOUT_VARS, **setenv):
    """levels below RAMSES_AMD_TILE_MIN_OCTS octs take the tree-walking sweep in production: the tests force the tiles; the
    switches of `clear` are unset, those of `setenv` set"""
    monkeypatch.setenv("RAMSES_AMD_TILE_MIN_OCTS", "0")
    for var, value in setenv.items():
        monkeypatch.setenv(var, value)
    for var in clear:
        monkeypatch.delenv(var, raising=False)


def reset_library():
    """no resident state, the coarse grid back to one cell (the setting holds for every later load of the process)"""
    import ramses_amd
    lib = ramses_amd.lib()
    lib.ramses_amd_amrres_invalidate()
    lib.ramses_amd_amrres_coarse_grid(1, 1, 1)


def two_level_tree(L, order, mask=None, slack=260000):
    """level L complete, level L+1 where mask says (default: the tile tests' shell)"""
    from ramses_amd import ic
    T = ic.uniform_tree(L, order=order, refine_mask=shell_mask(2 ** L) if mask is None else mask, slack=slack)
    T["L"] = L
    T["all_octs"] = {L: np.ascontiguousarray(np.sort(T["igrid"])), L + 1: np.ascontiguousarray(np.sort(T["igrid_fine"]))}
    T["lists"] = {L: np.ascontiguousarray(T["igrid"]), L + 1: np.ascontiguousarray(T["igrid_fine"])}
    return T


def _levels(T):
    return [T["all_octs"][lev] for lev in sorted(T["all_octs"])]


def load(Lb, T, u, f=None, levels=None, pfix=False, grid=None, xg=None):
    """a fresh resident state: the tree and u (the array every later sync writes into), the oct centres xg, the acceleration f
    of the octs of `levels` (default: both levels of two_level_tree), pressure_fix enabled"""
    from ramses_amd._capi import check
    check(Lb.ramses_amd_amrres_invalidate())
    if grid is not None:
        check(Lb.ramses_amd_amrres_coarse_grid(*grid))
    check(Lb.ramses_amd_amrres_load(u.shape[0], T["ngridmax"], T["ncoarse"], vp(u), vp(T["son"]), vp(T["nbor"]), vp(T["father"])))
    if xg is not None:
        check(Lb.ramses_amd_amrres_xg(vp(xg)))
    if f is not None:
        for ig in (_levels(T) if levels is None else levels):
            check(Lb.ramses_amd_amrres_load_f(len(ig), vp(ig), vp(f)))
    if pfix:
        check(Lb.ramses_amd_amrres_enable_pfix())


def set_unew(Lb, p, T, pfix=False):
    """set_unew on both levels; with pressure_fix: the divu / enew it leaves (host vectors)"""
    from ramses_amd._capi import check
    divu, enew = np.zeros(T["ncell"]), np.zeros(T["ncell"])
    for ig in _levels(T):
        if pfix:
            check(Lb.ramses_amd_amrres_set_unew_pfix(C.byref(p), len(ig), vp(ig)))
            check(Lb.ramses_amd_amrres_sync_pfix(len(ig), vp(ig), vp(divu), vp(enew)))
        else:
            check(Lb.ramses_amd_amrres_set_unew(len(ig), vp(ig)))
    return (divu, enew) if pfix else None


def sweep(Lb, p, T, lev, ivar, itype, dtfac=0.02):
    from ramses_amd._capi import check
    ig = T["lists"][lev]
    dx = 1.0 / 2 ** lev
    check(Lb.ramses_amd_amrres_godunov(C.byref(p), lev, len(ig), vp(ig), dx, dtfac * dx, 32, ivar, itype))


def sweep_levels(Lb, p, T, interp, dtfac=0.02):
    """godunov_fine of level L+1 then L (the order of amr_step); returns (sweeps through the tiles, sweeps through the tree)"""
    t0, w0 = Lb.ramses_amd_amrres_tile_sweeps(), Lb.ramses_amd_amrres_tree_sweeps()
    for lev in (T["L"] + 1, T["L"]):
        sweep(Lb, p, T, lev, interp[0], interp[1], dtfac)
    return Lb.ramses_amd_amrres_tile_sweeps() - t0, Lb.ramses_amd_amrres_tree_sweeps() - w0


def set_uold(Lb, p, T):
    from ramses_amd._capi import check
    for ig in _levels(T):
        check(Lb.ramses_amd_amrres_set_uold(C.byref(p), len(ig), vp(ig)))


def sync(Lb, T, u):
    from ramses_amd._capi import check
    for ig in _levels(T):
        check(Lb.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(u)))
    return u


def read_back(Lb, p, T, u, pfix=False):
    """set_uold and sync of both levels (u: the array the state was loaded from); with pressure_fix divu and enew before it"""
    from ramses_amd._capi import check
    divu, enew = np.zeros(T["ncell"]), np.zeros(T["ncell"])
    for ig in _levels(T):
        if pfix:
            check(Lb.ramses_amd_amrres_sync_pfix(len(ig), vp(ig), vp(divu), vp(enew)))
        check(Lb.ramses_amd_amrres_set_uold(C.byref(p), len(ig), vp(ig)))
        check(Lb.ramses_amd_amrres_sync_level(len(ig), vp(ig), vp(u)))
    return (u, divu, enew) if pfix else (u,)


def oracle_sweep(oracle, po, T, lev, uold, unew, ivar, itype, f=None, divu=None, enew=None, dtfac=0.02):
    dx = 1.0 / 2 ** lev
    oracle.godunov_fine_amr(po, T["lists"][lev], T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew, dx, dtfac * dx, 32,
                            ivar, itype, f=f, divu=divu, enew=enew)


def oracle_step(oracle, po, T, uold, f, interp, divu=None, enew=None):
    """godunov_fine of level L+1 then L by the oracle: unew; divu and enew are added to in place"""
    unew = uold.copy()
    for lev in (T["L"] + 1, T["L"]):
        oracle_sweep(oracle, po, T, lev, uold, unew, interp[0], interp[1], f=f, divu=divu, enew=enew)
    return unew


def compare(got, ref, cells, exact_solver, names=("unew", "divu", "enew")):
    """bit for bit in the cells; riemann = 'exact' calls pow(), whose last ulp is the device's: relative 1e-12 of each variable's
    maximum.  got / ref: one array or a tuple of them, named by names"""
    if isinstance(got, np.ndarray):
        got, ref = (got,), (ref,)
    for name, g, r in zip(names, got, ref):
        g, r = np.atleast_2d(g)[:, cells], np.atleast_2d(r)[:, cells]
        if exact_solver:
            scale = np.abs(r).max(axis=-1, keepdims=True)
            err = (np.abs(g - r) / scale).max()
            print(name, "max relative difference", err)
            assert err <= 1e-12, (name, err)
        else:
            print(name, "cells that differ", int((g != r).any(axis=0).sum()), "of", len(cells), "max abs difference", np.abs(g - r).max())
            assert np.array_equal(g, r), (name, np.abs(g - r).max())

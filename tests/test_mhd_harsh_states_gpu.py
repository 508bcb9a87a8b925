"""The device MHD sweep on the harsh state (tests/helpers.py harsh_mhd_brick: super-fast, floored, partly unmagnetised) and on
bricks that are no cubes: ramses_amd_mhd_godunov_brick through MhdLevel against the COMPILED REFERENCE used oct by oct
(StencilReference of tests/test_mhd_gpu.py), bit for bit in all eleven fields after each of two steps.

Shapes (nx, ny, nz), each for an edge of an index map of csrc/mhd_sweep.hip:
  4^3, 8^3        the smallest level and level 3 of the drop-in
  (38, 10, 6)     fused tiles 32 + 6 in x, 4 + 4 + 2 in y, 4 + 2 in z; nz < 8: two empty XCD slabs; N = 35 * 64 + 40
  (12, 18, 10)    y strip 16 + 2; three empty slabs; N = 33 * 64 + 48
  (70, 6, 12)     three x tiles; rows that straddle wavefronts
  (6, 4, 20)      three planes per slab: slab 6 holds two, slab 7 none
Every case computes the reference first and holds IT to caps set before any device ran: finite, > 0.9 of the cells changed,
densities <= 0 in at most 0.5 % of the cells and none below -0.1.  Two rows run again through the three-kernel path
(RAMSES_AMD_MHD_FUSED=0), and the fast build (RAMSES_AMD_MHD_FAST=1) is held to 1e-12 of each variable's maximum against the
reference after one step.  The resident entry points (courant / godunov / set_uold / sync) run on harsh cubes of level 3 and 4
with a scrambled oct list.  The CPU leg of the same state: tests/test_mhd_core_host.py, tests/test_mhd_harsh_state_branches.py."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.path.join(ROOT, "oracle", "_ref", "libref_kernels3d_mhd.so")
GAMMA, SMALLC, THETA, SEED = 5.0 / 3.0, 1e-10, 1.5, 12
DX = 1.0 / 32
DT = 0.02 * DX
TOL = 1e-12

# (riemann, riemann2d, slope_type | (slope_type, slope_mag_type), (nx, ny, nz), smallr): every 1-D and 2-D solver, slopes 0, 1, 2,
# 7, 8 and (3, 1), every shape at least twice, both floors.  (On (6, 4, 20) the floor 0.6 goes with roe / hlld: with the unlimited
# slopes of type 0 the REFERENCE leaves 3 of its 480 densities <= 0 after two steps, above the cap of 0.5 %.)
TABLE = [
    ("hlld", "hlld", 2, (38, 10, 6), 1e-10),
    ("hlld", "hlld", 2, (70, 6, 12), 0.6),
    ("llf", "llf", 1, (12, 18, 10), 0.6),
    ("hll", "hlla", 7, (12, 18, 10), 1e-10),
    ("roe", "roe", 1, (38, 10, 6), 0.6),
    ("roe", "hlld", 8, (6, 4, 20), 0.6),
    ("hll", "hll", 7, (70, 6, 12), 1e-10),
    ("upwind", "upwind", 1, (4, 4, 4), 0.6),
    ("hydro", "hlla", 2, (8, 8, 8), 1e-10),
    ("hlld", "roe", 0, (6, 4, 20), 1e-10),
    ("llf", "upwind", (3, 1), (8, 8, 8), 0.6),
    ("hlld", "llf", 8, (4, 4, 4), 1e-10),
    ("llf", "hll", 0, (12, 18, 10), 1e-10),
    ("upwind", "hlld", 7, (38, 10, 6), 1e-10),
]
THREE_KERNELS = [TABLE[0], TABLE[10]]          # both instances of the stand-alone trace kernel (slope_type 3 or not)
FAST = [(r, r2, s, shape, smallr) for smallr in (1e-10, 0.6)
        for r, r2, s, shape in (("hlld", "hlld", 2, (38, 10, 6)), ("hlld", "hlld", 2, (70, 6, 12)), ("llf", "llf", 1, (12, 18, 10)),
                                ("hll", "hlla", 7, (12, 18, 10)))]

_cache = {}


def _slopes(slope_type):
    return slope_type if isinstance(slope_type, tuple) else (slope_type, -1)


def reference(row):
    """(u0, [u after step 1, u after step 2]) of the compiled reference, computed once per row, read-only, and held to the caps"""
    if row in _cache:
        return _cache[row]
    from helpers import harsh_mhd_brick
    from ramses_amd.mhd import RIEMANN, RIEMANN2D
    from test_mhd_gpu import StencilReference
    riemann, riemann2d, slope_type, (nx, ny, nz), smallr = row
    st, sm = _slopes(slope_type)
    u0 = harsh_mhd_brick(nx, ny, nz, seed=SEED, gamma=GAMMA)
    ref = StencilReference(GAMMA, smallr, SMALLC, st, THETA, RIEMANN[riemann], RIEMANN2D[riemann2d], slope_mag_type=None if sm == -1 else sm)
    steps, u = [], u0
    for n in range(2):
        u = ref.step(u, DX, DT)
        nonpos = u[0] <= 0
        print("reference %s step %d: changed %.3f, rho <= 0 in %d of %d cells, min rho %.4g, growth of the maxima %s" % (
            row, n + 1, (u != u0).any(axis=0).mean(), nonpos.sum(), nonpos.size, u[0].min(),
            np.round(np.abs(u).reshape(11, -1).max(1) / np.maximum(np.abs(u0).reshape(11, -1).max(1), 1e-300), 2)))
        assert np.isfinite(u).all()
        assert (u != u0).any(axis=0).mean() > 0.9
        assert nonpos.mean() <= 0.005 and u[0].min() >= -0.1
        u.setflags(write=False)
        steps.append(u)
    u0.setflags(write=False)
    _cache[row] = (u0, steps)
    return _cache[row]


def _level(row):
    from ramses_amd.mhd import MhdLevel, make_mhd_params
    riemann, riemann2d, slope_type, (nx, ny, nz), smallr = row
    st, sm = _slopes(slope_type)
    return MhdLevel(nx, ny, nz, DX, params=make_mhd_params(gamma=GAMMA, smallr=smallr, smallc=SMALLC, slope_type=st, slope_mag_type=sm,
                                                           slope_theta=THETA, riemann=riemann, riemann2d=riemann2d))


def _structure(got):
    """right faces == the neighbours' left faces, bit for bit; div B at rounding (field units: face differences)"""
    for c, ax in ((0, 2), (1, 1), (2, 0)):
        assert np.array_equal(got[8 + c], np.roll(got[5 + c], -1, axis=ax))
    div = (got[8] - got[5]) + (got[9] - got[6]) + (got[10] - got[7])
    assert np.abs(div).max() <= 1e-13 * max(1.0, np.abs(got[5:11]).max())


def _strict(row):
    import torch
    u0, steps = reference(row)
    lev = _level(row)
    lev.upload(u0.copy())
    for n, want in enumerate(steps):
        lev.step(DT)
        torch.cuda.synchronize()
        got = lev.download()
        if not np.array_equal(got, want):
            bad = [int(v) for v in range(11) if not np.array_equal(got[v], want[v])]
            where = np.argwhere((got != want).any(axis=0))
            raise AssertionError("step %d: fields %s differ in %d cells, first (k, j, i) = %s, max |diff| %g" % (
                n + 1, bad, len(where), where[0], np.nanmax(np.abs(got - want))))
        _structure(got)


def _need_ref():
    if not os.path.exists(REF):
        pytest.skip("oracle/_ref/libref_kernels3d_mhd.so not built")


@pytest.mark.parametrize("row", TABLE, ids=lambda r: "%s-%s-%s-%dx%dx%d-%g" % (r[0], r[1], r[2], *r[3], r[4]))
def test_harsh_brick_equals_the_compiled_reference(gpu_lib, monkeypatch, row):
    _need_ref()
    monkeypatch.delenv("RAMSES_AMD_MHD_FAST", raising=False)
    monkeypatch.delenv("RAMSES_AMD_MHD_FUSED", raising=False)
    _strict(row)


@pytest.mark.parametrize("row", THREE_KERNELS, ids=lambda r: "%s-%s-%s-%dx%dx%d-%g" % (r[0], r[1], r[2], *r[3], r[4]))
def test_harsh_brick_through_the_three_kernel_path(gpu_lib, monkeypatch, row):
    """RAMSES_AMD_MHD_FUSED=0 (mhd_prim_kernel, mhd_efield_kernel, mhd_trace_kernel instead of the fused one), read on every call"""
    _need_ref()
    monkeypatch.delenv("RAMSES_AMD_MHD_FAST", raising=False)
    monkeypatch.setenv("RAMSES_AMD_MHD_FUSED", "0")
    _strict(row)


def _rel(got, ref):
    """the shared scales of test_mhd_fast_certificate_gpu._rel on the conservative fields: the three momenta share one scale, the
    six face fields share one (its layout is rho, three velocities, six fields, one more)"""
    from test_mhd_fast_certificate_gpu import _rel as rel
    order = [0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 4]
    return rel(got[order], ref[order])


@pytest.mark.parametrize("row", FAST, ids=lambda r: "%s-%s-%s-%dx%dx%d-%g" % (r[0], r[1], r[2], *r[3], r[4]))
def test_fast_build_within_1e12_of_the_reference_on_the_harsh_state(gpu_lib, monkeypatch, row):
    """one step of the fast build against the reference (never against the strict device build): rel-Linf <= 1e-12 of each
    variable's maximum; faces bit for bit; not the reference's bits, since fast did run.  The measured figures of an MI355X run
    are in profiles/mhd_harsh_fast.txt."""
    _need_ref()
    import torch
    u0, steps = reference(row)
    want = steps[0]
    if row[:2] == ("hll", "hlla"):       # (a solver that amplifies this state is compared bit for bit only)
        growth = np.abs(want).reshape(11, -1).max(1) / np.maximum(np.abs(u0).reshape(11, -1).max(1), 1e-300)
        assert (growth <= 2.0).all(), growth
    monkeypatch.delenv("RAMSES_AMD_MHD_FUSED", raising=False)
    monkeypatch.setenv("RAMSES_AMD_MHD_FAST", "1")
    lev = _level(row)
    lev.upload(u0.copy())
    lev.step(DT)
    torch.cuda.synchronize()
    got = lev.download()
    err = _rel(got, want)
    print("MHD_HARSH_FAST %s/%s slope %s %dx%dx%d smallr %g: rel-Linf (rho, 3 momenta, 6 fields, E) = %s" % (
        row[0], row[1], row[2], *row[3], row[4], " ".join("%.2e" % e for e in err)))
    assert np.isfinite(got).all()
    _structure(got)
    assert not np.array_equal(got, want)
    assert (err <= TOL).all(), err


# ---- the resident entry points at kernel level -----------------------------------------------------------------------------

def _cell_terms(u, vol):
    """the per-cell terms of courant_fine's four sums (mass, total, internal, magnetic energy), in the order of the kernel"""
    mass, etot = u[0] * vol, u[4] * vol
    ei, em = u[4] * vol, np.zeros_like(u[0])
    for d in range(3):
        b = u[5 + d] + u[8 + d]
        em = em + 0.125 * (b * b) * vol
        ei = ei - 0.5 * (u[1 + d] * u[1 + d]) / u[0] * vol - 0.125 * (b * b) * vol
    return mass, etot, ei, em


def _ref_dt(cells, dx, cfl, smallr):
    """min over the cells of the compiled cmpdt, nvec cells at a time"""
    ref = C.CDLL(REF)
    nd, nvar, nvec = C.c_int(), C.c_int(), C.c_int()
    ref.ref_mhd_get_dims(C.byref(nd), C.byref(nvar), C.byref(nvec))
    nvec = nvec.value
    ref.ref_mhd_set_params(C.c_double(GAMMA), C.c_double(smallr), C.c_double(SMALLC), 2, 2, C.c_double(THETA), 3, 5)
    ref.ref_mhd_cmpdt.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p]
    best = math.inf
    for b0 in range(0, cells.shape[1], nvec):
        n = min(nvec, cells.shape[1] - b0)
        work = np.zeros((11, nvec))
        work[:, :n] = cells[:, b0:b0 + n]
        dt = C.c_double()
        ref.ref_mhd_cmpdt(work.ctypes.data_as(C.c_void_p), dx, cfl, n, C.byref(dt))
        best = min(best, dt.value)
    return best


@pytest.mark.parametrize("smallr", [1e-10, 0.6])
@pytest.mark.parametrize("level", [3, 4])
def test_resident_entry_points_on_a_scrambled_oct_list(gpu_lib, monkeypatch, level, smallr):
    _need_ref()
    import torch
    from helpers import harsh_mhd_brick
    from ramses_amd._capi import check, lib
    from ramses_amd.mhd import MhdLevel, make_mhd_params
    monkeypatch.delenv("RAMSES_AMD_MHD_FAST", raising=False)
    monkeypatch.delenv("RAMSES_AMD_MHD_FUSED", raising=False)
    n = 1 << level
    dx, cfl = 1.0 / n, 0.8
    u = harsh_mhd_brick(n, n, n, seed=SEED, gamma=GAMMA)
    rng = np.random.default_rng(100 + level)
    ngrid = n ** 3 // 8
    ngridmax, ncoarse = ngrid + 37, 1
    ncell = ncoarse + 8 * ngridmax
    igrid = (rng.permutation(ngridmax)[:ngrid] + 1).astype(np.int32)          # the octs' slots, in list order
    octs = rng.permutation(ngrid)                                             # which oct of the lattice the g-th list entry is
    ok, oj, oi = np.unravel_index(octs, (n // 2, n // 2, n // 2))
    xg = np.full((3, ngridmax), -7.0)                                         # Fortran xg(1:ngridmax, 1:3): the oct centres
    for d, o in enumerate((oi, oj, ok)):
        xg[d, igrid - 1] = (2 * o + 1) / n
    poison = rng.uniform(1.0, 2.0, (11, ncell))                               # Fortran uold(1:ncell, 1:11)
    uold = poison.copy()
    cell = np.empty((8, ngrid), dtype=np.int64)                               # 0-based index of cell ind of list entry g
    for ind in range(8):
        cell[ind] = ncoarse + ind * ngridmax + (igrid - 1)
        uold[:, cell[ind]] = u[:, 2 * ok + (ind >> 2 & 1), 2 * oj + (ind >> 1 & 1), 2 * oi + (ind & 1)]
    inside = np.zeros(ncell, dtype=bool)
    inside[cell.ravel()] = True
    assert inside.sum() == n ** 3
    loaded = uold.copy()
    p = make_mhd_params(gamma=GAMMA, smallr=smallr, smallc=SMALLC, slope_type=2, slope_theta=THETA, riemann="hlld", riemann2d="hlld")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    args = (C.byref(p), level, ngrid, vp(igrid), vp(xg), ngridmax, ncoarse, 1, vp(uold))
    # what the reference says, before anything runs on the device
    cells = np.ascontiguousarray(u.reshape(11, -1))
    dt_ref = _ref_dt(cells, dx, cfl, smallr)
    sums = [math.fsum(t.ravel()) for t in _cell_terms(u, dx ** 3)]
    bits = lambda x: np.float64(x).view(np.int64)      # noqa: E731
    try:
        for dt_in in (2.0 * dt_ref, 0.5 * dt_ref):
            out5 = np.zeros(5)
            check(lib().ramses_amd_mhd_resident_courant_f90(*args, dx, dt_in, cfl, vp(out5)))
            assert bits(out5[0]) == bits(min(dt_in, dt_ref)), (out5[0], dt_in, dt_ref)
            for got, want in zip(out5[1:], sums):
                assert abs(got - want) <= 1e-12 * abs(want), (out5, sums)
        dt = 0.02 * dx
        check(lib().ramses_amd_mhd_resident_godunov_f90(*args, dx, dt))
        check(lib().ramses_amd_mhd_resident_set_uold_f90(level))
        check(lib().ramses_amd_mhd_resident_sync_host_f90(vp(uold)))
    finally:
        lib().ramses_amd_mhd_resident_sync_host_f90(vp(uold))      # (a failure above may have left the host array stale)
        check(lib().ramses_amd_mhd_resident_invalidate())
    # the brick path on the same state
    lev = MhdLevel(n, n, n, dx, params=p)
    lev.upload(u)
    lev.step(dt)
    torch.cuda.synchronize()
    want = lev.download()
    assert not np.array_equal(want, u)
    for ind in range(8):
        got = uold[:, cell[ind]]
        assert np.array_equal(got, want[:, 2 * ok + (ind >> 2 & 1), 2 * oj + (ind >> 1 & 1), 2 * oi + (ind & 1)]), ind
    assert np.array_equal(uold[:, ~inside].view(np.int64), loaded[:, ~inside].view(np.int64))      # every other cell untouched

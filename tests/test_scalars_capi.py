"""CPU tests of passive scalars beyond NVAR=7 at the C ABI: the brick entry points take 5+NENER <= NVAR <=
RAMSES_AMD_MAX_NVAR, everything outside that range -- and every AMR, tile and tree-walking entry point at NVAR > 7 --
is refused with RAMSES_AMD_EUNSUPPORTED and a message that names NVAR.  Validation runs before any device work, so
no GPU is needed.  The CPU oracle, which the GPU tests compare against, is checked beyond NVAR=7 by the independence of
the scalars it sweeps."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from helpers import random_brick

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUPPORTED, EINVAL = -2, -1


@pytest.fixture(scope="module")
def L():
    from ramses_amd import _capi, build
    build.build()
    return _capi.lib()


def _err(L):
    return L.ramses_amd_last_error().decode()


def _sweep(L, p):
    from ramses_amd import _capi
    b = _capi.dense_brick(16, 16, 16, 0)
    return L.ramses_amd_godunov_brick(C.byref(p), C.byref(b), C.c_void_p(8), None, C.c_void_p(16), 0.1, 0.01, None)


def test_header_and_binding_agree_on_max_nvar():
    from ramses_amd import _capi
    h = open(os.path.join(ROOT, "include", "ramses_amd.h")).read()
    assert int(re.search(r"#define RAMSES_AMD_MAX_NVAR (\d+)", h).group(1)) == _capi.MAX_NVAR == 16


def test_make_params_takes_nvar_16():
    from ramses_amd import _capi
    assert _capi.make_params(nvar=16).nvar == 16
    assert _capi.make_params(nvar=16, nener=2).nener == 2


def test_brick_sweep_refuses_nvar_17(L):
    from ramses_amd import _capi
    assert _sweep(L, _capi.make_params(nvar=17)) == EUNSUPPORTED
    assert "NVAR=17" in _err(L) and "ramses_amd_godunov_brick" in _err(L)


def test_brick_sweep_refuses_nvar_below_5_plus_nener(L):
    from ramses_amd import _capi
    assert _sweep(L, _capi.make_params(nvar=4)) == EUNSUPPORTED
    assert "NVAR=4" in _err(L)
    assert _sweep(L, _capi.make_params(nvar=6, nener=2)) == EUNSUPPORTED
    assert "NVAR >= 7" in _err(L) and "got 6" in _err(L)


def test_brick_sweep_refuses_plmde_with_scalars(L):
    from ramses_amd import _capi
    for nvar in (6, 8, 16):
        assert _sweep(L, _capi.make_params(nvar=nvar, scheme="plmde")) == EUNSUPPORTED
        assert "plmde" in _err(L) and ("NVAR=%d" % nvar) in _err(L)


def test_staged_and_mpi_resident_setup_refuse_nvar_17(L):
    from ramses_amd import _capi
    p = C.byref(_capi.make_params(nvar=17))
    z = None
    n0 = (C.c_int * 1)(0)
    assert L.ramses_amd_godunov_fine_host(p, 4, 512, C.c_void_p(8), C.c_void_p(8), 512, 1, 1, C.c_void_p(8), C.c_void_p(8),
                                          z, 0.1, 0.01) == EUNSUPPORTED
    assert "NVAR=17" in _err(L)
    assert L.ramses_amd_mpires_setup(p, 4, 512, C.c_void_p(8), C.c_void_p(8), 512, 1, 1, C.c_void_p(8), C.c_void_p(8),
                                     1, 1, n0, z, n0, z) == EUNSUPPORTED
    assert "NVAR=17" in _err(L) and "ramses_amd_mpires_setup" in _err(L)


def test_tile_tree_and_amr_entry_points_refuse_nvar_8(L):
    from ramses_amd import _capi
    p = C.byref(_capi.make_params(nvar=8))
    z = None
    calls = {
        "ramses_amd_godunov_fine_amr_host": lambda: L.ramses_amd_godunov_fine_amr_host(
            p, 4, 8, z, z, z, z, 8, 1, z, z, z, z, z, 0.1, 0.01, 32, 0, 1),
        "ramses_amd_godunov_fine_amr_f90": lambda: L.ramses_amd_godunov_fine_amr_f90(
            p, 4, 8, z, z, z, z, 8, 1, z, z, z, 0, z, z, 0, 0.1, 0.01, 32, 0, 1),
        "ramses_amd_godunov_fine_amr_device": lambda: L.ramses_amd_godunov_fine_amr_device(
            p, 4, 8, z, z, z, z, 8, 1, z, z, z, z, z, 0.1, 0.01, 32, 0, 1, z, z, z),
        "ramses_amd_godunov_fine_lowdim_f90": lambda: L.ramses_amd_godunov_fine_lowdim_f90(
            p, 4, 8, z, 1, z, z, 8, 1, z, z, z, z, 0.1, 0.01),
        "ramses_amd_amrres_godunov": lambda: L.ramses_amd_amrres_godunov(p, 4, 8, z, 0.1, 0.01, 32, 0, 1),
        "ramses_amd_amrres_courant": lambda: L.ramses_amd_amrres_courant(p, 4, z, 0.1, 0.01, z),
        "ramses_amd_amrres_set_uold": lambda: L.ramses_amd_amrres_set_uold(p, 8, z),
        "ramses_amd_amrres_upload_fine": lambda: L.ramses_amd_amrres_upload_fine(p, 4, z, 0),
    }
    for name, call in calls.items():
        assert call() == EUNSUPPORTED, name
        assert "NVAR=8" in _err(L) and name in _err(L), (name, _err(L))


def test_fortran_patch_lets_scalars_through_on_uniform_levels_only():
    iface = open(os.path.join(ROOT, "ramses_amd", "patch", "ramses_amd_iface.f90")).read()
    assert "nvar < ndim + 2 + nener .or. nvar > RAMSES_AMD_MAX_NVAR" in iface
    # the Fortran side names the limit once, and it is the header's
    assert int(re.search(r"integer, parameter :: RAMSES_AMD_MAX_NVAR = (\d+)", iface).group(1)) == 16
    assert "if (nener > 0) ramses_amd_amr_ok = .false." in iface
    assert "if (nvar > 7) ramses_amd_amr_ok = .false." in iface
    gf = open(os.path.join(ROOT, "ramses_amd", "patch", "godunov_fine.f90")).read()
    assert "amr_level.and.nener>0" in gf
    assert "if(amr_level.and.nvar>7)then" in gf and "godunov_fine (NVAR>7 on an AMR level / the tree walker)" in gf


# ---- the checker beyond NVAR=7 --------------------------------------------------------------------------------------


def test_oracle_sweeps_each_scalar_on_its_own():
    """The oracle at NVAR=10 gives the hydro rows of NVAR=5 and, for every scalar, the row that NVAR=6 gives it."""
    from oracle import pyoracle as po
    nx, ny, nz = 12, 10, 8
    u = random_brick(nx, ny, nz, seed=5, nvar=10)
    dx, dt = 1.0 / 32, 0.03 / 32
    for riemann, st in (("llf", 1), ("hllc", 2), ("exact", 7)):
        big = po.godunov_uniform(po.make_params(nvar=10, riemann=riemann, slope_type=st), u, dx, dt)
        hyd = po.godunov_uniform(po.make_params(nvar=5, riemann=riemann, slope_type=st), u[:5].copy(), dx, dt)
        assert np.array_equal(big[:5], hyd)
        for k in range(5, 10):
            one = po.godunov_uniform(po.make_params(nvar=6, riemann=riemann, slope_type=st),
                                     np.ascontiguousarray(u[[0, 1, 2, 3, 4, k]]), dx, dt)
            assert np.array_equal(big[k], one[5]), (riemann, k)

"""CPU tests of the non-thermal energies (NENER) at the C ABI: the struct that carries nener and gamma_rad has
the same layout in C, Python and Fortran, and every configuration outside the supported set (NENER = 1 with
NVAR 6 or 7, NENER = 2 with NVAR 7; muscl; llf, hll, hllc; no gravity, no difmag; the uniform brick entry
points) is refused with RAMSES_AMD_EUNSUPPORTED and a message.  Validation runs before any device work, so
no GPU is needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EUNSUPPORTED, EINVAL = -2, -1


@pytest.fixture(scope="module")
def L():
    from ramses_amd import _capi, build
    build.build()
    return _capi.lib()


def _p(**kw):
    from ramses_amd import _capi
    kw.setdefault("nener", 1)
    return _capi.make_params(**kw)


def _sweep(L, p, grav=None):
    from ramses_amd import _capi
    b = _capi.dense_brick(16, 16, 16, 0)
    return L.ramses_amd_godunov_brick(C.byref(p), C.byref(b), C.c_void_p(8), grav, C.c_void_p(16), 0.1, 0.01, None)


def _err(L):
    return L.ramses_amd_last_error().decode()


# ---- layouts -------------------------------------------------------------------------------------------------


def _c_fields():
    hdr = open(os.path.join(ROOT, "include", "ramses_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    body = re.search(r"typedef struct ramses_amd_hydro_params \{(.*?)\} ramses_amd_hydro_params;", hdr, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        typ, names = decl.split(None, 1)
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\w+)\])?", n)
            count = 1 if not m.group(2) else (2 if m.group(2) == "RAMSES_AMD_MAX_NENER" else int(m.group(2)))
            out.append((m.group(1), {"int32_t": "i4", "double": "f8"}[typ], count))
    return out


def _f_fields():
    src = open(os.path.join(ROOT, "ramses_amd", "patch", "ramses_amd_cabi.f90")).read()
    body = re.search(r"type, bind\(C\) :: ramses_amd_hydro_params\n(.*?)end type ramses_amd_hydro_params", src, re.S).group(1)
    out = []
    for line in body.splitlines():
        line = line.split("!")[0].strip()
        if not line:
            continue
        typ, names = line.split("::")
        kind = {"integer(c_int32_t)": "i4", "real(c_double)": "f8"}[typ.strip()]
        for n in names.split(","):
            m = re.match(r"\s*(\w+)(?:\((\d+)\))?", n)
            out.append((m.group(1), kind, int(m.group(2) or 1)))
    return out


def _py_fields():
    from ramses_amd import _capi
    out = []
    for name, t in _capi.HydroParams._fields_:
        if hasattr(t, "_length_"):
            out.append((name, {C.c_double: "f8", C.c_int32: "i4"}[t._type_], t._length_))
        else:
            out.append((name, {C.c_double: "f8", C.c_int32: "i4"}[t], 1))
    return out


def test_hydro_params_layout_agrees_in_c_python_and_fortran(L):
    from ramses_amd import _capi
    c, f, py = _c_fields(), _f_fields(), _py_fields()
    assert c == py == f
    assert ("nener", "i4", 1) in c and c[-1] == ("gamma_rad", "f8", 2)
    assert L.ramses_amd_abi_check(C.c_size_t(C.sizeof(_capi.HydroParams)), C.c_size_t(C.sizeof(_capi.Brick))) == 0
    # the stale layout (reserved, no gamma_rad) is caught
    assert L.ramses_amd_abi_check(C.c_size_t(C.sizeof(_capi.HydroParams) - 16), C.c_size_t(C.sizeof(_capi.Brick))) != 0


def test_make_params_defaults():
    from ramses_amd import _capi
    p = _capi.make_params()
    assert p.nener == 0 and p.nvar == 5
    assert list(p.gamma_rad) == [1.33333333334, 1.33333333334]     # hydro/hydro_parameters.f90:79
    p = _capi.make_params(nener=2, gamma_rad=(1.4, 1.6))
    assert p.nvar == 7 and list(p.gamma_rad) == [1.4, 1.6]
    assert _capi.make_params(nener=1, nvar=7).nvar == 7


# ---- refusals ------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kw, needle", [
    (dict(nener=3, nvar=7), "NENER=3"),
    (dict(nener=-1, nvar=6), "NENER=-1"),
    (dict(nener=2, nvar=6), "NVAR >= 7"),
    (dict(nener=1, nvar=5), "NVAR >= 6"),
    (dict(scheme="plmde"), "plmde"),
    (dict(riemann="exact"), "no NENER branch"),
    (dict(riemann="acoustic"), "no NENER branch"),
    (dict(difmag=0.1), "difmag"),
])
def test_brick_sweep_refuses_outside_the_supported_set(L, kw, needle):
    rc = _sweep(L, _p(**kw))
    assert rc == EUNSUPPORTED and needle in _err(L)


def test_brick_sweep_refuses_nener_with_gravity(L):
    assert _sweep(L, _p(), grav=C.c_void_p(24)) == EUNSUPPORTED and "gravity" in _err(L)


def test_courant_refuses_nener_with_gravity_and_bad_nvar(L):
    from ramses_amd import _capi
    b = _capi.dense_brick(16, 16, 16, 0)
    rc = L.ramses_amd_courant_brick(C.byref(_p()), C.byref(b), C.c_void_p(8), C.c_void_p(16), 0.1, C.c_void_p(24), None)
    assert rc == EUNSUPPORTED and "gravity" in _err(L)
    rc = L.ramses_amd_courant_brick(C.byref(_p(nener=2, nvar=6)), C.byref(b), C.c_void_p(8), None, 0.1, C.c_void_p(24), None)
    assert rc == EUNSUPPORTED


def test_pdv_brick_needs_non_thermal_energies(L):
    from ramses_amd import _capi
    b = _capi.dense_brick(16, 16, 16, 0)
    rc = L.ramses_amd_pdv_brick(C.byref(_capi.make_params()), C.byref(b), C.c_void_p(8), C.c_void_p(16), 0.1, 0.01, None)
    assert rc == EINVAL and "NENER=1 or 2" in _err(L)
    rc = L.ramses_amd_pdv_brick(C.byref(_p(nener=3, nvar=7)), C.byref(b), C.c_void_p(8), C.c_void_p(16), 0.1, 0.01, None)
    assert rc != 0
    rc = L.ramses_amd_pdv_brick(C.byref(_p()), C.byref(b), C.c_void_p(8), C.c_void_p(8), 0.1, 0.01, None)
    assert rc == EINVAL     # uold == unew


def test_tile_tree_and_amr_resident_entry_points_refuse_nener(L):
    p = C.byref(_p())
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
        assert "NENER=1" in _err(L) and name in _err(L), (name, _err(L))


def test_mpi_resident_setup_refuses_unsupported_nener(L):
    z = None
    n0 = (C.c_int * 1)(0)
    rc = L.ramses_amd_mpires_setup(C.byref(_p(nener=3, nvar=7)), 4, 512, C.c_void_p(8), C.c_void_p(8), 512, 1, 1,
                                   C.c_void_p(8), C.c_void_p(8), 1, 1, n0, z, n0, z)
    assert rc == EUNSUPPORTED and "NENER=3" in _err(L)
    rc = L.ramses_amd_mpires_set_uold_pdv(C.byref(_p()), 0.1, 0.01)
    assert rc == EINVAL     # no resident level


def test_fortran_patch_passes_nener_and_keeps_amr_residency_off():
    iface = open(os.path.join(ROOT, "ramses_amd", "patch", "ramses_amd_iface.f90")).read()
    assert "p%nener = nener" in iface and "p%reserved" not in iface
    assert "if (nener > 0) ramses_amd_amr_ok = .false." in iface
    gf = open(os.path.join(ROOT, "ramses_amd", "patch", "godunov_fine.f90")).read()
    assert "ramses_amd_resident_set_uold_pdv_f90" in gf and "ramses_amd_mpires_set_uold_pdv" in gf
    assert "amr_level.and.nener>0" in gf


def test_overlapped_step_of_a_nener_level_runs_set_uold_before_the_exchange():
    """With non-thermal energies set_uold changes the new state after the sweep: its ghosts may only leave after it."""
    from types import SimpleNamespace
    from ramses_amd.parallel import BrickDecomposition
    calls = []

    class Level:
        params = SimpleNamespace(nener=1)
        uold = unew = SimpleNamespace(device=SimpleNamespace(type="cuda"))
        nvar, f = 6, None

        def godunov_fine(self, dt):
            calls.append("godunov_fine")

        def godunov_fine_shell(self, dt):
            calls.append("shell")

        def godunov_fine_interior(self, dt):
            calls.append("interior")

        def set_uold(self):
            calls.append("set_uold")

    class Dec(BrickDecomposition):
        def exchange_direct(self, lev, t, nvar):
            calls.append("exchange uold" if t is lev.uold and calls[-1] == "set_uold" else "exchange")

    Dec((1, 1, 1), 0, 16, transport=object()).step_overlapped(Level(), 0.01)
    assert calls == ["godunov_fine", "set_uold", "exchange uold"]

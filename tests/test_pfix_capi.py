"""CPU tests of ramses_amd_amrres_sync_pfix (divu / enew of a resident pressure_fix run back to the host): exported, declared in
include/ramses_amd.h, bound in _capi.py and in patch/ramses_amd_cabi.f90 with matching arguments, and loud without its state.
Nothing here touches a GPU."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "ramses_amd_amrres_sync_pfix"


def _prototype():
    hdr = open(os.path.join(ROOT, "include", "ramses_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % NAME, hdr)
    assert m, "%s is not declared in include/ramses_amd.h" % NAME
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_sync_pfix_is_declared_exported_and_bound_in_python():
    from ramses_amd import _capi, build
    assert _prototype() == ["int ngrid", "const int *igrid", "double *divu", "double *enew"]
    lib = C.CDLL(build.build())
    assert hasattr(lib, NAME), "libramses_amd.so does not export %s" % NAME
    bound = {s[0]: s for s in _capi.SYMBOLS}
    assert NAME in bound
    _, restype, argtypes = bound[NAME]
    assert restype is C.c_int and argtypes == [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]


def test_sync_pfix_is_bound_in_the_fortran_interface_with_matching_arguments():
    src = open(os.path.join(ROOT, "ramses_amd", "patch", "ramses_amd_cabi.f90")).read()
    m = re.search(r"function\s+%s\s*\(([^)]*)\)\s*(?:&\s*\n\s*&\s*)?bind\(C,\s*name='%s'\)\s*result\(rc\)(.*?)end function %s" % (NAME, NAME, NAME),
                  src, flags=re.S)
    assert m, "%s is not bound in ramses_amd_cabi.f90" % NAME
    assert [a.strip() for a in m.group(1).split(",")] == ["ngrid", "igrid", "divu", "enew"]
    body = m.group(2)
    assert re.search(r"integer\(c_int\),\s*value\s*::\s*ngrid", body)              # int by value
    assert re.search(r"integer\(c_int\)\s*::\s*igrid\(\*\)", body)                   # const int *
    assert re.search(r"real\(c_double\)\s*::\s*divu\(\*\),\s*enew\(\*\)", body)      # double *, double *
    assert re.search(r"integer\(c_int\)\s*::\s*rc", body)


def test_sync_pfix_refuses_to_run_without_its_state():
    """EINVAL and a message when no resident state exists; the same when pressure_fix is not enabled (the second needs a loaded
    state, that is a GPU: tests/test_pfix_tiles_gpu.py reads the vectors back in every case)"""
    from ramses_amd import _capi
    L = _capi.lib()
    ig = np.array([1, 2], np.int32)
    divu, enew = np.zeros(64), np.zeros(64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    rc = L.ramses_amd_amrres_sync_pfix(2, vp(ig), vp(divu), vp(enew))
    assert rc == -1, rc
    assert b"sync_pfix" in L.ramses_amd_last_error() and b"no resident AMR state" in L.ramses_amd_last_error()
    assert not divu.any() and not enew.any()

"""CPU tests of the refinement criteria on the resident state at the C ABI (ramses_amd_amrres_refine_flag,
ramses_amd_amrres_mass_map, struct ramses_amd_refine_crit): header, library and binding agree on the symbols and on the size
of the struct; every refusal returns its code and names its argument before any device work (no GPU is needed); the patch no
longer keeps a run with jeans_refine / m_refine off the device and carries the switch that restores the old gating."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "ramses_amd", "patch")
EUNSUPPORTED, EINVAL = -2, -1
NEW = ("ramses_amd_amrres_refine_flag", "ramses_amd_amrres_mass_map")


@pytest.fixture(scope="module")
def L():
    from ramses_amd import _capi, build
    build.build()
    return _capi.lib()


def _err(L):
    return L.ramses_amd_last_error().decode()


def _read(*parts):
    return open(os.path.join(*parts)).read()


def test_header_library_binding_and_fortran_agree(L):
    from ramses_amd import _capi
    h = _read(ROOT, "include", "ramses_amd.h")
    cabi = _read(PATCH, "ramses_amd_cabi.f90")
    bound = {s[0]: s for s in _capi.SYMBOLS}
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, h), name
        assert name in bound and getattr(L, name) is not None
        assert "bind(C, name='%s')" % name in cabi
    assert len(bound["ramses_amd_amrres_refine_flag"][2]) == 6 and len(bound["ramses_amd_amrres_mass_map"][2]) == 10
    # the struct: the header's fields in order, 11 doubles and 2 int32 = 96 bytes in all three
    body = re.search(r"typedef struct ramses_amd_refine_crit \{(.*?)\} ramses_amd_refine_crit;", h, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for typ, names in re.findall(r"(double|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), typ) for n in names.split(",")]
    assert [f[0] for f in fields] == [f[0] for f in _capi.RefineCrit._fields_]
    assert [f[1] for f in fields] == ["double" if f[1] is C.c_double else "int32_t" for f in _capi.RefineCrit._fields_]
    assert L.ramses_amd_refine_crit_size() == C.sizeof(_capi.RefineCrit) == 96
    ftype = re.search(r"type, bind\(C\) :: ramses_amd_refine_crit(.*?)end type ramses_amd_refine_crit", cabi, re.S).group(1)
    fnames = [n.strip() for line in re.findall(r"::\s*(.+)", ftype) for n in line.split(",")]
    assert fnames == [f[0] for f in fields]


def _flag(L, p, crit, ngrid=0, igrid=None, cells=C.c_void_p(8), n=None):
    n = C.byref(C.c_int(7)) if n is None else n
    return L.ramses_amd_amrres_refine_flag(C.byref(p) if p is not None else None, ngrid, igrid,
                                           C.byref(crit) if crit is not None else None, cells, n)


def _map(L, p, ivar=0, cells=C.c_void_p(8), n=None, d_scale=1.0):
    n = C.byref(C.c_int(7)) if n is None else n
    return L.ramses_amd_amrres_mass_map(C.byref(p) if p is not None else None, 0, None, d_scale, 4.0, ivar, 0.5, None, cells, n)


def test_refusals_name_their_argument(L):
    from ramses_amd import _capi
    p, crit = _capi.make_params(), _capi.make_refine_crit()
    L.ramses_amd_amrres_invalidate()
    for who, call in (("ramses_amd_amrres_refine_flag", _flag), ("ramses_amd_amrres_mass_map", lambda L, p, c, **kw: _map(L, p, **kw))):
        assert call(L, None, crit) == EINVAL and who in _err(L) and "argument p" in _err(L)
        assert call(L, p, crit, cells=None) == EINVAL and "argument cells" in _err(L)
        assert call(L, p, crit, n=C.POINTER(C.c_int)()) == EINVAL and "argument ncells" in _err(L)
        # the AMR entry points' common opening (csrc/capi_shared.hpp refuse_amr)
        assert call(L, _capi.make_params(nener=1), crit) == EUNSUPPORTED and "NENER=1" in _err(L) and who in _err(L)
        assert call(L, _capi.make_params(nvar=8), crit) == EUNSUPPORTED and "NVAR=8" in _err(L) and who in _err(L)
    assert _flag(L, p, None) == EINVAL and "argument crit" in _err(L)
    # n_jeans > 0 needs the cell size
    for tail in (0.0, -0.25):
        assert _flag(L, p, _capi.make_refine_crit(n_jeans=4.0, tail_pix=tail)) == EINVAL
        assert "tail_pix" in _err(L) and "n_jeans" in _err(L)
    # ivar_refine: 0 or a passive scalar 6 .. nvar
    for nvar, ivar in ((5, 6), (6, 7), (7, 8), (7, 5), (7, 1), (7, -1)):
        pv = _capi.make_params(nvar=nvar)
        assert _flag(L, pv, _capi.make_refine_crit(thr_mode=2, ivar_refine=ivar, var_cut_refine=0.5)) == EINVAL
        assert "ivar_refine=%d" % ivar in _err(L)
        assert _map(L, pv, ivar=ivar) == EINVAL and "ivar_refine=%d" % ivar in _err(L)
    assert _flag(L, p, _capi.make_refine_crit(thr_mode=3)) == EINVAL and "thr_mode" in _err(L)
    assert _flag(L, p, _capi.make_refine_crit(thr_mode=2)) == EINVAL and "ivar_refine" in _err(L)
    assert _map(L, p, d_scale=0.0) == EINVAL and "d_scale" in _err(L)


def test_valid_arguments_reach_the_resident_state_check(L):
    """everything above passed: the next refusal is the missing resident state (still no device work), *ncells reset"""
    from ramses_amd import _capi
    L.ramses_amd_amrres_invalidate()
    n = C.c_int(7)
    p7 = _capi.make_params(nvar=7)
    crit = _capi.make_refine_crit(n_jeans=4.0, tail_pix=1.0 / 32, thr_mode=2, ivar_refine=6, var_cut_refine=0.5)
    assert _flag(L, p7, crit, n=C.byref(n)) == EINVAL and "no resident AMR state" in _err(L) and n.value == 0
    n = C.c_int(7)
    assert _map(L, p7, ivar=7, n=C.byref(n)) == EINVAL and "no resident AMR state" in _err(L) and n.value == 0


def test_patch_opens_the_gate_and_carries_the_switch():
    iface = _read(PATCH, "ramses_amd_iface.f90")
    gate = iface[iface.index("logical function ramses_amd_amr_config()"):iface.index("end function ramses_amd_amr_config")]
    assert "RAMSES_AMD_RESIDENT_REFINE" in gate
    # no loop that switches residency off for jeans_refine / m_refine outside that switch
    code = "\n".join(line.split("!")[0] for line in gate.splitlines())
    switch = code.index("RAMSES_AMD_RESIDENT_REFINE")
    assert "jeans_refine" not in code[:switch] and "m_refine" not in code[:switch]
    assert not re.search(r"if \((jeans_refine|m_refine)\(l\) > -1\.0d0\) ramses_amd_amr_ok = \.false\.", code)
    rho = _read(PATCH, "rho_fine.f90")
    dev = rho[rho.index("logical function ramses_amd_rho_amr_device"):rho.index("end function ramses_amd_rho_amr_device")]
    assert "m_refine" not in dev
    assert "ramses_amd_amrres_mass_map" in rho and "make_virtual_fine_int(cpu_map2(1),ilevel)" in rho
    assert "ramses_amd_amrres_refine_flag" in _read(PATCH, "hydro_flag.f90")
    fu = _read(PATCH, "flag_utils.f90")
    # (userflag_fine, the caller, lives in the same file: the definition alone is renamed, by prepare.sh)
    assert '#include "flag_utils_ref.f90"' in fu and "call poisson_refine_reference(ind_cell,ok,ncell,ilevel)" in fu
    assert "flag_utils_ref.f90" in _read(PATCH, "prepare.sh") and "flag_utils_ref.f90" in _read(PATCH, "Makefile")
    assert "ramses_amd_amrres_refine_flag" in fu and "ramses_amd_amrres_active()" in fu

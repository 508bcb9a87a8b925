"""The numpy checker of cooling_fine in a barotropic run of constant temperature (tests/eos_checker.py), the library's host
evaluation (ramses_amd_eos_eval) and the header itself under the sanitizers, against the reference program, without a GPU.

tests/golden/eos_ref.npz (tests/golden/make_golden_eos.py) holds uold and son of the cells of the active octs before and after two
calls of the unmodified reference's cooling_fine in each of three runs: 'isothermal' on one level, 'isothermal' on levels 4-5 with
a cube below smallr, the legacy idiom isothermal=.true. with g_star = 1.  Everything here is bit for bit; the device tests then
compare with the checker at tolerance zero.

The records must make the edge cases bind: densities below smallr, densities for which nH*scale_nH/scale_nH is not nH, split
cells that come back unchanged."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import eos_checker as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eos_ref.npz")
RECORDS = tuple("%s%d" % (tag, k) for tag in ("iso_uniform", "iso_amr", "legacy") for k in (0, 1))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def record(gold, name):
    """(uin, uout, son, T2c, scale_nH, scale_T2, smallr, gamma) of one call"""
    gamma, smallr, scale_nH, scale_T2, T2_eos, T2_star, g_star, jeans_ncells = gold[name + "_par"]
    if name.startswith("legacy"):
        assert g_star == 1.0 and not jeans_ncells > 0
        T2c = T2_star
    else:
        T2c = T2_eos
    assert np.array_equal(gold[name + "_sin"], gold[name + "_sout"])
    return gold[name + "_uin"], gold[name + "_uout"], gold[name + "_sin"], T2c, scale_nH, scale_T2, smallr, gamma


@pytest.mark.parametrize("name", RECORDS)
def test_checker_returns_the_reference_programs_bits(gold, name):
    uin, uout, son, T2c, scale_nH, scale_T2, smallr, gamma = record(gold, name)
    assert uin.shape == uout.shape == (5, son.size) and son.size >= 4096
    got = EC.cooling_fine(uin, son, T2c, scale_nH, scale_T2, smallr, gamma)
    print("%s: %d cells, %d leaves, %d energies rewritten to other bits" % (name, son.size, (son == 0).sum(), (EC.bits(uin[4]) != EC.bits(uout[4])).sum()))
    assert np.array_equal(EC.bits(got), EC.bits(uout))
    assert (EC.bits(uin[4]) != EC.bits(uout[4])).sum() > 500, "the call must have done something"


@pytest.mark.parametrize("name", RECORDS)
def test_library_host_evaluation_returns_the_reference_programs_bits(gold, name):
    from ramses_amd import _capi
    L = _capi.lib()
    uin, uout, son, T2c, scale_nH, scale_T2, smallr, gamma = record(gold, name)
    leaf = son == 0
    u5 = np.ascontiguousarray(uin[:, leaf])
    E = np.full(u5.shape[1], np.nan)
    p = _capi.make_params(gamma=gamma, smallr=smallr)
    assert L.ramses_amd_eos_set(T2c, scale_nH, scale_T2) == 0, L.ramses_amd_last_error()
    rc = L.ramses_amd_eos_eval(C.byref(p), u5.shape[1], u5.ctypes.data_as(C.c_void_p), E.ctypes.data_as(C.c_void_p))
    assert rc == 0, L.ramses_amd_last_error()
    assert np.array_equal(EC.bits(E), EC.bits(uout[4, leaf]))


def test_the_records_make_the_edge_cases_bind(gold):
    below = roundtrip = split = 0
    for name in RECORDS:
        uin, uout, son, T2c, scale_nH, scale_T2, smallr, gamma = record(gold, name)
        leaf = son == 0
        assert np.log2(scale_nH) != np.round(np.log2(scale_nH)), "scale_nH must not be a power of two"
        nH = np.maximum(uin[0, leaf], smallr)
        below += int((uin[0, leaf] < smallr).sum())
        roundtrip += int((nH * scale_nH / scale_nH != nH).sum())
        split += int((~leaf).sum())
        # rho, the momenta and every split cell are untouched in the records
        assert np.array_equal(EC.bits(uin[:4]), EC.bits(uout[:4]))
        assert np.array_equal(EC.bits(uin[4, ~leaf]), EC.bits(uout[4, ~leaf]))
    print("leaf cells below smallr: %d, with nH*scale_nH/scale_nH != nH: %d, split cells: %d" % (below, roundtrip, split))
    assert below > 100 and roundtrip > 100 and split > 100


def test_eos_set_refuses_what_it_cannot_use():
    from ramses_amd import _capi
    L = _capi.lib()
    for bad in ((-1.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, float("nan"))):
        assert L.ramses_amd_eos_set(*bad) == -1 and b"ramses_amd_eos_set" in L.ramses_amd_last_error()


def test_the_device_entries_fail_loudly_without_their_state():
    from ramses_amd import _capi
    L = _capi.lib()
    p = _capi.make_params()
    assert L.ramses_amd_eos_set(10.0, 2.0e3, 120.0) == 0
    ig = np.ones(4, np.int32)
    assert L.ramses_amd_amrres_cooling_fine(C.byref(p), 4, ig.ctypes.data_as(C.c_void_p)) == -1
    assert b"no resident AMR state" in L.ramses_amd_last_error()
    assert L.ramses_amd_resident_cooling_fine_f90(C.byref(p), 5) == -1 and b"cooling_fine: level 5 is not resident" in L.ramses_amd_last_error()
    assert L.ramses_amd_mpires_cooling_fine(C.byref(p)) == -1 and b"cooling_fine: no resident level" in L.ramses_amd_last_error()
    # NENER > 0 with an equation of state is not on the device (the err term): refused by name on AMR levels
    pn = _capi.make_params(nener=1)
    assert L.ramses_amd_amrres_cooling_fine(C.byref(pn), 4, ig.ctypes.data_as(C.c_void_p)) == -2
    assert b"ramses_amd_amrres_cooling_fine: NENER=1" in L.ramses_amd_last_error()


def test_header_under_the_sanitizers_over_the_records(gold, tmp_path):
    """csrc/eos_core.hpp compiled by the plain host compiler with -fsanitize=address,undefined into a program of its own
    (tests/native/eos_host_check.cpp) and run as a child process over every record"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "eos_host_check")
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "ramses_amd"),
                        os.path.join(ROOT, "tests", "native", "eos_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, "eos_core.hpp does not compile with the host compiler alone"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in RECORDS:
        uin, uout, son, T2c, scale_nH, scale_T2, smallr, gamma = record(gold, name)
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as fh:
            fh.write(np.int64(son.size).tobytes())
            fh.write(np.array([T2c, scale_nH, scale_T2, smallr, gamma]).tobytes())
            for row in (uin[0], uin[1], uin[2], uin[3], uin[4], uout[4]):
                fh.write(np.ascontiguousarray(row).tobytes())
            fh.write(son.astype(np.int32).tobytes())
        r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        print(name, r.stdout)
        assert r.returncode == 0 and r.stdout.split() == ["ok", str(int((son == 0).sum())), str(int((son != 0).sum()))], r.stdout

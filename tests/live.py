"""Shared test helpers: the patched program (oracle/_ref/*_patch) run live against the unpatched one."""
import collections
import importlib.util
import os
import re
import shutil

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MODULES = {}


def load_module(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def golden_module(which):
    """tests/golden/make_golden_<which>.py ('amr', 'baseline', 'cg', ...) as a module, loaded once"""
    if which not in _MODULES:
        _MODULES[which] = load_module(os.path.join(ROOT, "tests", "golden", "make_golden_%s.py" % which), "mk" + which)
    return _MODULES[which]


def run(nml, binary, nproc, env, timeout=3600):
    """run_reference with the variables of env on top of the caller's environment (a value of None: unset); returns (work, out)"""
    from oracle import ramses_snapshot as rs
    child = dict(os.environ)
    for k, v in env.items():
        if v is None:
            child.pop(k, None)
        else:
            child[k] = v
    return rs.run_reference(nml, binary=binary, nproc=nproc, timeout=timeout, env=child)


def binaries(mpi, solver="hydro"):
    """(patched, unpatched) program under oracle/_ref; skips the test where they are not built"""
    tail = "_mhd" if solver == "mhd" else ""
    names = ("ramses3d_mpi_patch" + 2 * tail, "ramses3d_mpi" + tail) if mpi else ("ramses3d_patch" + 2 * tail, "ramses3d" + tail)
    patched, ref = (os.path.join(ROOT, "oracle", "_ref", b) for b in names)
    if not (os.path.exists(patched) and os.path.exists(ref)):
        pytest.skip("oracle/_ref/%s, %s not built" % names)
    return patched, ref


def enough_cores(nproc):
    if nproc > (os.cpu_count() or 1):
        pytest.skip("fewer cores than ranks")


Leaves = collections.namedtuple("Leaves", "level x prim t grav")


def sorted_leaves(snap):
    """the leaf cells of a snapshot (load_leaf_cells) ordered by level, z, y, x"""
    order = np.lexsort((snap["x"][:, 0], snap["x"][:, 1], snap["x"][:, 2], snap["level"]))
    grav = snap["grav"][:, order] if "grav" in snap else None
    return Leaves(snap["level"][order], snap["x"][order], snap["prim"][:, order], snap["info"]["t"], grav)


def leaves(work, k=2, with_grav=False):
    from oracle import ramses_snapshot as rs
    return sorted_leaves(rs.load_leaf_cells(os.path.join(work, "output_%05d" % k), with_grav=with_grav))


def sweep_counts(out):
    """(sweeps of AMR levels through the dense kernel on tiles, through the tree-walking kernel) of the RAMSES_AMD_STATS exit line"""
    m = re.search(r"godunov_fine of AMR levels:\s*(\d+) sweeps through the dense kernel on tiles.*?(\d+) through the tree-walking kernel", out)
    assert m, out[-2000:]
    return int(m.group(1)), int(m.group(2))


def f_traffic(out):
    """[bytes to the device, bytes back] of the acceleration, one pair per rank (RAMSES_AMD_STATS exit lines)"""
    return [[int(a), int(b)] for a, b in re.findall(r"acceleration f over PCIe:\s*(\d+) bytes to the device,\s*(\d+) bytes back", out)]


def poisson_solves(out):
    """the (level, iterations) pairs the Poisson solvers print, as strings, in the order of the run"""
    return re.findall(r"==> Level=\s*(\d+) Step=\s*(\d+)", out)


def ab(nml, nproc, env, ref_env=None, expect_resident=None, resident_message=None, min_levels=0, min_octs=False):
    """The patched program with env on top of RAMSES_AMD=1, then the unpatched one with ref_env; both work directories removed.
    Asserts the same time, levels, cell centres and primitives (as values and as bits) in the leaf cells of the last snapshot.
    resident_message: the run says (True) or does not say (False) that the AMR levels stay resident; expect_resident: that and
    the device's make_boundary_hydro; min_levels: the unpatched run holds that many levels; min_octs: RAMSES_AMD_TILE_MIN_OCTS of
    the patched run (None: unset).  Returns (the patched program's output, the unpatched program's leaves)."""
    patched, ref = binaries(nproc > 1)
    e = {"RAMSES_AMD": "1"}
    if min_octs is not False:
        e["RAMSES_AMD_TILE_MIN_OCTS"] = min_octs
    e.update(env)
    work, out = run(nml, patched, nproc, e)
    try:
        for said in (expect_resident, resident_message):
            if said is not None:
                assert ("AMR levels stay resident on the GPU" in out) == said, out[-3000:]
        if expect_resident is not None:
            assert ("make_boundary_hydro (device)" in out) == expect_resident, out[-3000:]
        got = leaves(work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    work, _ = run(nml, ref, nproc, ref_env or {})
    try:
        want = leaves(work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    assert got.t == want.t
    assert len(set(int(l) for l in want.level)) >= min_levels, "the run must have refined"
    assert np.array_equal(got.level, want.level) and np.array_equal(got.x, want.x)
    assert np.array_equal(got.prim, want.prim), np.abs(got.prim - want.prim).max()
    assert np.array_equal(got.prim.view(np.int64), want.prim.view(np.int64))
    return out, want


def amr_namelist(lmin, lmax, nstep, riemann, slope, nsubcycle, ngridtot, poisson=False, extra=None, init=None):
    """sedov3d_namelist on levels lmin..lmax with nsubcycle and ngridtot as given.  extra None: the refinement criterion of the
    AMR goldens where lmax > lmin; poisson: the self-gravitating initial state of the AMR goldens and &POISSON_PARAMS."""
    from oracle import ramses_snapshot as rs
    mka = golden_module("amr")
    if extra is None:
        extra = mka.REFINE.format(ivar=0, itype=2) if lmax > lmin else ""
    kw = {} if init is None else {"init": init}
    if poisson:
        kw["init"] = mka.SELFGRAV_INIT
        extra += "&POISSON_PARAMS\nepsilon=1e-5\n/\n"
    nml = rs.sedov3d_namelist(level=lmin, nstepmax=nstep, foutput=nstep, riemann=riemann, slope_type=slope, extra=extra, mem_factor=1.0,
                              poisson=poisson, **kw)
    return replace_keys(nml, ("levelmax=%d" % lmin, "levelmax=%d" % lmax), ("nsubcycle=10*1", "nsubcycle=" + nsubcycle),
                        ("ngridtot=", "ngridtot=%d !" % ngridtot))


def replace_keys(nml, *pairs):
    """str.replace for each (old, new), after the check that old is there to be replaced"""
    for old, new in pairs:
        assert old in nml, "no %r in the namelist" % old
        nml = nml.replace(old, new)
    return nml

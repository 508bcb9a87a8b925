"""CPU record of the host dispatch of csrc/hydro_sweep.hip: which kernel every combination of runtime options launches.

The 14 hydro_sweep_*.o objects of the library need nine symbols of the HIP runtime; tests/native/hip_stub.cpp stands in for them
and records the launches instead of making them.  tests/native/sweep_dispatch_dump.cpp walks a fixed grid of options -- one value
beyond every accepted range included -- through the eight public launchers of both arithmetic modes and the three tile_sweep_rows
functions; its output must equal tests/golden/sweep_dispatch.json.gz: for every accepted call the kernels by name with grid, block,
dynamic LDS bytes and the hipFuncSetAttribute value, and A.nbox, A.nblocks, A.box[]; every other call of the grid must have
returned hipErrorInvalidValue without a launch.  No GPU is opened: the stub is linked into the dump program only.

A new kernel family or a new accepted option changes the table on purpose:  python tests/test_sweep_dispatch_host.py --record
"""
import glob
import gzip
import json
import os
import shutil
import subprocess

from helpers import hip_include
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
TABLE = os.path.join(ROOT, "tests", "golden", "sweep_dispatch.json.gz")

# (mode, family): (parameters of a row, calls of the grid, accepted calls).  Accepted = hipSuccess, a nothing-to-sweep return
# (an empty region, nevent = 0) included.
FAMILIES = {
    ("strict", "godunov_sweep"): ("st rs nvar scheme grav by layout", 117600, 13600),
    ("strict", "godunov_sweep_nener"): ("st rs nvar nener layout", 19600, 684),
    ("strict", "godunov_sweep_scalars"): ("st rs nvar nener grav by layout", 156800, 9036),
    ("strict", "godunov_sweep_pfix"): ("st rs nvar grav missing layout", 29400, 180),
    ("strict", "godunov_sweep_difmag"): ("st rs nvar grav missing layout", 19600, 180),
    ("strict", "surface_flux"): ("st rs nvar scheme grav nevent", 6300, 2580),
    ("strict", "surface_flux_pfix"): ("st rs nvar grav nevent", 2100, 1060),
    ("strict", "surface_flux_difmag"): ("st rs nvar grav nevent", 2100, 1060),
    ("fast", "godunov_sweep"): ("st rs nvar scheme grav by layout", 117600, 13600),
    ("fast", "godunov_sweep_nener"): ("st rs nvar nener layout", 19600, 684),
    ("fast", "godunov_sweep_scalars"): ("st rs nvar nener grav by layout", 156800, 9036),
    ("fast", "surface_flux"): ("st rs nvar scheme grav nevent", 6300, 2580),
}
# (mode, function): (parameters, values)
VALUES = {
    ("strict", "tile_sweep_rows"): ("st rs nvar scheme", 1050),
    ("fast", "tile_sweep_rows"): ("st rs nvar scheme", 1050),
    ("strict", "tile_sweep_rows_pfix"): ("st nvar", 50),
    ("strict", "tile_sweep_rows_difmag"): ("st nvar", 50),
}


def dump(objdir, workdir):
    """link the sweep objects with the stub and the dump program, run it: the lines it wrote"""
    objs = sorted(glob.glob(os.path.join(objdir, "hydro_sweep_*.o")))
    assert len(objs) == 14, objs
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(workdir, "sweep_dispatch_dump")
    subprocess.run([cxx, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", hip_include("hip_runtime.h"), "-I", os.path.join(ROOT, "ramses_amd"),
                    os.path.join(NATIVE, "sweep_dispatch_dump.cpp"), os.path.join(NATIVE, "hip_stub.cpp")] + objs + ["-o", exe],
                   check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return subprocess.run([exe], check=True, stdout=subprocess.PIPE, text=True).stdout.splitlines()


def table_of(lines):
    """the compact form: kernel names once, integer rows  params.. nbox nblocks 8*nbox nlaunch (kernel grid bx by lds attr)*nlaunch"""
    parsed, kernels, odd = [], set(), []
    for line in lines:
        kind = line[0]
        if kind == "X":
            odd.append(line)
        elif kind == "A":
            head, state, *launches = line.split("\t")
            _, mode, family, *params = head.split(" ")
            launches = [launch.rsplit("|", 1) for launch in launches]
            kernels.update(k for k, _ in launches)
            parsed.append((mode + "/" + family, [int(p) for p in params], [int(v) for v in state.split(" ")], launches))
    assert not odd, "calls that failed otherwise than hipErrorInvalidValue without a launch:\n" + "\n".join(odd[:10])
    kernels = sorted(kernels)
    index = {k: i for i, k in enumerate(kernels)}
    T = {"kernels": kernels, "families": {}, "values": {}}
    for line in lines:
        f = line.split(" ")
        if f[0] == "R":
            T["families"][f[1] + "/" + f[2]] = {"rejected": int(f[3]), "calls": int(f[4]), "rows": []}
        elif f[0] == "V":
            T["values"].setdefault(f[1] + "/" + f[2], []).append([int(v) for v in f[3:]])
    for key, params, state, launches in parsed:
        assert state[0] == 0 and len(state) == 3 + 8 * max(state[1], 0), (key, params, state)
        row = params + state[1:] + [len(launches)]
        for k, nums in launches:
            row += [index[k]] + [int(v) for v in nums.split(" ")]
        T["families"][key]["rows"].append(row)
    return T


def load_table():
    with gzip.open(TABLE, "rt") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def dispatch(tmp_path_factory):
    from ramses_amd import build
    build.build()
    return table_of(dump(build.BUILD, str(tmp_path_factory.mktemp("sweep_dispatch"))))


def test_the_record_holds_every_launcher_of_both_modes():
    T = load_table()
    assert set(T["families"]) == {m + "/" + f for m, f in FAMILIES}
    assert set(T["values"]) == {m + "/" + f for m, f in VALUES}
    for (mode, family), (params, calls, accepted) in FAMILIES.items():
        F = T["families"][mode + "/" + family]
        assert F["calls"] == calls and len(F["rows"]) == accepted > 0 and F["rejected"] == calls - accepted, (mode, family)
        assert any(r[len(params.split()) + 2 + 8 * max(r[len(params.split())], 0)] > 0 for r in F["rows"]), (mode, family, "no launch")
    for (mode, fn), (params, n) in VALUES.items():
        assert len(T["values"][mode + "/" + fn]) == n > 0
    for fn in ("godunov_sweep_kernel", "godunov_sweep_nener_kernel", "godunov_scalar_kernel", "surface_flux_kernel"):
        for mode in ("strictmode", "fastmode"):
            assert any("::%s::%s<" % (mode, fn) in k for k in T["kernels"]), (mode, fn)
    for fn in ("godunov_sweep_pfix_kernel", "godunov_sweep_difmag_kernel", "surface_flux_pfix_kernel", "surface_flux_difmag_kernel"):
        assert any("::strictmode::%s<" % fn in k for k in T["kernels"]), fn


def _readable(T, key, row):
    np_ = len(FAMILIES[tuple(key.split("/"))][0].split())
    nbox = max(row[np_], 0)
    at = np_ + 2 + 8 * nbox
    launches = [[T["kernels"][row[i]]] + row[i + 1:i + 6] for i in range(at + 1, len(row), 6)]
    return {"params": row[:np_], "nbox": row[np_], "nblocks": row[np_ + 1], "boxes": row[np_ + 2:at], "launches": launches}


def test_dispatch_equals_the_record(dispatch):
    T = load_table()
    assert dispatch["values"] == T["values"]
    for key in sorted(T["families"]):
        want, got = T["families"][key], dispatch["families"].get(key)
        assert got is not None, key + ": the launcher is gone"
        np_ = len(FAMILIES[tuple(key.split("/"))][0].split())
        w = {tuple(r[:np_]): _readable(T, key, r) for r in want["rows"]}
        g = {tuple(r[:np_]): _readable(dispatch, key, r) for r in got["rows"]}
        diff = [(p, w.get(p), g.get(p)) for p in sorted(set(w) | set(g)) if w.get(p) != g.get(p)]
        assert not diff, "%s: %d calls differ (parameters: %s), the first: %r" % (key, len(diff), FAMILIES[tuple(key.split("/"))][0], diff[:3])
        # every other call of the grid: hipErrorInvalidValue and no launch
        assert (got["calls"], got["rejected"]) == (want["calls"], want["rejected"]), key
    assert set(dispatch["families"]) == set(T["families"])
    assert dispatch["kernels"] == T["kernels"]


if __name__ == "__main__":
    # --record [OBJECT DIRECTORY]: write the table from the objects of the current build
    import tempfile
    assert sys.argv[1:2] == ["--record"], __doc__
    sys.path.insert(0, ROOT)
    from ramses_amd import build
    if len(sys.argv) > 2:
        objdir = sys.argv[2]
    else:
        build.build()
        objdir = build.BUILD
    with tempfile.TemporaryDirectory() as tmp:
        T = table_of(dump(objdir, tmp))
    with open(TABLE, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(T, separators=(",", ":")).encode())
    for key, F in sorted(T["families"].items()):
        print("%-32s calls %6d accepted %5d" % (key, F["calls"], len(F["rows"])))
    print(len(T["kernels"]), "kernels,", os.path.getsize(TABLE), "bytes")

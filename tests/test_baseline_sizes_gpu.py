"""GPU tests at the sizes BASELINE.json quotes.

1. The fast-arithmetic build of the sweep (FMA contraction, rcp/rsq + Newton, fused LLF)
   against the strict build (bit-identical to the reference): >= 20 steps of sedov3d.nml at
   64^3 and 128^3, both paths stepping on their own CFL dt like a namelist run, relative
   L-infinity on rho, rho*u, rho*v, rho*w and E checked at EVERY step against north_star's
   1e-12.  This is what certifies (or refuses) `config.arithmetic` of the bench line.
2. Live A/B of the two reference builds on the GPU box: oracle/_ref/ramses3d_mpi (untouched
   reference, MPI on the host cores) vs oracle/_ref/ramses3d_patch (the same program with
   ramses_amd/patch, level resident on the GPU) on sedov3d.nml as shipped (nstepmax=10) at
   128^3 and 256^3 (config C2): the assembled level must be equal bit for bit.
3. Config C4 stand-in at 128^3 (hydro + self-gravity, three coarse steps), config C5 at
   levels 7-9 and an AMR + self-gravity run at levels 6-8 through the patched program against
   checksums of the serial reference (tests/golden/baseline_sizes.json, made by
   tests/golden/make_golden_baseline.py).
"""
import json
import os
import shutil

import numpy as np
import pytest

import live

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MPI = os.path.join(ROOT, "oracle", "_ref", "ramses3d_mpi")
PATCHED = os.path.join(ROOT, "oracle", "_ref", "ramses3d_patch")
GOLD = os.path.join(ROOT, "tests", "golden", "baseline_sizes.json")
TOL = 1e-12     # north_star: "results within 1e-12 relative L-infinity of the F90 reference"


def _rel_linf_per_var(a, b):
    """max |a-b| / max |b| for every variable; the three momenta share one scale (|rho v| of the blast)"""
    out = []
    mom_scale = max(np.abs(b[1:4]).max(), 1e-300)
    for n in range(a.shape[0]):
        scale = mom_scale if 1 <= n <= 3 else max(np.abs(b[n]).max(), 1e-300)
        out.append(np.abs(a[n] - b[n]).max() / scale)
    return np.array(out)


@pytest.mark.parametrize("n,nsteps", [(64, 24), (128, 24)])
def test_fast_build_multistep_within_tolerance(gpu_lib, n, nsteps):
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    u, dx = ic.sedov3d(n)
    strict = HydroLevel(n, n, n, dx, params=ramses_amd.make_params(courant_factor=0.8, fast_math=0))
    fast = HydroLevel(n, n, n, dx, params=ramses_amd.make_params(courant_factor=0.8, fast_math=1))
    strict.upload(u)
    fast.upload(u)
    worst = np.zeros(5)
    for step in range(nsteps):
        dts = strict.courant_fine()[0]
        dtf = fast.courant_fine()[0]
        assert abs(dtf - dts) <= TOL * dts, (step, dts, dtf)
        strict.step(dts)
        fast.step(dtf)
        err = _rel_linf_per_var(fast.download(), strict.download())
        worst = np.maximum(worst, err)
        assert (err <= TOL).all(), "step %d: rel-Linf (rho, mx, my, mz, E) = %s" % (step + 1, err)
    print("fast vs strict, %d^3, %d steps: worst rel-Linf per variable %s" % (n, nsteps, worst))


@pytest.mark.parametrize("slope_type,nsteps", [(1, 40), (2, 40), (8, 24)])
def test_fast_hllc_multistep_within_tolerance(gpu_lib, slope_type, nsteps):
    """the fused fast HLLC flux (hydro_core.hpp hllc_flux_fast, round 6: one reciprocal per wave-speed sum, one star state,
    FMA forms) against the strict build -- the reference's own operations -- each on its own Courant dt, after EVERY step of a
    developing blast at 64^3 (the live certificates against the reference PROGRAM: tests/test_fast_certificate_gpu.py)"""
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    n = 64
    u, dx = ic.sedov3d(n)
    mk = lambda fm: HydroLevel(n, n, n, dx, params=ramses_amd.make_params(courant_factor=0.8, fast_math=fm, riemann="hllc", slope_type=slope_type))  # noqa: E731
    strict, fast = mk(0), mk(1)
    strict.upload(u)
    fast.upload(u)
    worst = np.zeros(5)
    for step in range(nsteps):
        dts = strict.courant_fine()[0]
        dtf = fast.courant_fine()[0]
        assert abs(dtf - dts) <= TOL * dts, (step, dts, dtf)
        strict.step(dts)
        fast.step(dtf)
        err = _rel_linf_per_var(fast.download(), strict.download())
        worst = np.maximum(worst, err)
        assert (err <= TOL).all(), "step %d: rel-Linf (rho, mx, my, mz, E) = %s" % (step + 1, err)
    assert worst.max() > 0.0          # (the fast build did run)
    print("fast vs strict HLLC, slope %d, %d^3, %d steps: worst rel-Linf per variable %s" % (slope_type, n, nsteps, worst))


def test_fast_build_at_the_size_of_the_bench_line(gpu_lib):
    """the certificate at the bench's OWN size (VERDICT round 4, next #7 i): 512^3, 20 steps of sedov3d.nml, the fast and the
    strict build stepping on their own Courant dt; relative L-infinity per variable after EVERY step <= 1e-12, on the device
    (the state is 5.4 GB per copy)"""
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    n, nsteps = 512, 20
    corner, back, dx = ic.sedov3d_corner_and_background(n)
    levs = []
    for fm in (0, 1):
        lev = HydroLevel(n, n, n, dx, params=ramses_amd.make_params(courant_factor=0.8, fast_math=fm), ng=0)
        for v in range(5):
            lev.uold[v].fill_(float(back[v]))
            lev.uold[v, 0, 0, 0] = float(corner[v])
        levs.append(lev)
    strict, fast = levs
    worst = np.zeros(5)
    for step in range(nsteps):
        dts, dtf = strict.courant_fine()[0], fast.courant_fine()[0]
        assert abs(dtf - dts) <= TOL * dts, (step, dts, dtf)
        strict.step(dts)
        fast.step(dtf)
        a, b = fast.uold, strict.uold
        mom_scale = max(float(b[1:4].abs().max().item()), 1e-300)
        err = np.zeros(5)
        for v in range(5):
            scale = mom_scale if 1 <= v <= 3 else max(float(b[v].abs().max().item()), 1e-300)
            err[v] = float((a[v] - b[v]).abs().max().item()) / scale
        worst = np.maximum(worst, err)
        assert (err <= TOL).all(), "step %d: rel-Linf (rho, mx, my, mz, E) = %s" % (step + 1, err)
    print("fast vs strict, 512^3, %d steps: worst rel-Linf per variable %s" % (nsteps, worst))


def _nproc():
    n = os.cpu_count() or 1
    p = 1
    while p * 2 <= min(n, 32):
        p *= 2
    return p


@pytest.mark.parametrize("level", [7, 8])
def test_live_reference_ab_c2(gpu_lib, level):
    """sedov3d.nml as shipped (LLF + minmod, nstepmax=10) at 128^3 / 256^3: the untouched reference
    under MPI on the host cores vs the patched program with the level resident on the GPU."""
    if not (os.path.exists(REF_MPI) and os.path.exists(PATCHED)):
        pytest.skip("oracle/_ref/ramses3d_mpi / ramses3d_patch not built")
    from oracle import ramses_snapshot as rs
    nproc = _nproc()
    nml = rs.sedov3d_namelist(level=level, nstepmax=10, foutput=10, mem_factor=1.3)
    os.environ["RAMSES_AMD"] = "1"
    workp, outp = rs.run_reference(nml, binary=PATCHED)
    try:
        assert "stays resident on the GPU" in outp
        got = rs.load_uniform_level(os.path.join(workp, "output_00002"), level)
    finally:
        shutil.rmtree(workp, ignore_errors=True)
    nml_mpi = rs.sedov3d_namelist(level=level, nstepmax=10, foutput=10, mem_factor=3.0 if nproc > 1 else 1.3)
    workr, outr = rs.run_reference(nml_mpi, binary=REF_MPI, nproc=nproc)
    try:
        ref = rs.load_uniform_level(os.path.join(workr, "output_00002"), level)
    finally:
        shutil.rmtree(workr, ignore_errors=True)
    assert got["info"]["t"] == ref["info"]["t"]
    assert np.array_equal(got["prim"], ref["prim"]), np.abs(got["prim"] - ref["prim"]).max()


def test_c4_standin_128_checksum(gpu_lib):
    """config C4 stand-in at 128^3: three coarse steps of hydro + self-gravity through the patched
    program (level resident: multigrid_fine, force_fine, rho_fine, synchro_hydro_fine, the gravity terms of
    courant_fine / godunov_fine / set_uold) == the serial reference, by checksum of (prim, phi, f)."""
    if not os.path.exists(PATCHED) or not os.path.exists(GOLD):
        pytest.skip("patched program or golden checksums missing")
    gold = json.load(open(GOLD)).get("c4_128")
    if gold is None:
        pytest.skip("no c4_128 checksum")
    from oracle import ramses_snapshot as rs
    mkb = live.golden_module("baseline")
    os.environ["RAMSES_AMD"] = "1"
    work, out = rs.run_reference(mkb.c4_namelist(), binary=PATCHED)
    try:
        assert "stays resident on the GPU" in out
        assert mkb.solves(out) == gold["solves"]
        snap = rs.load_uniform_level(os.path.join(work, "output_00002"), 7, with_grav=True)
        assert snap["info"]["t"] == gold["t"]
        assert snap["info"]["rho_tot"] == gold["rho_tot"]
        assert mkb.digest_uniform(snap) == gold["sha256"]
    finally:
        shutil.rmtree(work, ignore_errors=True)


@pytest.mark.parametrize("resident", ["1", "0"])
def test_c5_levels_7_9_checksum(gpu_lib, resident):
    """config C5 at levels 7-9 (8 coarse steps, ~2.1 M leaf cells): the tree-walking sweep on every
    level, with sub-cycling and regridding, == the serial reference by checksum of the sorted leaf data.
    resident = 1 (default): uold/unew and the tree stay on the device across set_unew / godunov_fine /
    set_uold / upload_fine / courant_fine / hydro_flag, levels travel only around refine_fine;
    0 (RAMSES_AMD_RESIDENT_AMR=0): the arrays are staged around every godunov_fine, the rest is host code."""
    if not os.path.exists(PATCHED) or not os.path.exists(GOLD):
        pytest.skip("patched program or golden checksums missing")
    gold = json.load(open(GOLD)).get("c5_79")
    if gold is None:
        pytest.skip("no c5_79 checksum")
    from oracle import ramses_snapshot as rs
    mkb = live.golden_module("baseline")
    os.environ["RAMSES_AMD"] = "1"
    os.environ["RAMSES_AMD_RESIDENT_AMR"] = resident
    os.environ["RAMSES_AMD_STATS"] = "1"
    os.environ["RAMSES_AMD_TILE_MIN_OCTS"] = "0"       # the small partial levels through the dense sweep too (production: the tree)
    try:
        work, out = rs.run_reference(mkb.c5_namelist(), binary=PATCHED)
    finally:
        os.environ.pop("RAMSES_AMD_RESIDENT_AMR", None)
        os.environ.pop("RAMSES_AMD_STATS", None)
        os.environ.pop("RAMSES_AMD_TILE_MIN_OCTS", None)
    try:
        assert ("AMR levels stay resident on the GPU" in out) == (resident == "1")
        if resident == "1":
            # round 5: the resident levels live in the device's tiles and take the DENSE sweep -- levelmin (fully refined) and
            # the partial levels alike; this run against the reference's checksum is their live parity test
            import re
            m = re.search(r"godunov_fine of AMR levels: (\d+) sweeps through the dense kernel on tiles \((\d+) of them fully refined levels\), (\d+) through the tree-walking", out)
            assert m, out[-1500:]
            dense, covered, tree = (int(x) for x in m.groups())
            print("C5 7-9: %d dense sweeps (%d of the fully refined levelmin), %d tree-walking" % (dense, covered, tree))
            assert covered >= 8 and dense > covered and tree == 0, (dense, covered, tree)
        snap = rs.load_leaf_cells(os.path.join(work, "output_00002"))
        assert [int((snap["level"] == l).sum()) for l in (7, 8, 9)] == gold["ncell"]
        assert snap["info"]["t"] == gold["t"]
        assert mkb.digest_leaves(snap) == gold["sha256"]
    finally:
        shutil.rmtree(work, ignore_errors=True)


def test_c5_levels_7_10_on_8_ranks_equals_the_mpi_reference(gpu_lib):
    """BASELINE config C5 as stated (sedov3d.nml, levelmin=7, levelmax=10, 8 ranks), 8 coarse steps: the patched MPI
    program with every rank's cell vectors and tree resident on the GPU and both virtual-boundary exchanges of every level
    on the device (the eight ranks share this box's one GPU: host-MPI transport) against the MPI reference on the same
    eight ranks, live: leaf cells (level, position, primitive variables) and the time, bit for bit."""
    ref_mpi = os.path.join(ROOT, "oracle", "_ref", "ramses3d_mpi")
    pat_mpi = os.path.join(ROOT, "oracle", "_ref", "ramses3d_mpi_patch")
    if not (os.path.exists(ref_mpi) and os.path.exists(pat_mpi)):
        pytest.skip("oracle/_ref/ramses3d_mpi[_patch] not built")
    from oracle import ramses_snapshot as rs
    mkb = live.golden_module("baseline")
    nml = mkb.c5_namelist(7, 10, 8, 3000000)
    os.environ["RAMSES_AMD"] = "1"
    work, out = rs.run_reference(nml, nproc=8, binary=pat_mpi)
    try:
        assert "AMR levels stay resident on the GPU" in out, out[-2000:]
        got = rs.load_leaf_cells(os.path.join(work, "output_00002"))
        dg = mkb.digest_leaves(got)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    os.environ["RAMSES_AMD"] = "0"
    try:
        work, out = rs.run_reference(nml, nproc=8, binary=ref_mpi)
    finally:
        os.environ["RAMSES_AMD"] = "1"
    try:
        ref = rs.load_leaf_cells(os.path.join(work, "output_00002"))
        dr = mkb.digest_leaves(ref)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    counts = [int((ref["level"] == l).sum()) for l in (7, 8, 9, 10)]
    assert min(counts) > 1000, counts                      # all four levels are populated
    assert [int((got["level"] == l).sum()) for l in (7, 8, 9, 10)] == counts
    assert got["info"]["t"] == ref["info"]["t"]
    assert dg == dr


def _c5_gravity_namelist(mkb, lmin, lmax, nstep, ngridtot, kind):
    """BASELINE config C5 WITH its multigrid: kind 'sedov' = sedov3d.nml + poisson=.true. (uniform density, the blast's
    shell is the source), 'blob' = the blob + blast setup of tests/golden/make_golden_amr.py moved to these levels"""
    from oracle import ramses_snapshot as rs
    if kind == "blob":
        return mkb.amr_grav_namelist(lmin, lmax, nstep).replace("ngridtot=600000 !", "ngridtot=%d !" % ngridtot)
    nml = rs.sedov3d_namelist(level=lmin, nstepmax=nstep, foutput=nstep, poisson=True,
                              extra=mkb.REFINE + "&POISSON_PARAMS\nepsilon=1d-5\n/\n")
    return nml.replace("levelmax=%d" % lmin, "levelmax=%d" % lmax).replace("ngridtot=", "ngridtot=%d !" % ngridtot)


@pytest.mark.parametrize("lmin,lmax,nproc,nstep,kind", [(7, 10, 8, 8, "sedov"), (7, 9, 4, 8, "sedov"), (7, 9, 4, 3, "blob")])
def test_c5_with_multigrid_equals_the_mpi_reference(gpu_lib, tmp_path, lmin, lmax, nproc, nstep, kind):
    """BASELINE config C5 as stated -- "sedov3d.nml with AMR levelmin=7 levelmax=10: Godunov + multigrid, 8 ranks" -- live
    against the MPI reference on the same ranks: leaf cells (level, position, primitive variables, phi, f), the time and the
    V-cycle count of every solve, bit for bit.  The whole gravity step of the patched program runs on the ranks' GPU (they
    share this box's one device, host-MPI transport): rho_fine's deposit with its three exchanges per level
    (ramses_amd_rho_fine_mpi), the multigrid with the levels resident, force_fine of every level
    (ramses_amd_force_fine_mpi / the distributed dense solve's brick at levelmin) -- asserted on the profile rows."""
    ref_mpi = os.path.join(ROOT, "oracle", "_ref", "ramses3d_mpi")
    pat_mpi = os.path.join(ROOT, "oracle", "_ref", "ramses3d_mpi_patch")
    if not (os.path.exists(ref_mpi) and os.path.exists(pat_mpi)):
        pytest.skip("oracle/_ref/ramses3d_mpi[_patch] not built")
    if nproc > (os.cpu_count() or 1):
        pytest.skip("fewer cores than ranks")
    import re
    from oracle import ramses_snapshot as rs
    mkb = live.golden_module("baseline")
    nml = _c5_gravity_namelist(mkb, lmin, lmax, nstep, 3000000 if lmax == 10 else 1500000, kind)
    pat = r"==> Level=\s*(\d+) Step=\s*(\d+)"
    prof = str(tmp_path / "profile.txt")
    os.environ["RAMSES_AMD"] = "1"
    os.environ["RAMSES_AMD_PROFILE"] = prof
    try:
        work, out = rs.run_reference(nml, nproc=nproc, binary=pat_mpi)
    finally:
        os.environ.pop("RAMSES_AMD_PROFILE", None)
    try:
        assert "AMR levels stay resident on the GPU" in out, out[-2000:]
        sol_p = re.findall(pat, out)
        got = rs.load_leaf_cells(os.path.join(work, "output_00002"), with_grav=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    rows = open(prof).read()
    assert "rho_fine (device, MPI)" in rows and "force_fine (device, MPI)" in rows, rows[-1500:]
    os.environ["RAMSES_AMD"] = "0"
    try:
        work, out = rs.run_reference(nml, nproc=nproc, binary=ref_mpi)
    finally:
        os.environ["RAMSES_AMD"] = "1"
    try:
        sol_r = re.findall(pat, out)
        ref = rs.load_leaf_cells(os.path.join(work, "output_00002"), with_grav=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    levels = list(range(lmin, lmax + 1))
    counts = [int((ref["level"] == l).sum()) for l in levels]
    assert min(counts) > 500, counts                      # every level is populated
    assert len(sol_r) > 0 and {int(a) for a, _ in sol_r} >= set(levels[:-1])
    assert sol_p == sol_r
    assert [int((got["level"] == l).sum()) for l in levels] == counts
    assert got["info"]["t"] == ref["info"]["t"]
    assert mkb.digest_leaves_grav(got) == mkb.digest_leaves_grav(ref), (
        np.abs(np.sort(got["grav"], axis=1) - np.sort(ref["grav"], axis=1)).max())


@pytest.mark.parametrize("mode", ["resident", "staged", "host-driver"])
def test_amr_self_gravity_levels_6_8_checksum(gpu_lib, mode):
    """AMR + self-gravity at levels 6-8 (0.53 M leaf cells, 3 coarse steps with regridding) through the patched
    program == the serial reference by checksum of the sorted leaf data (level, x, prim, phi, f) and V-cycle counts.
    resident (default): uold/unew, the tree and a copy of f stay on the device; multigrid_fine (driver and per-solve
    setup) and force_fine of the partially refined levels are device code, rho_fine gets the density back.
    staged (RAMSES_AMD_RESIDENT_GRAV=0): same solvers, the hydro arrays cross PCIe around every call.
    host-driver (+ RAMSES_AMD_MG_DRIVER=host): the reference's multigrid driver and force_fine with the device operators."""
    if not os.path.exists(PATCHED) or not os.path.exists(GOLD):
        pytest.skip("patched program or golden checksums missing")
    gold = json.load(open(GOLD)).get("amr_grav_68")
    if gold is None:
        pytest.skip("no amr_grav_68 checksum")
    from oracle import ramses_snapshot as rs
    mkb = live.golden_module("baseline")
    env = {"RAMSES_AMD": "1"}
    if mode != "resident":
        env["RAMSES_AMD_RESIDENT_GRAV"] = "0"
    if mode == "host-driver":
        env["RAMSES_AMD_MG_DRIVER"] = "host"
    os.environ.update(env)
    try:
        work, out = rs.run_reference(mkb.amr_grav_namelist(), binary=PATCHED)
    finally:
        for k in ("RAMSES_AMD_RESIDENT_GRAV", "RAMSES_AMD_MG_DRIVER"):
            os.environ.pop(k, None)
    try:
        assert ("AMR levels stay resident on the GPU" in out) == (mode == "resident")
        assert mkb.solves(out) == gold["solves"]
        snap = rs.load_leaf_cells(os.path.join(work, "output_00002"), with_grav=True)
        assert [int((snap["level"] == l).sum()) for l in (6, 7, 8)] == gold["ncell"]
        assert snap["info"]["t"] == gold["t"]
        assert mkb.digest_leaves_grav(snap) == gold["sha256"]
    finally:
        shutil.rmtree(work, ignore_errors=True)

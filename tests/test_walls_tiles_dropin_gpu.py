"""Live: the patched program between six walls with its levels in TILES (csrc/amr_layout.hpp with a coarse grid of 3 x 3 x 3
cells, ramses_amd_amrres_coarse_grid from patch/ramses_amd_iface.f90) against the untouched reference program: a point explosion
three cells off a corner, walls of mixed type with the no_inflow clamp, levels 6-7 (the coarsest levels whose 3 * 2^(l-1) octs
per side are whole tiles), sub-cycling and regrids -- leaf cells bit for bit, every godunov_fine of a level through the dense
kernel.  The namelist and the run helpers are those of tests/test_walls_resident_gpu.py."""
import re
import shutil

import numpy as np
import pytest

import live
import test_walls_resident_gpu as W

pytestmark = pytest.mark.gpu

ENV = {"RAMSES_AMD": "1", "RAMSES_AMD_STRICT": "1", "RAMSES_AMD_STATS": "1", "RAMSES_AMD_TILE_MIN_OCTS": "0", "RAMSES_AMD_PROFILE": "1"}
STATS = re.compile(r"godunov_fine of AMR levels:\s*(\d+) sweeps through the dense kernel on tiles.*?(\d+) through the tree-walking kernel; (\d+) levels in tiles")


@pytest.mark.parametrize("nproc", [1, 2])
def test_sedov_between_six_walls_sweeps_its_levels_in_tiles(gpu_lib, nproc):
    pat_bin, ref_bin = live.binaries(nproc > 1)
    nml = W._namelist(6, 7, "1,1,1,1,1,2,2", "hllc", 1, 3, "1, 2, 2, 1, 1, 2", True)
    nml = nml.replace("ngridtot=30000 !", "ngridtot=%d !" % (500000 * nproc))
    assert "levelmin=6" in nml and "levelmax=7" in nml and "ngridtot=%d" % (500000 * nproc) in nml and "no_inflow=.true." in nml
    workp, outp = live.run(nml, pat_bin, nproc, ENV)
    try:
        assert "AMR levels stay resident on the GPU" in outp and "make_boundary_hydro (device)" in outp, outp[-3000:]
        got = live.leaves(workp)
    finally:
        shutil.rmtree(workp, ignore_errors=True)
    lines = STATS.findall(outp)
    assert len(lines) == nproc, outp[-3000:]
    for tiles, tree, ntiled in lines:          # (levelmin = 6: every level of the run is a level >= 6)
        assert int(tiles) > 0 and int(tree) == 0 and int(ntiled) >= 1, lines
    workr, _ = live.run(nml, ref_bin, nproc, {})
    try:
        ref = live.leaves(workr)
    finally:
        shutil.rmtree(workr, ignore_errors=True)
    assert got[3] == ref[3]
    assert (ref[0] == 7).sum() > 1000, "the run must have refined"
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2].view(np.int64), ref[2].view(np.int64)), np.abs(got[2] - ref[2]).max()

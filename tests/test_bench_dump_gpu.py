"""bench.py --dump-outputs: the files hold what the timed steps computed -- the whole brick, bit for bit against the same steps
run here through HydroLevel -- and two runs with the same arguments write the same arrays (the sampled form, above
bench.DUMP_CELLS cells).  Only the headline leg runs (no spin-up, no extra legs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_ONLY = ["--spinup-ms", "0", "--stress-steps", "0", "--vcycle-level", "0", "--amr-level", "0", "--mhd-level", "0",
                 "--no-cpu-baseline"]


def _bench(out_dir, n, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--n", str(n), "--dump-outputs", str(out_dir)] + HEADLINE_ONLY
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-800:], r.stderr[-2000:])
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == steps and j["warmup"] == warmup and j["ms_per_step"] > 0
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in j["dumped_outputs"]["files"]) <= 64 << 20
    return j


def test_dump_is_the_state_of_the_last_timed_step(gpu_lib, tmp_path):
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    n, steps, warmup = 32, 4, 2
    j = _bench(tmp_path, n, steps, warmup)
    assert sorted(j["dumped_outputs"]["files"]) == ["state.npy", "state_sum.npy"]
    got = np.load(tmp_path / "state.npy")
    assert got.dtype == np.float64 and got.shape == (5, n, n, n)
    # bench.py's single-rank path: the fast build, one dt from the initial state, warm-up + timed steps of godunov_fine + set_uold
    lev = HydroLevel(n, n, n, 0.5 / n, params=ramses_amd.make_params(courant_factor=0.8, fast_math=True), ng=0)
    u, _ = ic.sedov3d(n)
    lev.upload(u)
    dt = lev.courant_fine()[0]
    for _ in range(warmup + steps):
        lev.godunov_fine(dt)
        lev.set_uold()
    want = lev.download()
    assert np.array_equal(got, want)
    # (summed on the device in another order; the momenta cancel to round-off, so the bound is relative to sum |u|)
    sums = np.load(tmp_path / "state_sum.npy")
    assert sums.dtype == np.float64
    assert np.all(np.abs(sums - want.sum(axis=(1, 2, 3))) <= 1e-12 * np.abs(want).sum(axis=(1, 2, 3)))


def test_dump_sample_is_the_same_in_every_run(gpu_lib, tmp_path):
    n, steps, warmup = 128, 3, 1
    runs = [_bench(tmp_path / ("run%d" % k), n, steps, warmup) for k in range(2)]
    files = sorted(runs[0]["dumped_outputs"]["files"])
    assert files == ["state_sample.npy", "state_sample_cells.npy", "state_sum.npy"]
    a = {f: np.load(tmp_path / "run0" / f) for f in files}
    b = {f: np.load(tmp_path / "run1" / f) for f in files}
    cells = a["state_sample_cells.npy"]
    assert a["state_sample.npy"].shape == (5, cells.size) and cells.size > 0
    assert np.all(np.diff(cells) > 0) and cells[0] >= 0 and cells[-1] < n ** 3
    for f in files:
        assert a[f].dtype == np.float64 and np.array_equal(a[f], b[f]), f
    # the sample is of a physical state: positive density and energy everywhere it looks
    assert np.all(a["state_sample.npy"][0] > 0) and np.all(a["state_sample.npy"][4] > 0)

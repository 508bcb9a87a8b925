"""The density floor of the traced states behind one wave-uniform test, and the left shift that hands lane 63 a zero.

The full rows of the fast dense sweep test the six traced densities of a cell against smallr once per wave and run the
selects only in the waves that hold a density below it (csrc/hydro_core.hpp trace3d_cell RHO6): a wave with a floored cell
takes another path through the rest of the iteration than a wave without one, and both must compute the same.  The left
shift of the x fluxes no longer hands lane 63 its own value but 0 (csrc/hydro_sweep.hip wave_shl1), in the strict build too.

Box: periodic, 72 x 20 x 12 cells -- two x tiles (60 + 12 owned columns), three y tiles of the 12-row kernel (8 + 8 + 4 owned
rows; five of the 8-row kernel), one z-chunk with its priming planes.
State: a dense slab across the box and, beside it, a small region of low density that is blown apart (a strong rarefaction),
with smallr raised to just below the lowest density: the trace undershoots smallr in that region and nowhere else, so only
the waves of a few rows and planes floor anything.  That this is so is asserted with the CPU oracle alone
(test_the_floor_acts_in_some_cells_only), before any GPU result is looked at.
"""
import numpy as np
import pytest

gpu = pytest.mark.gpu

NX, NY, NZ = 72, 20, 12
DX = 1.0 / NX
SHIFT = (7, 3, 5)          # cells along x, y, z
STEPS = 2
SMALLR = 0.05              # raised: the lowest density of the state is 0.06
CENTRE = (30.0, 9.0, 5.0)  # of the low-density region, in cells (x, y, z)
RADIUS = 5.0


def _state():
    """conserved variables [5, nz, ny, nx], every density above SMALLR"""
    z, y, x = np.meshgrid(np.arange(NZ) + 0.5, np.arange(NY) + 0.5, np.arange(NX) + 0.5, indexing="ij")
    rng = np.random.default_rng(20261)
    rx, ry, rz = x - CENTRE[0], y - CENTRE[1], z - CENTRE[2]
    s = np.sqrt(rx * rx + ry * ry + rz * rz) / RADIUS
    hole = np.exp(-s ** 4)                                   # 1 at the centre, 0 outside
    rho = 1.0 - 0.94 * hole                                  # 0.06 at the centre
    rho = rho + 3.0 * ((x > 40) & (x < 48))                  # the slab
    rho = rho * (1.0 + 0.01 * rng.standard_normal(rho.shape).clip(-2, 2) * (1.0 - hole))
    p = 0.05 * rho ** 1.4 + 0.02
    # blown apart: the velocity grows outwards through the region and falls off beyond it
    amp = 3.0 * s * np.exp(-0.5 * s ** 4) / np.maximum(s * RADIUS, 1e-30)
    u, v, w = amp * rx, amp * ry, amp * rz
    u = u + 0.05 * np.sin(2 * np.pi * y / NY)
    e = p / 0.4 + 0.5 * rho * (u * u + v * v + w * w)
    out = np.stack([rho, rho * u, rho * v, rho * w, e])
    assert out[0].min() > SMALLR
    return np.ascontiguousarray(out)


def _gravity():
    """a smooth periodic acceleration field [3, nz, ny, nx]"""
    z, y, x = np.meshgrid(np.arange(NZ) * (2 * np.pi / NZ), np.arange(NY) * (2 * np.pi / NY),
                          np.arange(NX) * (2 * np.pi / NX), indexing="ij")
    return np.stack([0.3 * np.sin(x) * np.cos(y), 0.2 * np.sin(y + z), -0.25 * np.cos(z) * np.sin(x)])


def _roll(a):
    return np.roll(a, (SHIFT[2], SHIFT[1], SHIFT[0]), axis=(-3, -2, -1))


_ORACLE = {}


def _oracle_runs(oracle):
    """the state, its time step and the oracle's result after STEPS steps with the raised smallr and with the default one:
    computed once, shared, never written to"""
    if not _ORACLE:
        u = _state()
        dt = oracle.courant_uniform(oracle.make_params(smallr=SMALLR), u, DX, 0.8)
        for key, smallr in (("raised", SMALLR), ("default", 1e-10)):
            p = oracle.make_params(smallr=smallr, slope_type=1, riemann="llf")
            a = u
            for _ in range(STEPS):
                a = oracle.godunov_uniform(p, a, DX, dt)
            a.setflags(write=False)
            _ORACLE[key] = a
        u.setflags(write=False)
        _ORACLE["u"], _ORACLE["dt"] = u, dt
    _floor_acts_in_some_cells_only(_ORACLE)       # every test stands on this
    return _ORACLE


def _floor_acts_in_some_cells_only(o):
    """the raised smallr changes the oracle's result (traced densities fall below it), and in fewer than half of the cells --
    and of the (y, z) rows, which are the sweep's waves -- so that waves with and without a floored cell both occur"""
    assert np.isfinite(o["raised"]).all() and np.isfinite(o["default"]).all()
    differs = (o["raised"] != o["default"]).any(axis=0)
    rows = differs.any(axis=-1)
    assert differs.any()
    assert differs.sum() < differs.size // 2
    assert rows.sum() < rows.size // 2
    return differs, rows


def _run(u, dt, grav, rows, fast):
    import torch
    import ramses_amd
    from ramses_amd.hydro import HydroLevel, godunov_tune
    p = ramses_amd.make_params(courant_factor=0.8, fast_math=fast, riemann="llf", slope_type=1, smallr=SMALLR)
    lev = HydroLevel(NX, NY, NZ, DX, params=p, ng=0, poisson=grav is not None)
    lev.upload(u)
    if grav is not None:
        lev.f.copy_(torch.as_tensor(grav, dtype=torch.float64).to(lev.device))
    godunov_tune(tile_rows=rows)
    try:
        for _ in range(STEPS):
            lev.step(dt)
        torch.cuda.synchronize()
    finally:
        godunov_tune()
    return lev.download().copy()


def test_the_floor_acts_in_some_cells_only(oracle):
    """a condition on the state, not a measurement: from the CPU oracle alone (needs no GPU)"""
    differs, rows = _floor_acts_in_some_cells_only(_oracle_runs(oracle))
    print("cells that feel the raised smallr: %d of %d; (y, z) rows with such a cell: %d of %d" % (
        differs.sum(), differs.size, rows.sum(), rows.size))


@gpu
@pytest.mark.parametrize("grav,rows", [(False, 0), (True, 0), (False, 8)])
def test_shifted_input_gives_the_shifted_output_bit_for_bit(gpu_lib, oracle, grav, rows):
    """fast LLF + minmod: the shift moves the floored cells into other waves, lanes, tile rows and plane parities"""
    o = _oracle_runs(oracle)
    g = _gravity() if grav else None
    a = _run(o["u"], o["dt"], g, rows, True)
    b = _run(_roll(o["u"]), o["dt"], None if g is None else _roll(g), rows, True)
    assert np.isfinite(a).all()
    assert not np.array_equal(a, o["u"])
    want = _roll(a)
    diff = np.abs(b - want).max()
    print("grav %s rows %d: max |shifted run - shifted result| = %g" % (grav, rows, diff))
    assert np.array_equal(b, want), "the sweep depends on where a cell falls in its tile: max abs diff %g" % diff


@gpu
def test_fast_build_against_the_oracle(gpu_lib, oracle):
    """to 1e-12 of each variable's scale (the momenta share one), the fast build's bound"""
    o = _oracle_runs(oracle)
    a = _run(o["u"], o["dt"], None, 0, True)
    b = o["raised"]
    scale = np.abs(b).reshape(5, -1).max(axis=1)
    scale[1:4] = scale[1:4].max()
    rel = np.abs(a - b).reshape(5, -1).max(axis=1) / scale
    print("fast vs oracle after %d steps: rel Linf per variable %s" % (STEPS, rel))
    assert (rel <= 1e-12).all(), rel


@gpu
@pytest.mark.parametrize("rows", [0, 8])
def test_strict_build_equals_the_oracle(gpu_lib, oracle, rows):
    o = _oracle_runs(oracle)
    a = _run(o["u"], o["dt"], None, rows, False)
    diff = np.abs(a - o["raised"]).max()
    print("strict rows %d vs oracle after %d steps: max abs diff %g" % (rows, STEPS, diff))
    assert np.array_equal(a, o["raised"])

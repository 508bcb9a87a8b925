"""The dense sweep computes a cell the same way wherever the cell falls in a tile.

The fast LLF kernels carry 1 / rho from one plane's ctoprim to the next iteration's trace and skip the density floor of
traced states in the flux (csrc/hydro_sweep.hip SWEEP_TRIM); a build with SWEEP_YDUTY=1 also shares the y fluxes out over
the waves of a workgroup (the flux through the face between rows 1 and 2 computed by the wave of row 0, the one between rows
BY-3 and BY-2 by the wave of row BY-1).  Every cell keeps its arithmetic either way, so on a periodic box a shift of the
input by (7, 3, 5) cells -- which moves every cell to another lane, another tile row and another plane parity -- must
shift the output bit for bit.  A flux taken from the wrong wave's slot, or a plane late, breaks exactly this.

Cases: the fast 12-row LLF kernels without gravity of every slope type (0, 1, 2, 7, 8: what SWEEP_YDUTY=1 switches), LLF
with gravity, HLLC, the 8-row kernel, and the strict build.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 128
SHIFT = (7, 3, 5)          # cells along x, y, z
DEVELOP = 30               # steps from the point explosion before the comparison starts
STEPS = 3


def _developed_blast(gpu_lib):
    """a 128^3 Sedov blast after DEVELOP steps of the strict LLF + minmod sweep: shock, rarefaction and floor all present"""
    import torch
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    u, dx = ic.sedov3d(N)
    lev = HydroLevel(N, N, N, dx, params=ramses_amd.make_params(courant_factor=0.8))
    lev.upload(u)
    for _ in range(DEVELOP):
        lev.step(lev.courant_fine()[0])
    torch.cuda.synchronize()
    out = lev.download().copy()
    dt = 0.5 * lev.courant_fine()[0]
    return out, dx, dt


_BLAST = {}


def _blast(gpu_lib):
    if not _BLAST:
        _BLAST["u"], _BLAST["dx"], _BLAST["dt"] = _developed_blast(gpu_lib)
    return _BLAST["u"], _BLAST["dx"], _BLAST["dt"]


def _gravity(dx):
    """a smooth periodic acceleration field [3, nz, ny, nx]"""
    z, y, x = np.meshgrid(*(np.arange(N) * (2 * np.pi / N),) * 3, indexing="ij")
    return np.stack([0.3 * np.sin(x) * np.cos(y), 0.2 * np.sin(y + z), -0.25 * np.cos(z) * np.sin(x)])


def _roll(a):
    return np.roll(a, (SHIFT[2], SHIFT[1], SHIFT[0]), axis=(-3, -2, -1))


def _run(u, dx, dt, riemann, slope, grav, rows, fast):
    import torch
    import ramses_amd
    from ramses_amd.hydro import HydroLevel, godunov_tune
    p = ramses_amd.make_params(courant_factor=0.8, fast_math=fast, riemann=riemann, slope_type=slope)
    lev = HydroLevel(N, N, N, dx, params=p, ng=0, poisson=grav is not None)
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


CASES = [
    # riemann, slope type, gravity, tile rows, fast
    ("llf", 1, False, 0, True),
    ("llf", 0, False, 0, True),
    ("llf", 2, False, 0, True),
    ("llf", 7, False, 0, True),
    ("llf", 8, False, 0, True),
    ("llf", 1, True, 0, True),
    ("hllc", 1, False, 0, True),
    ("hllc", 2, True, 0, True),
    ("llf", 1, False, 8, True),
    ("llf", 1, False, 0, False),
]


@pytest.mark.parametrize("riemann,slope,grav,rows,fast", CASES)
def test_shifted_input_gives_the_shifted_output_bit_for_bit(gpu_lib, riemann, slope, grav, rows, fast):
    u, dx, dt = _blast(gpu_lib)
    g = _gravity(dx) if grav else None
    a = _run(u, dx, dt, riemann, slope, g, rows, fast)
    b = _run(_roll(u), dx, dt, riemann, slope, None if g is None else _roll(g), rows, fast)
    assert np.isfinite(a).all()
    assert not np.array_equal(a, u)                     # the steps did something
    want = _roll(a)
    diff = np.abs(b - want).max()
    print("%s slope %d grav %s rows %d %s: max |shifted run - shifted result| = %g" % (
        riemann, slope, grav, rows, "fast" if fast else "strict", diff))
    assert np.array_equal(b, want), "the sweep depends on where a cell falls in its tile: max abs diff %g" % diff


def test_the_fast_sweep_stays_within_its_tolerance_of_the_strict_one(gpu_lib):
    """the trims keep the fast arithmetic: after STEPS steps of the developed blast fast and strict agree to 1e-12 of the
    variable's scale (the fast build's certificate, hydro_core.hpp "Arithmetic policy")"""
    u, dx, dt = _blast(gpu_lib)
    a = _run(u, dx, dt, "llf", 1, None, 0, True)
    b = _run(u, dx, dt, "llf", 1, None, 0, False)
    scale = np.abs(b).reshape(5, -1).max(axis=1)
    scale[1:4] = scale[1:4].max()
    rel = np.abs(a - b).reshape(5, -1).max(axis=1) / scale
    print("fast vs strict after %d steps: rel Linf per variable %s" % (STEPS, rel))
    assert (rel <= 1e-12).all(), rel

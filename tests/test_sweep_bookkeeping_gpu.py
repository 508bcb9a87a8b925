"""The marching loop's bookkeeping changes no bit: the store offset that is switched on once in the third trip of a chunk and
the ring addresses of a tracing row from one lane register and immediate offsets (csrc/hydro_sweep.hip sweep_march SO1, LB).
Both live in the fast LLF 12-row kernels of the brick only (BOOK), so the FAST cases below run the new code -- the default
parameters are LLF + minmod without gravity, the kernel bench.py measures; the strict cases run code that is the same with
and without it and pin the reference the fast cases are held against: the oracle, the chunking, the ghost planes, the boxes
of the shell.

What can go wrong there goes wrong at the ends of a z chunk and at the periodic wrap, so the boxes are small and the chunks
short: 70 x 9 x 7 cells (two tiles along x and y, the second nearly empty) and 64 x 12 x 3, marched in chunks of 1, 2, 3, 5
planes and the default -- chunks shorter than the three-plane pipeline, chunks that start at plane 0 and end at the last plane
(a wrap below and above), a last chunk shorter than the others.  The state is smooth with one hot cell at (0, 0, 0) and one in
the last plane, two steps per case.

  * strict build, ng = 0 against the CPU oracle, bit for bit;
  * the same with ng = 2 and ghost cells (the clamped, unwrapped plane path) against the periodic run, bit for bit;
  * fast build: every chunking gives the bits of the default chunking, a shift of the input by (7, 3, 5) cells shifts the
    output bit for bit, and fast stays within 1e-12 of strict (relative L-inf per variable, the scaling of
    tests/test_sweep_rebalance_gpu.py);
  * shell + interior == the whole sweep on a 128 x 24 x 10 brick with ng = 2 (six boxes with chunk lengths of their own).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DX = 1.0 / 64
STEPS = 2
SMALL = [(70, 9, 7), (64, 12, 3)]          # nx, ny, nz
WIDE = (128, 24, 10)
ZCHUNKS = [1, 2, 3, 5, 0]                  # 0: the default
SHIFT = (7, 3, 5)                          # cells along x, y, z


def _state(shape):
    """conserved variables [5, nz, ny, nx]: smooth and periodic, a hot cell at (0, 0, 0) and one in the last plane"""
    nx, ny, nz = shape
    z, y, x = np.meshgrid(np.arange(nz) * (2 * np.pi / nz), np.arange(ny) * (2 * np.pi / ny),
                          np.arange(nx) * (2 * np.pi / nx), indexing="ij")
    rho = 1.0 + 0.3 * np.sin(x) * np.cos(y) + 0.1 * np.sin(z + x)
    vx = 0.4 * np.sin(y + z)
    vy = -0.3 * np.cos(x) * np.sin(z)
    vz = 0.25 * np.sin(x + y)
    p = 1.0 + 0.2 * np.cos(x + y + z)
    p[0, 0, 0] *= 40.0
    p[nz - 1, ny // 2, nx - 3] *= 25.0
    e = p / 0.4 + 0.5 * rho * (vx * vx + vy * vy + vz * vz)
    return np.ascontiguousarray(np.stack([rho, rho * vx, rho * vy, rho * vz, e]))


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _dt(shape, oracle):
    """one time step for both steps of every run of a shape: half the oracle's Courant step of the initial state"""
    return _cached(("dt", shape), lambda: 0.5 * oracle.courant_uniform(oracle.make_params(), _state(shape), DX, 0.8))


def _run(u, shape, dt, fast, ng, zchunk, split=False):
    import torch
    import ramses_amd
    from ramses_amd.hydro import HydroLevel, godunov_tune
    nx, ny, nz = shape
    lev = HydroLevel(nx, ny, nz, DX, params=ramses_amd.make_params(courant_factor=0.8, fast_math=fast), ng=ng)
    lev.upload(u)
    lev.make_virtual_fine_dp()
    godunov_tune(zchunk=zchunk)
    try:
        for _ in range(STEPS):
            if split:
                lev.godunov_fine_shell(dt)
                lev.godunov_fine_interior(dt)
            else:
                lev.godunov_fine(dt)
            lev.set_uold()
            lev.make_virtual_fine_dp()
        torch.cuda.synchronize()
    finally:
        godunov_tune()
    return lev.download().copy()


def _oracle_step(oracle, po, u, dt):
    """One oracle step of a box with odd ny or nz.  The oracle sweeps oct by oct, as the reference does (oracle/hydro_oracle.c
    ora_godunov_uniform: nx / 2 x ny / 2 x nz / 2 octs), so it leaves the last row and the last plane of an odd box as they
    were -- but what it computes for the cells of whole octs is right, their stencils wrap through the whole box.  The box is
    periodic: shifted by one cell in y and / or z the last row / plane falls into a whole oct.  Up to four oracle sweeps of
    shifted copies, each taken for the cells it does compute, give every cell of the box from the oracle."""
    nvar, nz, ny, nx = u.shape
    assert nx % 2 == 0
    out, done = np.empty_like(u), np.zeros((nz, ny, nx), dtype=bool)
    for b in range(1 + nz % 2):
        for a in range(1 + ny % 2):
            r = oracle.godunov_uniform(po, np.ascontiguousarray(np.roll(u, (b, a), axis=(-3, -2))), DX, dt)
            ok = np.zeros((nz, ny, nx), dtype=bool)
            ok[:2 * (nz // 2), :2 * (ny // 2), :] = True
            r, ok = np.roll(r, (-b, -a), axis=(-3, -2)), np.roll(ok, (-b, -a), axis=(-3, -2)) & ~done
            out[:, ok] = r[:, ok]
            done |= ok
    assert done.all()
    return out


def _oracle_run(shape, oracle):
    def make():
        po, u = oracle.make_params(), _state(shape)
        for _ in range(STEPS):
            u = _oracle_step(oracle, po, u, _dt(shape, oracle))
        return u
    return _cached(("oracle", shape), make)


def _default_run(shape, fast, oracle):
    """the periodic run (ng = 0) with the default chunking"""
    return _cached(("default", shape, fast), lambda: _run(_state(shape), shape, _dt(shape, oracle), fast, 0, 0))


@pytest.mark.parametrize("zchunk", ZCHUNKS)
@pytest.mark.parametrize("shape", SMALL)
def test_strict_periodic_chunks_against_the_oracle(gpu_lib, oracle, shape, zchunk):
    want = _oracle_run(shape, oracle)
    got = _run(_state(shape), shape, _dt(shape, oracle), False, 0, zchunk)
    assert np.isfinite(got).all() and not np.array_equal(got, _state(shape))
    diff = np.abs(got - want).max()
    print("strict %s zchunk %d: max |sweep - oracle| = %g" % (shape, zchunk, diff))
    assert np.array_equal(got, want), "max abs diff %g" % diff


@pytest.mark.parametrize("zchunk", ZCHUNKS)
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("fast", [False, True])
def test_ghost_planes_give_the_periodic_run_bit_for_bit(gpu_lib, oracle, fast, shape, zchunk):
    want = _default_run(shape, fast, oracle)
    got = _run(_state(shape), shape, _dt(shape, oracle), fast, 2, zchunk)
    diff = np.abs(got - want).max()
    print("%s %s ng 2 zchunk %d: max |ghost run - periodic run| = %g" % ("fast" if fast else "strict", shape, zchunk, diff))
    assert np.array_equal(got, want), "max abs diff %g" % diff


@pytest.mark.parametrize("zchunk", ZCHUNKS[:-1])
@pytest.mark.parametrize("shape", [SMALL[0], WIDE])
def test_fast_chunks_give_the_bits_of_the_default_chunking(gpu_lib, oracle, shape, zchunk):
    want = _default_run(shape, True, oracle)
    got = _run(_state(shape), shape, _dt(shape, oracle), True, 0, zchunk)
    assert np.isfinite(got).all() and not np.array_equal(got, _state(shape))
    diff = np.abs(got - want).max()
    print("fast %s zchunk %d: max |chunked - default| = %g" % (shape, zchunk, diff))
    assert np.array_equal(got, want), "max abs diff %g" % diff


def _roll(a):
    return np.roll(a, (SHIFT[2], SHIFT[1], SHIFT[0]), axis=(-3, -2, -1))


@pytest.mark.parametrize("shape", [SMALL[0], WIDE])
def test_fast_shifted_input_gives_the_shifted_output(gpu_lib, oracle, shape):
    want = _roll(_default_run(shape, True, oracle))
    got = _run(_roll(_state(shape)), shape, _dt(shape, oracle), True, 0, 0)
    diff = np.abs(got - want).max()
    print("fast %s: max |shifted run - shifted result| = %g" % (shape, diff))
    assert np.array_equal(got, want), "max abs diff %g" % diff


@pytest.mark.parametrize("shape", [SMALL[0], WIDE])
def test_fast_stays_within_its_tolerance_of_strict(gpu_lib, oracle, shape):
    a, b = _default_run(shape, True, oracle), _default_run(shape, False, oracle)
    scale = np.abs(b).reshape(5, -1).max(axis=1)
    scale[1:4] = scale[1:4].max()
    rel = np.abs(a - b).reshape(5, -1).max(axis=1) / scale
    print("fast vs strict %s after %d steps: rel Linf per variable %s" % (shape, STEPS, rel))
    assert (rel <= 1e-12).all(), rel


@pytest.mark.parametrize("fast", [False, True])
def test_shell_plus_interior_is_the_whole_sweep(gpu_lib, oracle, fast):
    u, dt = _state(WIDE), _dt(WIDE, oracle)
    whole = _run(u, WIDE, dt, fast, 2, 0)
    parts = _run(u, WIDE, dt, fast, 2, 0, split=True)
    assert np.isfinite(whole).all() and not np.array_equal(whole, u)
    diff = np.abs(parts - whole).max()
    print("%s shell + interior: max |parts - whole| = %g" % ("fast" if fast else "strict", diff))
    assert np.array_equal(parts, whole), "max abs diff %g" % diff

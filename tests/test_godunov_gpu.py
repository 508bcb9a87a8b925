"""GPU parity tests of the Godunov sweep: HIP path (through the C ABI) vs the
CPU oracle (itself pinned bit-exact against the reference's unsplit)."""
import numpy as np
import pytest

from helpers import _set_uold_scalar_fix, random_brick, rel_linf

pytestmark = pytest.mark.gpu


def _sweep_gpu(u, dx, dt, ng=0, **kw):
    import ramses_amd
    from ramses_amd.hydro import HydroLevel
    nvar, nz, ny, nx = u.shape
    lev = HydroLevel(nx, ny, nz, dx, params=ramses_amd.make_params(**kw), ng=ng)
    lev.upload(u)
    lev.make_virtual_fine_dp()
    lev.godunov_fine(dt)
    import torch
    torch.cuda.synchronize()
    return lev.download(lev.unew)


def _oracle_params(oracle, **kw):
    kw = dict(kw)
    kw.pop("fast_math", None)
    kw.pop("courant_factor", None)
    return oracle.make_params(**kw)


@pytest.mark.parametrize("tile_rows,zchunk", [(0, 0), (8, 0), (12, 0), (12, 4), (8, 6)])
@pytest.mark.parametrize("shape", [(16, 12, 20), (64, 8, 8), (70, 10, 6), (8, 8, 8), (130, 22, 14)])
def test_llf_minmod_bit_exact(gpu_lib, oracle, shape, tile_rows, zchunk):
    from ramses_amd.hydro import godunov_tune
    godunov_tune(tile_rows, zchunk)
    nx, ny, nz = shape
    u = random_brick(nx, ny, nz, seed=nx * 1000 + ny)
    dx = 1.0 / 64
    dt = 0.05 * dx
    ref = oracle.godunov_uniform(_oracle_params(oracle), u, dx, dt)
    out = _sweep_gpu(u, dx, dt)
    godunov_tune(0, 0)
    assert np.isfinite(out).all()
    assert rel_linf(out, ref) <= 1e-13
    assert np.array_equal(out, ref), "strict mode must be bit-identical (max diff %g)" % np.abs(out - ref).max()


@pytest.mark.parametrize("scheme", ["muscl", "plmde"])
@pytest.mark.parametrize("riemann", ["llf", "hllc", "hll", "acoustic", "exact"])
@pytest.mark.parametrize("slope_type", [1, 2, 3, 7, 8])
def test_solver_matrix(gpu_lib, oracle, riemann, slope_type, scheme):
    nx, ny, nz = 24, 12, 10
    u = random_brick(nx, ny, nz, seed=7 + slope_type)
    dx = 1.0 / 32
    dt = 0.04 * dx
    kw = dict(riemann=riemann, slope_type=slope_type, scheme=scheme)
    ref = oracle.godunov_uniform(_oracle_params(oracle, **kw), u, dx, dt)
    out = _sweep_gpu(u, dx, dt, **kw)
    err = rel_linf(out, ref)
    assert err <= 1e-12, "rel Linf %g" % err
    if riemann != "exact":  # 'exact' calls pow(): device libm differs in the last ulp
        assert np.array_equal(out, ref), "max diff %g" % np.abs(out - ref).max()


def test_non_pow2_dx(gpu_lib, oracle):
    u = random_brick(20, 12, 10, seed=3)
    dx = 0.3 / 20
    dt = 0.05 * dx
    ref = oracle.godunov_uniform(_oracle_params(oracle), u, dx, dt)
    out = _sweep_gpu(u, dx, dt)
    assert np.array_equal(out, ref), "max diff %g" % np.abs(out - ref).max()


def test_ghost_brick_equals_wrap(gpu_lib, oracle):
    u = random_brick(30, 14, 11, seed=11)
    dx = 1.0 / 32
    dt = 0.05 * dx
    a = _sweep_gpu(u, dx, dt, ng=0)
    b = _sweep_gpu(u, dx, dt, ng=2)
    assert np.array_equal(a, b)


def test_fast_mode_within_tolerance(gpu_lib, oracle):
    u = random_brick(40, 16, 12, seed=21)
    dx = 1.0 / 64
    dt = 0.05 * dx
    ref = oracle.godunov_uniform(_oracle_params(oracle), u, dx, dt)
    out = _sweep_gpu(u, dx, dt, fast_math=True)
    err = rel_linf(out, ref)
    assert err <= 1e-12, "rel Linf %g" % err


def test_courant_matches_oracle(gpu_lib, oracle):
    import ramses_amd
    from ramses_amd.hydro import HydroLevel
    u = random_brick(33, 10, 7, seed=5)
    dx = 1.0 / 32
    for ng in (0, 2):
        lev = HydroLevel(33, 10, 7, dx, params=ramses_amd.make_params(courant_factor=0.8), ng=ng)
        lev.upload(u)
        dt, mass, etot, eint = lev.courant_fine()
        ref = oracle.courant_uniform(oracle.make_params(), u, dx, 0.8)
        assert dt == ref
        vol = dx ** 3
        assert abs(mass - u[0].sum() * vol) <= 1e-12 * abs(mass)
        assert abs(etot - u[4].sum() * vol) <= 1e-12 * abs(etot)


def test_sedov_steps_match_oracle(gpu_lib, oracle):
    """namelist/sedov3d.nml at 32^3: 4 fine steps (courant -> sweep -> set_uold)
    against the oracle; also pins the known-answer dt sequence of the
    reference run (3.076E-05 6.877E-05 7.752E-05 9.857E-05)."""
    import ramses_amd
    from ramses_amd import ic
    from ramses_amd.hydro import HydroLevel
    n = 32
    u, dx = ic.sedov3d(n)
    p = ramses_amd.make_params(courant_factor=0.8)
    po = oracle.make_params()
    lev = HydroLevel(n, n, n, dx, params=p)
    lev.upload(u)
    dts = []
    uo = u.copy()
    for _ in range(4):
        dt = lev.courant_fine()[0]
        dto = oracle.courant_uniform(po, uo, dx, 0.8)
        assert dt == dto
        dts.append(dt)
        lev.step(dt)
        uo = oracle.godunov_uniform(po, uo, dx, dto)
        out = lev.download()
        assert np.array_equal(out, uo), "max diff %g" % np.abs(out - uo).max()
    known = [3.076e-05, 6.877e-05, 7.752e-05, 9.857e-05]
    for a, b in zip(dts, known):
        assert abs(a - b) <= 5e-4 * b, (dts, known)


@pytest.mark.parametrize("nvar", [6, 7])
@pytest.mark.parametrize("riemann,slope_type", [("llf", 1), ("hllc", 2), ("hll", 3), ("acoustic", 8), ("exact", 7)])
def test_passive_scalars(gpu_lib, oracle, nvar, riemann, slope_type):
    nx, ny, nz = 20, 12, 10
    u = random_brick(nx, ny, nz, seed=nvar * 10 + slope_type, nvar=nvar)
    dx, dt = 1.0 / 32, 0.04 / 32
    for smallr in (1e-10, 0.6):      # 0.6 puts part of the box under the density floor
        kw = dict(riemann=riemann, slope_type=slope_type, nvar=nvar, smallr=smallr)
        ref = oracle.godunov_uniform(_oracle_params(oracle, **kw), u, dx, dt)
        ref = _set_uold_scalar_fix(u, ref, smallr)
        out = _sweep_gpu(u, dx, dt, **kw)
        if riemann == "exact":
            assert rel_linf(out, ref) <= 1e-12
        else:
            assert np.array_equal(out, ref), "max diff %g" % np.abs(out - ref).max()


def test_gravity_predictor_path(gpu_lib, oracle):
    """poisson=.true.: ctoprim's gravity predictor (gloc) and cmpdt's gravity term."""
    import torch
    import ramses_amd
    from ramses_amd.hydro import HydroLevel
    nx, ny, nz = 26, 12, 10
    u = random_brick(nx, ny, nz, seed=77)
    rng = np.random.default_rng(5)
    g = rng.normal(0, 2.0, (3, nz, ny, nx))
    dx, dt = 1.0 / 32, 0.03 / 32
    for ng in (0, 2):
        lev = HydroLevel(nx, ny, nz, dx, params=ramses_amd.make_params(riemann="hllc", slope_type=2, courant_factor=0.7),
                         ng=ng, poisson=True)
        lev.upload(u)
        lev.interior(lev.f).copy_(torch.as_tensor(g).cuda())
        lev.make_virtual_fine_dp()
        dtc = lev.courant_fine()[0]
        lev.godunov_fine(dt)
        torch.cuda.synchronize()
        po = oracle.make_params(riemann="hllc", slope_type=2)
        assert dtc == oracle.courant_uniform(po, u, dx, 0.7, grav=g)
        ref = oracle.godunov_uniform(po, u, dx, dt, grav=g)
        assert np.array_equal(lev.download(lev.unew), ref)


@pytest.mark.parametrize("fast", [False, True])
def test_full_size_properties_512(gpu_lib, fast):
    """BASELINE's metric configuration (512^3 per GPU) through size-independent
    properties, no oracle needed:
      * translation: sweeping a periodically shifted state == shifting the swept
        state, bit for bit (every tile edge, z-chunk seam and wrap is crossed by
        different data);
      * conservation: the periodic sums of the conserved variables do not change
        beyond rounding."""
    import torch
    import ramses_amd
    from ramses_amd.hydro import HydroLevel
    n = 512
    p = ramses_amd.make_params(courant_factor=0.8, fast_math=fast)
    lev = HydroLevel(n, n, n, 0.5 / n, params=p, ng=0)
    g = torch.Generator(device="cuda").manual_seed(7)
    u = lev.uold
    u[0] = 1.0 + torch.rand((n, n, n), generator=g, device="cuda", dtype=torch.float64)
    for d in (1, 2, 3):
        u[d] = u[0] * (torch.rand((n, n, n), generator=g, device="cuda", dtype=torch.float64) - 0.5)
    u[4] = 1.0 + torch.rand((n, n, n), generator=g, device="cuda", dtype=torch.float64) + \
        0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0]
    u[4, 100:110, 200:230, 17:40] *= 50.0          # a strong blast somewhere
    dt = 0.5 * lev.courant_fine()[0]
    lev.godunov_fine(dt)
    ref = lev.unew.clone()
    before = u.sum(dim=(1, 2, 3))
    after = ref.sum(dim=(1, 2, 3))
    assert torch.all((after - before).abs() <= 1e-9 * before.abs().clamp(min=1.0))
    shift = (37, 5, 201)                          # not a multiple of any tile size
    lev.uold.copy_(torch.roll(u.clone(), shifts=shift, dims=(1, 2, 3)))
    lev.godunov_fine(dt)
    assert torch.equal(lev.unew, torch.roll(ref, shifts=shift, dims=(1, 2, 3)))
    del ref
    torch.cuda.empty_cache()

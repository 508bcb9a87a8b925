"""Passive scalars beyond NVAR=7 on the device (a hydro pass, then scalar passes in groups: csrc/hydro_sweep.hip
godunov_scalar_kernel).  The strict build is held bit for bit to the CPU oracle (which the reference's own goldens pin
up to NVAR=7 and which sweeps every scalar on its own, tests/test_scalars_capi.py); with NENER, where the oracle has no
branch, each scalar is held to the NVAR=7 kernels that tests/test_nener_gpu.py pins to the reference."""
import ctypes as C

import numpy as np
import pytest

from helpers import random_brick, rel_linf

pytestmark = pytest.mark.gpu


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


def _fix(uold, unew, smallr, first=5):
    """set_uold's passive-scalar floor fix (hydro/godunov_fine.f90:176-190), numpy, test-side only"""
    out = unew.copy()
    a = (uold[0] < smallr) & (unew[0] > uold[0])
    b = ~a & (unew[0] < smallr) & (uold[0] > unew[0])
    for n in range(first, unew.shape[0]):
        out[n][a] = (uold[n] * np.maximum(unew[0], smallr) / smallr)[a]
        out[n][b] = (uold[n] * smallr / np.maximum(uold[0], smallr))[b]
    return out


def _level(u, dx, ng=0, poisson=False, **kw):
    import ramses_amd
    from ramses_amd.hydro import HydroLevel
    nvar, nz, ny, nx = u.shape
    lev = HydroLevel(nx, ny, nz, dx, params=ramses_amd.make_params(nvar=nvar, **kw), ng=ng, poisson=poisson)
    lev.upload(u)
    return lev


def _sweep(u, dx, dt, ng=0, **kw):
    import torch
    lev = _level(u, dx, ng=ng, **kw)
    lev.make_virtual_fine_dp()
    lev.godunov_fine(dt)
    torch.cuda.synchronize()
    return lev.download(lev.unew)


def _scalars(u, seed):
    """every scalar its own, non-symmetric profile: rho times a different smooth field plus noise"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = u.shape[1:]
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    for n in range(5, u.shape[0]):
        f = 0.5 + 0.4 * np.sin(2 * np.pi * (x * (n - 3) / nx + y * (n % 3 + 1) / ny + z * 0.37 * n / nz))
        u[n] = u[0] * (f + 0.1 * rng.uniform(0, 1, f.shape))
    return u


CASES = [  # (nvar, riemann, slope_type)
    (8, "llf", 1), (8, "exact", 7), (11, "hllc", 2), (11, "hll", 3), (11, "acoustic", 8),
    (16, "llf", 0), (16, "hllc", 8), (16, "exact", 3), (16, "hll", 1), (16, "acoustic", 2),
]


@pytest.mark.parametrize("nvar,riemann,slope_type", CASES)
def test_staged_brick_matches_the_oracle_bit_for_bit(gpu_lib, oracle, nvar, riemann, slope_type):
    nx, ny, nz = 70, 14, 10             # not multiples of the 60 x 4 / 60 x 8 tiles (the oracle sweeps octs: even sizes)
    u = _scalars(random_brick(nx, ny, nz, seed=nvar * 7 + slope_type, nvar=nvar), nvar)
    dx, dt = 1.0 / 64, 0.03 / 64
    for smallr, ng in ((1e-10, 0), (0.6, 2)):      # 0.6 puts part of the box under the density floor
        kw = dict(riemann=riemann, slope_type=slope_type, smallr=smallr)
        ref = _fix(u, oracle.godunov_uniform(oracle.make_params(nvar=nvar, **kw), u, dx, dt), smallr)
        out = _sweep(u, dx, dt, ng=ng, **kw)
        if riemann == "exact":               # pow(): device libm differs in the last ulp (as at NVAR <= 7)
            assert rel_linf(out, ref) <= 1e-12
        else:
            assert _bits_equal(out, ref), "smallr=%g ng=%d: max diff %g" % (smallr, ng, np.abs(out - ref).max())


def test_gravity_predictor_at_nvar_12(gpu_lib, oracle):
    import torch
    nx, ny, nz = 26, 12, 10
    u = _scalars(random_brick(nx, ny, nz, seed=77, nvar=12), 3)
    g = np.random.default_rng(5).normal(0, 2.0, (3, nz, ny, nx))
    dx, dt = 1.0 / 32, 0.03 / 32
    for ng in (0, 2):
        lev = _level(u, dx, ng=ng, poisson=True, riemann="hllc", slope_type=2, courant_factor=0.7)
        lev.interior(lev.f).copy_(torch.as_tensor(g).cuda())
        lev.make_virtual_fine_dp()
        dtc = lev.courant_fine()[0]
        lev.godunov_fine(dt)
        torch.cuda.synchronize()
        po = oracle.make_params(nvar=12, riemann="hllc", slope_type=2)
        assert dtc == oracle.courant_uniform(po, u, dx, 0.7, grav=g)
        assert _bits_equal(lev.download(lev.unew), _fix(u, oracle.godunov_uniform(po, u, dx, dt, grav=g), 1e-10))


def test_courant_dt_does_not_see_the_scalars(gpu_lib):
    u = _scalars(random_brick(20, 12, 10, seed=9, nvar=16), 4)
    a = _level(u, 1.0 / 32, courant_factor=0.8).courant_fine()[0]
    b = _level(np.ascontiguousarray(u[:5]), 1.0 / 32, courant_factor=0.8).courant_fine()[0]
    assert a == b


@pytest.mark.parametrize("fast", [False, True])
def test_hydro_rows_and_scalar_permutation(gpu_lib, fast):
    """the hydro rows of NVAR=16 are those of NVAR=5; permuting the scalar columns permutes the output exactly
    (a group offset that is off by one does not survive this)"""
    u = _scalars(random_brick(70, 14, 9, seed=21, nvar=16), 21)
    dx, dt = 1.0 / 64, 0.03 / 64
    for riemann, st in (("hllc", 1), ("llf", 3)):
        kw = dict(riemann=riemann, slope_type=st, smallr=0.6, fast_math=fast)
        big = _sweep(u, dx, dt, **kw)
        assert _bits_equal(big[:5], _sweep(np.ascontiguousarray(u[:5]), dx, dt, **kw))
        perm = np.r_[0:5, 5 + np.random.default_rng(3).permutation(11)]
        assert _bits_equal(_sweep(np.ascontiguousarray(u[perm]), dx, dt, **kw), big[perm])


@pytest.mark.parametrize("nener,nvar", [(1, 9), (1, 8), (2, 8), (2, 12)])
def test_nener_scalars_equal_the_pinned_nvar7_kernels(gpu_lib, nener, nvar):
    """NENER with scalars beyond NVAR=7: the hydro and non-thermal rows are the NVAR=5+NENER sweep's, each scalar the
    row that the NVAR=7 (NENER=1: one scalar; NENER=2: none) kernels give it, sweep and set_uold with pdV, 3 steps"""
    import torch
    nh = 5 + nener
    u = _scalars(random_brick(24, 12, 10, seed=nvar + 10 * nener, nvar=nvar), nvar)
    for e in range(nener):
        u[5 + e] = 0.3 * u[4] * (1 + 0.2 * e)
    dx = 1.0 / 32
    for riemann, st in (("llf", 1), ("hllc", 8), ("hll", 3)):
        kw = dict(riemann=riemann, slope_type=st, nener=nener, courant_factor=0.8)
        big = _level(u, dx, **kw)
        hyd = _level(np.ascontiguousarray(u[:nh]), dx, **kw)
        one = [_level(np.ascontiguousarray(u[list(range(nh)) + [k]]), dx, **kw) for k in range(nh, nvar)] if nener == 1 else []
        for step in range(3):
            dt = big.courant_fine()[0]
            assert dt == hyd.courant_fine()[0]
            for lv in [big, hyd] + one:
                lv.godunov_fine(dt)
                lv.set_uold()
            torch.cuda.synchronize()
            got = big.download()
            assert _bits_equal(got[:nh], hyd.download()), (riemann, step)
            for k, lv in zip(range(nh, nvar), one):
                assert _bits_equal(got[k], lv.download()[nh]), (riemann, step, k)


@pytest.mark.parametrize("riemann", ["llf", "hll", "hllc"])
def test_fast_stays_within_1e12_of_strict_over_20_steps(gpu_lib, riemann):
    u = _scalars(random_brick(32, 32, 32, seed=33, nvar=12, contrast=False), 12)
    dx = 1.0 / 32
    out = []
    for fast in (False, True):
        lev = _level(u, dx, riemann=riemann, slope_type=1, courant_factor=0.8, fast_math=fast)
        for _ in range(20):
            lev.step(0.2 * dx)
        out.append(lev.download())
    assert rel_linf(out[1], out[0]) <= 1e-12


@pytest.mark.parametrize("shape", [(48, 48, 48), (130, 12, 16)])
def test_shell_plus_interior_equals_the_full_sweep(gpu_lib, shape):
    """_interior first, then _shell: each stands alone (the scalar passes read back only densities of their own call);
    (130, 12, 16): the 12-row hydro pass cannot split the brick while 8-row tiles could"""
    import torch
    from ramses_amd import _capi
    L = _capi.lib()
    nx, ny, nz = shape
    u = _scalars(random_brick(nx, ny, nz, seed=4, nvar=13), 13)
    dx, dt = 1.0 / 64, 0.02 / 64
    for fast in (False, True):
        p = _capi.make_params(nvar=13, riemann="hllc", slope_type=2, smallr=0.6, fast_math=fast)
        b = _capi.dense_brick(nx, ny, nz, 0)
        d_u = torch.as_tensor(u).cuda().contiguous()
        full = torch.zeros_like(d_u)
        split = torch.zeros_like(d_u)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        _capi.check(L.ramses_amd_godunov_brick(C.byref(p), C.byref(b), vp(d_u), None, vp(full), dx, dt, None))
        _capi.check(L.ramses_amd_godunov_brick_interior(C.byref(p), C.byref(b), vp(d_u), None, vp(split), dx, dt, None))
        _capi.check(L.ramses_amd_godunov_brick_shell(C.byref(p), C.byref(b), vp(d_u), None, vp(split), dx, dt, None))
        torch.cuda.synchronize()
        assert _bits_equal(full.cpu().numpy(), split.cpu().numpy())


def test_brick_decomposition_on_one_and_two_ranks_equals_the_single_brick(gpu_lib):
    import torch
    import ramses_amd
    from ramses_amd.parallel import BrickDecomposition, rank_coords
    from ramses_amd.transport import LocalWorld
    n, nvar = 16, 10
    u = _scalars(random_brick(n, n, n, seed=12, nvar=nvar, contrast=False), 12)
    p = ramses_amd.make_params(nvar=nvar, riemann="hllc", slope_type=1, courant_factor=0.8)
    ref = _level(u, 1.0 / n, riemann="hllc", slope_type=1, courant_factor=0.8)
    dts = []
    for _ in range(3):
        dt = ref.courant_fine()[0]
        dts.append(dt)
        ref.step(dt)
    want = ref.download()

    dec = BrickDecomposition((1, 1, 1), 0, n, boxlen=1.0)
    lev = dec.make_level(p)
    lev.upload(u)
    dec.make_virtual_fine_dp(lev)
    for dt in dts:
        dec.step_overlapped(lev, dt)
    assert _bits_equal(lev.download(), want)

    def body(tr):
        d = BrickDecomposition((2, 1, 1), tr.rank, (8, n, n), boxlen=1.0, transport=tr)
        lv = d.make_level(p)
        x0 = 8 * rank_coords(tr.rank, (2, 1, 1))[0]
        lv.upload(np.ascontiguousarray(u[..., x0:x0 + 8]))
        d.make_virtual_fine_dp(lv)
        for dt in dts:
            d.step_overlapped(lv, dt)
        torch.cuda.synchronize()
        return _bits_equal(lv.download(), want[..., x0:x0 + 8])

    assert LocalWorld(2).run(body) == [True, True]

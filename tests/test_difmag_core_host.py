"""The artificial diffusion of the product (ramses_amd/csrc/difmag_core.hpp: cmpdivu_corner, consup_div1_x / _y / _z, consup_term,
the one text the marching kernel, the surface pass and this test share) compiled for the HOST (tests/native/
difmag_host_check.cpp) against the oracle's unsplit (oracle/hydro_oracle.c ora_cmpdivu / ora_consup, pinned on the reference's
dumps): unsplit is called on random 6^3 patches WITH gravity, once with difmag = d and once with difmag = 0; the host program
gets the same uin, gravin, dx, dt and the fluxes without difmag, takes the velocities as ctoprim leaves them -- with the half
kick of the gravity -- and adds its term.  The result must equal the fluxes with difmag bit for bit on every face and variable
(flux = flux + dt*div1*du is the reference's own last operation).  No GPU needed; the GPU leg is tests/test_difmag_tiles_gpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "difmag_host_check.cpp")
NPATCH = 32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("difmag") / "libdifmag_host_check.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", out, SRC])
    lib = C.CDLL(out)
    dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
    lib.difmag_host_add.argtypes = [C.c_int, C.c_int, dp, dp, C.c_double, C.c_double, C.c_double, C.c_double, dp]
    lib.difmag_host_add.restype = None
    return lib


def _patches(nvar, seed):
    """random 6^3 patches (the random state of the tile tests) and a gravity field of unit size"""
    rng = np.random.default_rng(seed)
    shape = (6, 6, 6, NPATCH)
    u = np.zeros((nvar,) + shape)
    u[0] = 1.0 + rng.random(shape)
    for d in (1, 2, 3):
        u[d] = u[0] * (rng.random(shape) - 0.5)
    u[4] = 1.0 + rng.random(shape) + 0.5 * (u[1] ** 2 + u[2] ** 2 + u[3] ** 2) / u[0]
    for v in range(5, nvar):
        u[v] = u[0] * rng.random(shape)
    g = rng.normal(size=(3,) + shape)
    return np.ascontiguousarray(u), np.ascontiguousarray(g)


def _own_faces(flux):
    """the faces consup touches: those of the oct's own 2^3 cells, 12 per direction -> [3][nvar][12 x NPATCH]"""
    return np.stack([flux[0][:, :2, :2, :, :].reshape(flux.shape[1], -1), flux[1][:, :2, :, :2, :].reshape(flux.shape[1], -1),
                     flux[2][:, :, :2, :2, :].reshape(flux.shape[1], -1)])


@pytest.mark.parametrize("nvar", [5, 7])
@pytest.mark.parametrize("riemann,slope,difmag", [("llf", 1, 0.1), ("hllc", 2, 0.05)])
def test_header_adds_the_oracles_diffusive_term(host, nvar, riemann, slope, difmag):
    uin, grav = _patches(nvar, 3)
    dx = 1.0 / 64
    dt = 0.02 * dx
    kw = dict(nvar=nvar, riemann=riemann, slope_type=slope)
    f_d, _ = pyoracle.unsplit(pyoracle.make_params(difmag=difmag, **kw), uin, grav, dx, dt)
    f_0, _ = pyoracle.unsplit(pyoracle.make_params(**kw), uin, grav, dx, dt)
    # not vacuous, from the oracle pair alone: the term changes more than 0.4 of the 1152 faces
    # (measured with seed 3, llf, minmod, difmag = 0.1: 609 of 1152 = 0.53, NVAR 5 and 7 alike)
    own_d, own_0 = _own_faces(f_d), _own_faces(f_0)
    assert own_d.shape == (3, nvar, 12 * NPATCH)
    changed = (own_d != own_0).any(axis=1)
    print("faces the term changes: %d of %d" % (changed.sum(), changed.size))
    assert changed.size == 1152 and changed.mean() > 0.4
    got = f_0.copy()
    host.difmag_host_add(nvar, NPATCH, uin, grav, dx, dt, 1e-10, difmag, got)
    print("flux entries that differ:", int((got != f_d).sum()), "max abs difference", np.abs(got - f_d).max())
    assert np.array_equal(got, f_d)
    assert np.array_equal(got.view(np.int64), f_d.view(np.int64))


def test_velocities_without_the_half_kick_miss_every_face_the_term_touches(host):
    """the same call with a gravity field of zeros handed to the host program (velocities without the kick) against the oracle WITH
    gravity: with a field of unit size every face the term touches comes out different, so the comparison above pins the kick"""
    nvar, difmag = 5, 0.1
    uin, grav = _patches(nvar, 3)
    dx = 1.0 / 64
    dt = 0.02 * dx
    kw = dict(nvar=nvar, riemann="llf", slope_type=1)
    f_d, _ = pyoracle.unsplit(pyoracle.make_params(difmag=difmag, **kw), uin, grav, dx, dt)
    f_0, _ = pyoracle.unsplit(pyoracle.make_params(**kw), uin, grav, dx, dt)
    got = f_0.copy()
    host.difmag_host_add(nvar, NPATCH, uin, np.zeros_like(grav), dx, dt, 1e-10, difmag, got)
    touched = (_own_faces(f_d) != _own_faces(f_0)).any(axis=1)
    missed = (_own_faces(got) != _own_faces(f_d)).any(axis=1)
    print("faces touched %d, of them missed without the kick %d" % (touched.sum(), (missed & touched).sum()))
    assert touched.sum() > 400 and (missed & touched).sum() == touched.sum()

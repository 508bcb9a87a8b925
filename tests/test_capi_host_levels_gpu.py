"""The entry points of csrc/capi_host.hip on a fully refined periodic level of the reference's own arrays, called directly
through ctypes: the staged Poisson pair (ramses_amd_multigrid_fine_f90, ramses_amd_force_fine_f90), the resident gravity
cycle, the resident Poisson chain and what each of them refuses.  Otherwise these run only inside the patched Fortran
program (test_dropin_gpu.py), which is slow and says little when it fails.

Every case works on a scrambled oct layout (helpers._octree_layout: octs in random slots and random list order, ngridmax
well above ngrid, ncoarse = 1, random garbage in every cell that is not the level's) at levels 3 and 4 (8^3, 16^3): the
smallest at which an oct permutation, the eight octants and a wrong pitch are all distinguishable.  Expected values come
from the oracle (oracle/pyoracle.py)."""
import ctypes as C
import math

import numpy as np
import pytest

from helpers import _octree_layout, random_brick

pytestmark = pytest.mark.gpu

NGRIDMAX = {3: 157, 4: 700}        # ngrid = 64, 512
EPS = 1e-6
EINVAL, EUNSUPPORTED = -1, -2


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


class Level:
    """bricks[name] = array [nvar, n, n, n] -> cell vectors [nvar, ncell] that share ONE scrambled oct layout"""

    def __init__(self, level, seed, **bricks):
        self.level, self.n = level, 2 ** level
        self.ngridmax, self.ncoarse = NGRIDMAX[level], 1
        self.ncell = self.ncoarse + 8 * self.ngridmax
        rng = np.random.default_rng(seed)
        names = list(bricks)
        stack = np.concatenate([bricks[k] for k in names])
        vec, self.igrid, self.xg, (ox, oy, oz) = _octree_layout(stack, level, rng, self.ngridmax, self.ncoarse)
        self.ngrid = len(self.igrid)
        assert self.ngridmax > 1.3 * self.ngrid
        self.vec, at = {}, 0
        for k in names:
            nv = bricks[k].shape[0]
            self.vec[k] = np.ascontiguousarray(vec[at:at + nv])
            at += nv
        # cell index [8, ngrid] of the level's cells and where each sits in the brick
        ind = np.arange(8)[:, None]
        self.icell = self.ncoarse + ind * self.ngridmax + (self.igrid.astype(np.int64) - 1)[None, :]
        self.bz = 2 * oz[None, :] + ((ind >> 2) & 1)
        self.by = 2 * oy[None, :] + ((ind >> 1) & 1)
        self.bx = 2 * ox[None, :] + (ind & 1)
        self.on = np.zeros(self.ncell, bool)
        self.on[self.icell] = True
        assert self.on.sum() == self.n ** 3

    def head(self, nx_loc=1, ngrid=None, xg=None):
        """(ilevel, ngrid, igrid, xg, ngridmax, ncoarse, nx_loc): how every entry point names the level"""
        return (self.level, self.ngrid if ngrid is None else ngrid, vp(self.igrid), vp(self.xg if xg is None else xg),
                self.ngridmax, self.ncoarse, nx_loc)

    def to_brick(self, vec):
        b = np.zeros((vec.shape[0], self.n, self.n, self.n))
        b[:, self.bz, self.by, self.bx] = vec[:, self.icell]
        return b

    def on_level(self, vec, brick):
        """the level's cells of the cell vectors equal the brick bit for bit"""
        return np.array_equal(vec[:, self.icell], brick[:, self.bz, self.by, self.bx])

    def off_level_kept(self, vec, before):
        return np.array_equal(vec[:, ~self.on], before[:, ~self.on])


def _rho_brick(n, seed):
    rng = np.random.default_rng(seed)
    rho = 1.0 + 0.5 * rng.random((n, n, n))
    rho[n // 4:n // 2, 1:n // 2 + 1, n // 2:n // 2 + 3] += 20.0          # a dense block
    return rho


def _err(lib):
    return lib.ramses_amd_last_error().decode()


def _refused(lib, rc, want_rc, text):
    assert rc == want_rc, (rc, _err(lib))
    assert text in _err(lib), _err(lib)


def _staged_multigrid(lib, L, rho, phi, rho_tot, head=None):
    safe, it, err = C.c_int(0), C.c_int(-1), C.c_double(-1.0)
    rc = lib.ramses_amd_multigrid_fine_f90(*(head or L.head()), vp(rho), vp(phi), rho_tot, 2 * 6.2831853, EPS,
                                           C.byref(safe), C.byref(it), C.byref(err))
    return rc, safe.value, it.value, err.value


@pytest.mark.parametrize("level", [3, 4])
def test_staged_multigrid_fine(gpu_lib, oracle, level):
    """phi on the level's cells is the oracle's bit for bit, iterations and safe_mode equal, every other cell of phi
    untouched.  err: both sides take the square root of a ratio of sums of N squares in different orders, relative
    difference <= 2 N 2^-53 (9.1e-13 at 16^3: 1e-12 there, in proportion at 8^3)."""
    n = 2 ** level
    rho_b = _rho_brick(n, 11 + level)
    L = Level(level, 100 + level, rho=rho_b[None], phi=np.zeros((1, n, n, n)))
    rho, phi = L.vec["rho"], L.vec["phi"]
    phi[0, L.on] = np.random.default_rng(1).normal(size=L.on.sum())        # the first guess is NOT what the host array holds
    before = phi.copy()
    rho_tot = float(rho_b.mean())
    want = oracle.mg_solve_uniform(rho_b, rho_tot, boxlen=1.0, epsilon=EPS)
    assert gpu_lib.ramses_amd_resident_invalidate() == 0
    rc, safe, it, err = _staged_multigrid(gpu_lib, L, rho[0], phi[0], rho_tot)
    assert rc == 0, _err(gpu_lib)
    print("level %d: iters %d / %d, err %.17g / %.17g, safe %d / %d" % (level, it, want["iters"], err, want["err"], safe, want["safe_mode"]))
    assert it == want["iters"] and it >= 2
    assert bool(safe) == want["safe_mode"]
    assert L.on_level(phi, want["phi"][None])
    assert L.off_level_kept(phi, before)
    assert abs(err - want["err"]) <= 1e-12 * (n ** 3 / 4096.0) * abs(want["err"])


@pytest.mark.parametrize("has_son", [0, 1])
@pytest.mark.parametrize("level", [3, 4])
def test_staged_force_fine(gpu_lib, oracle, level, has_son):
    """f on the level is gradient_phi of the oracle bit for bit, the other cells of f untouched, diag2[1] = max |rho| exactly.
    diag2[0] is a sum of 3 N terms fact * f^2 of one sign in an unspecified order: against the exact sum of the same terms
    over the leaf cells, relative bound 3 N 2^-53 (1.4e-12 at 16^3: 2e-12 there, in proportion at 8^3)."""
    n = 2 ** level
    rng = np.random.default_rng(20 + level)
    phi_b = rng.normal(size=(1, n, n, n))
    rho_b = rng.normal(size=(1, n, n, n)) * 3.0                            # both signs: the maximum is of |rho|
    L = Level(level, 200 + level + has_son, phi=phi_b, rho=rho_b, f=np.zeros((3, n, n, n)))
    f = L.vec["f"]
    f[:, L.on] = rng.normal(size=(3, L.on.sum()))
    before = f.copy()
    son = rng.integers(1, 1000, L.ncell).astype(np.int32)
    leaf_b = rng.random((1, n, n, n)) < 0.5                                # son == 0 on a random half of the level's cells
    son[L.icell] = np.where(leaf_b[0][L.bz, L.by, L.bx], 0, 7)
    fact = -0.37
    diag2 = np.full(2, -1.0)
    assert gpu_lib.ramses_amd_resident_invalidate() == 0
    rc = gpu_lib.ramses_amd_force_fine_f90(*L.head(), vp(L.vec["phi"]), vp(f), vp(L.vec["rho"]), vp(son), has_son, fact, vp(diag2))
    assert rc == 0, _err(gpu_lib)
    want = oracle.gradient_phi_uniform(phi_b[0])
    assert L.on_level(f, want)
    assert L.off_level_kept(f, before)
    assert diag2[1] == np.abs(rho_b).max()
    terms = fact * (want * want)
    if has_son:
        terms = terms[:, leaf_b[0]]
    epot = math.fsum(terms.ravel())
    print("level %d has_son %d: epot %.17g / %.17g, rel %.3g" % (level, has_son, diag2[0], epot, abs(diag2[0] - epot) / abs(epot)))
    assert abs(diag2[0] - epot) <= 2e-12 * (n ** 3 / 4096.0) * abs(epot)


def _hydro_level(level, seed):
    n = 2 ** level
    u = random_brick(n, n, n, seed=seed)
    fb = np.random.default_rng(seed + 1).normal(size=(3, n, n, n)) * 0.5
    return u, fb, Level(level, 300 + seed, u=u, f=fb)


@pytest.mark.parametrize("level", [3, 4])
def test_resident_gravity_cycle(gpu_lib, oracle, level):
    """two steps of synchro -> courant_grav -> godunov_grav -> set_uold_grav on the resident level against synchro_hydro,
    courant_uniform(grav=), godunov_uniform(grav=), add_gravity_source: dt equal, state bit for bit; the host array is
    untouched before the sync; the density-only sync changes variable 1 of the level's cells and nothing else.  (Both
    syncs go to the array the level was loaded from -- any other address is refused -- with a copy taken in between.)"""
    import ramses_amd
    u, fb, L = _hydro_level(level, 40 + level)
    uold, f = L.vec["u"], L.vec["f"]
    before = uold.copy()
    dx = 1.0 / L.n
    p = ramses_amd.make_params(courant_factor=0.8)
    po = oracle.make_params()
    args = (C.byref(p),) + L.head() + (vp(uold),)
    uo, fo = u.copy(), np.ascontiguousarray(fb)
    out4 = np.zeros(4)
    assert gpu_lib.ramses_amd_resident_invalidate() == 0
    for step in range(2):
        dteff = 1e-3 * (step + 1)
        assert gpu_lib.ramses_amd_resident_synchro_f90(*args, vp(f), dteff) == 0, _err(gpu_lib)
        oracle.synchro_hydro(uo, fo, dteff)
        assert gpu_lib.ramses_amd_resident_courant_grav_f90(*args, vp(f), dx, 1e30, vp(out4)) == 0, _err(gpu_lib)
        dto = oracle.courant_uniform(po, uo, dx, 0.8, grav=fo)
        assert out4[0] == dto
        assert gpu_lib.ramses_amd_resident_godunov_grav_f90(*args, vp(f), dx, dto) == 0, _err(gpu_lib)
        assert gpu_lib.ramses_amd_resident_set_uold_grav_f90(C.byref(p), level, dto) == 0, _err(gpu_lib)
        un = oracle.godunov_uniform(po, uo, dx, dto, grav=fo)
        oracle.add_gravity_source(un, uo, fo, dto)
        uo = un
        assert np.array_equal(uold, before)
    assert gpu_lib.ramses_amd_resident_sync_density_f90(vp(uold)) == 0, _err(gpu_lib)
    dens = uold.copy()
    assert L.on_level(dens[:1], uo[:1])
    assert np.array_equal(dens[1:], before[1:]) and L.off_level_kept(dens, before)
    assert (dens[0, L.on] != before[0, L.on]).any()
    assert gpu_lib.ramses_amd_resident_sync_host_f90(vp(uold)) == 0, _err(gpu_lib)
    assert L.on_level(uold, uo)
    assert L.off_level_kept(uold, before)
    assert gpu_lib.ramses_amd_resident_invalidate() == 0


@pytest.mark.parametrize("level", [3, 4])
def test_resident_poisson_chain(gpu_lib, oracle, level):
    """rho_fine -> multigrid -> force_fine on the resident level, then sync_poisson: phi and f are what the oracle gives for
    the rho that came back; cells off the level keep their host values in all three arrays; a second sync is a no-op."""
    import ramses_amd
    n = 2 ** level
    u = random_brick(n, n, n, seed=50 + level)
    u[0] = _rho_brick(n, 7)                                # (rho_fine reads the density alone)
    L = Level(level, 400 + level, u=u)
    uold = L.vec["u"]
    p = ramses_amd.make_params()
    rng = np.random.default_rng(3)
    phi, f, rho = rng.normal(size=(1, L.ncell)), rng.normal(size=(3, L.ncell)), rng.normal(size=(1, L.ncell))
    before = [a.copy() for a in (phi, f, rho)]
    mp = np.zeros(4)
    assert gpu_lib.ramses_amd_resident_invalidate() == 0
    rc = gpu_lib.ramses_amd_resident_rho_fine_f90(C.byref(p), *L.head(), vp(uold), 1.0, 32, vp(mp))
    assert rc == 0, _err(gpu_lib)
    rho_tot = float(mp[0])                                 # multipole(1) / scale**ndim, scale = boxlen = 1
    safe, it, err = C.c_int(0), C.c_int(-1), C.c_double(-1.0)
    rc = gpu_lib.ramses_amd_resident_multigrid_f90(level, rho_tot, 2 * 6.2831853, EPS, C.byref(safe), C.byref(it), C.byref(err))
    assert rc == 0, _err(gpu_lib)
    fact = 0.25
    diag2 = np.zeros(2)
    assert gpu_lib.ramses_amd_resident_force_fine_f90(level, fact, vp(diag2)) == 0, _err(gpu_lib)
    assert gpu_lib.ramses_amd_resident_sync_poisson_f90(vp(phi), vp(f), vp(rho)) == 0, _err(gpu_lib)
    rho_b = L.to_brick(rho)
    want = oracle.mg_solve_uniform(rho_b[0], rho_tot, boxlen=1.0, epsilon=EPS)
    print("level %d: iters %d / %d, err %.17g / %.17g" % (level, it.value, want["iters"], err.value, want["err"]))
    assert it.value == want["iters"] and it.value >= 2
    assert L.on_level(phi, want["phi"][None])
    want_f = oracle.gradient_phi_uniform(want["phi"])
    assert L.on_level(f, want_f)
    assert diag2[1] == np.abs(rho_b).max()
    for a, b in zip((phi, f, rho), before):
        assert L.off_level_kept(a, b)
    assert (rho[0, L.on] != before[2][0, L.on]).all()
    # nothing is stale any more: the arrays stay as they are
    for a in (phi, f, rho):
        a[:] = -7.0
    assert gpu_lib.ramses_amd_resident_sync_poisson_f90(vp(phi), vp(f), vp(rho)) == 0
    assert all((a == -7.0).all() for a in (phi, f, rho))
    assert gpu_lib.ramses_amd_resident_invalidate() == 0


def test_refusals_of_the_resident_state_machine(gpu_lib, oracle):
    """what the resident entry points refuse out of order, with return code and text"""
    import ramses_amd
    level = 3
    u, fb, L = _hydro_level(level, 60)
    uold, f = L.vec["u"], L.vec["f"]
    dx = 1.0 / L.n
    p = ramses_amd.make_params(courant_factor=0.8)
    args = (C.byref(p),) + L.head() + (vp(uold),)
    lib = gpu_lib
    out4, diag2 = np.zeros(4), np.zeros(2)
    safe, it, err = C.c_int(0), C.c_int(0), C.c_double(0.0)
    assert lib.ramses_amd_resident_invalidate() == 0
    assert lib.ramses_amd_resident_courant_f90(*args, dx, 1e30, vp(out4)) == 0, _err(lib)
    # the Poisson chain out of order
    _refused(lib, lib.ramses_amd_resident_multigrid_f90(level, 1.0, 2 * 6.2831853, EPS, C.byref(safe), C.byref(it), C.byref(err)),
             EINVAL, "no density deposit on the device")
    _refused(lib, lib.ramses_amd_resident_force_fine_f90(level, 0.25, vp(diag2)), EINVAL, "no potential on the device")
    mp = np.zeros(4)
    assert lib.ramses_amd_resident_rho_fine_f90(C.byref(p), *L.head(), vp(uold), 1.0, 32, vp(mp)) == 0, _err(lib)
    _refused(lib, lib.ramses_amd_resident_force_fine_f90(level, 0.25, vp(diag2)), EINVAL, "no potential on the device")
    # set_uold with gravity: no sweep pending; another level; a sweep pending but no acceleration on the device
    _refused(lib, lib.ramses_amd_resident_set_uold_grav_f90(C.byref(p), level, 1e-3), EINVAL, "no godunov_fine result pending")
    _refused(lib, lib.ramses_amd_resident_set_uold_grav_f90(C.byref(p), level + 1, 1e-3), EINVAL, "is not resident")
    assert lib.ramses_amd_resident_godunov_f90(*args, dx, 1e-3) == 0, _err(lib)
    _refused(lib, lib.ramses_amd_resident_set_uold_grav_f90(C.byref(p), level, 1e-3), EINVAL, "no acceleration on the device")
    # synchro between godunov and set_uold (it loads the acceleration first)
    _refused(lib, lib.ramses_amd_resident_synchro_f90(*args, vp(f), 1e-3), EINVAL, "between godunov_fine and set_uold")
    assert lib.ramses_amd_resident_set_uold_grav_f90(C.byref(p), level, 1e-3) == 0, _err(lib)
    assert lib.ramses_amd_resident_sync_host_f90(vp(uold)) == 0, _err(lib)
    assert lib.ramses_amd_resident_invalidate() == 0


def test_refusals_of_the_level_shape(gpu_lib, oracle):
    """nx_loc = 2, one oct too few and one oct off the lattice, at every entry point that takes the level's oct lists"""
    import ramses_amd
    level = 3
    n = 2 ** level
    u, fb, L = _hydro_level(level, 70)
    uold, f = L.vec["u"], L.vec["f"]
    unew = uold.copy()
    rho, phi = np.ascontiguousarray(uold[0]), np.zeros(L.ncell)
    p = ramses_amd.make_params()
    lib = gpu_lib
    dx, dt = 1.0 / n, 1e-3
    out4, diag2 = np.zeros(4), np.zeros(2)
    off = L.xg.copy()
    off[1, L.igrid[5] - 1] += 1.0 / n                     # one cell along y: an odd origin, or past the box
    entries = {
        "godunov_fine_host": lambda h: lib.ramses_amd_godunov_fine_host(C.byref(p), *h, vp(uold), vp(unew), None, dx, dt),
        "multigrid_fine_f90": lambda h: _staged_multigrid(lib, L, rho, phi, float(u[0].mean()), head=h)[0],
        "force_fine_f90": lambda h: lib.ramses_amd_force_fine_f90(*h, vp(phi), vp(f), vp(rho), None, 0, 0.25, vp(diag2)),
        "resident_courant_f90": lambda h: lib.ramses_amd_resident_courant_f90(C.byref(p), *h, vp(uold), dx, 1e30, vp(out4)),
    }
    for name, call in entries.items():
        assert lib.ramses_amd_resident_invalidate() == 0
        _refused(lib, call(L.head(nx_loc=2)), EUNSUPPORTED, "nx=ny=nz=1 (got nx_loc=2)")
        _refused(lib, call(L.head(ngrid=L.ngrid - 1)), EUNSUPPORTED, "level %d is not fully refined" % level)
        _refused(lib, call(L.head(xg=off)), EINVAL, "1 octs of level %d do not sit on the level" % level)
        # a doubly-wrong call reports the earlier of the two
        _refused(lib, call(L.head(nx_loc=2, ngrid=L.ngrid - 1)), EUNSUPPORTED, "nx_loc=2")
        assert call(L.head()) == 0, (name, _err(lib))
    assert np.array_equal(uold, L.vec["u"])
    assert lib.ramses_amd_resident_invalidate() == 0


def test_staged_entries_beside_a_stale_resident_level(gpu_lib, oracle):
    """While the device holds the only current copy of the hydro state: a staged godunov_fine is refused, a staged multigrid_fine
    of ANOTHER level is refused, a staged multigrid_fine of the SAME level succeeds and leaves the residency valid."""
    import ramses_amd
    level = 3
    n = 2 ** level
    u = random_brick(n, n, n, seed=80)
    rho_b = _rho_brick(n, 6)
    L = Level(level, 380, u=u, rho=rho_b[None], phi=np.zeros((1, n, n, n)))
    uold = L.vec["u"]
    before = uold.copy()
    unew = uold.copy()
    dx = 1.0 / L.n
    p = ramses_amd.make_params(courant_factor=0.8)
    po = oracle.make_params()
    lib = gpu_lib
    args = (C.byref(p),) + L.head() + (vp(uold),)
    assert lib.ramses_amd_resident_invalidate() == 0
    dt = 1e-3
    assert lib.ramses_amd_resident_godunov_f90(*args, dx, dt) == 0, _err(lib)
    assert lib.ramses_amd_resident_set_uold_f90(level) == 0, _err(lib)
    _refused(lib, lib.ramses_amd_godunov_fine_host(C.byref(p), *L.head(), vp(uold), vp(unew), None, dx, dt), EINVAL,
             "resident on the device and the host array is stale")
    # another level (its own scrambled layout)
    n4 = 16
    rho4 = _rho_brick(n4, 5)
    L4 = Level(4, 81, rho=rho4[None], phi=np.zeros((1, n4, n4, n4)))
    rc = _staged_multigrid(lib, L4, L4.vec["rho"][0], L4.vec["phi"][0], float(rho4.mean()))[0]
    _refused(lib, rc, EINVAL, "resident on the device and the host array is stale")
    # the same level: the Poisson solve runs next to the resident state
    rho, phi = L.vec["rho"], L.vec["phi"]
    rho_tot = float(rho_b.mean())
    rc, safe, it, err = _staged_multigrid(lib, L, rho[0], phi[0], rho_tot)
    assert rc == 0, _err(lib)
    want = oracle.mg_solve_uniform(rho_b, rho_tot, boxlen=1.0, epsilon=EPS)
    assert it == want["iters"] and L.on_level(phi, want["phi"][None])
    # still resident and still stale; the state comes back right
    _refused(lib, lib.ramses_amd_resident_invalidate(), EINVAL, "the host array is stale")
    assert np.array_equal(uold, before)
    assert lib.ramses_amd_resident_sync_host_f90(vp(uold)) == 0, _err(lib)
    assert L.on_level(uold, oracle.godunov_uniform(po, u, dx, dt))
    assert L.off_level_kept(uold, before)
    assert lib.ramses_amd_resident_invalidate() == 0

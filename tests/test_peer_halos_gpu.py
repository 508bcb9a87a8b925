"""The three device halos that share one peer exchange (csrc/peer_exchange.hpp) -- the resident AMR levels
(ramses_amd_amrres_halo_*), the levels of an AMR multigrid solve (ramses_amd_mgamr_halo_*) and the search direction of the CG
loop (ramses_amd_cgmpi_p_halo_*) -- through the host transport in ONE process that plays the peers' MPI itself: three ranks, the
middle one with nothing either way, one oct in the emission lists of both other peers.  What stage_out leaves in the pinned send
buffer is the reference's message per peer (amr/virtual_boundaries.f90:373-528, :693-983; poisson/multigrid_fine_commons.f90:
1172-1290, 1378-1475), what stage_in makes of fresh random messages is the numpy statement of the exchange, bit for bit, on every
cell.  In every reverse exchange the shared oct holds 1.0 and receives 1e16 from the first peer and -1e16 from the last:
(1.0 + 1e16) - 1e16 = 0.0 in icpu order, 1.0 in the other, so the order of accumulation is decided, not assumed."""
import ctypes as C

import numpy as np
import pytest

from resident import bits, i32, vp

pytestmark = pytest.mark.gpu

NGRIDMAX, NCOARSE = 64, 1
NCELL = NCOARSE + 8 * NGRIDMAX
BIG = 1e16


def _tree():
    return np.zeros(NCELL, np.int32), np.ones((6, NGRIDMAX), np.int32), np.ones(NGRIDMAX, np.int32)


def _cells(octs):
    """cell indices (0-based) of the 8 cells of each oct, [8, n]"""
    return NCOARSE + np.arange(8)[:, None] * NGRIDMAX + (np.asarray(octs)[None, :] - 1)


class _Staged:
    """the four things stage_out hands over, for ncpu = 3"""

    def __init__(self):
        self.hs, self.hr = C.c_int64(0), C.c_int64(0)
        self.so, self.ro = (C.c_int64 * 4)(*[-1] * 4), (C.c_int64 * 4)(*[-1] * 4)

    def args(self):
        return C.byref(self.hs), C.byref(self.hr), self.so, self.ro

    def sent(self, c):
        n = self.so[c + 1] - self.so[c]
        return np.ctypeslib.as_array((C.c_double * max(n, 1)).from_address(self.hs.value + 8 * self.so[c]))[:n].copy()

    def arrive(self, c, msg):
        assert msg.size == self.ro[c + 1] - self.ro[c]
        if msg.size:
            C.memmove(self.hr.value + 8 * self.ro[c], np.ascontiguousarray(msg).ctypes.data, 8 * msg.size)


def test_amrres_halo_three_peers(gpu_lib):
    import ramses_amd
    from ramses_amd._capi import check
    L = gpu_lib
    nvar, lvl = 5, 2
    rng = np.random.default_rng(21)
    son, nbor, father = _tree()
    u = rng.standard_normal((nvar, NCELL))
    u[0] = np.abs(u[0]) + 0.5
    perm = (rng.permutation(NGRIDMAX) + 1).astype(np.int32)
    shared = perm[0]
    em = [np.concatenate(([shared], perm[1:6])), perm[:0], np.concatenate((perm[6:9], [shared], perm[9:11]))]   # 6 + 0 + 6, one oct twice
    rc = [perm[20:27], perm[:0], perm[27:31]]                                                                     # 7 + 0 + 4
    u[:, _cells([shared])] = 1.0
    u0 = u.copy()
    allocts = np.arange(1, NGRIDMAX + 1, dtype=np.int32)
    em_all, rc_all = np.concatenate(em).astype(np.int32), np.concatenate(rc).astype(np.int32)
    check(L.ramses_amd_amrres_load(nvar, NGRIDMAX, NCOARSE, vp(u), vp(son), vp(nbor), vp(father)))
    try:
        check(L.ramses_amd_amrres_comm_set(lvl, 1, 3, i32(*[len(e) for e in em]), vp(em_all), i32(*[len(r) for r in rc]), vp(rc_all)))
        exp = u0.copy()

        def message(vec, octs):      # buf[(v*8 + ind)*n + i] = vec(cell(ind, oct i), v)
            return vec[:, _cells(octs)].reshape(-1)

        # reverse on unew (= uold after set_unew): the reception octs go out, what arrives is added to the emission octs
        check(L.ramses_amd_amrres_set_unew(NGRIDMAX, vp(allocts)))
        S = _Staged()
        check(L.ramses_amd_amrres_halo_stage_out(lvl, 1, 3, *S.args()))
        assert list(S.so) == [0, 40 * 7, 40 * 7, 40 * 11] and list(S.ro) == [0, 40 * 6, 40 * 6, 40 * 12]
        for c in range(3):
            assert np.array_equal(bits(S.sent(c)), bits(message(exp, rc[c])))
        for c, big in ((0, BIG), (2, -BIG)):
            m = rng.standard_normal((nvar, 8, len(em[c])))
            m[:, :, list(em[c]).index(shared)] = big
            S.arrive(c, m)
            cc = _cells(em[c])
            exp[:, cc] = exp[:, cc] + m
        assert np.all(exp[:, _cells([shared])] == 0.0)
        # (a stage_in that does not close this exchange is refused and leaves it open)
        assert L.ramses_amd_amrres_halo_stage_in(lvl, 0) != 0 and b"does not close the exchange" in L.ramses_amd_last_error()
        check(L.ramses_amd_amrres_halo_stage_in(lvl, 1))
        assert L.ramses_amd_amrres_halo_stage_in(lvl, 1) != 0
        p = ramses_amd.make_params(nvar=nvar)
        check(L.ramses_amd_amrres_set_uold(C.byref(p), NGRIDMAX, vp(allocts)))       # uold = unew

        # forward on uold: the emission octs go out, what arrives replaces the reception octs
        S = _Staged()
        check(L.ramses_amd_amrres_halo_stage_out(lvl, 0, 3, *S.args()))
        assert list(S.so) == [0, 40 * 6, 40 * 6, 40 * 12] and list(S.ro) == [0, 40 * 7, 40 * 7, 40 * 11]
        for c in range(3):
            assert np.array_equal(bits(S.sent(c)), bits(message(exp, em[c])))
        for c in (0, 2):
            m = rng.standard_normal((nvar, 8, len(rc[c])))
            S.arrive(c, m)
            exp[:, _cells(rc[c])] = m
        check(L.ramses_amd_amrres_halo_stage_in(lvl, 0))
        check(L.ramses_amd_amrres_sync_all(vp(u)))
        got = u.copy()
    finally:
        check(L.ramses_amd_amrres_invalidate())
    assert np.array_equal(bits(got), bits(exp))
    assert not np.array_equal(bits(got), bits(u0))


@pytest.mark.parametrize("list_is_octs", [0, 1])
def test_mgamr_halo_three_peers(gpu_lib, list_is_octs):
    from ramses_amd._capi import check
    L = gpu_lib
    ilevel, ngrid, nact = 3, 40, 24
    rng = np.random.default_rng(22)
    son, nbor, father = _tree()
    lookup = np.zeros(NGRIDMAX, np.int32)
    flag2 = np.zeros(NCELL, np.int32)
    igrid = (rng.permutation(NGRIDMAX)[:ngrid] + 1).astype(np.int32)      # 24 own octs, then the blocks of peer 1 (10) and peer 3 (6)
    pos = [np.array([3, 17, 1, 24, 9]), np.array([], int), np.array([12, 17, 5, 20])]      # 1-based positions in the own part; 17 twice
    shared = 17
    cells = _cells(igrid)                                                  # [8, 40] by position in the layout
    phi = rng.standard_normal(NCELL)
    phi[cells[:, shared - 1]] = 1.0
    f = rng.standard_normal((3, NCELL))
    phi0, f0 = phi.copy(), f.copy()
    em_list = np.concatenate(pos).astype(np.int32)
    if list_is_octs:
        em_list = igrid[em_list - 1].copy()
    blocks = [(nact, 10), (0, 0), (nact + 10, 6)]                          # (first position, octs) of each peer's reception block
    st0, st1 = (C.c_int64 * 4)(), (C.c_int64 * 4)()
    check(L.ramses_amd_mgamr_force_sync(0))
    check(L.ramses_amd_mgamr_begin(ilevel, NGRIDMAX, NCOARSE, vp(son), vp(nbor), vp(father), vp(lookup), vp(flag2), vp(phi), vp(f),
                                   ngrid, vp(igrid)))
    try:
        check(L.ramses_amd_mgamr_fine_active(nact))
        # (the own rank's entry of rc_n is not a reception block: whatever it says is ignored)
        check(L.ramses_amd_mgamr_comm_set(ilevel, 3, 2, i32(*[len(p) for p in pos]), vp(em_list), list_is_octs, i32(10, 24, 6)))
        uu = phi0[cells]                                                   # the component on the device: u(i + (ind-1)*ngrid)

        def stage_out(d):
            S = _Staged()
            check(L.ramses_amd_mgamr_stats(st0))
            check(L.ramses_amd_mgamr_halo_stage_out(ilevel, 1, d, 3, *S.args()))
            check(L.ramses_amd_mgamr_stats(st1))
            assert st1[2] - st0[2] == 8 * (S.so[3] + S.ro[3]) and st1[3] - st0[3] == 1 and st1[0] == st0[0] and st1[1] == st0[1]
            return S

        # forward: the emission positions go out, what arrives fills the peers' blocks
        S = stage_out(0)
        assert list(S.so) == [0, 40, 40, 72] and list(S.ro) == [0, 80, 80, 128]
        for c in range(3):
            assert np.array_equal(bits(S.sent(c)), bits(uu[:, pos[c] - 1].reshape(-1)))      # u(i + (ind-1)*n)
        for c in (0, 2):
            m = rng.standard_normal((8, blocks[c][1]))
            S.arrive(c, m)
            uu[:, blocks[c][0]:blocks[c][0] + blocks[c][1]] = m
        assert L.ramses_amd_mgamr_halo_stage_in(ilevel, 2, 0) != 0 and b"does not close the exchange" in L.ramses_amd_last_error()
        check(L.ramses_amd_mgamr_halo_stage_in(ilevel, 1, 0))
        assert L.ramses_amd_mgamr_halo_stage_in(ilevel, 1, 0) != 0

        # reverse: the blocks go out, what arrives is added to the emission positions peer by peer
        S = stage_out(1)
        assert list(S.so) == [0, 80, 80, 128] and list(S.ro) == [0, 40, 40, 72]
        for c in range(3):
            assert np.array_equal(bits(S.sent(c)), bits(uu[:, blocks[c][0]:blocks[c][0] + blocks[c][1]].reshape(-1)))
        for c, big in ((0, BIG), (2, -BIG)):
            m = rng.standard_normal((8, len(pos[c])))
            m[:, list(pos[c]).index(shared)] = big
            S.arrive(c, m)
            uu[:, pos[c] - 1] = uu[:, pos[c] - 1] + m
        assert np.all(uu[:, shared - 1] == 0.0)
        assert L.ramses_amd_mgamr_halo_stage_in(ilevel, 1, 0) != 0 and b"does not close the exchange" in L.ramses_amd_last_error()
        check(L.ramses_amd_mgamr_halo_stage_in(ilevel, 1, 1))
    finally:
        check(L.ramses_amd_mgamr_end())       # phi of the whole layout goes home
    exp = phi0.copy()
    exp[cells] = uu
    assert np.array_equal(bits(phi), bits(exp))
    assert not np.array_equal(bits(phi), bits(phi0))
    assert np.array_equal(bits(f), bits(f0))


def test_cgmpi_comm_set_between_the_stages_closes_the_exchange(gpu_lib):
    """New with the shared protocol (before it, the stage_in below indexed the offset table of three ranks with the ncpu of
    five): communicators for more ranks between p_halo_stage_out and p_halo_stage_in leave no exchange to close."""
    from ramses_amd._capi import check
    L = gpu_lib
    rng = np.random.default_rng(24)
    son, nbor, father = _tree()
    igrid = np.arange(1, 21, dtype=np.int32)
    phi, f, out2 = rng.standard_normal(NCELL), rng.standard_normal((3, NCELL)), np.zeros(2)
    f0 = f.copy()
    em, rc = np.array([1, 2, 3, 2], np.int32), np.array([30, 31, 32], np.int32)
    check(L.ramses_amd_cgmpi_begin(2, 20, vp(igrid), vp(son), vp(nbor), NGRIDMAX, NCOARSE, vp(phi), vp(f), None, 0.0, 1.0, 0, vp(out2)))
    try:
        check(L.ramses_amd_cgmpi_comm_set(3, i32(3, 0, 1), vp(em), i32(2, 0, 1), vp(rc)))
        S = _Staged()
        check(L.ramses_amd_cgmpi_p_halo_stage_out(3, *S.args()))
        check(L.ramses_amd_cgmpi_comm_set(5, i32(1, 0, 1, 1, 1), vp(em), i32(1, 0, 1, 0, 1), vp(rc)))
        assert L.ramses_amd_cgmpi_p_halo_stage_in() != 0
        assert b"cgmpi_p_halo_stage_in without cgmpi_p_halo_stage_out" in L.ramses_amd_last_error()
    finally:
        check(L.ramses_amd_cgmpi_end(vp(phi), vp(f)))
    assert np.array_equal(bits(f), bits(f0))


def test_cgmpi_p_halo_three_peers(gpu_lib):
    from ramses_amd._capi import check
    L = gpu_lib
    rng = np.random.default_rng(23)
    son, nbor, father = _tree()
    ngrid = 30
    perm = (rng.permutation(NGRIDMAX) + 1).astype(np.int32)
    igrid = perm[:ngrid].copy()
    shared = perm[0]
    em = [np.concatenate(([shared], perm[1:7])), perm[:0], np.concatenate((perm[7:10], [shared], perm[10:11]))]      # 7 + 0 + 5
    rc = [perm[40:46], perm[:0], perm[46:50]]                                                                          # 6 + 0 + 4
    phi = rng.standard_normal(NCELL)
    f = rng.standard_normal((3, NCELL))
    phi0, f0 = phi.copy(), f.copy()
    out2 = np.zeros(2)
    em_all, rc_all = np.concatenate(em).astype(np.int32), np.concatenate(rc).astype(np.int32)
    check(L.ramses_amd_cgmpi_begin(2, ngrid, vp(igrid), vp(son), vp(nbor), NGRIDMAX, NCOARSE, vp(phi), vp(f), None, 0.0, 1.0, 0, vp(out2)))
    ended = False
    try:
        check(L.ramses_amd_cgmpi_comm_set(3, i32(7, 0, 5), vp(em_all), i32(6, 0, 4), vp(rc_all)))
        S = _Staged()
        check(L.ramses_amd_cgmpi_p_halo_stage_out(3, *S.args()))
        assert list(S.so) == [0, 56, 56, 96] and list(S.ro) == [0, 48, 48, 80]
        exp = f0.copy()
        for c in range(3):
            assert np.array_equal(bits(S.sent(c)), bits(f0[1][_cells(em[c])].reshape(-1)))      # f(:,2) = p at the emission cells
        for c in (0, 2):
            m = rng.standard_normal((8, len(rc[c])))
            S.arrive(c, m)
            exp[1][_cells(rc[c])] = m
        check(L.ramses_amd_cgmpi_p_halo_stage_in())
        rc2 = L.ramses_amd_cgmpi_p_halo_stage_in()
        assert rc2 != 0 and b"cgmpi_p_halo_stage_in without cgmpi_p_halo_stage_out" in L.ramses_amd_last_error()
        ended = True
        check(L.ramses_amd_cgmpi_end(vp(phi), vp(f)))
    finally:
        if not ended:
            L.ramses_amd_cgmpi_end(vp(phi), vp(f))
    assert np.array_equal(bits(f[1]), bits(exp[1]))
    changed = np.zeros(NCELL, bool)
    changed[_cells(rc_all).reshape(-1)] = True
    assert np.all(bits(f[1])[changed] != bits(f0[1])[changed]) and np.array_equal(bits(f[1])[~changed], bits(f0[1])[~changed])
    assert np.array_equal(bits(phi), bits(phi0)) and np.array_equal(bits(f[0]), bits(f0[0])) and np.array_equal(bits(f[2]), bits(f0[2]))

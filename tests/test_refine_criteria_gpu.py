"""GPU test of the refinement criteria on the resident state (csrc/capi_amr.hip lvl_refine_kernel / lvl_mass_map_kernel behind
ramses_amd_amrres_refine_flag / ramses_amd_amrres_mass_map) against a numpy restatement, in the reference's operation order, of
  hydro_refine          hydro/godunov_utils.f90:147-233   (gradients of density, pressure, velocity; NDIM=3, NENER=0)
  the neighbour gather  hydro/hydro_flag.f90:106-131      (a missing neighbour cell is replaced by the neighbouring father cell)
  jeans_length_refine   hydro/hydro_flag.f90:209-256      (pi = twopi/2d0 with twopi = 6.2831853d0, amr/constants.f90:5-6)
  poisson_refine        amr/flag_utils.f90:465-470,480-485 (scalar cut without a floor; density threshold)
  rho_fine's map        pm/rho_fine.f90:96-118,201-211    (phi = rho/d_scale, with ivar_refine only behind the cut; phi >= m_refine)
on the refined shell (level L+1) of a synthetic tree whose level L is complete: L=4 in the host's numbering, L=6 in tiles and
with RAMSES_AMD_DEVICE_ORDER=0, octs created in scrambled and in Z order.  Every list must EQUAL the checker's, sorted.  The
state is helpers.harsh_tree_state with NVAR=7 and smallr=0.6; smallc and the thresholds are placed on quantiles of the checker's
own intermediate values, and the shares that make a pass mean something are asserted on the numpy result alone.
ramses_amd_amrres_hydro_flag runs the same kernel with the other criteria off: its lists are compared with the checker's directly,
not only with refine_flag's.  Both entries also run on short lists -- one oct (8 threads: one partial wavefront) and the 37 octs
of helpers.level_case (296 threads: a full workgroup and a partial wavefront of 40 lanes) -- where the wavefront compaction and
the guard of the last threads can go wrong, with thresholds on quantiles of the checker's values over that list's own cells."""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import harsh_tree_state, level_case, shell_mask
from resident import force_tiles, load, vp

pytestmark = pytest.mark.gpu

GAMMA, SMALLR, NVAR = 1.4, 0.6, 7
PI = 6.2831853 / 2.0
FLOOR = 1e-10


@pytest.fixture(autouse=True)
def _tiles_on_small_levels_too(monkeypatch):
    force_tiles(monkeypatch, clear=())


def _prim(u, c):
    """hydro/godunov_utils.f90:147-187"""
    d = np.maximum(u[0, c], SMALLR)
    v = [u[1 + k, c] / d for k in range(3)]
    ek = np.zeros_like(d)
    for k in range(3):
        ek = ek + 0.5 * d * v[k] ** 2
    return d, v, (GAMMA - 1.0) * (u[4, c] - ek)


def _grad_errors(qg, qm, qd):
    """hydro/godunov_utils.f90:200-233: the three error terms of one direction"""
    (dg, vg, pg), (dm, vm, pm), (dd, vd, pd) = qg, qm, qd
    e_d = 2.0 * np.maximum(np.abs((dd - dm) / (dd + dm + FLOOR)), np.abs((dm - dg) / (dm + dg + FLOOR)))
    e_p = 2.0 * np.maximum(np.abs((pd - pm) / (pd + pm + FLOOR)), np.abs((pm - pg) / (pm + pg + FLOOR)))
    cg = np.sqrt(np.maximum(GAMMA * pg / dg, FLOOR ** 2))
    cm = np.sqrt(np.maximum(GAMMA * pm / dm, FLOOR ** 2))
    cd = np.sqrt(np.maximum(GAMMA * pd / dd, FLOOR ** 2))
    e_u = np.zeros_like(e_d)
    for k in range(3):
        e = 2.0 * np.maximum(np.abs((vd[k] - vm[k]) / (cd + cm + np.abs(vd[k]) + np.abs(vm[k]) + FLOOR)),
                             np.abs((vm[k] - vg[k]) / (cm + cg + np.abs(vm[k]) + np.abs(vg[k]) + FLOOR)))
        e_u = np.maximum(e_u, e)
    return e_d, e_p, e_u


@functools.lru_cache(maxsize=None)
def _case(L, order):
    """tree, state and what the checker needs of the level-(L+1) cells, computed once and left unchanged"""
    from ramses_amd import ic
    T = ic.uniform_tree(L, order=order, refine_mask=shell_mask(2 ** L), slack=260000 if L >= 6 else 7)
    u = harsh_tree_state(T, L, 31 + L, nvar=NVAR, gamma=GAMMA)
    ngm, nco = T["ngridmax"], T["ncoarse"]
    ig = np.ascontiguousarray(T["igrid_fine"]).astype(np.int32)
    g = np.tile(ig.astype(np.int64), 8)
    ind = np.repeat(np.arange(8), len(ig))
    c = nco + ind * ngm + g - 1                                    # 0-based cells of the level, octant by octant
    son, nbor = T["son"], T["nbor"]
    # the gradient criteria: the largest error over the three directions, per criterion
    qm = _prim(u, c)
    err = [np.zeros(len(c)) for _ in range(3)]
    ncoarser = 0
    for d in range(3):
        cn = []
        for side in range(2):
            inside = ((ind >> d) & 1) != side                        # the neighbour is a sibling
            sib = c + (1 if side else -1) * (1 << d) * ngm
            nb = nbor[2 * d + side, g - 1].astype(np.int64)          # the neighbouring father cell (1-based)
            g2 = son[nb - 1].astype(np.int64)
            out = np.where(g2 > 0, nco + (ind ^ (1 << d)) * ngm + g2 - 1, nb - 1)
            ncoarser += int((~inside & (g2 == 0)).sum())
            cn.append(np.where(inside, sib, out))
        e = _grad_errors(_prim(u, cn[0]), qm, _prim(u, cn[1]))
        err = [np.maximum(a, b) for a, b in zip(err, e)]
    # jeans_length_refine's temperature before the floor, hydro/hydro_flag.f90:217-248
    dens = np.maximum(u[0, c], SMALLR)
    eth = u[4, c].copy()
    for k in (1, 2, 3):
        eth = eth - 0.5 * u[k, c] ** 2 / dens
    tempe = eth / dens * (GAMMA - 1.0)
    smallc = float(np.sqrt(np.quantile(tempe, 0.2)))                  # a fifth of the cells take the smallc**2 floor
    lamb = np.sqrt(np.maximum(tempe, smallc ** 2) * PI / dens / 1.0)
    rng = np.random.default_rng(7 + L)
    rho = np.zeros(T["ncell"])
    rho[c] = u[0, c] * rng.uniform(0.5, 1.5, len(c))                # a deposit of its own (host vector)
    K = dict(T=T, u=u, ig=ig, c=c, err=err, ncoarser=ncoarser, dens_raw=u[0, c], tempe=tempe, smallc=smallc, lamb=lamb, rho=rho,
             tail_pix=1.0 / 2 ** (L + 1))
    # thresholds on quantiles of the checker's values
    K["egd"], K["egp"], K["egu"] = (float(np.quantile(e, q)) for e, q in zip(err, (0.5, 0.6, 0.4)))
    K["n_jeans"] = float(np.quantile(lamb, 0.45)) / K["tail_pix"]
    K["thr"] = float(np.quantile(u[0, c], 0.55))
    K["cut"] = float(np.quantile(u[5, c] / u[0, c], 0.5))
    K["d_scale"] = 0.37
    K["m_refine"] = float(np.quantile(rho[c] / K["d_scale"], 0.5))
    # the checker's flags per criterion
    F = {"d": err[0] > K["egd"], "p": err[1] > K["egp"], "u": err[2] > K["egu"],
         "jeans": K["n_jeans"] * K["tail_pix"] >= lamb,
         "thr": u[0, c] >= K["thr"],
         "cut": u[5, c] / u[0, c] > K["cut"]}
    K["flags"] = F
    phi0 = rho[c] / K["d_scale"]
    phi6 = np.where(u[5, c] / np.maximum(u[0, c], SMALLR) > K["cut"], rho[c] / K["d_scale"], 0.0)
    K["map"] = {0: phi0 >= K["m_refine"], 6: phi6 >= K["m_refine"]}
    return K


def _cells(K, mask):
    return np.sort(K["c"][mask] + 1).astype(np.int32)


def _load(gpu_lib, K):
    assert K["u"].shape[0] == NVAR
    load(gpu_lib, K["T"], K["u"])


def _params(K):
    import ramses_amd
    return ramses_amd.make_params(nvar=NVAR, gamma=GAMMA, smallr=SMALLR, smallc=K["smallc"])


def _flag(gpu_lib, K, ig=None, **kw):
    from ramses_amd._capi import check, make_refine_crit
    ig = K["ig"] if ig is None else ig
    cells = np.zeros(8 * len(ig), np.int32)
    n = C.c_int(-1)
    crit = make_refine_crit(floor_d=FLOOR, floor_p=FLOOR, floor_u=FLOOR, **kw)
    p = _params(K)
    check(gpu_lib.ramses_amd_amrres_refine_flag(C.byref(p), len(ig), vp(ig), C.byref(crit), vp(cells), C.byref(n)))
    return cells[:n.value].copy()


def _hydro_flag(gpu_lib, K, egd, egp, egu, ig=None):
    """ramses_amd_amrres_hydro_flag's list"""
    from ramses_amd._capi import check
    ig = K["ig"] if ig is None else ig
    cells = np.zeros(8 * len(ig), np.int32)
    n = C.c_int(-1)
    p = _params(K)
    check(gpu_lib.ramses_amd_amrres_hydro_flag(C.byref(p), len(ig), vp(ig), egd, egp, egu, FLOOR, FLOOR, FLOOR, vp(cells), C.byref(n)))
    return cells[:n.value].copy()


@functools.lru_cache(maxsize=None)
def _short(L, order, n):
    """A short list of the level's octs -- the 37 that helpers.level_case draws from the same tree, or one of them -- with the
    checker's values of its own cells: thresholds on their quantiles (a quarter of the cells per gradient criterion, a fifth for
    the Jeans length and the density), the flags per criterion and the cells as the device lists them (1-based, ascending).
    An oct below the density floor has eight equal densities and no density gradient, one on the smallc floor eight equal Jeans
    lengths: no threshold splits those.  The one-oct list is the first of the 37 that every criterion splits."""
    K = _case(L, order)
    ig = np.ascontiguousarray(level_case(L, order)[0]["lists"][L + 1]["sub"])
    if n == 1:
        for g in ig:
            S = _short_of(K, np.array([g], np.int32))
            if all(0.1 <= f.mean() <= 0.9 for f in S["flags"].values()):
                return S
    assert len(ig) == n
    return _short_of(K, ig)


def _short_of(K, ig):
    where = {int(g): i for i, g in enumerate(K["ig"])}
    pos = np.array([where[int(g)] for g in ig])                    # (KeyError: not the tree of _case)
    at = (np.arange(8)[:, None] * len(K["ig"]) + pos[None, :]).ravel()
    S = dict(ig=ig, c=K["c"][at])
    S["egd"], S["egp"], S["egu"] = (float(np.quantile(e[at], 0.75)) for e in K["err"])
    S["n_jeans"] = float(np.quantile(K["lamb"][at], 0.2)) / K["tail_pix"]
    S["thr"] = float(np.quantile(K["dens_raw"][at], 0.8))
    S["flags"] = {"d": K["err"][0][at] > S["egd"], "p": K["err"][1][at] > S["egp"], "u": K["err"][2][at] > S["egu"],
                  "jeans": S["n_jeans"] * K["tail_pix"] >= K["lamb"][at], "thr": K["dens_raw"][at] >= S["thr"]}
    S["grad"] = S["flags"]["d"] | S["flags"]["p"] | S["flags"]["u"]
    S["mixed"] = S["flags"]["d"] | S["flags"]["jeans"] | S["flags"]["thr"]
    return S


def _crit_args(K, name):
    return {"d": dict(err_grad_d=K["egd"]), "p": dict(err_grad_p=K["egp"]), "u": dict(err_grad_u=K["egu"]),
            "jeans": dict(n_jeans=K["n_jeans"], tail_pix=K["tail_pix"], factG=1.0),
            "thr": dict(thr_mode=1, thr=K["thr"]),
            "cut": dict(thr_mode=2, ivar_refine=6, var_cut_refine=K["cut"])}[name]


SHORT = [(4, "scrambled", None, 1), (4, "scrambled", None, 37), (6, "scrambled", "1", 1), (6, "scrambled", "1", 37)]
CASES = [(4, "scrambled", None), (6, "scrambled", "1"), (6, "scrambled", "0"), (6, "morton", "1"), (6, "morton", "0")]


def test_the_input_exercises_every_criterion_and_floor():
    """(on the numpy result alone) each criterion flags 10 % .. 90 % of the level's cells, at least 1 % of them take the
    smallc**2 floor and 1 % the smallr floor, some lie next to a coarser neighbour; the two maps differ"""
    for L, order in ((4, "scrambled"), (6, "scrambled"), (6, "morton")):
        K = _case(L, order)
        for name, f in list(K["flags"].items()) + [("map0", K["map"][0]), ("map6", K["map"][6])]:
            assert 0.1 <= f.mean() <= 0.9, (L, order, name, f.mean())
        assert (K["tempe"] < K["smallc"] ** 2).mean() >= 0.01
        assert (K["dens_raw"] < SMALLR).mean() >= 0.01
        assert K["ncoarser"] > 0
        assert (K["map"][0] != K["map"][6]).any()
        union = np.zeros(len(K["c"]), bool)
        for f in K["flags"].values():
            union |= f
        assert any((union != f).any() for f in K["flags"].values())


def test_the_short_lists_flag_a_share_of_their_cells():
    """(on the numpy result alone) on the one-oct and the 37-oct lists every criterion alone, the three gradients together and
    density gradient | Jeans | threshold together flag 10 % .. 90 % of the list's cells: neither 'all' nor 'none' passes"""
    for L, order, n in sorted({(L, order, n) for L, order, _, n in SHORT}):
        S = _short(L, order, n)
        assert len(S["c"]) == 8 * n and len(np.unique(S["ig"])) == n
        for name, f in list(S["flags"].items()) + [("grad", S["grad"]), ("mixed", S["mixed"])]:
            assert 0.1 <= f.mean() <= 0.9, (L, order, n, name, f.mean())


@pytest.mark.parametrize("L,order,device_order,n", SHORT)
def test_short_lists_equal_the_restated_reference(gpu_lib, monkeypatch, L, order, device_order, n):
    """one partial wavefront (n = 1), one full workgroup and a partial wavefront (n = 37): hydro_flag and refine_flag against the
    checker, in the host's numbering (L = 4) and in tiles (L = 6)"""
    if device_order is None:
        monkeypatch.delenv("RAMSES_AMD_DEVICE_ORDER", raising=False)
    else:
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", device_order)
    K, S = _case(L, order), _short(L, order, n)
    _load(gpu_lib, K)
    assert gpu_lib.ramses_amd_amrres_tiled_levels() == (2 if L == 6 else 0)
    want = _cells(S, S["grad"])
    got = _hydro_flag(gpu_lib, K, S["egd"], S["egp"], S["egu"], ig=S["ig"])
    assert np.array_equal(got, want), ("hydro_flag", len(got), len(want))
    got = _flag(gpu_lib, K, ig=S["ig"], err_grad_d=S["egd"], err_grad_p=S["egp"], err_grad_u=S["egu"])
    assert np.array_equal(got, want), ("refine_flag", len(got), len(want))
    for name, eg in (("d", (S["egd"], -1.0, -1.0)), ("p", (-1.0, S["egp"], -1.0)), ("u", (-1.0, -1.0, S["egu"]))):
        got = _hydro_flag(gpu_lib, K, *eg, ig=S["ig"])
        assert np.array_equal(got, _cells(S, S["flags"][name])), (name, len(got))
    got = _flag(gpu_lib, K, ig=S["ig"], err_grad_d=S["egd"], n_jeans=S["n_jeans"], tail_pix=K["tail_pix"], factG=1.0, thr_mode=1, thr=S["thr"])
    assert np.array_equal(got, _cells(S, S["mixed"])), ("mixed", len(got))
    # the kernel without the neighbour gathers on the same partial wavefronts
    got = _flag(gpu_lib, K, ig=S["ig"], n_jeans=S["n_jeans"], tail_pix=K["tail_pix"], factG=1.0)
    assert np.array_equal(got, _cells(S, S["flags"]["jeans"])), ("jeans", len(got))
    assert len(_hydro_flag(gpu_lib, K, -1.0, -1.0, -1.0, ig=S["ig"])) == 0
    gpu_lib.ramses_amd_amrres_invalidate()


@pytest.mark.parametrize("L,order,device_order", CASES)
def test_every_criterion_equals_the_restated_reference(gpu_lib, monkeypatch, L, order, device_order):
    from ramses_amd._capi import check
    if device_order is None:
        monkeypatch.delenv("RAMSES_AMD_DEVICE_ORDER", raising=False)
    else:
        monkeypatch.setenv("RAMSES_AMD_DEVICE_ORDER", device_order)
    K = _case(L, order)
    _load(gpu_lib, K)
    if L == 6:
        assert gpu_lib.ramses_amd_amrres_tiled_levels() == (2 if device_order == "1" else 0)
    F = K["flags"]
    # each criterion alone
    for name in F:
        got = _flag(gpu_lib, K, **_crit_args(K, name))
        assert np.array_equal(got, _cells(K, F[name])), (name, len(got), int(F[name].sum()))
    # all together (the threshold mode holds one of its two criteria at a time) == the union of the lists each gives alone
    for mode in ("thr", "cut"):
        kw = {}
        union = np.zeros(len(K["c"]), bool)
        for name in ("d", "p", "u", "jeans", mode):
            kw.update(_crit_args(K, name))
            union |= F[name]
        assert np.array_equal(_flag(gpu_lib, K, **kw), _cells(K, union)), mode
    # ramses_amd_amrres_hydro_flag on the same state: the checker's list for the gradients that are on (all three, each alone),
    # which is also what refine_flag returns for them; all three off: an empty list and no error
    ig = K["ig"]
    p = _params(K)
    for names in (("d", "p", "u"), ("d",), ("p",), ("u",)):
        egd, egp, egu = (K["eg" + k] if k in names else -1.0 for k in ("d", "p", "u"))
        want = np.zeros(len(K["c"]), bool)
        for k in names:
            want |= F[k]
        cells = _hydro_flag(gpu_lib, K, egd, egp, egu)
        assert len(cells) > 0
        assert np.array_equal(cells, _cells(K, want)), (names, len(cells), int(want.sum()))
        assert np.array_equal(_flag(gpu_lib, K, err_grad_d=egd, err_grad_p=egp, err_grad_u=egu), cells)
    assert len(_hydro_flag(gpu_lib, K, -1.0, -1.0, -1.0)) == 0
    # nothing asked for: nothing flagged
    assert len(_flag(gpu_lib, K)) == 0
    # the map, from the host's deposit and then from the copy that call left on the device
    for ivar in (0, 6):
        want = _cells(K, K["map"][ivar])
        for rho in (K["rho"], None):
            cells = np.zeros(8 * len(ig), np.int32)
            n = C.c_int(-1)
            check(gpu_lib.ramses_amd_amrres_mass_map(C.byref(p), len(ig), vp(ig), K["d_scale"], K["m_refine"], ivar, K["cut"], vp(rho),
                                                     vp(cells), C.byref(n)))
            assert np.array_equal(cells[:n.value], want), (ivar, rho is None, n.value, len(want))
    # the state did not move
    v = K["u"].copy()
    check(gpu_lib.ramses_amd_amrres_sync_all(vp(K["u"])))
    assert np.array_equal(v, K["u"])
    gpu_lib.ramses_amd_amrres_invalidate()

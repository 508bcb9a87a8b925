"""Shared test helpers: seeded synthetic states in the brick layout."""
import math
import os
import shutil

import numpy as np


def hip_include(header="hip_runtime_api.h"):
    """the include directory of the ROCm installation that holds hip/<header>: for the tests that compile with the host compiler"""
    cands = [os.environ.get("ROCM_PATH"), os.environ.get("HIP_PATH")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        cands.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    cands.append("/opt/rocm")
    for c in cands:
        if c and os.path.exists(os.path.join(c, "include", "hip", header)):
            return os.path.join(c, "include")
    raise RuntimeError("hip/%s not found" % header)


def random_brick(nx, ny, nz, seed, gamma=1.4, contrast=True, nvar=5):
    """Positive-density/pressure random state u[nvar,nz,ny,nx] with shocks:
    piecewise-constant blocks + noise, pressure spanning several decades."""
    rng = np.random.default_rng(seed)
    shp = (nz, ny, nx)
    rho = rng.uniform(0.2, 2.0, shp)
    vel = rng.normal(0.0, 0.7, (3,) + shp)
    p = rng.uniform(0.05, 2.0, shp)
    if contrast:
        # blocky jumps so the limiters and Riemann branches all fire
        bz, by, bx = max(nz // 3, 1), max(ny // 3, 1), max(nx // 3, 1)
        jump = 10.0 ** rng.uniform(-3, 2, (nz // bz + 1, ny // by + 1, nx // bx + 1))
        jump = np.repeat(np.repeat(np.repeat(jump, bz, 0), by, 1), bx, 2)[:nz, :ny, :nx]
        p = p * jump
        rho = rho * np.sqrt(jump)
    u = np.zeros((nvar,) + shp)
    u[0] = rho
    u[1:4] = rho * vel
    u[4] = p / (gamma - 1.0) + 0.5 * rho * (vel ** 2).sum(0)
    for n in range(5, nvar):
        u[n] = rho * rng.uniform(0, 1, shp)
    return u


def _octree_layout(u, level, rng, ngridmax, ncoarse=1):
    """Scatter brick u[nvar,n,n,n] into RAMSES cell vectors with octs of the
    level placed in random slots; returns (cellvec[nvar,ncell], igrid, xg, (ox, oy, oz))."""
    nvar, n = u.shape[0], u.shape[1]
    no = n // 2
    ngrid = no ** 3
    ncell = ncoarse + 8 * ngridmax
    slots = rng.permutation(ngridmax)[:ngrid] + 1            # 1-based oct slots
    igrid = rng.permutation(slots).astype(np.int32)          # active list order
    xg = np.zeros((3, ngridmax))
    vec = rng.normal(size=(nvar, ncell))                     # garbage elsewhere
    # oct g of the active list sits at a random oct position
    pos = rng.permutation(ngrid)
    oz, oy, ox = np.unravel_index(pos, (no, no, no))
    for d, o in enumerate((ox, oy, oz)):
        xg[d, igrid - 1] = (2 * o + 1) / n
    for ind in range(8):
        ix, iy, iz = ind & 1, (ind >> 1) & 1, (ind >> 2) & 1
        icell = ncoarse + ind * ngridmax + (igrid - 1)
        vec[:, icell] = u[:, 2 * oz + iz, 2 * oy + iy, 2 * ox + ix]
    return vec, igrid, xg, (ox, oy, oz)


def rel_linf(a, b):
    """max |a-b| / max |b| per variable, maximised over variables."""
    worst = 0.0
    for n in range(a.shape[0]):
        scale = np.abs(b[n]).max()
        if scale == 0.0:
            scale = 1.0
        worst = max(worst, np.abs(a[n] - b[n]).max() / scale)
    return worst


def _set_uold_scalar_fix(uold, unew, smallr):
    """numpy restatement of the passive-scalar floor fix of set_uold
    (hydro/godunov_fine.f90:176-190); test-side only.  Works on bricks u[nvar,nz,ny,nx] and on cell vectors u[nvar,ncell]."""
    out = unew.copy()
    a = (uold[0] < smallr) & (unew[0] > uold[0])
    b = ~a & (unew[0] < smallr) & (uold[0] > unew[0])
    for n in range(5, unew.shape[0]):
        out[n][a] = (uold[n] * np.maximum(unew[0], smallr) / smallr)[a]
        out[n][b] = (uold[n] * smallr / np.maximum(uold[0], smallr))[b]
    return out


def shell_mask(nc, lo=0.23, hi=0.36, seam=True):
    """the refined level-L cells of the tile tests' tree, mask[z, y, x]: a spherical shell, and cells on the periodic seam"""
    z, y, x = np.meshgrid(np.arange(nc), np.arange(nc), np.arange(nc), indexing="ij")
    r = np.sqrt((x - nc / 2 + 0.5) ** 2 + (y - nc / 2 + 0.5) ** 2 + (z - nc / 2 + 0.5) ** 2)
    mask = (r >= lo * nc) & (r <= hi * nc)
    if seam:
        mask[0, 0, :5] = True              # refined cells on the periodic seam too (tiles wrap)
        mask[nc - 1, nc - 1, nc - 3:] = True
    return mask


def mild_tree_state(T, seed, nvar=5):
    """the mild state of the AMR tile tests: density in [1, 2), momenta rho (U - 1/2), internal energy in
    [1, 2), passive scalars rho x a fraction -- subsonic, above every floor"""
    rng = np.random.default_rng(seed)
    n = T["ncell"] - 1
    u = np.zeros((nvar, T["ncell"]))
    u[0, 1:] = 1.0 + rng.random(n)
    for d in (1, 2, 3):
        u[d, 1:] = u[0, 1:] * (rng.random(n) - 0.5)
    u[4, 1:] = 1.0 + rng.random(n) + 0.5 * (u[1, 1:] ** 2 + u[2, 1:] ** 2 + u[3, 1:] ** 2) / u[0, 1:]
    for v in range(5, nvar):
        u[v, 1:] = u[0, 1:] * rng.random(n)
    u[:, 0] = u[:, 1]
    return u


def tree_cell_kind(T, L, cell):
    """what kind of cell (0-based index) of levels L / L+1 of a synthetic tree with level L complete: for the report of a difference"""
    ngm, nco = T["ngridmax"], T["ncoarse"]
    g = (cell - nco) % ngm + 1                                          # its oct (1-based)
    ind = (cell - nco) // ngm
    lev = L + 1 if np.isin(g, T["igrid_fine"]) else L
    nb = T["nbor"][:, g - 1].astype(np.int64)                           # the six neighbouring father cells of the oct
    if T["son"][cell] != 0:
        kind = "refined cell (its fluxes are reset)"
    elif lev == L + 1:
        kind = "ghost-adjacent (a neighbouring oct is interpolated)" if (T["son"][nb - 1] == 0).any() else "interior"
    else:
        kind = "interior"
        for axis in range(3):
            up = (ind >> axis) & 1
            sg = T["son"][nb[2 * axis + up] - 1]                        # the oct across the oct's face (level L is complete)
            across = nco + (ind ^ (1 << axis)) * ngm + sg - 1
            sibling = nco + (ind ^ (1 << axis)) * ngm + g - 1
            if T["son"][across] != 0 or T["son"][sibling] != 0:
                kind = "coarse leaf corrected by level %d" % (L + 1)
    return "cell %d of level %d, %s" % (cell, lev, kind)


def harsh_tree_state(T, L, seed, nvar=5, gamma=1.4):
    """A supersonic state with densities below and above a floor of 0.6 on a synthetic tree T = uniform_tree(L, refine_mask=...):
    cell vector u[nvar, ncell].  Level L is random_brick(2^L, ...) (blocky pressure jumps over five decades, velocities of
    sigma 0.7: more than half of the cells above Mach 1, half of the densities below 0.6).  A level-(L+1) cell is its father
    cell's state times a factor in [0.9, 1.1] of its own, each momentum component perturbed by another +-15 %; the total energy
    is put together again from the father's internal energy times the same factor, so the pressure stays positive.  Cells that
    belong to neither level (coarser levels, free slots) hold gas at rest with density and pressure 1; cell 0 is a copy of
    cell 1.  The first five variables do not depend on nvar (the scalars are drawn last)."""
    n = 2 ** L
    rng = np.random.default_rng(seed + 1)
    u = np.zeros((nvar, T["ncell"]))
    u[0] = 1.0
    u[4] = 1.0 / (gamma - 1.0)
    T["to_cells"](random_brick(n, n, n, seed, gamma=gamma, nvar=nvar), u)
    ig = np.asarray(T["igrid_fine"], np.int64)
    fc = T["father"][ig - 1].astype(np.int64) - 1                 # (0-based) father cell of every level-(L+1) oct
    coarse = u[:, fc]
    eint = coarse[4] - 0.5 * (coarse[1:4] ** 2).sum(0) / coarse[0]
    assert (eint > 0).all()
    fac = rng.uniform(0.9, 1.1, (8, len(ig)))
    kick = rng.uniform(0.85, 1.15, (8, 3, len(ig)))
    for ind in range(8):
        c = T["ncoarse"] + ind * T["ngridmax"] + ig - 1
        u[:, c] = coarse * fac[ind]
        u[1:4, c] = u[1:4, c] * kick[ind]
        u[4, c] = eint * fac[ind] + 0.5 * (u[1:4, c] ** 2).sum(0) / u[0, c]
    u[:, 0] = u[:, 1]
    return u


def tree_state_shares(T, L, u, smallr=0.6, gamma=1.4):
    """(share of the cells of levels L and L+1 above Mach 1, share of them with a density below smallr)"""
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([T["igrid"], T["igrid_fine"]]).astype(np.int64) - 1
                            for ind in range(8)])
    rho, m, e = u[0, cells], u[1:4, cells], u[4, cells]
    v2 = (m ** 2).sum(0) / rho ** 2
    c2 = gamma * (gamma - 1.0) * (e - 0.5 * rho * v2) / rho
    return float((v2 > c2).mean()), float((rho < smallr).mean())


# ---- checkers of the small routines amr_step calls between sweeps on an AMR level (tests/test_amr_level_kernels_gpu.py,
# tests/test_amr_level_checkers.py): the C oracle where it has the routine, numpy restatements of the reference elsewhere --------


def oct_cells(T, octs):
    """the (0-based) cells of the octs (1-based) of a synthetic tree, octant by octant: [8 * len(octs)]"""
    g = np.asarray(octs, np.int64)
    return np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + g - 1 for ind in range(8)])


def leaf_cells(T, octs):
    c = oct_cells(T, octs)
    return c[T["son"][c] == 0]


def coarser_faces(T, octs):
    """how many cell faces of the octs (four per oct face) look at a father cell without an oct of its own: the faces where the
    pdV term takes its neighbour at 1.5 dx"""
    g = np.asarray(octs, np.int64)
    return 4 * int((T["son"][T["nbor"][:, g - 1].astype(np.int64) - 1] == 0).sum())


def courant_dt_oracle(oracle, po, u, f, cells, dx, courant_factor):
    """courant_fine's time step over the given cells: the C oracle's cmpdt (flat over cells; pinned to the reference's by
    tests/test_oracle_pinned.py) on the cells gathered into a (5, 1, 1, n) brick; no cell: the initial courant_factor dx / smallc"""
    if len(cells) == 0:
        return courant_factor * dx / po.smallc
    uu = np.ascontiguousarray(u[:5, cells]).reshape(5, 1, 1, -1)
    gg = None if f is None else np.ascontiguousarray(f[:, cells]).reshape(3, 1, 1, -1)
    return oracle.courant_uniform(po, uu, dx, courant_factor, grav=gg)


def courant_sum_terms(u, cells, dx, smallr):
    """the terms courant_fine adds up (hydro/courant_fine.f90:94-112), per cell and in its operation order: (mass terms, total
    energy terms, internal energy terms -- four per cell: E vol and - 0.5 m_k^2 / max(rho, smallr) vol for k = 1, 2, 3)"""
    vol = dx * dx * dx
    rho = np.maximum(u[0, cells], smallr)
    mass = u[0, cells] * vol
    etot = u[4, cells] * vol
    eint = [etot] + [-(0.5 * u[k, cells] ** 2 / rho * vol) for k in (1, 2, 3)]
    return mass, etot, np.concatenate(eint)


def fsum_bound(terms):
    """(exactly rounded sum, n 2^-53 sum |t|): the bound, to first order in 2^-53, on the error of ANY order of summing the n terms in
    double precision -- every partial sum is at most sum |t| and each of the n - 1 additions rounds by at most 2^-53 of it; the
    n-th 2^-53 covers the rounding of the exact sum itself, terms of order n^2 2^-106 are left out.  It is a bound on the ADDING
    alone: the terms themselves must be the reference's bit for bit, which holds for a kernel built without contraction of
    multiply-adds (csrc/capi_amr.hip is: -ffp-contract=off).  Nothing measured goes into it."""
    return math.fsum(terms), len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms))


def synchro_oracle(oracle, u, f, cells, dteff, smallr):
    """synchro_hydro_fine on the cells: the C oracle on the gathered cells, scattered into a copy of u"""
    out = u.copy()
    ug, fg = np.ascontiguousarray(u[:, cells]), np.ascontiguousarray(f[:, cells])
    oracle.synchro_hydro(ug, fg, dteff, smallr=smallr)
    out[:, cells] = ug
    return out


def gravity_source_oracle(oracle, unew, uold, f, cells, dt, smallr):
    """add_gravity_source_terms on the cells (C oracle on the gathered cells): unew[:, cells] after it"""
    ng, og, fg = (np.ascontiguousarray(a[:, cells]) for a in (unew, uold, f))
    oracle.add_gravity_source(ng, og, fg, dt, smallr=smallr)
    return ng


def set_uold_grav_expected(oracle, uold, unew, f, cells, dt, smallr):
    """set_uold with poisson (hydro/godunov_fine.f90:159-197) on the cells: the gravity source on unew, the passive-scalar floor
    fix, uold = unew; returns the new uold (a copy)"""
    out = uold.copy()
    ng = gravity_source_oracle(oracle, unew, uold, f, cells, dt, smallr)
    out[:, cells] = _set_uold_scalar_fix(np.ascontiguousarray(uold[:, cells]), ng, smallr)
    return out


def upl_oracle(oracle, T, u, octs, interpol_var, smallr):
    """upload_fine on the octs: every split cell of theirs = the C oracle's upl (pinned to the reference's by tests/test_amr_ops.py)
    of its eight children; returns (the new state, a copy; the split cells)"""
    nvar = u.shape[0]
    c = oct_cells(T, octs)
    c = c[T["son"][c] > 0]
    out = u.copy()
    if len(c):
        gs = T["son"][c].astype(np.int64)
        child = np.ascontiguousarray(np.stack([u[:, T["ncoarse"] + k * T["ngridmax"] + gs - 1] for k in range(8)], axis=1))   # [nvar, 8, n]
        pa = np.zeros((nvar, len(c)))
        oracle.lib().ora_upl(child, pa, len(c), len(c), nvar, interpol_var, smallr)
        out[:, c] = pa
    return out, c


def _kinetic(uold, c, smallr):
    """d = max(rho, smallr), e_kin = 0.5 d (u^2 + v^2 + w^2) with u, v, w = momenta / d: hydro/godunov_fine.f90:207-212, 405-410"""
    d = np.maximum(uold[0, c], smallr)
    u, v, w = uold[1, c] / d, uold[2, c] / d, uold[3, c] / d
    return d, 0.5 * d * (u ** 2 + v ** 2 + w ** 2)


def pdv_numpy(T, octs, uold, enew, dx_loc, dt, gamma, smallr):
    """add_pdv_source_terms with pressure_fix, NDIM = 3, NENER = 0 (hydro/godunov_fine.f90:294-481) on the octs of a level, in
    the reference's operation order; enew is updated in place.  Returns (the cells, div u per cell)."""
    ngm, nco, son, nbor = T["ngridmax"], T["ncoarse"], T["son"], T["nbor"]
    g = np.tile(np.asarray(octs, np.int64), 8)
    ind = np.repeat(np.arange(8), len(octs))
    c = nco + ind * ngm + g - 1                                       # :360-363
    # igridn(:, 0:6): the oct itself and the octs in its six neighbouring father cells (0: none), :344-354
    ind_nbor = nbor[:, g - 1].astype(np.int64)                        # ind_left (rows 0, 2, 4) / ind_right (rows 1, 3, 5), 1-based cells
    igridn = np.concatenate([g[None], son[ind_nbor - 1].astype(np.int64)])

    def gather(idim, ig, idc, ind_coarse):
        """the idim velocity and the distance of one neighbour: cell idc (1..8) of igridn(:, ig) where that oct exists (:370-372,
        :381-383), else the neighbouring father cell at 1.5 dx (:373-375, :384-386)"""
        ih = nco + (idc - 1) * ngm
        grid = igridn[ig, np.arange(len(g))]
        cell = np.where(grid > 0, grid + ih, ind_coarse) - 1
        return uold[1 + idim, cell] / np.maximum(uold[0, cell], smallr), np.where(grid > 0, dx_loc, dx_loc * 1.5)

    divu_loc = np.zeros(len(c))                                       # :393
    for idim in range(3):
        bit = (ind >> idim) & 1
        # the tables iii / jjj (:326-331): the cell across the face in direction idim is cell jjj of the oct itself (iii = 0) when
        # it lies inside the oct, of the left neighbour 2 idim - 1 or the right neighbour 2 idim otherwise
        jjj = (ind ^ (1 << idim)) + 1
        ig1 = np.where(bit == 0, 2 * idim + 1, 0)                     # iii(idim, 1, ind)
        ig2 = np.where(bit == 1, 2 * idim + 2, 0)                     # iii(idim, 2, ind)
        velg, dx_g = gather(idim, ig1, jjj, ind_nbor[2 * idim])       # :367-377
        veld, dx_d = gather(idim, ig2, jjj, ind_nbor[2 * idim + 1])   # :378-388
        divu_loc = divu_loc + (veld - velg) / (dx_g + dx_d)           # :396-397
    d, ekin = _kinetic(uold, c, smallr)
    eold = uold[4, c] - ekin                                          # :405-410
    enew[c] = enew[c] - (gamma - 1.0) * eold * divu_loc * dt          # :417-418
    return c, divu_loc


def pdv_cell_loop(T, cell, uold, enew_before, dx_loc, dt, gamma, smallr):
    """the same for ONE cell (0-based) with plain Python scalars: the brute-force check of pdv_numpy's index arithmetic"""
    ngm, nco, son, nbor = T["ngridmax"], T["ncoarse"], T["son"], T["nbor"]
    ind, g = divmod(int(cell) - nco, ngm)
    g += 1
    div = 0.0
    for idim in range(3):
        bit = (ind >> idim) & 1
        v, h = [0.0, 0.0], [0.0, 0.0]
        for side in (0, 1):
            if bit != side:                                           # the sibling inside the oct
                cn, h[side] = nco + (ind ^ (1 << idim)) * ngm + g - 1, dx_loc
            else:
                nb = int(nbor[2 * idim + side, g - 1])
                gn = int(son[nb - 1])
                if gn > 0:
                    cn, h[side] = nco + (ind ^ (1 << idim)) * ngm + gn - 1, dx_loc
                else:
                    cn, h[side] = nb - 1, dx_loc * 1.5
            v[side] = float(uold[1 + idim, cn]) / max(float(uold[0, cn]), smallr)
        div = div + (v[1] - v[0]) / (h[0] + h[1])
    d = max(float(uold[0, cell]), smallr)
    u, v_, w = float(uold[1, cell]) / d, float(uold[2, cell]) / d, float(uold[3, cell]) / d
    eold = float(uold[4, cell]) - 0.5 * d * (u * u + v_ * v_ + w * w)
    return float(enew_before[cell]) - (gamma - 1.0) * eold * div * dt


def pfix_switch_numpy(uold, enew, divu, c, dx, dt, beta_fix, hexp, smallr):
    """set_uold's energy switch (hydro/godunov_fine.f90:203-227) on the cells c, after uold = unew; uold[4] is corrected in
    place.  Returns (the cells where it fired, e_cons / d of every cell)"""
    d, e_kin = _kinetic(uold, c, smallr)                              # :207-212
    e_cons = uold[4, c] - e_kin                                       # :218
    e_prim = enew[c]                                                  # :219
    div = np.abs(divu[c]) * dx / dt                                   # :221
    e_trunc = beta_fix * d * np.maximum(div, 3.0 * hexp * dx) ** 2    # :222
    fired = e_cons < e_trunc                                          # :223
    uold[4, c[fired]] = (e_prim + e_kin)[fired]                       # :224
    return fired, e_cons / d


def set_uold_pfix_numpy(oracle, T, octs, uold, unew, divu, enew, f, dx, dt, beta_fix, hexp, gamma, smallr):
    """set_uold of one level with pressure_fix (hydro/godunov_fine.f90:159-228): the gravity source on unew when there is an
    acceleration (the C oracle), the pdV term on enew, the scalar fix and uold = unew, the energy switch.  uold and enew are
    updated in place (unew is left alone).  Returns dict(cells, fired, econs_over_d, divu_loc, before: E before the switch)"""
    c = oct_cells(T, octs)
    ng = gravity_source_oracle(oracle, unew, uold, f, c, dt, smallr) if f is not None else np.ascontiguousarray(unew[:, c])
    c2, divu_loc = pdv_numpy(T, octs, uold, enew, dx, dt, gamma, smallr)
    assert np.array_equal(c, c2)
    uold[:, c] = _set_uold_scalar_fix(np.ascontiguousarray(uold[:, c]), ng, smallr)
    before = uold[4, c].copy()
    fired, eod = pfix_switch_numpy(uold, enew, divu, c, dx, dt, beta_fix, hexp, smallr)
    return dict(cells=c, fired=fired, econs_over_d=eod, divu_loc=divu_loc, before=before)


def hexp_for_share(econs_over_d, dx, beta_fix, share):
    """hexp with beta_fix (3 hexp dx)^2 on the given quantile of e_cons / d: with divu = 0 the switch fires in that share of the cells"""
    return float(np.sqrt(np.quantile(econs_over_d, share) / beta_fix)) / (3.0 * dx)


def set_unew_pfix_numpy(uold, cells, smallr, ncell):
    """what set_unew leaves in divu / enew under pressure_fix (hydro/godunov_fine.f90:71-81) in the cells: divu = 0, enew = E - e_kin"""
    divu, enew = np.zeros(ncell), np.zeros(ncell)
    d, ekin = _kinetic(uold, cells, smallr)
    enew[cells] = uold[4, cells] - ekin
    return divu, enew


def pfix_no_sweep_expected(oracle, T, u, f, lists, smallr, gamma, beta_fix=0.5, share=0.4, dtfac=0.02):
    """set_unew (with pressure_fix) on the full lists of both levels, no sweep, then set_uold with pressure_fix on lists[L+1] and
    on lists[L] (amr_step's order) on the evolving uold, dt = dtfac dx.  divu is zero then, so the switch compares e_cons with
    beta_fix d (3 hexp dx)^2 alone: hexp of each level is chosen from the checker's own e_cons / d (a dry run with hexp = 0) so
    that this lies on their `share` quantile.  Returns dict(uold, enew, divu, enew0: after set_unew, levels: {lev: what
    set_uold_pfix_numpy returns + hexp, dx, dt})"""
    L = T["L"]
    uold, unew = u.copy(), u.copy()
    divu, enew = set_unew_pfix_numpy(uold, T["both"], smallr, T["ncell"])
    out = dict(enew0=enew.copy(), levels={})
    for lev in (L + 1, L):
        octs = lists[lev]
        if len(octs) == 0:
            continue
        dx = 1.0 / 2 ** lev
        dt = dtfac * dx
        dry = set_uold_pfix_numpy(oracle, T, octs, uold.copy(), unew, divu, enew.copy(), f, dx, dt, beta_fix, 0.0, gamma, smallr)
        hexp = hexp_for_share(dry["econs_over_d"], dx, beta_fix, share)
        r = set_uold_pfix_numpy(oracle, T, octs, uold, unew, divu, enew, f, dx, dt, beta_fix, hexp, gamma, smallr)
        r.update(hexp=hexp, dx=dx, dt=dt)
        out["levels"][lev] = r
    out.update(uold=uold, enew=enew, divu=divu)
    return out


def smallc_on_quantile(u, cells, smallr, gamma, q):
    """(smallc on the q quantile of the cells' sound speeds as cmpdt forms them (hydro/godunov_utils.f90:5-120, before its floor),
    the share of the cells whose pressure then takes the floor rho smallc^2 / gamma)"""
    d, ekin = _kinetic(u, cells, smallr)
    c2 = gamma * ((gamma - 1.0) * (u[4, cells] - ekin)) / d
    smallc = float(np.sqrt(np.quantile(c2, q)))
    return smallc, float(((gamma - 1.0) * (u[4, cells] - ekin) < d * (smallc * smallc / gamma)).mean())


_LEVEL_CASES = {}


def level_case(L, order, seed=12):
    """The input of the level-kernel tests, made once per (L, oct order) and left unchanged: the tile tests' tree (level L
    complete, level L+1 in a spherical shell and on the periodic seam; L = 4 keeps the host's oct numbers, L = 6 is laid out in
    tiles), harsh_tree_state with NVAR = 7, an acceleration of N(0, 1) in every cell, and per level the three oct lists every
    routine is called with: 'full' (the level's list in its own order), 'sub' (37 octs drawn from it, in an array of their
    own: 296 cells, one full workgroup and a partial one) and 'none' (ngrid = 0); for courant_fine also 'cold1e-10' and 'cold0.6'
    (below)."""
    key = (L, order, seed)
    if key in _LEVEL_CASES:
        return _LEVEL_CASES[key]
    from ramses_amd import ic
    T = ic.uniform_tree(L, order=order, refine_mask=shell_mask(2 ** L), slack=260000 if L >= 6 else 7)
    rng = np.random.default_rng(seed + 100)
    T["L"] = L
    T["lists"] = {}
    for lev, ig in ((L, T["igrid"]), (L + 1, T["igrid_fine"])):
        ig = np.ascontiguousarray(ig, dtype=np.int32)
        sub = np.ascontiguousarray(ig[np.sort(rng.choice(len(ig), 37, replace=False))])
        T["lists"][lev] = {"full": ig, "sub": sub, "none": np.zeros(0, np.int32), "sorted": np.ascontiguousarray(np.sort(ig))}
    T["cells"] = {lev: oct_cells(T, T["lists"][lev]["full"]) for lev in (L, L + 1)}
    T["both"] = np.concatenate([T["cells"][L], T["cells"][L + 1]])
    u = harsh_tree_state(T, L, seed, nvar=7)
    u.setflags(write=False)
    # courant_fine only: 'cold<smallr>', a list whose time step is set by a cell ON THE PRESSURE FLOOR rho smallc^2 / gamma (smallc on
    # the 0.2 quantile of the sound speeds, T["smallc"][smallr]).  A time step is a minimum over cells, and over the other lists a
    # warm cell sets it.  Here: the oct whose fastest leaf cell (signal speed 3 c + |u| + |v| + |w| with the floors, cmpdt's w) is a
    # floored one, the fastest such oct of the level, and the 36 slowest octs below it -- slow enough for cmpdt's gravity term too
    T["smallc"] = {}
    for smallr in (1e-10, 0.6):
        smallc = T["smallc"][smallr] = smallc_on_quantile(u, T["both"], smallr, 1.4, 0.2)[0]
        for lev in (L, L + 1):
            ig = T["lists"][lev]["full"]
            c = oct_cells(T, ig).reshape(8, len(ig))
            d, ekin = _kinetic(u, c, smallr)
            cs = np.sqrt(np.maximum(1.4 * 0.4 * (u[4, c] - ekin) / d, 0.0))
            w = np.where(T["son"][c] == 0, 3.0 * np.maximum(cs, smallc) + np.abs(u[1:4, c] / d).sum(0), -np.inf)
            W = w.max(axis=0)                                          # the oct's fastest leaf cell
            floored = np.isfinite(W) & (np.take_along_axis(cs, w.argmax(axis=0)[None], 0)[0] < smallc)
            top = int(np.argmax(np.where(floored, W, -np.inf)))
            below = np.nonzero(np.isfinite(W) & (W < W[top]))[0]
            pick = np.concatenate([[top], below[np.argsort(W[below], kind="stable")[:36]]])
            T["lists"][lev]["cold%g" % smallr] = np.ascontiguousarray(ig[np.sort(pick)])
    f = rng.normal(size=(3, T["ncell"]))
    f.setflags(write=False)
    _LEVEL_CASES[key] = (T, u, f)
    return _LEVEL_CASES[key]


def courant_floors_bind(oracle, T, u, f, smallr, courant_factor, gamma=1.4):
    """From the oracle alone, for both levels: over the list 'cold<smallr>' the time step with smallc on the 0.2 quantile differs
    from the one with smallc = 1e-10 (the pressure floor sets it), with an acceleration f it differs from the one without, and over
    one of the two cold lists it differs between smallr = 0.6 and 1e-10 (max(rho, smallr) inside cmpdt).  A kernel that dropped one
    of the three cannot pass the comparisons over these lists.  Returns the figures for printing."""
    L = T["L"]
    other = 0.6 if smallr < 0.1 else 1e-10
    out = []
    for lev in (L + 1, L):
        dx = 1.0 / 2 ** lev

        def dt(kind, smallc, sr, g):
            po = oracle.make_params(smallr=sr, nvar=5, gamma=gamma, smallc=smallc)
            return courant_dt_oracle(oracle, po, u, g, leaf_cells(T, T["lists"][lev][kind]), dx, courant_factor)
        own = "cold%g" % smallr
        a, b = dt(own, T["smallc"][smallr], smallr, f), dt(own, 1e-10, smallr, f)
        assert a != b, (lev, smallr, a)
        if f is not None:
            assert dt(own, T["smallc"][smallr], smallr, None) != a and dt(own, 1e-10, smallr, None) != b, (lev, smallr)
        assert any(dt(k, 1e-10, smallr, f) != dt(k, 1e-10, other, f) for k in ("cold1e-10", "cold0.6")), (lev, smallr)
        out.append("level %d, list %s: dt %.6e with smallc on the 0.2 quantile, %.6e with smallc = 1e-10" % (lev, own, a, b))
    return out


def plant_fast_split_cell(T, u, gamma=1.4):
    """a copy of u with a velocity of 1e3 times the largest of the state in ONE split cell of level L -- a cell of the first oct of
    the 'sub' list, so that it is in the full and in the ragged list (its pressure is kept): courant_fine must not see it.
    Returns (the state, the cell)"""
    L = T["L"]
    c = oct_cells(T, T["lists"][L]["sub"][:1])
    split = c[T["son"][c] > 0]
    if len(split) == 0:                                               # (the first oct with a split cell then)
        c = oct_cells(T, T["lists"][L]["sub"])
        split = c[T["son"][c] > 0]
    cell = int(split[0])
    both = T["both"]
    vmax = float(np.abs(u[1:4, both] / u[0, both]).max())
    out = u.copy()
    eint = out[4, cell] - 0.5 * (out[1:4, cell] ** 2).sum() / out[0, cell]
    out[1, cell] = out[0, cell] * 1e3 * vmax
    out[4, cell] = eint + 0.5 * (out[1:4, cell] ** 2).sum() / out[0, cell]
    return out, cell


# the cases that come after a sweep: name -> (NVAR, solver, slope_type, smallr, (interpol_var, interpol_type))
SWEPT = {"llf-floor": (7, "llf", 1, 0.6, (1, 2)), "hllc": (5, "hllc", 2, 1e-10, (0, 1))}
_SWEEPS = {}


def oracle_sweeps(L, order, which, gamma=1.4, dtfac=0.02):
    """godunov_fine of level L+1 then L of level_case(L, order) with gravity (the order of amr_step, dt = dtfac dx) by the C oracle,
    made once and left unchanged: (unew, divu, enew), the latter two from what set_unew leaves under pressure_fix"""
    key = (L, order, which)
    if key not in _SWEEPS:
        from oracle import pyoracle
        nvar, riemann, slope, smallr, interp = SWEPT[which]
        T, u7, f = level_case(L, order)
        uold = np.ascontiguousarray(u7[:nvar])
        po = pyoracle.make_params(nvar=nvar, gamma=gamma, smallr=smallr, riemann=riemann, slope_type=slope)
        unew = uold.copy()
        divu, enew = set_unew_pfix_numpy(uold, T["both"], smallr, T["ncell"])
        for lev in (L + 1, L):
            dx = 1.0 / 2 ** lev
            pyoracle.godunov_fine_amr(po, T["lists"][lev]["full"], T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], uold, unew,
                                      dx, dtfac * dx, 32, interp[0], interp[1], f=np.ascontiguousarray(f), divu=divu, enew=enew)
        assert np.isfinite(unew[:, T["both"]]).all() and (unew[:, T["both"]] != uold[:, T["both"]]).any(axis=0).mean() > 0.9
        for a in (unew, divu, enew):
            a.setflags(write=False)
        _SWEEPS[key] = (unew, divu, enew)
    return _SWEEPS[key]


def harsh_mhd_brick(nx, ny, nz, seed, gamma=5.0 / 3.0):
    """A super-fast, floored, partly unmagnetised state of the eleven MHD fields on a periodic nx x ny x nz brick (even extents
    >= 4): u[11, nz, ny, nx] = rho, rho u, rho v, rho w, E, the field on the left faces, the field on the right faces.

    rho, velocity and pressure are those of random_brick (blocky pressure jumps over five decades, velocities of sigma 0.7, half
    of the densities below 0.6).  The face fields are the discrete curl of an edge potential (already divided by dx) of N(0, 1)
    times 0.15 where i < nx/2 and 0.8 elsewhere -- plasma beta on either side of 1 -- set to zero in the corner
    [: nz/2 + 1, : ny/2 + 1, : nx/3 + 1], so that the cells [: nz/2, : ny/2, : nx/3] carry B == 0 exactly; div B = 0 to rounding
    and the right faces are the neighbours' left faces bit for bit.  Two features are laid over that:

      * a weak-field block (nz/2 <= k < nz/2 + 2, i < min(4, nx/2), every j) of cold gas above the floor (rho >= 1, p = 0.05 rho)
        moving diagonally at +-4 per component, the signs changing every two cells: several fast speeds in every direction, all
        four sign pairs around the edges (the doubly super-fast corners of the 2-D HLLD solver);
      * where the unmagnetised corner has room for it (nx/3 >= 4, ny/2 >= 3, nz/2 >= 3): a thin flux tube Bx = 1 along the whole
        line j = k = 1, threading a patch [0:3, 0:3, 0:4] of nearly uniform gas (rho = 1, p = 0.1, u = 0.3 to 1e-6, v = w = 0.3)
        whose Alfven speed exceeds its sound speed.  The tube's own cells have v = w = 0, so its field stays purely normal: c_fast
        = c_Alfven there, the degenerate star states of HLLD and Roe's slow = sound speed."""
    assert min(nx, ny, nz) >= 4 and nx % 2 == 0 and ny % 2 == 0 and nz % 2 == 0, "even extents >= 4 (the reference works oct by oct)"
    u5 = random_brick(nx, ny, nz, seed, gamma=gamma)
    rho = u5[0].copy()
    vel = u5[1:4] / rho
    p = (gamma - 1.0) * (u5[4] - 0.5 * rho * (vel ** 2).sum(0))
    rng = np.random.default_rng(seed + 1000)
    shp = (nz, ny, nx)
    amp = np.where(np.arange(nx) < nx // 2, 0.15, 0.8)[None, None, :]
    A = [rng.standard_normal(shp) * amp for _ in range(3)]          # Ax, Ay, Az on the low x-, y-, z-edges of each cell
    for a in A:
        a[: nz // 2 + 1, : ny // 2 + 1, : nx // 3 + 1] = 0.0
    # the cold diagonal block
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    blk = (k >= nz // 2) & (k < nz // 2 + 2) & (i < min(4, nx // 2))
    rho = np.where(blk, np.maximum(rho, 1.0), rho)
    p = np.where(blk, 0.05 * rho, p)
    for d, idx in enumerate((i, j, k)):
        vel[d] = np.where(blk, 4.0 * np.where((idx // 2) % 2 == 0, 1.0, -1.0), vel[d])
    rollp = lambda a, ax: np.roll(a, -1, axis=ax)      # noqa: E731  value at +1 along ax (axes: 0 z, 1 y, 2 x)
    bx = (rollp(A[2], 1) - A[2]) - (rollp(A[1], 0) - A[1])          # on low x faces
    by = (rollp(A[0], 0) - A[0]) - (rollp(A[2], 2) - A[2])          # on low y faces
    bz = (rollp(A[1], 2) - A[1]) - (rollp(A[0], 1) - A[0])          # on low z faces
    if nx // 3 >= 4 and ny // 2 >= 3 and nz // 2 >= 3:
        bx[1, 1, :] += 1.0
        patch = (slice(0, 3), slice(0, 3), slice(0, 4))
        rho[patch] = 1.0 + 1e-6 * rng.uniform(-1, 1, (3, 3, 4))
        p[patch] = 0.1 * (1.0 + 1e-6 * rng.uniform(-1, 1, (3, 3, 4)))
        vel[0][patch] = 0.3 * (1.0 + 1e-6 * rng.uniform(-1, 1, (3, 3, 4)))
        vel[1][patch] = 0.3                            # (gas at rest across an unmagnetised edge is 0 / 0 in the HLLA solver)
        vel[2][patch] = 0.3
        vel[1][1, 1, :] = 0.0
        vel[2][1, 1, :] = 0.0
    u = np.zeros((11,) + shp)
    u[5], u[6], u[7] = bx, by, bz
    u[8], u[9], u[10] = rollp(bx, 2), rollp(by, 1), rollp(bz, 0)
    bc = [0.5 * (u[5 + c] + u[8 + c]) for c in range(3)]
    u[0] = rho
    for c in range(3):
        u[1 + c] = rho * vel[c]
    u[4] = p / (gamma - 1.0) + 0.5 * rho * (vel ** 2).sum(0) + 0.5 * sum(b * b for b in bc)
    return u


def oct_stencils(u):
    """the 6^3 stencils godfine1 gathers around the octs of a periodic brick u[nvar, nz, ny, nx] (even extents), octs in z, y, x
    order: [nvar, 6, 6, 6, nocts] in C order, which is the reference's uin(1:nocts, -1:4, -1:4, -1:4, 1:nvar)"""
    nz, ny, nx = u.shape[1:]
    off = np.arange(-2, 4)
    kk = (2 * np.arange(nz // 2)[:, None] + off) % nz            # [oct][6]
    jj = (2 * np.arange(ny // 2)[:, None] + off) % ny
    ii = (2 * np.arange(nx // 2)[:, None] + off) % nx
    s = u[:, kk[:, None, None, :, None, None], jj[None, :, None, None, :, None], ii[None, None, :, None, None, :]]   # [v][ok][oj][oi][6][6][6]
    s = s.reshape(u.shape[0], -1, 6, 6, 6)
    return np.ascontiguousarray(np.moveaxis(s, 1, -1))


def mhd_brick_shares(u, gamma=5.0 / 3.0, smallr=0.6):
    """what harsh_mhd_brick promises, from the state alone: dict of min p, the shares of cells above the fast speed, above the
    sound speed, with rho < smallr, with plasma beta < 1 and with B == 0 exactly, max |div B| (field units: dx = 1) and whether
    the right faces are the neighbours' left faces bit for bit"""
    rho = u[0]
    v2 = (u[1:4] ** 2).sum(0) / rho ** 2
    bc = 0.5 * (u[5:8] + u[8:11])
    b2 = (bc ** 2).sum(0)
    p = (gamma - 1.0) * (u[4] - 0.5 * rho * v2 - 0.5 * b2)
    c2 = gamma * p / rho
    fast2 = c2 + b2 / rho                      # the largest fast speed over directions (field across the direction)
    with np.errstate(divide="ignore"):
        beta = np.where(b2 > 0, p / np.where(b2 > 0, 0.5 * b2, 1.0), np.inf)
    div = (u[8] - u[5]) + (u[9] - u[6]) + (u[10] - u[7])
    faces = all(np.array_equal(u[8 + c], np.roll(u[5 + c], -1, axis=ax)) for c, ax in ((0, 2), (1, 1), (2, 0)))
    return dict(pmin=float(p.min()), fast=float((v2 > fast2).mean()), sonic=float((v2 > c2).mean()), low=float((rho < smallr).mean()),
                beta=float((beta < 1).mean()), b0=float(((np.abs(u[5:11]) == 0).all(0)).mean()), divb=float(np.abs(div).max()), faces=faces)


from ramses_amd.ic import _morton_rank, uniform_tree  # noqa: E402,F401  (synthetic trees live with the other synthetic inputs)

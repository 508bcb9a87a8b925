"""Shared test helpers: seeded synthetic states in the brick layout."""
import numpy as np


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
    """the mild state of the AMR tile tests (their _random_state): density in [1, 2), momenta rho (U - 1/2), internal energy in
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

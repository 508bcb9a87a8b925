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


from ramses_amd.ic import _morton_rank, uniform_tree  # noqa: E402,F401  (synthetic trees live with the other synthetic inputs)

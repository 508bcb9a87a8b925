"""numpy restatements of the reference's analytic gravity, in the reference's operation order (IEEE double, one rounding per
operation, no contraction: numpy's elementwise arithmetic): what csrc/gravana_core.hpp and the kernels built on it are held to,
bit for bit.

  gravana           poisson/gravana.f90:27-62, gravity_type 1 and 2
  cell_centres      poisson/force_fine.f90:46-87: x = (xg + xc - skip) * scale
  tree_xg           the oct centres of a synthetic tree (ramses_amd.ic), from the tree alone
  force_ana         force_fine's analytic branch over an oct list (:58-103)
  boundary_force    make_boundary_force's loop over one region as written (poisson/boundary_potential.f90:92-167): chunks of nvector
                    octs, inside a chunk cell index by cell index, gather of the whole chunk before its scatter, in place
"""
import numpy as np

IND_REF = {1: (2, 1, 4, 3, 6, 5, 8, 7), 2: (2, 1, 4, 3, 6, 5, 8, 7), 3: (3, 4, 1, 2, 7, 8, 5, 6), 4: (3, 4, 1, 2, 7, 8, 5, 6),
           5: (5, 6, 7, 8, 1, 2, 3, 4), 6: (5, 6, 7, 8, 1, 2, 3, 4),
           11: (1, 1, 3, 3, 5, 5, 7, 7), 12: (2, 2, 4, 4, 6, 6, 8, 8), 13: (1, 2, 1, 2, 5, 6, 5, 6), 14: (3, 4, 3, 4, 7, 8, 7, 8),
           15: (1, 2, 3, 4, 1, 2, 3, 4), 16: (5, 6, 7, 8, 5, 6, 7, 8)}
for _k in range(1, 7):
    IND_REF[20 + _k] = IND_REF[10 + _k]
INBOR = {1: 2, 2: 1, 3: 4, 4: 3, 5: 6, 6: 5}


def gravana(gtype, params, x):
    """x[3, n] (user units) -> (f[3, n], rr[n]); rr is None for gravity_type 1"""
    x = np.asarray(x, dtype=np.float64)
    p = [float(v) for v in params]
    if gtype == 1:
        return np.stack([np.full(x.shape[1], p[d]) for d in range(3)]), None
    assert gtype == 2
    gmass, emass = p[0], p[1]
    rx, ry, rz = x[0] - p[2], x[1] - p[3], x[2] - p[4]
    rr = np.sqrt(rx * rx + ry * ry + rz * rz + emass * emass)
    r3 = rr * rr * rr
    return np.stack([-gmass * rx / r3, -gmass * ry / r3, -gmass * rz / r3]), rr


def cell_centres(xg, ind, dx, skip, scale):
    """xg[3, n] oct centres (code units), ind 0..7 (scalar or [n]) -> x[3, n] in user units"""
    ind = np.asarray(ind)
    return np.stack([(xg[d] + (((ind >> d) & 1).astype(np.float64) - 0.5) * dx - float(skip[d])) * float(scale) for d in range(3)])


def tree_xg(T, grid=(1, 1, 1)):
    """xg[3, ngridmax] of every oct of the tree (zero where there is none), walking son() down from the coarse cells: coarse
    cell (i, j, k) = 1 + i + nx j + nx ny k has its centre at (i + 0.5, j + 0.5, k + 0.5)"""
    nx, ny, nz = grid
    ncoarse, ngm, son = T["ncoarse"], T["ngridmax"], T["son"]
    assert ncoarse == nx * ny * nz
    xg = np.zeros((3, ngm))
    c = np.arange(ncoarse)
    cells = c                                                    # 0-based cell indices of the level above
    centre = np.stack([c % nx + 0.5, (c // nx) % ny + 0.5, c // (nx * ny) + 0.5])
    dx = 1.0
    while cells.size:
        g = son[cells].astype(np.int64)
        has = g > 0
        g, centre = g[has], centre[:, has]
        if g.size == 0:
            break
        xg[:, g - 1] = centre
        dx *= 0.5
        nxt, ctr = [], []
        for ind in range(8):
            nxt.append(ncoarse + ind * ngm + g - 1)
            ctr.append(np.stack([centre[d] + (((ind >> d) & 1) - 0.5) * dx for d in range(3)]))
        cells, centre = np.concatenate(nxt), np.concatenate(ctr, axis=1)
    return xg


def force_ana(T, xg, f, octs, gtype, params, dx, skip, scale):
    """f[3, ncell] with the cells of the listed octs replaced by gravana at their centres (a copy)"""
    out = f.copy()
    g = np.asarray(octs, dtype=np.int64)
    for ind in range(8):
        cells = T["ncoarse"] + ind * T["ngridmax"] + g - 1
        out[:, cells] = gravana(gtype, params, cell_centres(xg[:, g - 1], ind, dx, skip, scale))[0]
    return out


def boundary_force(f, son, nbor, ncoarse, ngridmax, btype, octs, nvector, gravity=None, xg=None, dx=None):
    """one region of make_boundary_force, in place on f[3, ncell]; gravity = (gtype, params, skip, scale) for imposed regions"""
    bdir, kind = btype % 10, btype // 10
    inbor, axis = INBOR[bdir], (bdir - 1) // 2
    octs = [int(g) for g in octs]
    for s in range(0, len(octs), nvector):
        chunk = np.array(octs[s:s + nvector], dtype=np.int64)
        ref = son[nbor[inbor - 1, chunk - 1].astype(np.int64) - 1].astype(np.int64)
        for ind in range(1, 9):
            cells = ncoarse + (ind - 1) * ngridmax + chunk - 1
            if kind != 2:
                cref = ncoarse + (IND_REF[btype][ind - 1] - 1) * ngridmax + ref - 1
                ff = f[:, cref].copy()
                if kind == 0:
                    ff[axis] = ff[axis] * -1.0
            else:
                gtype, params, skip, scale = gravity
                ff = gravana(gtype, params, cell_centres(xg[:, chunk - 1], ind - 1, dx, skip, scale))[0]
            f[:, cells] = ff


def matches(gtype, params, x, f):
    """per cell: does f[:, i] equal gravana at x[:, i] bit for bit?"""
    want = gravana(gtype, params, x)[0]
    return (want.view(np.int64) == np.asarray(f, dtype=np.float64).view(np.int64)).all(axis=0)

"""ramses_amd.ic.coarse_grid_tree: the test trees of a box whose coarse grid has several cells (walls, elongated periodic boxes),
pinned without a GPU.  An elongated periodic box (2, 1, 1) whose state is a (1, 1, 1) periodic state repeated twice in x is, to
every oct, the (1, 1, 1) box: the oracle's godunov_fine (oracle/amr_godfine_oracle.c, which moves through nbor / father / son
only) must give the (1, 1, 1) result in each half bit for bit -- across the seam between the two coarse cells and across the
periodic ends, which only holds if nbor of the level-1 octs points to the neighbouring coarse cell (amr/init_amr.f90) and every
level below inherits it."""
import numpy as np
import pytest

L = 4
NVEC = 4096         # >= every list here: one batch, so the order of the corrections a coarse cell receives is (direction, side) alone


def _mask1():
    n = 2 ** L
    z, y, x = np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij")
    m = (np.abs(x - 7.5) < 3) & (np.abs(y - 6.5) < 4) & (np.abs(z - 8.5) < 3)
    m[3:6, 2:5, :3] = True           # refined cells on both sides of the x seam
    m[3:6, 2:5, n - 2:] = True
    m[0, 0, 5:8] = True              # and on the y / z seam
    return m


def _neighbour_oct(T, g, d):
    """the oct on side d of oct g (same level), 0: none"""
    c = T["nbor"][d, g - 1]
    return np.where(c > 0, T["son"][np.maximum(c, 1) - 1], 0)


@pytest.mark.parametrize("order", ["scrambled", "morton"])
def test_one_coarse_cell_reproduces_uniform_tree(order):
    from ramses_amd import ic
    m = _mask1()
    A = ic.uniform_tree(L, order=order, refine_mask=m, slack=11)
    B = ic.coarse_grid_tree((1, 1, 1), L, order=order, refine_mask=m, slack=11)
    for k in ("son", "nbor", "father", "igrid", "igrid_fine"):
        assert np.array_equal(A[k], B[k]), k
    assert (A["ncoarse"], A["ngridmax"], A["ncell"]) == (B["ncoarse"], B["ngridmax"], B["ncell"])


@pytest.mark.parametrize("grid", [(2, 1, 1), (3, 1, 1), (1, 3, 2), (3, 3, 3)])
def test_nbor_is_an_involution_across_coarse_cells(grid):
    """the oct on side d of the oct on side d^1 of g is g, on every level, and the coarse cells' own indices follow
    1 + i + nx j + nx ny k"""
    from ramses_amd import ic
    nx, ny, nz = grid
    n = 2 ** 3
    rng = np.random.default_rng(1)
    mask = rng.random((nz * n, ny * n, nx * n)) < 0.2
    T = ic.coarse_grid_tree(grid, 3, order="scrambled", refine_mask=mask)
    assert T["ncoarse"] == nx * ny * nz
    # level 1: the oct of coarse cell (i, j, k), its father and its neighbours in coarse-cell indices
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                c = 1 + i + nx * j + nx * ny * k
                g = T["son"][c - 1]
                assert g > 0 and T["father"][g - 1] == c and g == T["oct_ids"][1][k, j, i]
                want = [1 + (i - 1) % nx + nx * j + nx * ny * k, 1 + (i + 1) % nx + nx * j + nx * ny * k,
                        1 + i + nx * ((j - 1) % ny) + nx * ny * k, 1 + i + nx * ((j + 1) % ny) + nx * ny * k,
                        1 + i + nx * j + nx * ny * ((k - 1) % nz), 1 + i + nx * j + nx * ny * ((k + 1) % nz)]
                assert list(T["nbor"][:, g - 1]) == want
    for l in (1, 2, 3):
        g = T["oct_ids"][l].reshape(-1)
        for d in range(6):
            nb = _neighbour_oct(T, g, d)
            assert (nb > 0).all()                      # complete levels: every neighbour exists
            assert np.array_equal(_neighbour_oct(T, nb, d ^ 1), g)
    # level L+1 (partial): where the neighbour oct exists, it points back; the father cell's son is the oct
    g = T["fine_ids"]
    assert np.array_equal(T["son"][T["father"][g - 1] - 1], g)
    some = 0
    for d in range(6):
        nb = _neighbour_oct(T, g, d)
        have = nb > 0
        some += int(have.sum())
        assert np.array_equal(_neighbour_oct(T, nb[have], d ^ 1), g[have])
    assert some > 0
    # every oct is reachable exactly once
    allocts = np.concatenate([T["oct_ids"][l].reshape(-1) for l in (1, 2, 3)] + [g])
    assert len(np.unique(allocts)) == len(allocts) and allocts.max() <= T["ngridmax"]


@pytest.mark.parametrize("order,riemann,slope,grav", [("scrambled", "hllc", 1, False), ("morton", "llf", 2, True)])
def test_an_elongated_periodic_box_is_the_one_cell_box_twice(oracle, order, riemann, slope, grav):
    from ramses_amd import ic
    n = 2 ** L
    m1 = _mask1()
    T1 = ic.coarse_grid_tree((1, 1, 1), L, order=order, refine_mask=m1)
    T2 = ic.coarse_grid_tree((2, 1, 1), L, order=order, refine_mask=np.concatenate([m1, m1], axis=2))
    assert T2["ncoarse"] == 2
    rng = np.random.default_rng(3)
    nvar = 5
    u1 = np.zeros((nvar, T1["ncell"]))
    u1[0] = 1.0 + rng.random(T1["ncell"])
    for d in (1, 2, 3):
        u1[d] = u1[0] * (rng.random(T1["ncell"]) - 0.5)
    u1[4] = 1.0 + rng.random(T1["ncell"]) + 0.5 * (u1[1] ** 2 + u1[2] ** 2 + u1[3] ** 2) / u1[0]
    f1 = rng.normal(size=(3, T1["ncell"])) if grav else None
    # the same state twice in x, level by level (cells the trees do not hold stay zero on both sides)
    u2 = np.zeros((nvar, T2["ncell"]))
    f2 = np.zeros((3, T2["ncell"])) if grav else None
    pairs = []                                              # (cells of tree 2, cells of tree 1) per level and half
    for l in range(0, L + 2):
        nl = 2 ** l
        z, y, x = (a.reshape(-1) for a in np.meshgrid(np.arange(nl), np.arange(nl), np.arange(nl), indexing="ij"))
        c1 = T1["cell_of"](l, x, y, z)
        for half in (0, 1):
            c2 = T2["cell_of"](l, x + half * nl, y, z)
            assert np.array_equal(c1 > 0, c2 > 0)
            have = c1 > 0
            pairs.append((l, half, c2[have] - 1, c1[have] - 1))
            u2[:, c2[have] - 1] = u1[:, c1[have] - 1]
            if grav:
                f2[:, c2[have] - 1] = f1[:, c1[have] - 1]
    po = oracle.make_params(riemann=riemann, slope_type=slope)

    def step(T, u, f):
        unew = u.copy()
        for lev, ig in ((L + 1, T["igrid_fine"]), (L, T["igrid"])):
            dx = 1.0 / 2 ** lev
            oracle.godunov_fine_amr(po, ig, T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], u, unew, dx, 0.02 * dx, NVEC, 1, 2, f=f)
        return unew
    r1, r2 = step(T1, u1, f1), step(T2, u2, f2)
    changed = total = 0
    for l, half, c2, c1 in pairs:
        assert np.array_equal(r2[:, c2].view(np.int64), r1[:, c1].view(np.int64)), (l, half, np.abs(r2[:, c2] - r1[:, c1]).max())
        if l >= L:
            leaf = T1["son"][c1] == 0
            changed += int((r1[:, c1[leaf]] != u1[:, c1[leaf]]).any(0).sum())
            total += int(leaf.sum())
    assert total > n ** 3 and changed > 0.9 * total           # (the leaf cells of levels L and L+1, in both halves)

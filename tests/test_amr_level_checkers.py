"""What tests/test_amr_level_kernels_gpu.py relies on, asserted from its checkers alone (no GPU): the inputs make every branch the
GPU comparisons are there for bind, so a pass on the device cannot be a vacuous one; and the numpy restatement of the pdV term
equals a brute-force per-cell loop.  Everything on the L = 4 tree (512 + 640 octs, 9857 cells), both oct orders."""
import numpy as np
import pytest

import helpers as H

L = 4
GAMMA = 1.4
FLOOR = 0.6
ORDERS = ("scrambled", "morton")


@pytest.mark.parametrize("order", ORDERS)
def test_the_tree_and_the_state_are_what_the_cases_need(order):
    T, u, f = H.level_case(L, order)
    assert T["ncell"] == 9857
    full = {lev: T["lists"][lev]["full"] for lev in (L, L + 1)}
    assert len(full[L]) == 512 and len(full[L + 1]) == 640
    leaves = (T["son"][T["cells"][L]] == 0).mean()
    assert abs(leaves - 0.844) < 1e-3, leaves
    assert (T["son"][T["cells"][L + 1]] == 0).all()
    assert H.coarser_faces(T, full[L + 1]) == 3888 and H.coarser_faces(T, full[L]) == 0
    mach, low = H.tree_state_shares(T, L, u, FLOOR)
    print("share of cells above Mach 1 %.3f, below a density of %.1f: %.3f" % (mach, FLOOR, low))
    assert abs(mach - 0.66) < 0.01 and abs(low - 0.66) < 0.01
    for lev in (L, L + 1):
        sub = T["lists"][lev]["sub"]
        assert len(sub) == 37 and len(np.unique(sub)) == 37 and np.isin(sub, full[lev]).all()
        assert sub.base is None or sub.base is not full[lev]           # an array of its own (the list cache fingerprints the pointer)
        assert len(T["lists"][lev]["none"]) == 0
    sub_split = (T["son"][H.oct_cells(T, T["lists"][L]["sub"])] > 0).sum()
    assert sub_split >= 8, sub_split                                   # the ragged list has split cells too


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("smallr", [1e-10, FLOOR])
def test_courant_checker_sees_split_cells_gravity_and_the_pressure_floor(oracle, order, smallr):
    T, u0, f = H.level_case(L, order)
    u, cell = H.plant_fast_split_cell(T, u0)
    assert T["son"][cell] > 0 and (u[:, np.arange(T["ncell"]) != cell] == u0[:, np.arange(T["ncell"]) != cell]).all()
    dx, cf = 1.0 / 2 ** L, 0.8
    po = oracle.make_params(smallr=smallr, nvar=5)
    for kind in ("full", "sub"):
        octs = T["lists"][L][kind]
        assert cell in H.oct_cells(T, octs)
        dt_leaf = H.courant_dt_oracle(oracle, po, u, f, H.leaf_cells(T, octs), dx, cf)
        dt_all = H.courant_dt_oracle(oracle, po, u, f, H.oct_cells(T, octs), dx, cf)
        dt_nograv = H.courant_dt_oracle(oracle, po, u, None, H.leaf_cells(T, octs), dx, cf)
        print("%s list: dt over the leaves %.6e, over all cells %.6e, leaves without gravity %.6e" % (kind, dt_leaf, dt_all, dt_nograv))
        assert dt_all < dt_leaf                                        # a split cell entering the minimum would show
        assert dt_nograv != dt_leaf                                    # so would a missing acceleration
    # smallc on the 0.2 quantile of the sound speeds: the pressure floor binds in a fifth of the cells.  Over the full and the
    # ragged list that does NOT move dt (a warm, fast cell sets the minimum, and no floor touches it); over the 'cold' lists it
    # does, and so do smallr and the acceleration -- with and without gravity
    smallc, share = H.smallc_on_quantile(u0, T["both"], smallr, GAMMA, 0.2)
    assert smallc == T["smallc"][smallr] and abs(share - 0.2) < 0.01, share
    for g in (f, None):
        print("\n".join(H.courant_floors_bind(oracle, T, u, g, smallr, cf, GAMMA)))
    for lev in (L, L + 1):
        cold = T["lists"][lev]["cold%g" % smallr]
        assert 8 <= len(cold) <= 37 and len(np.unique(cold)) == len(cold) and np.isin(cold, T["lists"][lev]["full"]).all()
    leaves = H.leaf_cells(T, T["lists"][L]["full"])
    # the floor of the density enters the internal-energy sum
    if smallr == FLOOR:
        a = H.fsum_bound(H.courant_sum_terms(u, leaves, dx, smallr)[2])
        b = H.fsum_bound(H.courant_sum_terms(u, leaves, dx, 1e-10)[2])
        assert abs(a[0] - b[0]) > 1e3 * (a[1] + b[1])


@pytest.mark.parametrize("order", ORDERS)
def test_upl_checker_depends_on_interpol_var_and_on_the_floor(oracle, order):
    T, u, f = H.level_case(L, order)
    octs = T["lists"][L]["full"]
    res = {iv: H.upl_oracle(oracle, T, u, octs, iv, 1e-10) for iv in (0, 1, 2)}
    split = res[0][1]
    assert len(split) == 640
    # interpol_var 1 and 2 restrict alike (one branch, hydro/interpol_hydro.f90:207; they differ in the interpolation only), and
    # both differ from 0
    assert np.array_equal(res[1][0], res[2][0])
    d01 = (res[0][0][4, split] != res[1][0][4, split]).mean()
    d02 = (res[0][0][4, split] != res[2][0][4, split]).mean()
    print("split cells whose restricted energy differs between interpol_var 0 and 1: %.3f, 0 and 2: %.3f" % (d01, d02))
    assert d01 > 0.5 and d02 > 0.5
    floored = H.upl_oracle(oracle, T, u, octs, 0, FLOOR)[0]
    n = int((floored[0, split] != res[0][0][0, split]).sum())
    print("split cells whose restricted density the floor of %.1f changes: %d of %d" % (FLOOR, n, len(split)))
    assert n > 0
    leaves = H.leaf_cells(T, octs)
    assert np.array_equal(floored[:, leaves], u[:, leaves])
    # level L+1 has no split cell: nothing to do
    out, none = H.upl_oracle(oracle, T, u, T["lists"][L + 1]["full"], 1, FLOOR)
    assert len(none) == 0 and np.array_equal(out, u)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("smallr", [1e-10, FLOOR])
@pytest.mark.parametrize("grav", [False, True])
def test_pfix_checker_without_a_sweep_fires_in_two_fifths_of_the_cells(oracle, order, smallr, grav):
    T, u, f = H.level_case(L, order)
    R = H.pfix_no_sweep_expected(oracle, T, u, f if grav else None, {lev: T["lists"][lev]["full"] for lev in (L + 1, L)}, smallr, GAMMA)
    for lev in (L + 1, L):
        r = R["levels"][lev]
        share = r["fired"].mean()
        c = r["cells"]
        changed = R["uold"][4, c[r["fired"]]] != r["before"][r["fired"]]
        rel = np.abs(R["uold"][4, c[r["fired"]]] / r["before"][r["fired"]] - 1.0)
        dt = 0.02 / 2 ** lev
        print("level %d: hexp %.4f, fired share %.3f, median relative change of the fired cells' energy %.2e, max |div u| dt %.3f, "
              "smallest enew %.3e" % (lev, r["hexp"], share, np.median(rel), np.abs(r["divu_loc"]).max() * dt, R["enew"][c].min()))
        assert 0.2 < share < 0.6, share
        assert changed.all()
        assert np.abs(r["divu_loc"]).max() * dt <= 0.07
        assert R["enew"][c].min() > 0
    assert H.coarser_faces(T, T["lists"][L + 1]["full"]) > 0        # the 1.5 dx branch


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("which", sorted(H.SWEPT))
def test_pfix_checker_after_a_sweep_fires_somewhere_and_not_everywhere(oracle, order, which):
    nvar, riemann, slope, smallr, interp = H.SWEPT[which]
    T, u7, f = H.level_case(L, order)
    unew, divu, enew = H.oracle_sweeps(L, order, which)
    uold, enew = np.ascontiguousarray(u7[:nvar]).copy(), enew.copy()
    cells = T["both"]
    assert (divu[cells] != 0).mean() > 0.7
    for lev in (L + 1, L):
        dx = 1.0 / 2 ** lev
        before = uold.copy()
        r = H.set_uold_pfix_numpy(oracle, T, T["lists"][lev]["full"], uold, unew, divu, enew, f, dx, 0.02 * dx, 0.5, 0.0, GAMMA, smallr)
        share = r["fired"].mean()
        print("%s, level %d: the switch fires in %.3f of the cells" % (which, lev, share))
        assert 0 < share < 1
        if nvar > 5 and smallr == FLOOR:
            c = r["cells"]
            unfixed = H.gravity_source_oracle(oracle, unew, before, f, c, 0.02 * dx, smallr)
            fixed = int((uold[5:, c] != unfixed[5:]).any(axis=0).sum())
            print("level %d: cells whose passive scalars set_uold's floor fix changes: %d of %d" % (lev, fixed, len(c)))
            assert fixed > 0.1 * len(c)
    assert np.isfinite(uold[:, cells]).all()


@pytest.mark.parametrize("order", ORDERS)
def test_pdv_checker_equals_a_per_cell_loop(order):
    T, u, f = H.level_case(L, order)
    rng = np.random.default_rng(3)
    for smallr in (1e-10, FLOOR):
        for lev in (L + 1, L):
            dx = 1.0 / 2 ** lev
            dt = 0.02 * dx
            e0 = rng.uniform(0.5, 2.0, T["ncell"])
            enew = e0.copy()
            c, _ = H.pdv_numpy(T, T["lists"][lev]["full"], u, enew, dx, dt, GAMMA, smallr)
            other = np.setdiff1d(np.arange(T["ncell"]), c)
            assert np.array_equal(enew[other], e0[other]) and (enew[c] != e0[c]).all()
            for cell in rng.choice(c, 100, replace=False):
                assert enew[cell] == H.pdv_cell_loop(T, cell, u, e0, dx, dt, GAMMA, smallr), (lev, cell)

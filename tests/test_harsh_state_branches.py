"""The harsh state of tests/helpers.py (harsh_tree_state) reaches every data-dependent branch of the oracle's slopes, trace, Riemann
solvers and cmpdivu / consup -- measured with gcov on a copy of the oracle built with `gcc -O0 --coverage`
(scripts/oracle_branch_coverage.py; host code, no GPU).  That is what makes tests/test_amr_harsh_states_gpu.py a test of the
supersonic and floored paths of the AMR kernels: where the oracle does not go, a comparison with it says nothing.  The mild state
of the other AMR tests leaves those branches untaken (profiles/harsh_state_branches.txt holds both lists side by side)."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

from helpers import harsh_tree_state, shell_mask, tree_cell_kind, tree_state_shares

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location("oracle_branch_coverage", os.path.join(ROOT, "scripts", "oracle_branch_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def coverage():
    if shutil.which("gcov") is None or shutil.which("gcc") is None:
        pytest.skip("gcov not installed")
    cov = _script()
    return cov, {state: cov.never_taken(state, level=4) for state in ("harsh", "mild")}


def _open_physics(cov, res):
    return [(name, func, ln, what, text) for name, rows in res.items() for func, ln, text, what, why in rows
            if why is None and func in cov.PHYSICS]


def test_harsh_state_takes_every_branch_of_the_slopes_the_trace_and_the_solvers(coverage):
    cov, res = coverage
    left = _open_physics(cov, res["harsh"])
    assert not left, "\n".join("%s %s:%d %s: %s" % r for r in left)
    # the allow-list is short and about the dimension, the 1-D slopes, the Newton bound and the abort()s only
    reasons = {why for rows in res["harsh"].values() for func, ln, text, what, why in rows if why is not None and func in cov.PHYSICS}
    assert reasons <= {w for _, w in cov.ALLOWED} | {"the 1-D slope types 4-6"}


def test_mild_state_leaves_the_supersonic_and_floored_branches_untaken(coverage):
    """(why the harsh state exists: were this to fail, the mild state would have become as good and the record out of date)"""
    cov, res = coverage
    left = {(func, text) for _, func, _, _, text in _open_physics(cov, res["mild"])}
    funcs = {f for f, _ in left}
    assert {"riemann_hllc", "riemann_acoustic", "ora_trace", "ora_trace_plmde"} <= funcs, sorted(left)
    assert any("SL > 0.0" in t for _, t in left) and any("v < p->smallr" in t for _, t in left)


def test_the_committed_record_says_the_same(coverage):
    """profiles/harsh_state_branches.txt is the script's output for both states: the same open branches of the physics functions,
    by function and source text, as a run now finds -- some for the mild state, none for the harsh one"""
    cov, res = coverage
    with open(os.path.join(ROOT, "profiles", "harsh_state_branches.txt")) as fh:
        record = fh.read().split("\n")
    tail = " of them in the slope / trace / Riemann / cmpdivu / consup functions"
    starts = {state: record.index([s for s in record if s.startswith("== %s state" % state)][0]) for state in ("mild", "harsh")}
    assert starts["mild"] < starts["harsh"]
    for state, lo, hi in (("mild", starts["mild"], starts["harsh"]), ("harsh", starts["harsh"], len(record))):
        rows = [s.split() for s in record[lo:hi] if " OPEN " in s]
        filed = {(r[1], " ".join(r[r.index("OPEN") + 1:])) for r in rows if r[1] in cov.PHYSICS}
        live = {(func, " ".join(text.split())) for _, func, _, _, text in _open_physics(cov, res[state])}
        assert filed == live, (state, sorted(filed ^ live))
        summary = [s for s in record[lo:hi] if s.startswith("-- %s: " % state) and s.endswith(tail)]
        assert len(summary) == 1 and summary[0].endswith(", %d%s" % (len(_open_physics(cov, res[state])), tail))
    assert not _open_physics(cov, res["harsh"]) and _open_physics(cov, res["mild"])


@pytest.mark.parametrize("level", [4, 5])
def test_harsh_state_on_a_small_tree(oracle, level):
    """the state's own promises on the trees the coverage run uses: positive pressure everywhere, more than 0.3 of the cells above
    Mach 1, between 0.3 and 0.7 of them below a floor of 0.6, NVAR only adds variables, the level-(L+1) cells stay within
    [0.9, 1.1] of their father cell's density, and the oracle's step from it is finite and changes more than 0.9 of the cells"""
    cov = _script()
    from ramses_amd import ic
    L = level
    T = ic.uniform_tree(L, order="scrambled", refine_mask=shell_mask(2 ** L), slack=7)
    u7, u5 = harsh_tree_state(T, L, cov.SEED, nvar=7), harsh_tree_state(T, L, cov.SEED, nvar=5)
    assert np.array_equal(u7[:5], u5) and np.array_equal(u5[:, 0], u5[:, 1])
    eint = u5[4] - 0.5 * (u5[1:4] ** 2).sum(0) / u5[0]
    assert (u5[0] > 0).all() and (eint > 0).all() and (u7[5:] >= 0).all() and (u7[5:] <= u7[0]).all()
    mach, low = tree_state_shares(T, L, u5, 0.6)
    assert mach > 0.3 and 0.3 < low < 0.7, (mach, low)
    fine = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + T["igrid_fine"].astype(np.int64) - 1 for ind in range(8)])
    ratio = u5[0, fine] / np.tile(u5[0, T["father"][T["igrid_fine"] - 1].astype(np.int64) - 1], 8)
    assert 0.9 <= ratio.min() < 0.91 and 1.09 < ratio.max() <= 1.1
    cells = np.concatenate([fine] + [T["ncoarse"] + ind * T["ngridmax"] + T["igrid"].astype(np.int64) - 1 for ind in range(8)])
    po = oracle.make_params(riemann="hllc", slope_type=2, smallr=0.6)
    unew = u5.copy()
    for lev, ig in ((L + 1, T["igrid_fine"]), (L, T["igrid"])):
        dx = 1.0 / 2 ** lev
        oracle.godunov_fine_amr(po, ig, T["son"], T["nbor"], T["father"], T["ngridmax"], T["ncoarse"], u5, unew, dx, 0.02 * dx, 32, 1, 2)
    assert np.isfinite(unew[:, cells]).all() and (unew[0, cells] > 0).all()
    assert (unew[:, cells] != u5[:, cells]).any(axis=0).mean() > 0.9


def test_every_kind_of_cell_is_told_apart():
    """tree_cell_kind (the report of a difference in tests/test_amr_harsh_states_gpu.py) on the level-4 tree: all five kinds occur"""
    from ramses_amd import ic
    T = ic.uniform_tree(4, order="scrambled", refine_mask=shell_mask(16), slack=7)
    cells = np.concatenate([T["ncoarse"] + ind * T["ngridmax"] + np.concatenate([T["igrid"], T["igrid_fine"]]).astype(np.int64) - 1 for ind in range(8)])
    kinds = {tree_cell_kind(T, 4, c).split(", ", 1)[0].split(" of ")[1] + ": " + tree_cell_kind(T, 4, c).split(", ", 1)[1].split(" (")[0] for c in cells[::7]}
    assert kinds == {"level 4: refined cell", "level 4: interior", "level 4: coarse leaf corrected by level 5",
                     "level 5: interior", "level 5: ghost-adjacent"}, kinds

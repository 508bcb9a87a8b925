"""The harsh MHD state of tests/helpers.py (harsh_mhd_brick) reaches every data-dependent branch of the product's MHD headers
(ramses_amd/csrc/mhd_core.hpp, mhd_assemble.hpp: slopes, trace, the 1-D and 2-D Riemann solvers) -- measured with gcov on
tests/native/mhd_host_check.cpp built with `g++ -O0 --coverage` (scripts/mhd_branch_coverage.py; host code, no GPU, no reference).
That is what makes the "harsh" kind of tests/test_mhd_core_host.py a test of the super-fast, degenerate and floored paths: where the input does not go, a comparison says nothing.  The smooth and jump stencils of the host
test leave those branches untaken (profiles/mhd_harsh_state_branches.txt holds both lists side by side)."""
import importlib.util
import os
import shutil

import numpy as np
import pytest

from helpers import harsh_mhd_brick, mhd_brick_shares, oct_stencils

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(4, 4, 4), (8, 8, 8), (38, 10, 6), (12, 18, 10), (70, 6, 12), (6, 4, 20)]       # cubes of levels 2 and 3, and bricks with partial tiles, slabs and groups


def _script():
    spec = importlib.util.spec_from_file_location("mhd_branch_coverage", os.path.join(ROOT, "scripts", "mhd_branch_coverage.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def coverage():
    if shutil.which("gcov") is None or shutil.which("g++") is None:
        pytest.skip("gcov not installed")
    cov = _script()
    return cov, {state: cov.never_taken(state) for state in ("harsh", "tests")}


def _open_physics(cov, res):
    return [(name, func, ln, what, text) for name, rows in res.items() for func, ln, text, what, why in rows
            if why is None and func in cov.PHYSICS]


def test_harsh_state_takes_every_branch_of_the_slopes_the_trace_and_the_solvers(coverage):
    cov, res = coverage
    left = _open_physics(cov, res["harsh"])
    assert not left, "\n".join("%s %s:%d %s: %s" % r for r in left)
    # nothing outside the physics functions either, and the allow-list is short: every entry carries its reason
    assert not [r for rows in res["harsh"].values() for r in rows if r[4] is None]
    assert len(cov.ALLOWED) <= 4 and all(len(why) > 20 for _, why in cov.ALLOWED)
    used = {why for rows in res["harsh"].values() for *_, why in rows if why is not None}
    assert used <= {w for _, w in cov.ALLOWED}
    # the one allow-listed branch of a solver is Roe's exact equality
    assert {text for rows in res["harsh"].values() for func, ln, text, what, why in rows if func in cov.PHYSICS} == \
        {"if ((cfsq - cssq) == 0.0) { alpha_f = 1.0; alpha_s = 0.0; }"}


def test_the_old_stencils_leave_the_super_fast_and_floored_branches_untaken(coverage):
    """(why the harsh state exists: were this to fail, the smooth / jump stencils would have become as good and the record out of date)"""
    cov, res = coverage
    left = {(func, text) for _, func, _, _, text in _open_physics(cov, res["tests"])}
    text_of = lambda f: {t for g, t in left if g == f}      # noqa: E731
    assert "if (s[0] < smallr) s[0] = S.c(0);" in text_of("trace_state")
    assert {"if (SL > 0.0) {", "} else if (SR > 0.0) {"} <= text_of("hlld")
    assert sum("fabs(estar) < (double)1e-4f" in t for t in text_of("hlld")) == 1 and \
        len([1 for rows in res["tests"].values() for func, ln, text, what, why in rows if func == "hlld" and "fabs(estar)" in text]) == 2
    assert {"if (SB > 0.0) {", "} else if (ST < 0.0) {", "} else if (SL > 0.0) {", "} else if (SR < 0.0) {", "if (SL > 0.0) E = ELL;",
            "else if (SR < 0.0) E = ERL;", "if (SL > 0.0) E = ELR;", "else if (SR < 0.0) E = ERR;"} <= text_of("cmp_mag_flx_edge")
    assert "if (cssq <= 0.0) cssq = 0.0;" in text_of("roe_eigenvalues") and "if (cssq <= 0.0) cssq = 0.0;" in text_of("roe_eigen_cons")
    assert {"if (bt == 0.0) {", "else if ((twid_asq - cssq) <= 0.0) { alpha_f = 0.0; alpha_s = 1.0; }",
            "else if ((cfsq - twid_asq) <= 0.0) { alpha_f = 1.0; alpha_s = 0.0; }"} <= text_of("roe_eigen_cons")
    assert {"if (dim <= 0.0 || etm <= 0.0) llf = true;", "if (llf) {"} <= text_of("athena_roe")
    assert any(t.startswith("if (spout < 0.0)") for t in text_of("hydro_acoustic"))


def test_the_committed_record_says_the_same(coverage):
    """profiles/mhd_harsh_state_branches.txt is the script's output for both inputs: the same never-taken branches, by function and
    source text, allowed ones included, as a run now finds -- many for the tests' stencils, none outside the allow-list for the
    harsh state"""
    cov, res = coverage
    with open(os.path.join(ROOT, "profiles", "mhd_harsh_state_branches.txt")) as fh:
        record = fh.read().split("\n")
    tail = " of them in the slope / trace / solver functions"
    starts = {state: record.index([s for s in record if s.startswith("== %s input" % state)][0]) for state in ("tests", "harsh")}
    assert starts["tests"] < starts["harsh"]
    for state, lo, hi in (("tests", starts["tests"], starts["harsh"]), ("harsh", starts["harsh"], len(record))):
        rows = [s.split() for s in record[lo:hi] if s.startswith("mhd_")]
        filed = set()
        for r in rows:
            at = r.index("OPEN") if "OPEN" in r[:7] else r.index("allowed")
            filed.add((r[1], r[at], " ".join(r[at + 1:])))
        live = {(func, "allowed" if why else "OPEN", " ".join(text.split())) for rows_ in res[state].values() for func, ln, text, what, why in rows_}
        assert filed == live, (state, sorted(filed ^ live))
        summary = [s for s in record[lo:hi] if s.startswith("-- %s: " % state) and s.endswith(tail)]
        assert len(summary) == 1 and summary[0].endswith(", %d%s" % (len(_open_physics(cov, res[state])), tail))
    assert not _open_physics(cov, res["harsh"]) and len(_open_physics(cov, res["tests"])) >= 20


@pytest.mark.parametrize("shape", SHAPES)
def test_harsh_mhd_brick_keeps_its_promises(shape):
    """from the state alone, on cubes and non-cubic bricks: positive pressure, more than 0.15 of the cells above the fast speed,
    between 0.3 and 0.7 of the densities below a floor of 0.6, more than 0.3 of the cells with plasma beta < 1, more than 0.05 with
    B == 0 exactly, div B at rounding (field units) and right faces == the neighbours' left faces bit for bit"""
    cov = _script()
    u = harsh_mhd_brick(*shape, seed=cov.SEED)
    nx, ny, nz = shape
    assert u.shape == (11, nz, ny, nx) and np.isfinite(u).all()
    s = mhd_brick_shares(u, smallr=0.6)
    assert s["pmin"] > 0 and (u[0] > 0).all(), s
    assert s["fast"] > 0.15 and 0.3 < s["low"] < 0.7 and s["beta"] > 0.3 and s["b0"] > 0.05, s
    assert s["divb"] <= 1e-13 and s["faces"], s
    assert np.array_equal(u, harsh_mhd_brick(*shape, seed=cov.SEED))                     # seeded
    assert not np.array_equal(u, harsh_mhd_brick(*shape, seed=cov.SEED + 1))


def test_odd_or_tiny_extents_are_refused():
    for shape in ((5, 4, 4), (4, 2, 4), (4, 4, 7)):
        with pytest.raises(AssertionError):
            harsh_mhd_brick(*shape, seed=1)


def test_oct_stencils_are_the_periodic_neighbourhoods_of_the_octs():
    u = harsh_mhd_brick(6, 4, 8, seed=3)
    st = oct_stencils(u)
    assert st.shape == (11, 6, 6, 6, 4 * 2 * 3) and st.flags["C_CONTIGUOUS"]
    off = np.arange(-2, 4)
    for ok, oj, oi in ((0, 0, 0), (3, 1, 2), (2, 0, 1)):
        kk, jj, ii = (2 * ok + off) % 8, (2 * oj + off) % 4, (2 * oi + off) % 6
        assert np.array_equal(st[..., (ok * 2 + oj) * 3 + oi], u[:, kk[:, None, None], jj[None, :, None], ii[None, None, :]])

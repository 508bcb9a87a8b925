"""Live GPU test of the barotropic equation of state on the device (RAMSES_AMD_EOS=1): the patched program against the untouched
reference program (oracle/_ref), level, cell centres and primitive variables of the leaf cells of the last snapshot bit for bit
(live.ab).  The runs are those of tests/golden/make_golden_eos.py -- 16^3 coarse cells, a drifting background of density 1, a cube
of density 20 and a cube of density 0.1 below smallr = 0.3, units whose scale_nH is no power of two, T2c = 4.8 K (a sound speed
squared of 0.04) -- over 6 steps:
  (a) one uniform level 5, hydro only                                         the resident brick
  (b) levels 4-6, self-gravity by multigrid, jeans_refine = 4 on every level  resident AMR levels; must refine to three levels
  (c) levels 4-6, hydro only, gradient criteria, 2 ranks                      resident AMR levels under MPI
  (d) one uniform level 5 on 2 ranks                                          the MPI-resident brick
  (e) levels 4-5, the legacy idiom isothermal=.true., g_star = 1, T2_star     resident AMR levels
  (f) = (b) without the switch: staged as before, none of the lines, still bit-identical
  (g) barotropic_eos_form = 'double_polytrope' with the switch: rank 1 names the form, the run stays staged and bit-identical
With the switch the program must say that the EOS is evaluated on the GPU and that the state stays resident, and its profile must
count calls of 'cooling_fine (device, barotropic)'."""
import re

import pytest

import live

pytestmark = pytest.mark.gpu

NSTEP = 6
ON_GPU = "is evaluated on the GPU"
RESIDENT = {"amr": "AMR levels stay resident on the GPU", "brick": "stays resident on the GPU", "mpibrick": "stays resident on the GPUs (one brick per rank)"}
JEANS = "&REFINE_PARAMS\ninterpol_var=0\ninterpol_type=1\njeans_refine=4.,4.,4.\n/\n"
# case -> (form, levelmin, levelmax, ranks, self-gravity, which residency)
CASES = {
    "a": ("isothermal", 5, 5, 1, False, "brick"),
    "b": ("isothermal", 4, 6, 1, True, "amr"),
    "c": ("isothermal", 4, 6, 2, False, "amr"),
    "d": ("isothermal", 5, 5, 2, False, "mpibrick"),
    "e": ("legacy", 4, 5, 1, False, "amr"),
}
ENV = {"RAMSES_AMD_EOS": "1", "RAMSES_AMD_PROFILE": "1", "RAMSES_AMD_STATS": "1"}


def _namelist(form, lmin, lmax, nproc, gravity):
    mk = live.golden_module("eos")
    kw = {"refine": JEANS} if gravity else {}
    return mk.namelist(form, lmin, lmax, NSTEP, poisson=gravity, ngridtot=60000 * nproc, **kw)


def _said(out, text):
    """text is in the program's output, whatever line breaks list-directed output put into a long message"""
    return re.sub(r"\s+", "", text) in re.sub(r"\s+", "", out)


def _device_calls(out):
    """calls of cooling_fine that ran on the device, summed over the levels and ranks of the profile"""
    return sum(int(n) for n in re.findall(r"cooling_fine \(device, barotropic\)\s+level\s+\d+\s+calls\s+(\d+)", out))


@pytest.mark.parametrize("case", sorted(CASES))
def test_resident_run_with_a_barotropic_eos_equals_the_reference(gpu_lib, case):
    form, lmin, lmax, nproc, gravity, where = CASES[case]
    live.enough_cores(nproc)
    out, want = live.ab(_namelist(form, lmin, lmax, nproc, gravity), nproc, ENV, min_levels=3 if case == "b" else lmax - lmin + 1)
    assert _said(out, "ramses_amd: barotropic EOS (%s) %s" % (form, ON_GPU)), out[-3000:]
    assert _said(out, RESIDENT[where]), out[:3000]
    assert _device_calls(out) > 0, out[-3000:]
    assert re.search(r"cooling_fine \(device, barotropic\): \d+ calls", out), out[-3000:]
    assert not re.search(r"\n\s+cooling_fine\s+level", out), "a call of cooling_fine took the reference's routine"


def test_without_the_switch_nothing_changes(gpu_lib):
    form, lmin, lmax, nproc, gravity, _ = CASES["b"]
    env = dict(ENV, RAMSES_AMD_EOS=None)
    out, _ = live.ab(_namelist(form, lmin, lmax, nproc, gravity), nproc, env, min_levels=3)
    assert ON_GPU not in out and "stay resident" not in out and "stays resident" not in out, out[-3000:]
    assert _device_calls(out) == 0 and "RAMSES_AMD_EOS" not in out


def test_a_form_with_a_power_law_stays_staged_and_says_so(gpu_lib):
    _, lmin, lmax, nproc, gravity, _ = CASES["b"]
    out, _ = live.ab(_namelist("double_polytrope", lmin, lmax, nproc, gravity), nproc, ENV, min_levels=2)
    assert _said(out, "RAMSES_AMD_EOS=1 but barotropic_eos_form='double_polytrope' is not evaluated on the device"), out[-3000:]
    assert ON_GPU not in out and "stay resident" not in out and "stays resident" not in out, out[-3000:]
    assert _device_calls(out) == 0

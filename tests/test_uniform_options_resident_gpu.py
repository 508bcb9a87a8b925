"""GPU tests: a run with ONE uniform level that no brick path carries -- pressure_fix, difmag, several ranks whose domains
are not boxes, nremap > 0 under MPI -- stays device-resident through the AMR path (cell vectors + tree on the GPU, the
tree-walking sweep with its PFIX / DIFMAG branches; ramses_amd_iface: ramses_amd_amr_config) instead of being staged around
every call.  Live against the untouched reference program, leaf cells bit for bit."""
import pytest

import live

pytestmark = pytest.mark.gpu


def _namelist(level, nstep, riemann, slope, opts, poisson=False, nremap=0):
    from oracle import ramses_snapshot as rs
    mka = live.golden_module("amr")
    r = riemann + "'\n" + opts + "\n!'" if opts else riemann
    kw = {"init": mka.SELFGRAV_INIT} if poisson else {}
    extra = "&POISSON_PARAMS\nepsilon=1e-5\n/\n" if poisson else ""
    nml = rs.sedov3d_namelist(level=level, nstepmax=nstep, foutput=nstep, riemann=r, slope_type=slope, extra=extra,
                              poisson=poisson, mem_factor=3.0, **kw)
    return nml.replace("nremap=0", "nremap=%d" % nremap)


def _ab(nml, nproc, env, resident_message=True):
    live.ab(nml, nproc, env, resident_message=resident_message)


@pytest.mark.parametrize("opts,riemann,slope", [
    ("pressure_fix=.true.\nbeta_fix=0.5", "hllc", 1),
    ("difmag=0.1", "llf", 2),
    ("pressure_fix=.true.\nbeta_fix=0.5\ndifmag=0.05", "hll", 1),
], ids=["pressure_fix", "difmag", "both"])
def test_uniform_level_with_options_of_the_tree_walking_sweep_is_resident(gpu_lib, opts, riemann, slope):
    _ab(_namelist(5, 10, riemann, slope, opts), 1, {})


def test_resident_switch_off_keeps_the_staging_path(gpu_lib):
    _ab(_namelist(5, 6, "hllc", 1, "pressure_fix=.true.\nbeta_fix=0.5"), 1, {"RAMSES_AMD_RESIDENT": "0"}, resident_message=False)


def test_uniform_level_with_pressure_fix_and_self_gravity_on_one_rank(gpu_lib):
    _ab(_namelist(5, 4, "llf", 1, "pressure_fix=.true.\nbeta_fix=0.5", poisson=True), 1, {})


@pytest.mark.parametrize("nproc,opts,nremap", [(2, "pressure_fix=.true.\nbeta_fix=0.5", 0), (3, "", 0), (2, "", 2)],
                         ids=["2ranks-pressure_fix", "3ranks-domains-are-not-boxes", "2ranks-nremap"])
def test_uniform_level_under_mpi_without_a_brick_path_is_resident(gpu_lib, nproc, opts, nremap):
    _ab(_namelist(5, 8, "hllc", 1, opts, nremap=nremap), nproc, {})

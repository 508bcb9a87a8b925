// mhd_host.hpp -- what the host sides of the MHD units share (csrc/mhd_sweep.hip: bricks, csrc/mhd_amr.hip: AMR levels):
// the kernels' constants from the parameters of the C ABI.
#pragma once
#include "host_util.hpp"
#include "mhd_core.hpp"

namespace ramses_amd {
namespace mhd {

static inline int make_const(const ramses_amd_mhd_params *p, MhdConst &P) {
  if (!p) return fail(RAMSES_AMD_EINVAL, "params is NULL");
  P.gamma = p->gamma; P.smallr = p->smallr; P.smallc = p->smallc; P.slope_theta = p->slope_theta;
  P.slope_type = p->slope_type;
  P.slope_mag_type = p->slope_mag_type == -1 ? p->slope_type : p->slope_mag_type;      // hydro/read_hydro_params.f90:528-530
  P.riemann = p->riemann; P.riemann2d = p->riemann2d;
  if (!(p->gamma > 1.0)) return fail(RAMSES_AMD_EINVAL, "gamma must be > 1");
  if (!slope_type_supported(P.slope_type) || !slope_mag_type_supported(P.slope_mag_type))
    return fail(RAMSES_AMD_EUNSUPPORTED, "MHD sweep: slope_type 0, 1, 2, 3, 7, 8 and slope_mag_type 0, 1, 2, 7, 8 are on the device (got %d / %d)", P.slope_type, P.slope_mag_type);
  if (!riemann_supported(P.riemann)) return fail(RAMSES_AMD_EINVAL, "MHD sweep: riemann must be 0 (llf) .. 5 (hydro) (got %d)", P.riemann);
  if (!riemann2d_supported(P.riemann2d)) return fail(RAMSES_AMD_EINVAL, "MHD sweep: riemann2d must be 0 (llf) .. 5 (hlld) (got %d)", P.riemann2d);
  return 0;
}

}  // namespace mhd
}  // namespace ramses_amd

// capi_shared.hpp -- what the translation units of the C ABI share (capi.hip: bricks, halos, dense multigrid;
// capi_host.hip: the staged and the resident entry points on the reference's host arrays; capi_tree_poisson.hip: the
// multigrid and conjugate-gradient solves on AMR levels) beyond the host helpers of host_util.hpp: the constants of the hydro
// kernels, what the entry points refuse by name.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/ramses_amd.h"
#include "host_util.hpp"
#include "hydro_core.hpp"

namespace ramses_amd {

static inline HydroConst make_const(const ramses_amd_hydro_params *p) {
  HydroConst P;
  P.gamma = p->gamma;
  P.smallr = p->smallr;
  P.smallc = p->smallc;
  P.smallc2 = p->smallc * p->smallc;
  P.smallp = P.smallc2 / p->gamma;                       // smallc**2/gamma
  P.smalle = P.smallc2 / p->gamma / (p->gamma - 1.0);    // smallc**2/gamma/(gamma-one)
  P.entho = 1.0 / (p->gamma - 1.0);
  P.gm1 = p->gamma - 1.0;
  P.gamma6 = (p->gamma + 1.0) / (2.0 * p->gamma);
  P.smallpp = p->smallr * P.smallp;
  P.oneovergamma = 1.0 / p->gamma;
  P.slope_theta = p->slope_theta;
  P.niter_riemann = p->niter_riemann;
  for (int i = 0; i < 2; i++) {
    const bool on = i < p->nener;
    P.gamma_rad[i] = on ? p->gamma_rad[i] : 0.0;
    P.gm1_rad[i] = on ? p->gamma_rad[i] - 1.0 : 0.0;   // (gamma_rad(irad)-one)
  }
  return P;
}

// NENER > 0 (non-thermal energies) runs on the uniform brick paths only: every other entry point refuses it by name
static inline int refuse_nener(const ramses_amd_hydro_params *p, const char *who) {
  if (p && p->nener != 0)
    return fail(RAMSES_AMD_EUNSUPPORTED, "%s: NENER=%d (non-thermal energies) is implemented on the uniform brick paths only "
                "(staged, resident and MPI-resident bricks), not on AMR levels or tiles", who, p->nener);
  return 0;
}
// what a brick sweep with NENER > 0 needs: nener 1 or 2, NVAR >= 5+nener, 3-D, muscl, llf / hll / hllc, no gravity, no difmag
static inline int check_nener(const ramses_amd_hydro_params *p, bool grav) {
  if (p->nener == 0) return 0;
  if (p->nener < 0 || p->nener > RAMSES_AMD_MAX_NENER)
    return fail(RAMSES_AMD_EUNSUPPORTED, "NENER=%d: the device path implements NENER=0, 1, 2", p->nener);
  if (p->nvar < 5 + p->nener) return fail(RAMSES_AMD_EUNSUPPORTED, "NENER=%d needs NVAR >= %d (got %d)", p->nener, 5 + p->nener, p->nvar);
  if (p->ndim != 3) return fail(RAMSES_AMD_EUNSUPPORTED, "NENER>0 needs NDIM=3 (got %d)", p->ndim);
  if (p->scheme != RAMSES_AMD_SCHEME_MUSCL) return fail(RAMSES_AMD_EUNSUPPORTED, "NENER>0 with scheme='plmde' is not on the device");
  if (p->riemann != RAMSES_AMD_RIEMANN_LLF && p->riemann != RAMSES_AMD_RIEMANN_HLL && p->riemann != RAMSES_AMD_RIEMANN_HLLC)
    return fail(RAMSES_AMD_EUNSUPPORTED, "NENER>0 with riemann=%d: the reference's acoustic and exact solvers have no NENER branch "
                "(llf, hll, hllc only)", p->riemann);
  if (grav) return fail(RAMSES_AMD_EUNSUPPORTED, "NENER>0 with gravity is not on the device");
  if (p->difmag > 0.0) return fail(RAMSES_AMD_EUNSUPPORTED, "NENER>0 with difmag>0 is not on the device");
  for (int i = 0; i < p->nener; i++)
    if (!(p->gamma_rad[i] > 1.0)) return fail(RAMSES_AMD_EINVAL, "gamma_rad(%d)=%g must be > 1", i + 1, p->gamma_rad[i]);
  return 0;
}

// NVAR of a brick sweep (every brick entry point): 5+NENER <= NVAR <= RAMSES_AMD_MAX_NVAR; passive scalars with muscl only
static_assert(RAMSES_AMD_MAX_NVAR == MAX_NVAR, "include/ramses_amd.h and csrc/sweep_args.hpp agree on NVAR");
static inline int check_nvar(const ramses_amd_hydro_params *p, const char *who) {
  if (p->nvar < 5 + (p->nener > 0 ? p->nener : 0) || p->nvar > RAMSES_AMD_MAX_NVAR)
    return fail(RAMSES_AMD_EUNSUPPORTED, "%s: NVAR=%d with NENER=%d: the device sweep implements 5+NENER <= NVAR <= %d", who, p->nvar,
                p->nener, RAMSES_AMD_MAX_NVAR);
  if (p->nvar != 5 && p->scheme != RAMSES_AMD_SCHEME_MUSCL)
    return fail(RAMSES_AMD_EUNSUPPORTED, "%s: passive scalars (NVAR=%d) with scheme='plmde' are not on the device", who, p->nvar);
  return 0;
}
// NVAR > 7 (more than two passive scalars, or NENER with more than 7 variables) runs on the uniform brick paths only: every AMR,
// tile and tree-walking entry point refuses it by name
static inline int refuse_scalars(const ramses_amd_hydro_params *p, const char *who) {
  if (p && p->nvar > 7)
    return fail(RAMSES_AMD_EUNSUPPORTED, "%s: NVAR=%d: more than 7 variables are implemented on the uniform brick paths only (staged, "
                "resident and MPI-resident bricks), not on AMR levels, tiles or the tree walker", who, p->nvar);
  return 0;
}
// both, in this order: how every entry point of the AMR levels opens
static inline int refuse_amr(const ramses_amd_hydro_params *p, const char *who) {
  if (int rc = refuse_nener(p, who)) return rc;
  return refuse_scalars(p, who);
}

// capi_host.hip: the staged entry points reuse the staging buffers of the resident level; refuses while that level holds
// the only current copy of the hydro state
int capi_resident_release(const char *who);

// capi_amr.hip: what ramses_amd_gravana_set stored (csrc/gravana_core.hpp), or null before it
struct GravAna;
const GravAna *capi_gravana();
// capi_amr.hip: what ramses_amd_eos_set stored (csrc/eos_core.hpp), or null before it
struct EosConst;
const EosConst *capi_eos();
void capi_eos_called();      // one more cooling_fine ran on the device (the RAMSES_AMD_STATS exit line counts them)

}  // namespace ramses_amd

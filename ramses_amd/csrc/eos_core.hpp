// eos_core.hpp -- cooling_fine of a barotropic run without cooling (hydro/cooling_fine.f90:162-181,264-308,331-347,537-540,
// 563-566,576-579), one leaf cell at a time: the total energy is rewritten from the density, the momenta and ONE constant
// temperature T2c.
//
// T2c is a constant in exactly two forms:
//   barotropic_eos_form = 'isothermal'                      T2c = T2_eos                     (hydro/eos.f90:14-15)
//   barotropic_eos_form = 'legacy', jeans_ncells <= 0 and g_star == 1 exactly
//                                                           T2c = T2_star * x**(+0.0) = T2_star  (hydro/cooling_fine.f90:344)
// Every other form raises the density to a power: a pow call of the reference's runtime library, whose bits the source does not
// determine.  Those are NOT here.
//
// The function restates the reference's operations in the reference's ORDER (IEEE double, no contraction: the units that
// include this header are compiled with -ffp-contract=off; the divides are the correctly rounded ones), so the result carries
// the reference's bits.  The header also compiles for the host (plain C++): ramses_amd_eos_eval and tests/native/eos_host_check.cpp.
#pragma once

#if defined(__HIPCC__)
#define EOS_FN __host__ __device__ __forceinline__
#else
#define EOS_FN inline
#endif

namespace ramses_amd {

// T2c (above) and the two conversion factors of the program's own units(): scale_nH, scale_T2
struct EosConst {
  double T2c;
  double scale_nH;
  double scale_T2;
};

// uold(ndim+2) of a leaf cell, NDIM = 3, NENER = 0, SOLVER=hydro (err = emag = 0.0, added in the reference's order)
EOS_FN double eos_energy(const EosConst &C, double rho, double mx, double my, double mz, double smallr, double gamma) {
  const double nH = rho > smallr ? rho : smallr;      // :180  MAX(uold(:,1), smallr)
  double ekk = 0.0;                                   // :269-275, idim = 2..4
  ekk = ekk + 0.5 * (mx * mx) / nH;
  ekk = ekk + 0.5 * (my * my) / nH;
  ekk = ekk + 0.5 * (mz * mz) / nH;
  const double err = 0.0, emag = 0.0;                 // :277, :287
  const double nHcc = nH * C.scale_nH;                // :307  into H/cc ...
  const double nH2 = nHcc / C.scale_nH;               // :539  ... and back: NOT the identity, both roundings are kept
  const double e = C.T2c * nH2 / C.scale_T2 / (gamma - 1.0);      // :565, left to right
  return ((e + ekk) + err) + emag;                    // :578
}

}  // namespace ramses_amd

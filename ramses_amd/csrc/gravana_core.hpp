// gravana_core.hpp -- the analytic acceleration of a run with gravity_type = 1 (constant vector) or 2 (point mass),
// poisson/gravana.f90:27-62, and the cell centre force_fine hands it (poisson/force_fine.f90:46-87), one cell at a time.
//
// Every function restates the reference's operations in the reference's ORDER (IEEE double, no contraction: the units
// that include this header are compiled with -ffp-contract=off; sqrt and the divide are the correctly rounded ones), so the
// result carries the reference's bits.  The header also compiles for the host (plain C++): ramses_amd_gravana_eval's
// argument checks and the CPU tests' checker share its meaning.
//
// gravity_type = 3 is NOT here: its (rz**2+z0**2)**0.5 is a pow call of the reference's runtime library, whose bits the source
// does not determine.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define GRAVANA_FN __host__ __device__ __forceinline__
#else
#define GRAVANA_FN inline
#endif

namespace ramses_amd {

// gravity_type, gravity_params(1:10) (poisson/poisson_parameters.f90) and force_fine's rescaling: skip = icoarse_min, jcoarse_min,
// kcoarse_min; scale = boxlen / nx_loc
struct GravAna {
  int type;
  double p[10];
  double skip[3];
  double scale;
};

// the centre of cell ind (0..7) of an oct whose centre is xg, in user units: xc = (dble(ix)-0.5)*dx, x = (xg + xc - skip)*scale
GRAVANA_FN void gravana_centre(const GravAna &G, const double (&xg)[3], int ind, double dx, double (&x)[3]) {
#pragma unroll
  for (int d = 0; d < 3; d++) {
    const double xc = ((double)((ind >> d) & 1) - 0.5) * dx;
    x[d] = ((xg[d] + xc) - G.skip[d]) * G.scale;
  }
}

// gravana for one cell, NDIM = 3.  type 1: f = gravity_params(1:3).  type 2: gmass = p(1), emass = p(2) (the `emass = dx` line
// above it is dead), the mass at p(3:5); rr = sqrt(rx**2+ry**2+rz**2+emass**2), f = -gmass*r/rr**3 with rr**3 = rr*rr*rr
GRAVANA_FN void gravana_cell(const GravAna &G, const double (&x)[3], double (&f)[3]) {
  if (G.type == 1) {
    f[0] = G.p[0]; f[1] = G.p[1]; f[2] = G.p[2];
    return;
  }
  const double gmass = G.p[0], emass = G.p[1];
  const double rx = x[0] - G.p[2], ry = x[1] - G.p[3], rz = x[2] - G.p[4];
  const double rr = __builtin_sqrt(((rx * rx + ry * ry) + rz * rz) + emass * emass);
  const double r3 = (rr * rr) * rr;
  f[0] = (-gmass * rx) / r3;
  f[1] = (-gmass * ry) / r3;
  f[2] = (-gmass * rz) / r3;
}

}  // namespace ramses_amd

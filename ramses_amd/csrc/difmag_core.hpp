// difmag_core.hpp -- the artificial diffusion of the hydro solver (difmag > 0), NDIM = 3: cmpdivu and consup of the reference
// (hydro/uplmde.f90:702-764, 769-866, called at the end of unsplit, hydro/umuscl.f90:166-168), one corner and one face at a time.
//
// Every function restates the reference's operations in the reference's ORDER (IEEE double, no contraction: the units that
// include this header are compiled with -ffp-contract=off), so that the marching kernel and the surface pass of a level in
// tiles (csrc/hydro_sweep.hip) return the reference's bits.  Nothing of the HIP runtime is included: the header also compiles
// for the host (plain C++), where tests/test_difmag_core_host.py runs these very functions against the oracle's unsplit.
#pragma once

#if defined(__HIPCC__)
#define DIFMAG_FN __host__ __device__ __forceinline__
#else
#define DIFMAG_FN inline
#endif

namespace ramses_amd {
namespace difmag {

// cmpdivu: the velocity divergence at the LOW corner of cell (i, j, k) from the primitive velocities -- ctoprim's, the gravity
// half kick included -- of the eight cells round it.  v[d][dk][dj][di]: component d of the cell at (i-1+di, j-1+dj, k-1+dk);
// fx, fy, fz = 0.25 / dx, 0.25 / dy, 0.25 / dz.
// (the three sums one by one -- v[dk][dj][di] of one component -- for a caller that gathers one component at a time)
DIFMAG_FN double cmpdivu_ux(const double (&v)[2][2][2], double fx) {
  double ux = 0.0;
  ux = ux + fx * (v[1][1][1] - v[1][1][0]);
  ux = ux + fx * (v[1][0][1] - v[1][0][0]);
  ux = ux + fx * (v[0][1][1] - v[0][1][0] + v[0][0][1] - v[0][0][0]);
  return ux;
}
DIFMAG_FN double cmpdivu_vy(const double (&v)[2][2][2], double fy) {
  double vy = 0.0;
  vy = vy + fy * (v[1][1][1] - v[1][0][1] + v[1][1][0] - v[1][0][0]);
  vy = vy + fy * (v[0][1][1] - v[0][0][1] + v[0][1][0] - v[0][0][0]);
  return vy;
}
DIFMAG_FN double cmpdivu_wz(const double (&v)[2][2][2], double fz) {
  double wz = 0.0;
  wz = wz + fz * (v[1][1][1] - v[0][1][1] + v[1][0][1] - v[0][0][1] + v[1][1][0] - v[0][1][0] + v[1][0][0] - v[0][0][0]);
  return wz;
}
DIFMAG_FN double cmpdivu_corner(const double (&v)[3][2][2][2], double fx, double fy, double fz) {
  return cmpdivu_ux(v[0], fx) + cmpdivu_vy(v[1], fy) + cmpdivu_wz(v[2], fz);
}

// consup: the divergence of a face = the four corners of the face, each direction in its own order.
// The x face of cell (i, j, k) (between i-1 and i): corners (i,j,k), (i,j+1,k), (i,j,k+1), (i,j+1,k+1)
DIFMAG_FN double consup_div1_x(double d_jk, double d_j1k, double d_jk1, double d_j1k1) {
  double div1 = 0.25 * d_jk;
  div1 = div1 + 0.25 * d_j1k;
  div1 = div1 + 0.25 * (d_jk1 + d_j1k1);
  return div1;
}
// The y face of cell (i, j, k) (between j-1 and j): corners (i,j,k), (i+1,j,k), (i,j,k+1), (i+1,j,k+1)
DIFMAG_FN double consup_div1_y(double d_ik, double d_i1k, double d_ik1, double d_i1k1) {
  double div1 = 0.0;
  div1 = div1 + 0.25 * (d_ik + d_i1k);
  div1 = div1 + 0.25 * (d_ik1 + d_i1k1);
  return div1;
}
// The z face of cell (i, j, k) (between k-1 and k): corners (i,j,k), (i+1,j,k), (i,j+1,k), (i+1,j+1,k)
DIFMAG_FN double consup_div1_z(double d_ij, double d_i1j, double d_ij1, double d_i1j1) {
  return 0.25 * (d_ij + d_i1j + d_ij1 + d_i1j1);
}
// direction DIR with the corners in the face's own (lower transverse axis, upper transverse axis) frame: c[a][b] = the corner
// at +a along the lower and +b along the upper transverse axis
template <int DIR>
DIFMAG_FN double consup_div1(const double (&c)[2][2]) {
  if (DIR == 0) return consup_div1_x(c[0][0], c[1][0], c[0][1], c[1][1]);
  if (DIR == 1) return consup_div1_y(c[0][0], c[1][0], c[0][1], c[1][1]);
  return consup_div1_z(c[0][0], c[1][0], c[0][1], c[1][1]);
}
// the factor of a face: difmag * min(0, div1)
DIFMAG_FN double consup_coef(double difmag, double div1) { return difmag * __builtin_fmin(0.0, div1); }
// the flux of one variable through the face, scaled by dt / dx already, with the diffusive term: ucell / uprev = the CONSERVED
// variable of the cell and of the cell before it along the face normal; coef = consup_coef of the face
// (consup_add: the same with the difference du = ucell - uprev taken by the caller)
DIFMAG_FN double consup_add(double flux, double dt, double coef, double du) { return flux + dt * coef * du; }
DIFMAG_FN double consup_term(double flux, double dt, double coef, double ucell, double uprev) {
  return consup_add(flux, dt, coef, ucell - uprev);
}

}  // namespace difmag
}  // namespace ramses_amd

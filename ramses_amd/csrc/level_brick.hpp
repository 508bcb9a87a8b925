// level_brick.hpp -- a fully refined periodic level of the reference's own arrays as a dense n^3 brick on the device: what the
// staged and the resident entry points of capi_host.hip and mhd_sweep.hip ask of the level, how its octs reach the device, and
// the argument block of the copies between the brick and the cell vectors.  Host code only, on top of host_util.hpp and
// pack_args.hpp; a unit that takes (ilevel, ngrid, igrid, xg, ngridmax, ncoarse, nx_loc) includes this header instead of
// writing the sequence out again.
#pragma once
#include <hip/hip_runtime.h>

#include "host_util.hpp"
#include "pack_args.hpp"

namespace ramses_amd {

struct LevelShape {
  int n;          // cells per direction, 2^ilevel
  long N, ncell;  // cells of the level; length of the cell vectors, ncoarse + 8 ngridmax
};

// What every entry point asks of the level, refused in this order: one coarse cell (nx = ny = nz = 1, the periodic box), a level
// in lmin..lmax (the callers differ), all of its octs on this rank.  `who` opens the nx_loc message.
static inline int level_shape(const char *who, int ilevel, int lmin, int lmax, int ngrid, int nx_loc, long ngridmax, long ncoarse,
                              LevelShape *S) {
  if (nx_loc != 1) return fail(RAMSES_AMD_EUNSUPPORTED, "%s needs a periodic box with nx=ny=nz=1 (got nx_loc=%d)", who, nx_loc);
  if (ilevel < lmin || ilevel > lmax) return fail(RAMSES_AMD_EINVAL, "level out of range");
  S->n = 1 << ilevel;
  S->N = (long)S->n * S->n * S->n;
  if ((long)ngrid * 8 != S->N)
    return fail(RAMSES_AMD_EUNSUPPORTED, "level %d is not fully refined on this rank (ngrid=%d, need %ld)", ilevel, ngrid, S->N / 8);
  S->ncell = ncoarse + 8 * ngridmax;
  return 0;
}

// the level's octs on the device: active(ilevel)%igrid, xg, the brick index of each oct's (0,0,0) cell, the count of misplaced octs
struct LevelOcts {
  DevBuf igrid, xg, octorg, flag;
};

// igrid(1:ngrid) and xg(1:ngridmax,1:3) go up, octorg is computed from them; one stream synchronisation.  Refuses octs whose
// centre is not that of an oct of the level-ilevel lattice inside the box.
static inline int level_octs_upload(LevelOcts &O, int ilevel, int n, int ngrid, const int *igrid, const double *xg, long ngridmax,
                                    hipStream_t s) {
  HCHK(O.igrid.ensure(sizeof(int) * ngrid), "hipMalloc igrid");
  HCHK(O.xg.ensure(sizeof(double) * 3 * ngridmax), "hipMalloc xg");
  HCHK(O.octorg.ensure(sizeof(long) * ngrid), "hipMalloc octorg");
  HCHK(O.flag.ensure(sizeof(int)), "hipMalloc flag");
  HCHK(hipMemcpyAsync(O.igrid.p, igrid, sizeof(int) * ngrid, hipMemcpyHostToDevice, s), "H2D igrid");
  HCHK(hipMemcpyAsync(O.xg.p, xg, sizeof(double) * 3 * ngridmax, hipMemcpyHostToDevice, s), "H2D xg");
  HCHK(hipMemsetAsync(O.flag.p, 0, sizeof(int), s), "memset");
  const double skip[3] = {0.0, 0.0, 0.0};   // icoarse_min = 0 for nx = 1
  HCHK(launch_oct_origin(O.igrid.as<int>(), O.xg.as<double>(), ngridmax, ngrid, n, skip, O.octorg.as<long>(), O.flag.as<int>(), s),
       "oct origin launch");
  int bad = 0;
  HCHK(hipMemcpyAsync(&bad, O.flag.p, sizeof(int), hipMemcpyDeviceToHost, s), "D2H flag");
  HCHK(hipStreamSynchronize(s), "sync");
  if (bad) return fail(RAMSES_AMD_EINVAL, "%d octs of level %d do not sit on the level lattice", bad, ilevel);
  return 0;
}

// the copy between the dense brick [nvar][n][n][n] and the cell vectors (1:ncell,1:nvar) of the level (launch_oct_copy: gather
// or scatter; launch_oct_leaf)
static inline PackArgs level_pack(const LevelOcts &O, int ngrid, int n, int nvar, long ncoarse, long ngridmax, double *brick,
                                  double *cellvec) {
  PackArgs A;
  A.igrid = O.igrid.as<const int>(); A.octorg = O.octorg.as<const long>();
  A.ngrid = ngrid; A.n = n; A.nvar = nvar;
  A.ncoarse = ncoarse; A.ngridmax = ngridmax; A.ncell = ncoarse + 8 * ngridmax; A.pitch_var = (long)n * n * n;
  A.brick = brick; A.cellvec = cellvec;
  return A;
}

}  // namespace ramses_amd

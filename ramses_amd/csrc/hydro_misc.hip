// hydro_misc.hip -- streaming kernels around the sweep: CFL reduction
// (courant_fine/cmpdt), periodic ghost fill and halo slab pack/unpack
// (the pack/unpack loops of make_virtual_fine_dp).  All are pure HBM-bound
// copies/reductions: coalesced 512 B row segments per wavefront, wavefront
// shuffles + one atomic per workgroup for the reductions.
#include <hip/hip_runtime.h>

#include "hydro_core.hpp"
#include "misc_args.hpp"

namespace ramses_amd {

// ---------------------------------------------------------------------------
// courant_fine (hydro/courant_fine.f90:1-159) + cmpdt
// out[0] = min dt (bit pattern min: valid for positive doubles)
// out[1] = sum rho*vol, out[2] = sum E*vol, out[3] = sum e_int*vol
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = __builtin_fmin(v, __shfl_down(v, off, 64));
  return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// NE > 0: cmpdt with the non-thermal energies and eint_loc less them (courant_fine.f90:113-118); the kernel
// of NE = 0 (courant_kernel) is the body instantiated as before
template <bool GRAV, int NE>
__device__ __forceinline__ void courant_body(const CourantArgs &A) {
  constexpr int NV = 5 + NE;
  const HydroConst &P = A.P;
  const long nrow = (long)A.ny * A.nz;
  double dtmin = A.dt_init;
  double mass = 0.0, etot = 0.0, eint = 0.0;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long nwaves = (long)gridDim.x * 4;
  for (long row = (long)blockIdx.x * 4 + wave; row < nrow; row += nwaves) {
    const int k = (int)(row / A.ny), j = (int)(row % A.ny);
    const long base = (long)(j + A.ng) * A.pitch_y + (long)(k + A.ng) * A.pitch_z + A.ng;
    for (int i = lane; i < A.nx; i += 64) {
      double u[NV], g[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int n = 0; n < NV; n++) u[n] = A.uold[base + i + (long)n * A.pitch_var];
      if (GRAV) {
#pragma unroll
        for (int d = 0; d < 3; d++) g[d] = A.grav[base + i + (long)d * A.pitch_var];
      }
      dtmin = __builtin_fmin(dtmin, cmpdt_cell<NV, GRAV, NE>(u, g, A.dx, A.courant_factor, P, A.ndimf));
      mass += u[0] * A.vol;
      etot += u[4] * A.vol;
      double ei = u[4] * A.vol;
      const double rho = __builtin_fmax(u[0], P.smallr);
      ei -= 0.5 * (u[1] * u[1]) / rho * A.vol;
      ei -= 0.5 * (u[2] * u[2]) / rho * A.vol;
      ei -= 0.5 * (u[3] * u[3]) / rho * A.vol;
#pragma unroll
      for (int n = 0; n < NE; n++) ei -= u[5 + n] * A.vol;
      eint += ei;
    }
  }
  dtmin = wave_min(dtmin);
  mass = wave_sum(mass); etot = wave_sum(etot); eint = wave_sum(eint);
  __shared__ double red[4][4];
  if (lane == 0) { red[wave][0] = dtmin; red[wave][1] = mass; red[wave][2] = etot; red[wave][3] = eint; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double d = red[0][0], m = red[0][1], e = red[0][2], ei = red[0][3];
    for (int w = 1; w < 4; w++) { d = __builtin_fmin(d, red[w][0]); m += red[w][1]; e += red[w][2]; ei += red[w][3]; }
    // positive doubles order like their bit patterns
    atomicMin(reinterpret_cast<unsigned long long *>(A.out), (unsigned long long)__double_as_longlong(d));
    atomicAdd(A.out + 1, m);
    atomicAdd(A.out + 2, e);
    atomicAdd(A.out + 3, ei);
  }
}

template <bool GRAV>
__global__ __launch_bounds__(256) void courant_kernel(CourantArgs A) {
  courant_body<GRAV, 0>(A);
}

template <int NE>
__global__ __launch_bounds__(256) void courant_nener_kernel(CourantArgs A) {
  courant_body<false, NE>(A);
}

__global__ void courant_init_kernel(double *out, double dt_init) {
  out[0] = dt_init; out[1] = 0.0; out[2] = 0.0; out[3] = 0.0;
}

hipError_t launch_courant_init(double *out, double dt_init, hipStream_t s) {
  hipLaunchKernelGGL(courant_init_kernel, dim3(1), dim3(1), 0, s, out, dt_init);
  return hipGetLastError();
}

hipError_t launch_courant(const CourantArgs &A, bool grav, int nener, hipStream_t s) {
  const long nrow = (long)A.ny * A.nz;
  int grid = (int)((nrow + 3) / 4);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  if (nener == 1 && !grav) hipLaunchKernelGGL(courant_nener_kernel<1>, dim3(grid), dim3(256), 0, s, A);
  else if (nener == 2 && !grav) hipLaunchKernelGGL(courant_nener_kernel<2>, dim3(grid), dim3(256), 0, s, A);
  else if (nener != 0) return hipErrorInvalidValue;
  else if (grav) hipLaunchKernelGGL(courant_kernel<true>, dim3(grid), dim3(256), 0, s, A);
  else hipLaunchKernelGGL(courant_kernel<false>, dim3(grid), dim3(256), 0, s, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The pdV term of the non-thermal energies (add_pdv_source_terms, hydro/godunov_fine.f90:294-481, loop :422-429) on a
// fully refined brick, before set_uold's swap:
//   divu = sum over idim of (veld - velg)/(dx_g + dx_d),  vel = uold(mom)/max(uold(rho), smallr) of the two neighbours
//   unew(e_irad) = unew(e_irad) - (gamma_rad-1)*uold(e_irad)*divu*dt
// Every neighbour of a cell of a fully refined level exists (dx_g = dx_d = dx).  One lane per cell along x, one wavefront
// per row segment of 64 cells: the six neighbour loads of a lane are coalesced row reads (x +- 1 are the lanes beside it).
// ng = 0: periodic wrap; ng >= 2: the ghost layers of uold hold the neighbours.
// ---------------------------------------------------------------------------
template <int NE>
__global__ __launch_bounds__(256) void pdv_kernel(PdvArgs A) {
  const long nrow = (long)A.ny * A.nz;
  const int lane = threadIdx.x & 63;
  const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nwaves = (long)gridDim.x * 4;
  const double dxs = A.dx + A.dx;
  for (long row = wave; row < nrow; row += nwaves) {
    const int k = (int)(row / A.ny), j = (int)(row % A.ny);
    for (int i = lane; i < A.nx; i += 64) {
      long c, nb[6];
      if (A.ng == 0) {
        const int im = i == 0 ? A.nx - 1 : i - 1, ip = i == A.nx - 1 ? 0 : i + 1;
        const int jm = j == 0 ? A.ny - 1 : j - 1, jp = j == A.ny - 1 ? 0 : j + 1;
        const int km = k == 0 ? A.nz - 1 : k - 1, kp = k == A.nz - 1 ? 0 : k + 1;
        const long yz = (long)j * A.pitch_y + (long)k * A.pitch_z;
        c = yz + i;
        nb[0] = yz + im; nb[1] = yz + ip;
        nb[2] = (long)jm * A.pitch_y + (long)k * A.pitch_z + i; nb[3] = (long)jp * A.pitch_y + (long)k * A.pitch_z + i;
        nb[4] = (long)j * A.pitch_y + (long)km * A.pitch_z + i; nb[5] = (long)j * A.pitch_y + (long)kp * A.pitch_z + i;
      } else {
        c = (long)(j + A.ng) * A.pitch_y + (long)(k + A.ng) * A.pitch_z + A.ng + i;
        nb[0] = c - 1; nb[1] = c + 1;
        nb[2] = c - A.pitch_y; nb[3] = c + A.pitch_y;
        nb[4] = c - A.pitch_z; nb[5] = c + A.pitch_z;
      }
      double divu = 0.0;
#pragma unroll
      for (int d = 0; d < 3; d++) {
        const double velg = A.uold[nb[2 * d] + (long)(1 + d) * A.pitch_var] / __builtin_fmax(A.uold[nb[2 * d]], A.smallr);
        const double veld = A.uold[nb[2 * d + 1] + (long)(1 + d) * A.pitch_var] / __builtin_fmax(A.uold[nb[2 * d + 1]], A.smallr);
        divu = divu + (veld - velg) / dxs;
      }
#pragma unroll
      for (int n = 0; n < NE; n++) {
        const long o = c + (long)(5 + n) * A.pitch_var;
        A.unew[o] = A.unew[o] - A.gm1_rad[n] * A.uold[o] * divu * A.dt;
      }
    }
  }
}

hipError_t launch_pdv(const PdvArgs &A, int nener, hipStream_t s) {
  const long nrow = (long)A.ny * A.nz;
  int grid = (int)((nrow + 3) / 4);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  if (nener == 1) hipLaunchKernelGGL(pdv_kernel<1>, dim3(grid), dim3(256), 0, s, A);
  else if (nener == 2) hipLaunchKernelGGL(pdv_kernel<2>, dim3(grid), dim3(256), 0, s, A);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Generic box copy between two strided SoA layouts: the one kernel behind the
// periodic ghost fill and the halo slab pack/unpack.  One wavefront copies one
// x-row segment (coalesced on the side whose x stride is 1, which is both
// sides for y/z slabs; for x slabs the row is only 2 cells long and the slab
// is tiny).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void box_copy_kernel(BoxCopyArgs A) {
  const long nrows = (long)A.ey * A.ez * A.nvar;
  const int lane = threadIdx.x & 63;
  const long w0 = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const long nw = (long)gridDim.x * 4;
  if (A.ex >= 16) {
    for (long row = w0; row < nrows; row += nw) {
      const int j = (int)(row % A.ey);
      const int k = (int)((row / A.ey) % A.ez);
      const int n = (int)(row / ((long)A.ey * A.ez));
      const long so = A.s_off + (long)j * A.s_py + (long)k * A.s_pz + (long)n * A.s_pv;
      const long dof = A.d_off + (long)j * A.d_py + (long)k * A.d_pz + (long)n * A.d_pv;
      for (int i = lane; i < A.ex; i += 64) A.dst[dof + i] = A.src[so + i];
    }
  } else {
    // thin-x boxes: flatten (i,j) across lanes
    const long nplanes = (long)A.ez * A.nvar;
    const int rowlen = A.ex * A.ey;
    for (long pl = w0; pl < nplanes; pl += nw) {
      const int k = (int)(pl % A.ez);
      const int n = (int)(pl / A.ez);
      const long so = A.s_off + (long)k * A.s_pz + (long)n * A.s_pv;
      const long dof = A.d_off + (long)k * A.d_pz + (long)n * A.d_pv;
      for (int t = lane; t < rowlen; t += 64) {
        const int i = t % A.ex, j = t / A.ex;
        A.dst[dof + i + (long)j * A.d_py] = A.src[so + i + (long)j * A.s_py];
      }
    }
  }
}

hipError_t launch_box_copy(const BoxCopyArgs &A, hipStream_t s) {
  const long nrows = A.ex >= 16 ? (long)A.ey * A.ez * A.nvar : (long)A.ez * A.nvar;
  if (nrows <= 0 || A.ex <= 0) return hipSuccess;
  long grid = (nrows + 3) / 4;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(box_copy_kernel, dim3((int)grid), dim3(256), 0, s, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// One-shot halo: every face, edge and corner region of the brick packed into (or
// unpacked from) one buffer by a single launch, so that the exchange is ONE
// grouped send/recv with one message per peer, all xGMI links busy at once
// (instead of three dependent axis rounds over one link each).  One wavefront
// copies one x-row of one region.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void multi_box_kernel(MultiBoxArgs A) {
  const long nrows = A.rows_before[A.nbox];
  const int lane = threadIdx.x & 63;
  const long nw = (long)gridDim.x * 4;
  for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < nrows; row += nw) {
    int r = 0;
#pragma unroll 1
    while (r + 1 < A.nbox && row >= A.rows_before[r + 1]) r++;
    const long lr = row - A.rows_before[r];
    const int ex = A.ext[r][0], ey = A.ext[r][1], ez = A.ext[r][2];
    const int j = (int)(lr % ey);
    const int k = (int)((lr / ey) % ez);
    const int v = (int)(lr / ((long)ey * ez));
    const long bo = (long)A.org[r][0] + (long)(A.org[r][1] + j) * A.pitch_y + (long)(A.org[r][2] + k) * A.pitch_z +
                    (long)v * A.pitch_var;
    const long po = A.off[r] + ((long)v * ez + k) * (long)ey * ex + (long)j * ex;
    if (A.pack) {
      for (int i = lane; i < ex; i += 64) A.buf[po + i] = A.brick[bo + i];
    } else {
      for (int i = lane; i < ex; i += 64) A.brick[bo + i] = A.buf[po + i];
    }
  }
}

hipError_t launch_multi_box(const MultiBoxArgs &A, hipStream_t s) {
  const long nrows = A.rows_before[A.nbox];
  if (nrows <= 0) return hipSuccess;
  long grid = (nrows + 3) / 4;
  if (grid > 8192) grid = 8192;
  hipLaunchKernelGGL(multi_box_kernel, dim3((int)grid), dim3(256), 0, s, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// make_boundary_hydro (hydro/hydro_boundary.f90:5-269) on a ghost-layer brick:
// the ghost layers of one face, over the full extent of the other directions
// (call the faces in x, y, z order so that edges and corners are filled from
// already filled ghosts, as the halo exchange does).
//   reflexive: ghost cell g layers outside the wall = interior cell g layers
//              inside (ind_ref = mirror octant), normal momentum sign flipped
//   outflow:   every ghost layer = the first interior layer (ind_ref = the
//              boundary-side octant), optional no_inflow clamp with the kinetic
//              energy removed before and added back after
//   imposed:   boundana's constant state
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void boundary_kernel(BoundaryArgs A) {
  const int axis = A.face >> 1, hi = A.face & 1;
  const int n[3] = {A.nx, A.ny, A.nz};
  int ext[3] = {A.nx + 2 * A.ng, A.ny + 2 * A.ng, A.nz + 2 * A.ng};
  ext[axis] = A.ng;
  const long total = (long)ext[0] * ext[1] * ext[2];
  const long pitch[3] = {1, A.pitch_y, A.pitch_z};
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    int c[3];
    c[0] = (int)(t % ext[0]);
    c[1] = (int)((t / ext[0]) % ext[1]);
    c[2] = (int)(t / ((long)ext[0] * ext[1]));
    const int layer = c[axis];                    // 0 .. ng-1, counted from the wall outwards
    int cg[3] = {c[0], c[1], c[2]}, cr[3] = {c[0], c[1], c[2]};
    // allocated coordinates of the ghost cell and of its reference cell
    cg[axis] = hi ? A.ng + n[axis] + layer : A.ng - 1 - layer;
    const int mirror = A.type == 1 ? layer : 0;
    cr[axis] = hi ? A.ng + n[axis] - 1 - mirror : A.ng + mirror;
    const long og = cg[0] * pitch[0] + cg[1] * pitch[1] + cg[2] * pitch[2];
    const long orf = cr[0] * pitch[0] + cr[1] * pitch[1] + cr[2] * pitch[2];
    if (A.type == 3) {
      for (int v = 0; v < A.nvar; v++) A.u[og + (long)v * A.pitch_var] = A.value[v];
      continue;
    }
    double uu[8];
    for (int v = 0; v < A.nvar; v++) uu[v] = A.u[orf + (long)v * A.pitch_var];
    if (A.type == 1) {
      uu[1 + axis] = uu[1 + axis] * -1.0;
    } else {
      // free boundary: the reference takes the kinetic energy out and puts it back
      // (around the optional no_inflow clamp) -- (E - ek) + ek is kept as is
      double ekin = 0.0;
      double d = __builtin_fmax(uu[0], A.smallr);
      for (int k = 0; k < 3; k++) { const double vel = uu[1 + k] / d; ekin = ekin + 0.5 * d * (vel * vel); }
      uu[4] = uu[4] - ekin;
      if (A.no_inflow) uu[1 + axis] = hi ? __builtin_fmax(0.0, uu[1 + axis]) : __builtin_fmin(0.0, uu[1 + axis]);
      ekin = 0.0;
      d = __builtin_fmax(uu[0], A.smallr);
      for (int k = 0; k < 3; k++) { const double vel = uu[1 + k] / d; ekin = ekin + 0.5 * d * (vel * vel); }
      uu[4] = uu[4] + ekin;
    }
    for (int v = 0; v < A.nvar; v++) A.u[og + (long)v * A.pitch_var] = uu[v];
  }
}

hipError_t launch_boundary(const BoundaryArgs &A, hipStream_t s) {
  const int axis = A.face >> 1;
  long ext[3] = {A.nx + 2 * A.ng, A.ny + 2 * A.ng, A.nz + 2 * A.ng};
  ext[axis] = A.ng;
  const long total = ext[0] * ext[1] * ext[2];
  if (total <= 0) return hipSuccess;
  long grid = (total + 255) / 256;
  if (grid > 4096) grid = 4096;
  hipLaunchKernelGGL(boundary_kernel, dim3((int)grid), dim3(256), 0, s, A);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Gravity source terms on the device-resident level (NDIM = 3; variables rho, rho*u, rho*v,
// rho*w, E at u[0..4][N], passive scalars untouched).  Operation order is the reference's
// (this unit is compiled with -ffp-contract=off).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void synchro_hydro_kernel(double *__restrict__ u, const double *__restrict__ f, long N,
                                                             double dteff, double smallr) {
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (long)gridDim.x * blockDim.x) {
    const double d = fmax(u[c], smallr);
    double m[3] = {u[N + c], u[2 * N + c], u[3 * N + c]};
    // remove the kinetic energy (:65-73)
    double pp = u[4 * N + c];
#pragma unroll
    for (int k = 0; k < 3; k++) pp = pp - 0.5 * (m[k] * m[k]) / d;
    // momentum kick (:76-100)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      m[k] = m[k] + d * f[(long)k * N + c] * dteff;
      u[(long)(k + 1) * N + c] = m[k];
    }
    // put the kinetic energy of the new momenta back (:103-113)
#pragma unroll
    for (int k = 0; k < 3; k++) pp = pp + 0.5 * (m[k] * m[k]) / d;
    u[4 * N + c] = pp;
  }
}

__global__ __launch_bounds__(256) void add_gravity_source_kernel(double *__restrict__ un, const double *__restrict__ uo,
                                                                  const double *__restrict__ f, long N, double dt, double smallr) {
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (long)gridDim.x * blockDim.x) {
    const double d = fmax(un[c], smallr);
    double u = un[N + c] / d, v = un[2 * N + c] / d, w = un[3 * N + c] / d;
    double e_kin = 0.5 * d * (u * u + v * v + w * w);
    const double e_prim = un[4 * N + c] - e_kin;
    const double d_old = fmax(uo[c], smallr);
    const double req = 0.0;                                  // strict_equilibrium = 0
    const double fact = (d_old - req) / d * 0.5 * dt;
    u = u + f[c] * fact;
    un[N + c] = d * u;
    v = v + f[N + c] * fact;
    un[2 * N + c] = d * v;
    w = w + f[2 * N + c] * fact;
    un[3 * N + c] = d * w;
    e_kin = 0.5 * d * (u * u + v * v + w * w);
    un[4 * N + c] = e_prim + e_kin;
  }
}

// ---------------------------------------------------------------------------
// Diagnostics of force_fine (poisson/force_fine.f90:158-190) on a level brick: the potential
// energy  sum over leaf cells and directions of fact*f**2  and the maximum of |rho|.  The
// maximum is exact; the sum is a fixed two-stage tree (deterministic; differs from the
// reference's serial loop by rounding only -- epot_tot feeds the energy-conservation print).
// leaf == nullptr: every cell is a leaf.
// ---------------------------------------------------------------------------
constexpr int DIAG_BLOCKS = 512;
__global__ __launch_bounds__(256) void force_diag_kernel(const double *__restrict__ f, const double *__restrict__ rho,
                                                          const int *__restrict__ leaf, long N, double fact,
                                                          double *__restrict__ partial) {
  double e = 0.0, rmax = 0.0;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (long)gridDim.x * blockDim.x) {
    if (!leaf || leaf[c]) {
#pragma unroll
      for (int d = 0; d < 3; d++) { const double v = f[(long)d * N + c]; e = e + fact * (v * v); }
    }
    rmax = __builtin_fmax(rmax, __builtin_fabs(rho[c]));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  e = wave_sum(e);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) rmax = __builtin_fmax(rmax, __shfl_down(rmax, off, 64));
  __shared__ double red[4][2];
  if (lane == 0) { red[wave][0] = e; red[wave][1] = rmax; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double es = red[0][0], rm = red[0][1];
    for (int w = 1; w < 4; w++) { es += red[w][0]; rm = __builtin_fmax(rm, red[w][1]); }
    partial[2 * blockIdx.x] = es;
    partial[2 * blockIdx.x + 1] = rm;
  }
}
__global__ void force_diag_final_kernel(const double *__restrict__ partial, int nblocks, double *__restrict__ out) {
  double es = 0.0, rm = 0.0;
  for (int b = 0; b < nblocks; b++) { es += partial[2 * b]; rm = __builtin_fmax(rm, partial[2 * b + 1]); }
  out[0] = es; out[1] = rm;
}
// partial: 2*DIAG_BLOCKS doubles of scratch; out: {epot, rho_max}
hipError_t launch_force_diag(const double *f, const double *rho, const int *leaf, long N, double fact, double *partial,
                             double *out, hipStream_t s) {
  long g = (N + 255) / 256;
  if (g > DIAG_BLOCKS) g = DIAG_BLOCKS;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(force_diag_kernel, dim3((int)g), dim3(256), 0, s, f, rho, leaf, N, fact, partial);
  hipLaunchKernelGGL(force_diag_final_kernel, dim3(1), dim3(1), 0, s, partial, (int)g, out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// force_fine's analytic branch on a level brick (gravity_type 1 | 2, csrc/gravana_core.hpp): cell c = i + n (j + n k) has its
// centre at (i + 0.5) dx in code units -- exact, so it carries the bits of the reference's xg + xc -- and force_fine's
// rescaling (x - skip) * scale follows.  One lane per cell.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gravana_brick_kernel(GravAna G, int n, double dx, double *__restrict__ f) {
  const long N = (long)n * n * n;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (long)gridDim.x * blockDim.x) {
    const int i = (int)(c % n), j = (int)((c / n) % n), k = (int)(c / ((long)n * n));
    const double x[3] = {(((double)i + 0.5) * dx - G.skip[0]) * G.scale, (((double)j + 0.5) * dx - G.skip[1]) * G.scale,
                         (((double)k + 0.5) * dx - G.skip[2]) * G.scale};
    double ff[3];
    gravana_cell(G, x, ff);
    f[c] = ff[0]; f[N + c] = ff[1]; f[2 * N + c] = ff[2];
  }
}

// ---------------------------------------------------------------------------
// cooling_fine of a barotropic run without cooling on a level brick (csrc/eos_core.hpp): every cell of a fully refined level is
// a leaf, so the total energy of each interior cell is rewritten from its density and momenta.  One lane per cell, 4 reads and 1
// write; the ghost layers (a brick of the MPI-resident level has them) and every other variable are left alone.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void eos_brick_kernel(EosBrickArgs A) {
  const long N = (long)A.nx * A.ny * A.nz;
  for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < N; c += (long)gridDim.x * blockDim.x) {
    const int i = (int)(c % A.nx), j = (int)((c / A.nx) % A.ny), k = (int)(c / ((long)A.nx * A.ny));
    double *u = A.u + A.off + i + (long)j * A.pitch_y + (long)k * A.pitch_z;
    u[4 * A.pitch_var] = eos_energy(A.C, u[0], u[A.pitch_var], u[2 * A.pitch_var], u[3 * A.pitch_var], A.smallr, A.gamma);
  }
}

static inline int misc_grid(long work) {
  long g = (work + 255) / 256;
  if (g < 1) g = 1;
  if (g > 8192) g = 8192;
  return (int)g;
}
hipError_t launch_synchro_hydro(double *u, const double *f, long N, double dteff, double smallr, hipStream_t s) {
  hipLaunchKernelGGL(synchro_hydro_kernel, dim3(misc_grid(N)), dim3(256), 0, s, u, f, N, dteff, smallr);
  return hipGetLastError();
}
hipError_t launch_add_gravity_source(double *unew, const double *uold, const double *f, long N, double dt, double smallr,
                                     hipStream_t s) {
  hipLaunchKernelGGL(add_gravity_source_kernel, dim3(misc_grid(N)), dim3(256), 0, s, unew, uold, f, N, dt, smallr);
  return hipGetLastError();
}
hipError_t launch_gravana_brick(const GravAna &G, int n, double dx, double *f, hipStream_t s) {
  hipLaunchKernelGGL(gravana_brick_kernel, dim3(misc_grid((long)n * n * n)), dim3(256), 0, s, G, n, dx, f);
  return hipGetLastError();
}
hipError_t launch_eos_brick(const EosBrickArgs &A, hipStream_t s) {
  if (A.nx < 1 || A.ny < 1 || A.nz < 1) return hipSuccess;
  hipLaunchKernelGGL(eos_brick_kernel, dim3(misc_grid((long)A.nx * A.ny * A.nz)), dim3(256), 0, s, A);
  return hipGetLastError();
}

}  // namespace ramses_amd

#include "warm.hpp"
RAMSES_AMD_TU_WARM(hydro_misc)

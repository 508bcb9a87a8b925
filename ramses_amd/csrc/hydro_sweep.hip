// hydro_sweep.hip -- the Godunov sweep of one fully refined level brick on
// MI355X (gfx950): set_unew + godunov_fine/godfine1 + unsplit fused in one
// kernel (reference: hydro/godunov_fine.f90:5-130,486-911, hydro/umuscl.f90).
//
// Design (see DESIGN.md "Godunov sweep kernel"):
//  * a workgroup owns a (64-4) x (BY-4) column tile in (x,y) and MARCHES along
//    z; one wavefront = one y row of 64 x-columns, so every HBM access of a
//    wave is a contiguous 512 B row segment;
//  * the primitive planes c-1, c, c+1 live in an LDS ring (y/x neighbours and
//    the thread's own z neighbours are LDS reads); the traced +y state and the
//    y flux cross waves through LDS; the traced +x state and the x flux cross
//    lanes with wavefront DPP shifts (no LDS); the z direction stays in
//    registers (previous plane's +z state, z flux, partial update);
//  * every cell is converted to primitives once, traced once, and every
//    interface flux is computed once per tile (the reference recomputes a 6^3
//    stencil per 2^3 oct: 27x load and ~8x flop redundancy);
//  * halo rows exit early by role (wave-uniform), so the 2-cell ghost ring
//    costs ctoprim+trace only;
//  * uold is read once from HBM (+ tile halo and one L2 re-read) and unew
//    written once: 80 B per cell update algorithmic HBM traffic.
//
// Compiled twice: strict (-ffp-contract=off, reference operation order,
// bit-identical to the reference) and fast (-DRAMSES_AMD_FAST: FMA
// contraction, rcp/rsq-based division and square root, fused LLF).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "difmag_core.hpp"
#include "hydro_core.hpp"
#include "sweep_args.hpp"

namespace ramses_amd {

#ifdef RAMSES_AMD_FAST
#define SWEEP_NS fastmode
#else
#define SWEEP_NS strictmode
#endif

namespace SWEEP_NS {

constexpr int BX = 64;   // lanes along x = one wavefront
#ifndef TILE_SWEEP_BY
#define TILE_SWEEP_BY 12   // rows of a workgroup of the sweep of a level in tiles (8: two waves per SIMD, 256 VGPRs)
#endif

// LDS plane of NV doubles per column: [n][ty][tx]; NV = rho, u, v, w, P + passive scalars
template <int BY, int NV>
struct Plane {
  double v[NV][BY][BX];
};

// The LDS of a workgroup.  The primitives of plane c-1 are read by their own column only (the z slope), so unless the 27-point
// slope is in use the ring holds TWO planes: plane c+1 takes the slot of plane c-1 once the thread has taken its z slope
// (nobody else reads that slot between the barrier of iteration c-1 and the one of iteration c).  PARK (the sweep of a level
// in tiles, and the 12-row kernels with gravity: both spill otherwise): the partial update of plane c-1 that the full rows carry
// across the trace of plane c -- u + x flux difference and the own -y flux -- waits in LDS instead of in 20 VGPRs; the y slots
// then hold the rows that use them (1 .. BY-2) only.
// (NX: components that ride beside the NV fluxes through the y slots and the parked partial update -- the two face quantities
// of pressure_fix)
// (DUTY: the two slot planes of one row -- y_duty below -- through which row 2 hands its -y face to the wave of row 0)
// (R3: three ring planes whatever the slope type -- difmag, whose corner divergences read the neighbours' planes c and c+1 AFTER
//  the barrier, while the quickest waves already write plane c+2)
// (DPN: doubles per column of a full row that the difmag kernels park beside it -- dif_parked() below)
template <int ST, int BY, int NV, bool MASK, bool GRAV, int NX = 0, bool DUTY = false, bool R3 = false, int DPN = 0>
struct Lds {
  static constexpr int NF = NV + NX;
  static constexpr int RING = (ST == 3 || R3) ? 3 : 2;
#ifndef SWEEP_PARK_PLAIN
#ifdef RAMSES_AMD_FAST
#define SWEEP_PARK_PLAIN 1     // the fast 12-row kernels park too: with the plane held in registers (KEEP) 3.23 -> 3.08 ms at 512^3
#else
#define SWEEP_PARK_PLAIN 0     // (the strict ones do not: 5.40 -> 5.50 ms; profiles/r06_ab_sweep.txt)
#endif
#endif
  static constexpr bool PARK = MASK || ((GRAV || SWEEP_PARK_PLAIN) && BY == 12);
  static constexpr int MR = PARK ? BY - 2 : BY;          // rows of a y slot plane
  static constexpr int M0 = PARK ? 1 : 0;                // first row that owns a slot
  static constexpr size_t q_off = 0;
  static constexpr size_t m_off = q_off + RING * sizeof(Plane<BY, NV>);
  static constexpr size_t park_off = m_off + 2 * sizeof(Plane<MR, NF>);
  static constexpr size_t duty_off = park_off + (PARK ? sizeof(double) * 2 * NF * (BY - 4) * BX : 0);   // DUTY: [2][NF][BX], by plane parity
  static constexpr size_t mask_off = duty_off + (DUTY ? sizeof(double) * 2 * NF * BX : 0);   // MASK: [3][BY][BX] status bytes
  static constexpr size_t sloc_off = mask_off + (MASK ? 3 * BY * BX : 0);                                // MASK: [BY][BX] lane part of the cell index
  static constexpr size_t dpark_off = sloc_off + (MASK ? 4 * BY * BX : 0);                               // DPN: [DPN][BY - 4][BX]
  static constexpr size_t bytes = dpark_off + sizeof(double) * DPN * (BY - 4) * BX;
};
// difmag: what a full row carries from plane to plane waits in LDS where the registers run out and the LDS has room -- the
// Newton solver (it spills otherwise, NV = 5 too) and NV = 6: the z flux of plane c-1's face and the two corner divergences
// (NV + 2 doubles), at NV = 5 the +z traced state as well (2 NV + 2).  NV = 7 fills the LDS with its three ring planes.
template <int RS, int NV>
constexpr int dif_parked() { return (NV == 5 && RS == RIEMANN_EXACT) ? 2 * NV + 2 : ((NV == 6) ? NV + 2 : 0); }

// wavefront shift by one lane: lane i receives the value of lane i-1 (shr) or
// i+1 (shl).  shr: lane 0 keeps its own value.  shl: lane 63 receives 0 (old = 0, bound_ctrl) -- the shift then writes a fresh
// register and a source that stays live (px = ucur + (fx - wave_shl1(fx))) is not copied first, ten v_mov_b32 per plane of a
// full row; shr's sources are dead at the shift and are shifted in place.  Either edge lane is a halo lane: a cell is owned
// by lanes 2 .. 61 (r_upd: sweep_march, the tile kernels and scalar_march alike) and only those store.  The one thing lane 63
// gets from a left shift is the -x face flux "of column 64" in its own x flux difference: that ends in lane 63's own partial
// update (px -> registers or park[..][63], read by lane 63 alone) and is dropped by the store's range check.  No other lane
// reads it: shr hands lane 63's values to nobody, and what lane 62 takes from lane 63 (fx) is unshifted.
__device__ __forceinline__ double wave_shr1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, 0x138, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, 0x138, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// (TIED: the shift as it was, lane 63 keeps its own value -- for the difmag tile kernels, strict only and at 256 VGPRs with
// scratch: the untied form costs their NV = 6, 7 instantiations 4 - 8 B more of it.  There lane 63's corner divergences at
// tx+1, and through them the coefficients of its own y and z faces, come from a left shift too, with the same fate: lane 63's
// own fluxes, parked or in the y slots at [..][63], which lane 63 of rows ty-1 and ty+1 reads)
template <bool TIED = false>
__device__ __forceinline__ double wave_shl1(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = TIED ? __builtin_amdgcn_update_dpp(lo, lo, 0x130, 0xf, 0xf, false) : __builtin_amdgcn_update_dpp(0, lo, 0x130, 0xf, 0xf, true);
  hi = TIED ? __builtin_amdgcn_update_dpp(hi, hi, 0x130, 0xf, 0xf, false) : __builtin_amdgcn_update_dpp(0, hi, 0x130, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// Row roles.  One wave = one tile row, and what a row has to produce depends
// only on its position in the tile, so each role gets its own straight-line
// instantiation of the marching loop (no per-plane role branches, no dead
// results kept alive); all of them execute the same barriers.
//   ROLE_HALO    : row 0        primitives only
//   ROLE_LOW     : row 1        + slopes, the traced +y state (left state of row 2's y flux)
//   ROLE_FULL    : rows 2..BY-3 everything, and the update
//   ROLE_HIGH    : row BY-2     + slopes, the y flux through its -y face (the +y face flux of row BY-3)
//   ROLE_HALO_HI : row BY-1     primitives only
//   ROLE_FULL_LO : row 2 where the y fluxes are shared out (SWEEP_YDUTY): a full row whose -y face flux another wave computes
enum { ROLE_HALO = 0, ROLE_LOW = 1, ROLE_HIGH = 2, ROLE_FULL = 3, ROLE_HALO_HI = 4, ROLE_FULL_LO = 5 };

// Who computes which y flux: an A/B knob, OFF (measured, and slower: below).  The hardware deals the 12 waves of a workgroup
// round the four SIMDs, rows r, r+4 and r+8 together (profiles/r07_sweep_balance.txt), so every SIMD holds two full rows, one
// of them row BY-2 -- slopes, trace and a y flux, half a full row -- on top, and two of them a halo row, which converts a plane
// and waits at the barrier for 70 - 95 % of it.  The flux through a y face needs nothing its row keeps in registers but the
// row's -y traced state, and both its inputs and its result already cross waves through the slots, so WHICH wave computes it
// is a table:
//   face f (between rows f-1 and f), f = 2 .. BY-2  ->  wave yflux_wave(f)
// With SWEEP_YDUTY=1 face 2 goes to the wave of row 0 and face BY-2 to the wave of row BY-1.  A row that hands its -y face
// away writes its -y state to a slot before the barrier -- row BY-2 into its own +y slot, which nobody reads; row 2 into a
// slot pair of its own, Lds::duty_off -- the computing wave reads both states after the barrier, calls the same flux routine
// on the same values and leaves the result where the rows beside the face read it after the NEXT barrier: face BY-2 in row
// BY-3's slot as before, face 2 over row 2's -y state (row 1 takes no flux).  Every slot is rewritten only by the wave that
// last read it, or a barrier later: still ONE barrier per plane, the same bits (tests/test_sweep_rebalance_gpu.py).
// Measured at 512^3, five alternating runs each: 2.975 -> 3.136 ms with the duties shared out (2.939 -> 3.088 with the trims
// below) although the busiest SIMD issues 7 % fewer VALU instructions per plane: rows 6 and 8, which close the barrier
// with or without it, take 17 - 23 % longer from the barrier to the loop end once a flux is computed beside them.
// (Round 2 found the same with face BY-2 alone on a much earlier kernel, profiles/r02_ab_sweep.txt.)
#ifndef SWEEP_YDUTY
#define SWEEP_YDUTY 0
#endif
template <int ST, int RS, int BY, bool GRAV, int SCHEME, int NV, bool MASK, int NE = 0, bool PFIX = false>
constexpr bool y_duty() {
  return SWEEP_YDUTY && SWEEP_PARK_PLAIN && RS == RIEMANN_LLF && BY == 12 && ST != 3 && !GRAV && SCHEME == 0 && NV == 5 && !MASK && NE == 0 && !PFIX;
}
template <int BY, bool DUTY>
constexpr int yflux_wave(int f) { return !DUTY ? f : (f == 2 ? 0 : (f == BY - 2 ? BY - 1 : f)); }

// The trims of the full rows' instruction stream (fast build, muscl): the interface fluxes skip the density floor of states
// that trace3d_cell has floored already (hydro_core.hpp llf_flux_fast FLOORED), and the trace takes 1 / rho from the
// ctoprim_cell of the same cell one iteration earlier instead of a second v_rcp_f64 + Newton step: 503 -> 489 VALU
// instructions per plane of a full row (12 v_max_f64, one v_rcp_f64, two FMAs less, one copy more), 154 VGPRs as before, same
// bits; 512^3 LLF + minmod 2.975 -> 2.939 ms (medians of five alternating runs, profiles/r07_sweep_balance.txt).
#ifndef SWEEP_TRIM
#ifdef RAMSES_AMD_FAST
#define SWEEP_TRIM 1
#else
#define SWEEP_TRIM 0
#endif
#endif
// The loop's bookkeeping (sweep_march BOOK: the fast LLF 12-row kernels of the brick, slope types 1 and 7): the ring addresses
// of a tracing row from one lane register and immediate offsets (LB), the store's lane offset switched on once (SO1): 605 ->
// 593 instructions per plane of a full row of the fast minmod kernel (468 -> 460 VALU), 152 VGPRs as before, same bits; 512^3
// LLF + minmod 2.925 -> 2.892 ms (medians of five alternating runs), below the bar of three spreads.  Carried plane offsets without the wrap ladders, and the y slots and the
// parked update through such registers, shorten the listing to 549 instructions and measured SLOWER (2.93 -> 3.12 and 3.03
// ms): left out, the numbers are in profiles/r09_sweep_bookkeeping.txt.

// SWEEP_CYCLE_PROBE=1 (a build of its own, never the shipped one: with 0 nothing of it is compiled): every wave sums, per
// plane, the shader clocks from the loop top to the barrier, inside the barrier and from the barrier to the loop end, and
// lane 0 leaves the sums with the wave's row and its HW_ID register (SIMD: bits 5:4) per (block, row) after the march;
// scripts/sweep_probe.py --balance reads them back through ramses_amd_sweep_cycle_probe.
#ifndef SWEEP_CYCLE_PROBE
#define SWEEP_CYCLE_PROBE 0
#endif
#if SWEEP_CYCLE_PROBE
constexpr int PROBE_BLOCKS = 8192, PROBE_ROWS = 12, PROBE_WORDS = 6;
static __device__ unsigned long long sweep_cycle_probe[PROBE_BLOCKS][PROBE_ROWS][PROBE_WORDS];
#endif

// Raw buffer access: one scalar resource descriptor per variable (base of the
// variable's brick), a wave-uniform byte offset of the plane (soffset) and one
// 32-bit lane byte offset of the column, so that all address arithmetic of the
// marching loop is scalar.  A lane offset beyond num_records makes the hardware
// drop that lane's store: masked lanes and masked iterations need no branch,
// every memory instruction of the loop is issued unconditionally, and the
// compiler's vmcnt bookkeeping never has to wait for a store to be acknowledged
// before it can use a prefetched load.
typedef unsigned int v2u32 __attribute__((ext_vector_type(2)));
constexpr unsigned BUF_RANGE = 0x7fffffffu;     // lane offsets below this are in range
constexpr unsigned BUF_OOB = 0xffffffffu;       // dropped by the range check
#ifndef SWEEP_STORE_AUX
#define SWEEP_STORE_AUX 0     // cache policy of the stores of unew (gfx950: 1 sc0, 2 nt, 16 sc1); A/B knob, profiles/r06_store_policy.txt
#endif
__device__ __forceinline__ double plane_load(const double *var_base, unsigned plane_bytes, unsigned off) {
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(var_base), 0, BUF_RANGE, 0x00020000);
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(r, off, plane_bytes, 0));
}
__device__ __forceinline__ void plane_store(double *var_base, unsigned plane_bytes, unsigned off, double x) {
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(var_base, 0, BUF_RANGE, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32, x), r, off, plane_bytes, SWEEP_STORE_AUX);
}

// LDS through an address register and an immediate offset, both chosen by hand (sweep_march, the ring reads of a tracing
// row).  lds_reg() hands the compiler an address it cannot take apart again: what is added to it afterwards is a constant
// and goes into the instruction's offset field, and two accesses whose offsets are multiples of 512 pair into one
// ds_read2st64 / ds_write2st64 without a new base register.
typedef __attribute__((address_space(3))) double lds_f64;
__device__ __forceinline__ unsigned lds_reg(unsigned a) {
  asm("" : "+v"(a));
  return a;
}
__device__ __forceinline__ unsigned lds_addr(const void *p) {
  return (unsigned)(size_t)(const __attribute__((address_space(3))) unsigned char *)p;
}
__device__ __forceinline__ double lds_ld(unsigned reg, unsigned imm) { return *(const lds_f64 *)(size_t)(reg + imm); }
__device__ __forceinline__ void lds_st(unsigned reg, unsigned imm, double x) { *(lds_f64 *)(size_t)(reg + imm) = x; }

__device__ __forceinline__ int wave_shr1_i(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ int wave_shl1_i(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, true); }   // (lane 63: 0, as wave_shl1)
// status byte of a cell: lane part and wave-uniform part of the cell index; a lane without a tile (index beyond ncell) reads 0
__device__ __forceinline__ int stat_load(const unsigned char *base, unsigned ncell, unsigned lane_cell, unsigned plane_cell) {
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char *>(base), 0, ncell, 0x00020000);
  return (int)__builtin_amdgcn_raw_buffer_load_b8(r, lane_cell, plane_cell, 0);
}
// the tile directory entry of (tile column of the lane, tile plane): col and plane in ints
__device__ __forceinline__ int dir_load(const int *base, unsigned plane_ints, unsigned col) {
  __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(base), 0, BUF_RANGE, 0x00020000);
  return (int)__builtin_amdgcn_raw_buffer_load_b32(r, col * 4u, plane_ints * 4u, 0);
}

// MASK: the sweep of a level of a resident AMR run IN PLACE on the device's cell vectors (see SweepArgs::stat / dir / work):
// the level is stored in tiles of 32 x 4 x 4 octs, a lane finds the cell of its (plane, column) through the tile directory
// (one 4-byte load per 8 planes, issued four planes ahead; 256-byte runs of a variable along x inside a tile), the status byte of
// the cell says whether it is refined (fluxes reset), updated (stored) or a ghost (interpolated: fluxes filed for the coarser level)
// PFIX (MASK, strict arithmetic only): pressure_fix -- the face velocity and the internal-energy flux of every interface
// (hydro/umuscl.f90:843-850) ride beside the NV fluxes as components NV and NV + 1 through the same differencing and the same
// resets, and land in divu / enew of the cells whose unew is stored (hydro/godunov_fine.f90:720-790)
// DIFMAG: the conserved variables of one cell of a level in tiles again (pb: the plane's part of the cell index in bytes, off: the
// lane's): an L2 hit.  (Free functions, not lambdas of sweep_march: what difmag needs stays out of the scope that every
// instantiation of sweep_march compiles, so that the kernels without difmag stay the code they were.)
template <int NV>
__device__ __forceinline__ void load_uold_cell(const double *uold, long pitch_var, unsigned odd_var, unsigned pb, unsigned off, double (&u)[NV]) {
#pragma unroll
  for (int n = 0; n < NV; n++) u[n] = plane_load(uold + (long)(n & ~1) * pitch_var, pb + (n & 1) * odd_var, off);
}
// the tile base of row ty-1's cell: by z-tile parity and x-tile A / B, as sweep_march's tbp picks the row's own
__device__ __forceinline__ unsigned tile_base_ym(int par, bool inB, unsigned a0, unsigned a1, unsigned b0, unsigned b1) {
  const unsigned a = par ? a1 : a0, b = par ? b1 : b0;
  return inB ? b : a;
}
// DIFMAG (MASK, strict arithmetic only): difmag > 0 -- cmpdivu / consup of csrc/difmag_core.hpp.  The diffusive term of a face
// needs the velocity divergence at the face's four corners, and the corners of plane c+1 need the neighbours' primitives of
// plane c+1, which the ring shows after the barrier only.  So the x and z fluxes of phase A cross the barrier as they are, and
// phase B finishes all three: every thread takes the corners (tx, ty) and (tx, ty+1) of plane c+1 from the velocities of planes
// c and c+1 in the ring -- its own column from LDS, column tx-1 by DPP -- keeps them for the next plane (where they are the
// corners of plane c), gets the corners at tx+1 by DPP, adds the term to each flux BEFORE the reset at refined cells and the
// differencing, and goes on as without difmag.  No corner array in LDS and no second barrier; the price is a third ring plane
// (Lds R3), 18 LDS reads and the conserved variables of plane c (own, row ty-1) and c-1 (own) read again from L2.
template <int ST, int RS, int BY, bool GRAV, int SCHEME, int NV, int ROLE, bool MASK, int NE = 0, bool PFIX = false, bool DIFMAG = false>
__device__ __forceinline__ void sweep_march(const SweepArgs &A, unsigned char *smem_raw, const SweepPfix &X = SweepPfix(),
                                            const SweepDifmag &D = SweepDifmag()) {
  static_assert(!PFIX || (MASK && NE == 0 && SCHEME == 0), "pressure_fix: the sweep of a level in tiles, muscl");
  static_assert(!DIFMAG || (MASK && NE == 0 && SCHEME == 0 && !PFIX), "difmag: the sweep of a level in tiles, muscl, no pressure_fix");
  constexpr int NF = NV + (PFIX ? 2 : 0);   // components differenced
  const bool DXPOW2 = A.pow2 != 0;   // uniform
  constexpr bool DUTY = y_duty<ST, RS, BY, GRAV, SCHEME, NV, MASK, NE, PFIX>();
  static_assert(DUTY || ROLE != ROLE_FULL_LO, "row 2 is a full row like the others unless the y fluxes are shared out");
  constexpr int DPN = DIFMAG ? dif_parked<RS, NV>() : 0;
  typedef Lds<ST, BY, NV, MASK, GRAV, NF - NV, DUTY, DIFMAG, DPN> L;
  double (*dpark)[BY - 4][BX] = reinterpret_cast<double (*)[BY - 4][BX]>(smem_raw + L::dpark_off);   // DPN: fzlo, the two corners (, qmz) of the full rows
  constexpr int RING = L::RING;
  constexpr bool PARK = L::PARK;
  constexpr int M0 = L::M0;
  Plane<BY, NV> *qring = reinterpret_cast<Plane<BY, NV> *>(smem_raw + L::q_off);  // [RING] primitives of planes c-1, c (, c+1)
  Plane<L::MR, NF> *mring = reinterpret_cast<Plane<L::MR, NF> *>(smem_raw + L::m_off);   // [2] +y traced state / y flux slots, by plane parity
  double (*park)[BY - 4][BX] = reinterpret_cast<double (*)[BY - 4][BX]>(smem_raw + L::park_off);   // PARK: [2 NF] of the full rows
  double (*yduty)[NF][BX] = reinterpret_cast<double (*)[NF][BX]>(smem_raw + L::duty_off);           // DUTY: [2] row 2's -y state / -y flux, by plane parity

  const int tx = threadIdx.x, ty = threadIdx.y;
  const HydroConst &P = A.P;

  // ---- tile decode (XCD-aware: block b runs on XCD b%8; give each XCD a
  // contiguous run of tiles so the halo re-reads of neighbouring tiles hit
  // the same L2) -------------------------------------------------------------
  // a launch covers up to 6 boxes of tiles x planes (one for a whole-brick or
  // interior sweep, six for the boundary shell); find this block's box (uniform)
  const int hb = blockIdx.x;
  int bi = 0;
#pragma unroll
  for (int i = 1; i < 6; i++)
    if (i < A.nbox && hb >= A.box[i].first) bi = i;
  const SweepBox &B = A.box[bi];
  // XCD-aware: block b runs on XCD b%8; inside its box a block is handed a tile so that each XCD works on a contiguous
  // run of them (neighbouring tiles then re-read each other's halo rows and columns in ONE L2) -- box by box, because the
  // blocks of different boxes cost very differently (the shell's 2-plane slabs next to its 32-plane columns) and every
  // XCD has to get its share of each kind: one run over the whole shell launch left five XCDs with the slabs (shell
  // 1.29 -> 1.04 ms at 512^3, the overlapped step 4.23 -> 4.00 ms)
  int lb = hb - B.first;
  {
    const int nxcd = 8;
    const int cnt = (bi + 1 < A.nbox ? A.box[bi + 1].first : (int)gridDim.x) - B.first;
    if (cnt % nxcd == 0) {
      const int per = cnt / nxcd;
      lb = (lb % nxcd) * per + lb / nxcd;
    }
  }
#ifndef SWEEP_TILE_YFAST
#define SWEEP_TILE_YFAST 0     // A/B knob: tiles of a box in y-first order (profiles/r06_store_policy.txt)
#endif
#if SWEEP_TILE_YFAST
  const int tiy = B.ty0 + lb % B.nty;
  const int tix = B.tx0 + (lb / B.nty) % B.ntx;
#else
  const int tix = B.tx0 + lb % B.ntx;
  const int tiy = B.ty0 + (lb / B.ntx) % B.nty;
#endif
  const int tiz = lb / (B.ntx * B.nty);
  int x0 = tix * (BX - 4);
  int y0 = tiy * (BY - 4);
  int z0 = B.zlo + tiz * B.zchunk;
  int z1 = min(z0 + B.zchunk, B.zhi);
  if (MASK) {
    // the launch's work list (the host put it in the order the XCDs should see it)
    const int4 w = reinterpret_cast<const int4 *>(A.work)[hb];
    x0 = w.x; y0 = w.y; z0 = w.z; z1 = w.w;
  }

  // ---- this thread's column ------------------------------------------------
  const int xu = x0 - 2 + tx;  // unwrapped interior coordinate
  const int yu = y0 - 2 + ty;
  int xi, yi;
  if (A.ng == 0) {
    xi = xu < 0 ? xu + A.nx : (xu >= A.nx ? xu - A.nx : xu);
    xi = xi >= A.nx ? xi % A.nx : xi;
    yi = yu < 0 ? yu + A.ny : (yu >= A.ny ? yu - A.ny : yu);
    yi = yi >= A.ny ? yi % A.ny : yi;
  } else {
    xi = min(max(xu, -A.ng), A.nx + A.ng - 1) + A.ng;
    yi = min(max(yu, -A.ng), A.ny + A.ng - 1) + A.ng;
  }
  // column offset inside a plane as a 32-bit lane value; plane/variable bases
  // are wave-uniform (scalar base + 32-bit lane offset addressing)
  // (byte offset < 2 GB per plane, checked by the launcher)
  const unsigned colb = (unsigned)(xi + yi * (int)A.pitch_y) * 8u;
  // MASK (the level in tiles, periodic box, ng = 0): the lane's tile column in a plane of the directory, its part of the
  // cell index inside a tile (octant bits of x and y at stride ngd, oct column and oct row) and of the octant position
  // Everything about the tiles is wave-uniform except the lane's place inside one: a row of 64 lanes lies in one tile row and
  // in (at most) two neighbouring tiles along x, so the directory entries are SCALAR loads into scalar registers, the lane
  // picks one of two with a constant lane mask, and the lane's own part of the cell index is parked in LDS -- the marching
  // loop is at its register limit, and a vector register spilled to scratch costs a full vmcnt(0) drain per use.
  int tyu = 0, yis = 0, xa = 0, tA = 0, tB = 0, drow = 0;
  bool inB = false;
  unsigned *sloc = reinterpret_cast<unsigned *>(smem_raw + L::sloc_off);   // MASK: [BY][BX] lane part of the cell index (bytes)
  if (MASK) {
    tyu = __builtin_amdgcn_readfirstlane(ty);
    const int ys = y0 - 2 + tyu;
    yis = ys < 0 ? ys + A.ny : (ys >= A.ny ? ys - A.ny : ys);
    const int xs = x0 - 2;
    xa = xs < 0 ? xs + A.nx : xs;                      // column of lane 0 (x0 < nx)
    tA = xa >> 6; tB = tA + 1 < A.ntx ? tA + 1 : 0;
    inB = (xa & 63) + tx >= 64;
    drow = A.ntx * (yis >> 3);
    const int lind = (xi & 1) + 2 * (yis & 1);
    sloc[ty * BX + tx] = ((unsigned)((long)lind * A.ngd) + (unsigned)(((xi >> 1) & (TILE_OX - 1)) + TILE_OX * ((yis >> 1) & (TILE_OY - 1)))) * 8u;
  }
  const double *__restrict__ uold = A.uold;
  double *__restrict__ unew = A.unew;
  const double *__restrict__ grav = A.grav;

#ifndef SWEEP_LATE_BASE
#define SWEEP_LATE_BASE 0      // (measured on MI355X, round 6: 512^3 fast 3.237 -> 3.272 ms, the tiled 256^3 level unchanged: the wait at the x flux is not what costs)
#endif
  constexpr bool LATE = SWEEP_LATE_BASE && NV == 5;   // (the passive-scalar fix of NV > 5 wants the old state in phase A)
  // KEEP (the fast build of the sweep of a level in tiles: the instantiations with ten registers to spare): the
  // conservative state of plane c+1 is held from its arrival to the x flux of the NEXT iteration, where the update of that plane
  // starts from it -- on a level that starts from uold (base_uold) the re-read of the plane disappears: 5 of the 11 loads a full
  // lane issues per plane.  That kernel is bound by L2 misses, not by instruction issue (profiles/r06_tile_sweep_pmc.txt).
#ifndef SWEEP_KEEP_PLAIN
#define SWEEP_KEEP_PLAIN 1     // the plain fast 12-row kernel holds the plane too instead of re-reading it from L2 (profiles/r06_ab_sweep.txt)
#endif
#ifndef SWEEP_KEEP_STRICT
#define SWEEP_KEEP_STRICT 0    // (A/B knob: the strict build holds the plane too)
#endif
#if defined(RAMSES_AMD_FAST) || SWEEP_KEEP_STRICT
#ifndef SWEEP_KEEP_LLF_ONLY
#define SWEEP_KEEP_LLF_ONLY 0   // A/B knob: only the LLF kernels hold the plane (the others are at the register limit without it)
#endif
#ifndef SWEEP_KEEP_NOT_HLLC
#define SWEEP_KEEP_NOT_HLLC 1   // the HLLC kernels do not hold the plane: with the fused fast HLLC flux they are at the register limit (hydro_core.hpp hllc_flux_fast)
#endif
  constexpr bool KEEP = (MASK || (SWEEP_KEEP_PLAIN && BY == 12)) && NV == 5 && !LATE && (!SWEEP_KEEP_LLF_ONLY || RS == RIEMANN_LLF) &&
                        (!SWEEP_KEEP_NOT_HLLC || RS != RIEMANN_HLLC);
#else
  constexpr bool KEEP = false;
#endif
  constexpr bool r_fxz = ROLE == ROLE_FULL || ROLE == ROLE_FULL_LO;
  constexpr bool r_trace = ROLE == ROLE_LOW || ROLE == ROLE_HIGH || r_fxz;
  // the y flux duties (yflux_wave): the flux through this row's -y face is another wave's / this wave computes the flux of face DUTY_F
  constexpr bool y_give = DUTY && (ROLE == ROLE_FULL_LO || ROLE == ROLE_HIGH);
  constexpr bool y_take = DUTY && (ROLE == ROLE_HALO || ROLE == ROLE_HALO_HI);
  constexpr int DUTY_F = ROLE == ROLE_HALO ? 2 : BY - 2;
  static_assert(!DUTY || (yflux_wave<BY, DUTY>(2) == 0 && yflux_wave<BY, DUTY>(BY - 2) == BY - 1 && yflux_wave<BY, DUTY>(3) == 3),
                "the roles below implement this table");
  // (the traced states of trace3d_cell are floored: llf_flux_fast FLOORED; 1 / rho rides from ctoprim_cell to the trace)
  // (the LLF kernels: the others sit at their register limit and keep the instructions they had)
  constexpr bool TRIM = SWEEP_TRIM != 0 && RS == RIEMANN_LLF && SCHEME == 0 && NE == 0 && !PFIX;
  // BOOK: the kernels whose marching loop takes the two bookkeeping steps below (LB, SO1) -- the fast LLF 12-row kernels of
  // the brick without gravity with the minmod and the type-7 slopes, which keep their VGPR counts (152, 144).  Everywhere else
  // the loop stays the code it was: slope types 0, 2 and 8 of the same family would take one or two VGPRs more (150 -> 151,
  // 144 -> 146), and the strict 12-row kernels, HLLC, gravity, the 8-row and the tile kernels sit at 166 - 168 or 256 VGPRs,
  // where a changed schedule costs scratch.  (What LB and SO1 carry from trip to trip is declared before the loop like the
  // rest of the carried state; where BOOK is false nothing reads it and none of it is compiled.)
#ifdef RAMSES_AMD_FAST
  constexpr bool BOOK = (ST == 1 || ST == 7) && RS == RIEMANN_LLF && BY == 12 && !GRAV && SCHEME == 0 && NV == 5 && !MASK && NE == 0 &&
                        !PFIX && !DIFMAG;
#else
  constexpr bool BOOK = false;
#endif
  const bool r_upd = r_fxz && (tx >= 2) && (tx <= BX - 3) && (xu < A.nx) && (yu < A.ny);
  const unsigned colb_upd = r_upd ? colb : BUF_OOB;   // lanes that own no cell store nowhere

  const double dtdx = A.dt / A.dx;
  const double dtxhalf = A.dt * 0.5;

  auto plane_off = [&](int p) -> unsigned {   // uniform byte offset of plane p inside a variable
    int pz;
    if (A.ng == 0) { pz = p < 0 ? p + A.nz : (p >= A.nz ? p - A.nz : p); }
    else { pz = p + A.ng; }
    return (unsigned)pz * (unsigned)(A.pitch_z * 8);
  };
  auto wrap_z = [&](int p) -> int { return p < 0 ? p + A.nz : (p >= A.nz ? p - A.nz : p); };
  // MASK: a cell's index in a cell vector = tile base (scalar: sdir, by z-tile parity and x-tile A / B) + the lane's part
  // (LDS) + the plane's part (scalar, rides in the scalar offset of the buffer instructions).  TILE_VOID where the level has
  // no tile: with the lane's part still beyond every buffer range, so such a lane loads zeros and stores nothing.
  constexpr unsigned TILE_VOID = 0x80000000u;
  unsigned sA0 = TILE_VOID, sA1 = TILE_VOID, sB0 = TILE_VOID, sB1 = TILE_VOID;    // (four scalars: an indexed local array would live in scratch)
  unsigned mA0 = TILE_VOID, mA1 = TILE_VOID, mB0 = TILE_VOID, mB1 = TILE_VOID;    // DIFMAG: the same of row ty-1 (another tile row where yis % 8 == 0)
  int drow_m = 0;
  if constexpr (DIFMAG) {
    const int ym = yis > 0 ? yis - 1 : A.ny - 1;
    drow_m = A.ntx * (ym >> 3);
  }
  auto tile_of_plane = [&](int p) -> int { return wrap_z(p) >> 3; };
  auto tile_set = [&](int tz) {
    // (through the constant address space: the directory is not written during the launch, and only such a load is scalar)
    typedef const int __attribute__((address_space(4))) *cdir_p;
    const cdir_p row = (cdir_p)(A.dir + (long)tz * (A.ntx * A.nty) + drow);
    const int ra = row[tA], rb = row[tB];
    const unsigned a = ra < 0 ? TILE_VOID : (unsigned)ra * 8u, b = rb < 0 ? TILE_VOID : (unsigned)rb * 8u;
    if (tz & 1) { sA1 = a; sB1 = b; } else { sA0 = a; sB0 = b; }
    if constexpr (DIFMAG) {
      const cdir_p rowm = (cdir_p)(A.dir + (long)tz * (A.ntx * A.nty) + drow_m);
      const int qa = rowm[tA], qb = rowm[tB];
      const unsigned am = qa < 0 ? TILE_VOID : (unsigned)qa * 8u, bm = qb < 0 ? TILE_VOID : (unsigned)qb * 8u;
      if (tz & 1) { mA1 = am; mB1 = bm; } else { mA0 = am; mB0 = bm; }
    }
  };
  auto zpart = [&](int p) -> unsigned {          // cells
    const int pz = wrap_z(p);
    return (unsigned)((long)(pz & 1) * 4 * A.ngd) + (unsigned)(TILE_OX * TILE_OY * ((pz >> 1) & (TILE_OZ - 1)));
  };
  auto tbp = [&](int p) -> unsigned {
    const int par = tile_of_plane(p) & 1;
    const unsigned a = par ? sA1 : sA0, b = par ? sB1 : sB0;
    return (inB ? b : a) + sloc[ty * BX + tx];
  };
  // (MASK: plane p through the tiles; else plane offset + column)
  // (MASK: two variables share a buffer descriptor -- the odd one rides in the scalar offset: 16 scalar registers the
  //  masked instantiation does not have; pitch_var * 8 + the plane part < 2^32, checked by the launcher)
  const unsigned odd_var = (unsigned)(A.pitch_var * 8);
  auto load_u = [&](int p, double (&u)[NV]) {
    const unsigned pb = MASK ? zpart(p) * 8u : plane_off(p), off = MASK ? tbp(p) : colb;
#pragma unroll
    for (int n = 0; n < NV; n++)
      u[n] = MASK ? plane_load(uold + (long)(n & ~1) * A.pitch_var, pb + (n & 1) * odd_var, off) : plane_load(uold + (long)n * A.pitch_var, pb, off);
  };
  // MASK: the state the update starts from: unew, in place -- it holds what the finer level owes to this one (:752-790) -- or, on a
  // level without finer octs (set_unew has just made unew = uold there), uold again: the planes this workgroup read two iterations
  // ago, from L2 instead of a second stream from HBM
  const double *__restrict__ bsrc = A.base_uold ? uold : unew;
  auto load_base = [&](int p, double (&u)[NF]) {
    const unsigned pb = zpart(p) * 8u, off = tbp(p);
#pragma unroll
    for (int n = 0; n < NV; n++) u[n] = plane_load(bsrc + (long)(n & ~1) * A.pitch_var, pb + (n & 1) * odd_var, off);
    // (divu / enew are read whatever base_uold says: they hold what set_unew and the finer level left there)
    if constexpr (PFIX) { u[NV] = plane_load(X.divu, pb, off); u[NV + 1] = plane_load(X.enew, pb, off); }
  };
  double dif_cy = 0.0;                 // DIFMAG: difmag * min(0, div1) of this row's -y face of plane c (set and used in phase B)
  double dif_c0 = 0.0, dif_c1 = 0.0;   // DIFMAG: the corner divergences of plane c at (tx, ty) and (tx, ty+1)
  int ok_zlo = 0;   // MASK: plane c-1's status byte of this column
  int spre = 0;     // MASK: plane c+1's status byte, on its way
  unsigned char *smask = smem_raw + L::mask_off;   // MASK: [3][BY][BX] status bytes of planes c-1, c, c+1, by plane mod 3
  auto load_g = [&](int p, double (&g)[3]) {
    if (GRAV) {
      const unsigned pb = MASK ? zpart(p) * 8u : plane_off(p), off = MASK ? tbp(p) : colb;
#pragma unroll
      for (int d = 0; d < 3; d++) g[d] = plane_load(grav + (long)d * A.pitch_var, pb, off);
    } else {
      g[0] = g[1] = g[2] = 0.0;
    }
  };

  // ---- register state carried along z --------------------------------------
  double qmz[NV];                 // qm along z of plane c-1 (state on its +z face)
  double fzlo[NF];                // z flux through the -z face of plane c-1
  double upre[NV], gpre[3];       // prefetch: plane c+1 on entry of iteration c
  double rold = 0.0, sold[NV > 5 ? NV - 5 : 1];   // uold density / scalars of plane c-1 (NV>5 only)
  double ukeep[NV];               // KEEP: the conservative state of plane c
#pragma unroll
  for (int n = 0; n < NV; n++) ukeep[n] = 0.0;

  double rinv_c = 0.0;            // TRIM: 1 / rho of this column's cell of plane c (ctoprim_cell's)
#if SWEEP_CYCLE_PROBE
  unsigned long long pr_a = 0, pr_w = 0, pr_b = 0, pr_n = 0;
#endif

  // ring slots of planes c-1, c, c+1
  int sa = 0, sb = 1, sc = 2;

  // prologue: primitives of planes z0-2 -> slot sa, z0-1 -> slot sb; c starts at z0-1
  // MASK: the z-tile of plane z0-2 and the next one (the planes in flight -- c-1 .. c+2 -- never span more than two)
  if (MASK) {
    const int t0 = tile_of_plane(z0 - 2), t1 = t0 + 1 < A.ntz ? t0 + 1 : 0;
    tile_set(t0);
    tile_set(t1);
    __syncthreads();      // (sloc is read by its own thread only; the barrier orders the LDS write for the compiler's sake)
    if (r_trace) spre = stat_load(A.stat, (unsigned)A.pitch_var, tbp(z0 - 1) >> 3, zpart(z0 - 1));
  }
  {
    double u[NV], g[3], q[NV];
    load_u(z0 - 2, u); load_g(z0 - 2, g);
    ctoprim_cell<NV, GRAV, NE>(u, g, dtxhalf, P, q);
#pragma unroll
    for (int n = 0; n < NV; n++) qring[sa].v[n][ty][tx] = q[n];
    load_u(z0 - 1, u); load_g(z0 - 1, g);
    if (KEEP) {
#pragma unroll
      for (int n = 0; n < NV; n++) ukeep[n] = u[n];
    }
    if constexpr (TRIM && r_trace) ctoprim_cell<NV, GRAV, NE>(u, g, dtxhalf, P, q, &rinv_c);
    else ctoprim_cell<NV, GRAV, NE>(u, g, dtxhalf, P, q);
#pragma unroll
    for (int n = 0; n < NV; n++) qring[sb].v[n][ty][tx] = q[n];
    load_u(z0, upre); load_g(z0, gpre);
#pragma unroll
    for (int n = 0; n < NV; n++) qmz[n] = 1.0;
#pragma unroll
    for (int n = 0; n < NF; n++) fzlo[n] = 0.0;
  }
  // Enter the loop with no load in flight: otherwise the loop header inherits
  // "prefetch pending" from this path and waits (in issue order) behind the
  // stores of the previous iteration on every trip.
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
  __syncthreads();

  // Neighbour columns by constant offsets from the thread's own LDS address (one address register,
  // immediate offsets).  Lanes 0 and 63 and a tile's first and last row then read a neighbouring row,
  // variable or nothing at all (out-of-range LDS reads return 0): whatever they compute from it stays in
  // the two halo columns / rows, which are never stored (rows 0 and BY-1 take no slopes, lanes 0, 1, 62, 63
  // own no cell, and the x flux an owned cell uses reaches two lanes at most).
  const int txm = tx - 1, txp = tx + 1;
  const int tym = ty - 1, typ = ty + 1;

  // ---- ONE barrier per plane --------------------------------------------------------------
  // The +y traced state and the y flux share ONE LDS slot per row, double-buffered by plane
  // parity: slot M[c&1][ty] is written by row ty with its +y state before the barrier of
  // iteration c, read after it by row ty+1, which then overwrites it with the flux through
  // that face; row ty picks the flux up after the NEXT barrier, when it finishes plane c-1
  // -> c.  Nobody else touches the slot, so the second barrier of the two-barrier loop (and
  // the lock-step of the heavy waves it enforced) is gone.  Same operations in the same
  // order per cell: ((u + (fx- - fx+)) + (fy- - fy+)) + (fz- - fz+).
  double partx[NF];                      // u + x flux difference of plane c-1
  double fyown[NF];                      // y flux through the -y face of plane c-1 (computed by this row; its copy
                                         // in slot ty-1 belongs to row ty-1, which reuses the slot without a barrier)
  double rnew = 0.0, snew[NV > 5 ? NV - 5 : 1];
  double bcar[NV];                       // LATE: the state the update of plane c-1 starts from
#pragma unroll
  for (int n = 0; n < NV; n++) bcar[n] = 0.0;
#pragma unroll
  for (int n = 0; n < NF; n++) { partx[n] = 0.0; fyown[n] = 0.0; }
  if (PARK && r_fxz) {
#pragma unroll
    for (int n = 0; n < 2 * NF; n++) park[n][ty - 2][tx] = 0.0;
  }
  if constexpr (DUTY && ROLE == ROLE_FULL_LO) {
#pragma unroll
    for (int n = 0; n < NF; n++) yduty[0][n][tx] = yduty[1][n][tx] = 0.0;
  }
  if constexpr (DPN > 0 && (ROLE == ROLE_FULL || ROLE == ROLE_FULL_LO)) {
#pragma unroll
    for (int n = 0; n < DPN; n++) dpark[n][ty - 2][tx] = n < NV + 2 ? 0.0 : 1.0;      // (as fzlo, the corners and qmz start)
  }

  // SO1: the store's lane offset is colb_upd from the third trip of a chunk on (c >= z0 + 1) and beyond every range before:
  // an all-ones word (BUF_OOB) that is or-ed on and cleared once, instead of a predicate rebuilt every plane
  constexpr bool SO1 = BOOK;
  unsigned so_oob = BUF_OOB;
  // LB: the ring addresses of a tracing row (two ring planes, the seven-point slopes) -- the thread's column one row up in
  // slot 0, and the byte offsets of the slots of planes c and c-1, which change places every trip (slots 0 and 1: one xor
  // each).  Rows 1 .. BY-2 trace, so row ty-1 exists and no address register is below the ring's first byte; the cells read
  // are the ones read before, those of lanes 0 and 63 (the end of the row above, the start of the row below) and of rows 1
  // and BY-2 (the halo rows' cells) included: what they return stays in columns and rows that are never stored, as before.
  constexpr bool LB = BOOK && r_trace;
  static_assert(!BOOK || RING == 2, "BOOK: two ring planes, the seven-point slopes");
  constexpr unsigned QROW = BX * 8u, QVAR = BY * BX * 8u, QSLOT = (unsigned)sizeof(Plane<BY, NV>);
  const unsigned q_lane = lds_addr(qring) + (unsigned)((ty - 1) * BX + tx) * 8u;
  unsigned q_cur = QSLOT, q_prev = 0u;          // (sb = 1, sa = 0)

  for (int c = z0 - 1; c <= z1; c++) {
    Plane<L::MR, NF> &M = mring[c & 1];
    Plane<L::MR, NF> &Mprev = mring[(c & 1) ^ 1];
#if SWEEP_CYCLE_PROBE
    const unsigned long long pr_t0 = __builtin_readcyclecounter();
#endif
    // ---- phase A: plane c+1 arrives; trace plane c; x and z fluxes ------------------
    double qc[NV];
    double rinv_n = 0.0;
    if constexpr (TRIM && r_trace) ctoprim_cell<NV, GRAV, NE>(upre, gpre, dtxhalf, P, qc, &rinv_n);
    else ctoprim_cell<NV, GRAV, NE>(upre, gpre, dtxhalf, P, qc);
    // plane c+1 goes into the ring: into its own slot (RING 3), or into the slot of plane c-1 as soon as this thread has taken
    // its z slope from it (RING 2; the rows that take no slopes have nothing to wait for)
    if (RING == 3 || !r_trace) {
#pragma unroll
      for (int n = 0; n < NV; n++) qring[RING == 3 ? sc : sa].v[n][ty][tx] = qc[n];
    }
    double ucur[NF];
    if (r_fxz && !LATE && !DIFMAG) {
      if (KEEP && (!MASK || A.base_uold)) {
#pragma unroll
        for (int n = 0; n < NV; n++) ucur[n] = ukeep[n];          // plane c, held since it arrived
      } else if constexpr (MASK) load_base(c, ucur);
      else load_u(c, ucur);
    }
    if (KEEP && r_fxz) {
#pragma unroll
      for (int n = 0; n < NV; n++) ukeep[n] = upre[n];            // plane c+1, for the next iteration
    }
    int okc = 0, ok_ym = 0;
    if (MASK && r_trace) {
      okc = spre;                  // loaded one plane ahead: nothing at the top of an iteration waits for memory
      smask[((c + 3) % 3 * BY + ty) * BX + tx] = (unsigned char)okc;   // row ty+1 reads it after the barrier (its -y neighbour), row ty-1 one plane later
    }

    double qpy[NV], dz[NF], px[NF];
    if (ST == 3) __syncthreads();  // the 27-point slope reads the neighbours' plane c+1 just written
    if constexpr (r_trace) {
      const Plane<BY, NV> &qs = qring[sb];
      const Plane<BY, NV> &qprev = qring[sa];
      double qb[NV], dq[3][NV];
      if (ST == 3) {
        const Plane<BY, NV> &qnext = qring[sc];
        const int xs[3] = {txm, tx, txp}, ys[3] = {tym, ty, typ};
#pragma unroll
        for (int n = 0; n < NV; n++) {
          double nb[27], d3[3];
#pragma unroll
          for (int dj = 0; dj < 3; dj++)
#pragma unroll
            for (int di = 0; di < 3; di++) {
              nb[di + 3 * dj] = qprev.v[n][ys[dj]][xs[di]];
              nb[di + 3 * dj + 9] = qs.v[n][ys[dj]][xs[di]];
              nb[di + 3 * dj + 18] = qnext.v[n][ys[dj]][xs[di]];
            }
          qb[n] = nb[13];
          slope3_var(nb, d3);
          dq[0][n] = d3[0]; dq[1][n] = d3[1]; dq[2][n] = d3[2];
        }
      } else if (ST == 4 || ST == 5 || ST == 6) {
        // the NDIM=1 slope types (embedded 1-D problems: ny = nz = 1, the transverse differences vanish)
#pragma unroll
        for (int n = 0; n < NV; n++) qb[n] = qs.v[n][ty][tx];
        const double dc0 = qb[1] * A.dt / A.dx, dc1 = qb[2] * A.dt / A.dx, dc2 = qb[3] * A.dt / A.dx;
#pragma unroll
        for (int n = 0; n < NV; n++) {
          dq[0][n] = slope1_1d<ST>(qs.v[n][ty][txm], qb[n], qs.v[n][ty][txp], dc0, n);
          dq[1][n] = slope1_1d<ST>(qs.v[n][tym][tx], qb[n], qs.v[n][typ][tx], dc1, n);
          dq[2][n] = slope1_1d<ST>(qprev.v[n][ty][tx], qb[n], qc[n], dc2, n);
        }
      } else if constexpr (LB) {
        // the same 5 NV cells of the ring at the same addresses, through three address registers of plane c -- column tx from
        // row ty-1 on (q_c: rows ty-1, ty, ty+1 at 0, QROW, 2 QROW), columns tx-1 and tx+1 of row ty (q_m, q_p) -- and one of
        // plane c-1's slot (q_s), every variable a multiple of 512 B further on: no address is computed per cell
        const unsigned q_c = lds_reg(q_lane + q_cur), q_s = lds_reg(q_lane + q_prev);
        const unsigned q_m = lds_reg(q_c + (QROW - 8u)), q_p = lds_reg(q_c + (QROW + 8u));
#pragma unroll
        for (int n = 0; n < NV; n++) {
          qb[n] = lds_ld(q_c, QROW + n * QVAR);
          dq[0][n] = slope1<ST>(lds_ld(q_m, n * QVAR), qb[n], lds_ld(q_p, n * QVAR), P);
          dq[1][n] = slope1<ST>(lds_ld(q_c, n * QVAR), qb[n], lds_ld(q_c, 2 * QROW + n * QVAR), P);
          dq[2][n] = slope1<ST>(lds_ld(q_s, QROW + n * QVAR), qb[n], qc[n], P);
        }
#pragma unroll
        for (int n = 0; n < NV; n++) lds_st(q_s, QROW + n * QVAR, qc[n]);
      } else {
#pragma unroll
        for (int n = 0; n < NV; n++) {
          qb[n] = qs.v[n][ty][tx];
          dq[0][n] = slope1<ST>(qs.v[n][ty][txm], qb[n], qs.v[n][ty][txp], P);
          dq[1][n] = slope1<ST>(qs.v[n][tym][tx], qb[n], qs.v[n][typ][tx], P);
          dq[2][n] = slope1<ST>(qprev.v[n][ty][tx], qb[n], qc[n], P);
        }
      }
      if (RING == 2 && !LB) {
#pragma unroll
        for (int n = 0; n < NV; n++) qring[sa].v[n][ty][tx] = qc[n];
      }
      double qm[3][NV], qp[3][NV];
      if (SCHEME == 0) {
        // (a full row consumes all six traced densities: their floor behind one wave-uniform test, trace3d_cell RHO6)
        if constexpr (TRIM) trace3d_cell<NV, NE, r_fxz>(qb, dq, dtdx, dtdx, dtdx, P, qm, qp, &rinv_c);
        else trace3d_cell<NV, NE, r_fxz>(qb, dq, dtdx, dtdx, dtdx, P, qm, qp);
      } else {
        const double cc = ctoprim_sound(qb[0], qb[4], P);
        tracexyz_cell<NV>(qb, dq, cc, dtdx, dtdx, dtdx, P, qm, qp);
      }
      // (DUTY: nobody reads row BY-2's +y state -- its slot takes the -y state, for the wave of row BY-1)
#pragma unroll
      for (int n = 0; n < NV; n++) M.v[n][ty - M0][tx] = (DUTY && ROLE == ROLE_HIGH) ? qp[1][n] : qm[1][n];
#pragma unroll
      for (int n = 0; n < NV; n++) qpy[n] = qp[1][n];
      if constexpr (DUTY && ROLE == ROLE_FULL_LO) {
#pragma unroll
        for (int n = 0; n < NV; n++) yduty[c & 1][n][tx] = qp[1][n];      // for the wave of row 0
      }
      if constexpr (r_fxz) {
        double qL[NV], fx[NF], fz[NF];
#pragma unroll
        for (int n = 0; n < NV; n++) qL[n] = wave_shr1(qm[0][n]);  // +x state of column tx-1
        if constexpr (PFIX) {
          double f[NV], t[2];
          scaled_interface_flux_tmp<RS, NV, 0>(qL, qp[0], P, A.dt, A.dx, A.rdx, DXPOW2, f, t);
#pragma unroll
          for (int n = 0; n < NV; n++) fx[n] = f[n];
          fx[NV] = t[0]; fx[NV + 1] = t[1];
          scaled_interface_flux_tmp<RS, NV, 2>(qmz, qp[2], P, A.dt, A.dx, A.rdx, DXPOW2, f, t);
#pragma unroll
          for (int n = 0; n < NV; n++) fz[n] = f[n];
          fz[NV] = t[0]; fz[NV + 1] = t[1];
        } else {
        scaled_interface_flux<RS, NV, 0, !MASK, NE, TRIM>(qL, qp[0], P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, fx);
        // z flux through the face between planes c-1 and c
        if constexpr (DPN > NV + 2) {
#pragma unroll
          for (int n = 0; n < NV; n++) qmz[n] = dpark[NV + 2 + n][ty - 2][tx];
        }
        scaled_interface_flux<RS, NV, 2, !MASK, NE, TRIM>(qmz, qp[2], P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, fz);
        }
        if (MASK && !DIFMAG) {
          // hydro/godunov_fine.f90:720-747: the flux through a face is reset when the cell on either side is refined
          const int s_xm = wave_shr1_i(okc);
          const bool zx = ((okc | s_xm) & CELL_REFINED) != 0, zz = ((okc | ok_zlo) & CELL_REFINED) != 0;
#pragma unroll
          for (int n = 0; n < NF; n++) { fx[n] = zx ? 0.0 : fx[n]; fz[n] = zz ? 0.0 : fz[n]; }
        }
        double fxh[NF];
#pragma unroll
        for (int n = 0; n < NV; n++) qmz[n] = qm[2][n];
        if constexpr (DPN > NV + 2) {
#pragma unroll
          for (int n = 0; n < NV; n++) dpark[NV + 2 + n][ty - 2][tx] = qm[2][n];
        }
        if constexpr (DIFMAG) {
          // the x and z fluxes cross the barrier as they are: their diffusive term, the resets and the differencing in phase B
#pragma unroll
          for (int n = 0; n < NF; n++) { px[n] = fx[n]; dz[n] = fz[n]; }
        } else {
#pragma unroll
        for (int n = 0; n < NF; n++) {
          dz[n] = fzlo[n] - fz[n];          // z flux difference of plane c-1
          fzlo[n] = fz[n];
          fxh[n] = wave_shl1(fx[n]);        // -x face flux of column tx+1
          // (LATE: the state the update starts from joins in phase B of the next iteration -- a whole trace after its load)
          px[n] = LATE ? (fx[n] - fxh[n]) : ucur[n] + (fx[n] - fxh[n]);
        }
        }
        if (NV > 5 + NE && !MASK) {
          rnew = ucur[0];
#pragma unroll
          for (int n = 5 + NE; n < NV; n++) snew[n - 5] = ucur[n];
        }
      }
    }
    // prefetch plane c+2 after the register peak of the trace and flux phase (still ~1 us ahead of its use)
    __builtin_amdgcn_sched_barrier(0);
    // DIFMAG: uold of plane c -- this cell's and row ty-1's -- and of plane c-1, for the conserved differences of phase B; requested
    // before the prefetch, so that waiting for them does not wait for plane c+2.  They wait in three arrays that a difmag kernel
    // leaves idle (ukeep: KEEP, bcar: LATE, partx: without PARK), under other names: a local declared in this loop's body, used
    // or not, leaves its lifetime markers in EVERY instantiation and moved scalar code of the exact-solver tile kernels
    // (profiles/difmag_asm_diff.txt) -- what difmag adds to the loop's scope lives inside if constexpr (DIFMAG) or before the loop.
    if constexpr (DIFMAG && (r_fxz || ROLE == ROLE_HIGH)) {
      static_assert(!KEEP && !LATE && PARK, "difmag borrows ukeep, bcar and partx");
      double (&dif_u)[NV] = ukeep, (&dif_uym)[NV] = bcar, (&dif_uzm)[NV] = partx;
      // (row ty-1 parked its lane part of the cell index in sloc before the first barrier)
      load_uold_cell<NV>(uold, A.pitch_var, odd_var, zpart(c) * 8u, tbp(c), dif_u);
      if constexpr (!r_fxz)
        load_uold_cell<NV>(uold, A.pitch_var, odd_var, zpart(c) * 8u,
                           tile_base_ym(tile_of_plane(c) & 1, inB, mA0, mA1, mB0, mB1) + sloc[(ty - 1) * BX + tx], dif_uym);
      if constexpr (r_fxz) {
        load_uold_cell<NV>(uold, A.pitch_var, odd_var, zpart(c - 1) * 8u, tbp(c - 1), dif_uzm);
        load_base(c, ucur);      // (the state the update starts from: not needed before phase B either)
      }
    }
    {
      const int pn = min(c + 2, z1 + 1);
      if (MASK) {
        // the directory entries of the NEXT z-tile: loaded (scalar) when the prefetch is half way through this one, into the
        // registers of the tile before it, which no plane in flight uses any more
        const int lp = wrap_z(pn) & 7;
        const int tn = tile_of_plane(pn) + 1 < A.ntz ? tile_of_plane(pn) + 1 : 0;
        if (lp == 4) tile_set(tn);
      }
      load_u(pn, upre); load_g(pn, gpre);
      if (MASK && r_trace) { const int ps = min(c + 1, z1 + 1); spre = stat_load(A.stat, (unsigned)A.pitch_var, tbp(ps) >> 3, zpart(ps)); }
    }
    __builtin_amdgcn_sched_barrier(0);
#if SWEEP_CYCLE_PROBE
    const unsigned long long pr_t1 = __builtin_readcyclecounter();
#endif
    __syncthreads();  // the one barrier: +y states of plane c and y fluxes of plane c-1 visible
#if SWEEP_CYCLE_PROBE
    const unsigned long long pr_t2 = __builtin_readcyclecounter();
#endif

    // ---- phase B: y flux of plane c; finish plane c-1 --------------------------------
    if constexpr (DIFMAG && (r_fxz || ROLE == ROLE_HIGH)) {
      double (&dif_u)[NV] = ukeep, (&dif_uym)[NV] = bcar, (&dif_uzm)[NV] = partx;
      const Plane<BY, NV> &q0 = qring[sb], &q1 = qring[sc];     // planes c and c+1, every row's and lane's
      constexpr int NR = r_fxz ? 3 : 2;                         // rows ty-1, ty (, ty+1)
      const double fdiv = 0.25 / A.dx;
      double dsum[3][2];                                        // the three sums of cmpdivu at the corners (tx, ty) and (tx, ty+1) of plane c+1
#pragma unroll
      for (int d = 0; d < 3; d++) {
        // one component at a time (the registers of 12 velocities, not of 36): column tx from LDS, column tx-1 by DPP
        double vo[2][NR], vl[2][NR];                            // [plane][row]
#pragma unroll
        for (int r = 0; r < NR; r++) {
          vo[0][r] = q0.v[1 + d][tym + r][tx];
          vo[1][r] = q1.v[1 + d][tym + r][tx];
          vl[0][r] = wave_shr1(vo[0][r]);
          vl[1][r] = wave_shr1(vo[1][r]);
        }
#pragma unroll
        for (int r0 = 0; r0 < NR - 1; r0++) {
          double v[2][2][2];
#pragma unroll
          for (int dk = 0; dk < 2; dk++)
#pragma unroll
            for (int dj = 0; dj < 2; dj++) { v[dk][dj][0] = vl[dk][r0 + dj]; v[dk][dj][1] = vo[dk][r0 + dj]; }
          dsum[d][r0] = d == 0 ? difmag::cmpdivu_ux(v, fdiv) : (d == 1 ? difmag::cmpdivu_vy(v, fdiv) : difmag::cmpdivu_wz(v, fdiv));
        }
        if (NR == 2) dsum[d][1] = 0.0;
      }
      const double dn[2] = {dsum[0][0] + dsum[1][0] + dsum[2][0], dsum[0][1] + dsum[1][1] + dsum[2][1]};
      if constexpr (DPN > 0 && r_fxz) {
        dif_c0 = dpark[NV][ty - 2][tx]; dif_c1 = dpark[NV + 1][ty - 2][tx];
#pragma unroll
        for (int n = 0; n < NV; n++) fzlo[n] = dpark[n][ty - 2][tx];
      }
      const double c0x = wave_shl1<true>(dif_c0), n0x = wave_shl1<true>(dn[0]);     // the corners at tx+1
      dif_cy = difmag::consup_coef(D.difmag, difmag::consup_div1_y(dif_c0, c0x, dn[0], n0x));
      if constexpr (r_fxz) {
        const double c1x = wave_shl1<true>(dif_c1);
        const double cx = difmag::consup_coef(D.difmag, difmag::consup_div1_x(dif_c0, dif_c1, dn[0], dn[1]));
        const double cz = difmag::consup_coef(D.difmag, difmag::consup_div1_z(dif_c0, c0x, dif_c1, c1x));
        // hydro/godunov_fine.f90:720-747 after consup: the flux through a face is reset when the cell on either side is refined
        const int s_xm = wave_shr1_i(okc);
        const bool zx = ((okc | s_xm) & CELL_REFINED) != 0, zz = ((okc | ok_zlo) & CELL_REFINED) != 0;
#pragma unroll
        for (int n = 0; n < NV; n++) {
          const double fxd = difmag::consup_term(px[n], A.dt, cx, dif_u[n], wave_shr1(dif_u[n]));
          const double fzd = difmag::consup_term(dz[n], A.dt, cz, dif_u[n], dif_uzm[n]);
          const double fxn = zx ? 0.0 : fxd, fzn = zz ? 0.0 : fzd;
          dz[n] = fzlo[n] - fzn;              // z flux difference of plane c-1
          fzlo[n] = fzn;
          px[n] = ucur[n] + (fxn - wave_shl1<true>(fxn));
        }
      }
      dif_c0 = dn[0]; dif_c1 = dn[1];
      if constexpr (DPN > 0 && r_fxz) {
        dpark[NV][ty - 2][tx] = dn[0]; dpark[NV + 1][ty - 2][tx] = dn[1];
#pragma unroll
        for (int n = 0; n < NV; n++) dpark[n][ty - 2][tx] = fzlo[n];
      }
      // (a full row asks for row ty-1's conserved variables only now: they arrive while the Riemann solver of the y face runs)
      if constexpr (r_fxz)
        load_uold_cell<NV>(uold, A.pitch_var, odd_var, zpart(c) * 8u,
                           tile_base_ym(tile_of_plane(c) & 1, inB, mA0, mA1, mB0, mB1) + sloc[(ty - 1) * BX + tx], dif_uym);
    }
    double fy[NF];
    if constexpr (y_take) {
      // the flux through face DUTY_F, between rows DUTY_F-1 and DUTY_F, for the rows beside it
      double qL[NV], qR[NV];
#pragma unroll
      for (int n = 0; n < NV; n++) {
        qL[n] = M.v[n][DUTY_F - 1 - M0][tx];
        qR[n] = ROLE == ROLE_HALO ? yduty[c & 1][n][tx] : M.v[n][DUTY_F - M0][tx];
      }
      scaled_interface_flux<RS, NV, 1, !MASK, NE, TRIM>(qL, qR, P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, fy);
#pragma unroll
      for (int n = 0; n < NF; n++) {
        if (ROLE == ROLE_HALO) yduty[c & 1][n][tx] = fy[n];       // row 2 picks it up after the next barrier
        else M.v[n][DUTY_F - 1 - M0][tx] = fy[n];                 // row BY-3's slot, where row BY-2 used to leave it
      }
    }
    if constexpr ((r_fxz || ROLE == ROLE_HIGH) && !y_give) {
      double qL[NV];
#pragma unroll
      for (int n = 0; n < NV; n++) qL[n] = M.v[n][tym - M0][tx];
      if constexpr (PFIX) {
        double f[NV], t[2];
        scaled_interface_flux_tmp<RS, NV, 1>(qL, qpy, P, A.dt, A.dx, A.rdx, DXPOW2, f, t);
#pragma unroll
        for (int n = 0; n < NV; n++) fy[n] = f[n];
        fy[NV] = t[0]; fy[NV + 1] = t[1];
      } else {
      scaled_interface_flux<RS, NV, 1, !MASK, NE, TRIM>(qL, qpy, P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, fy);
      }
      if constexpr (DIFMAG) {
        double (&dif_u)[NV] = ukeep, (&dif_uym)[NV] = bcar;
#pragma unroll
        for (int n = 0; n < NV; n++) fy[n] = difmag::consup_term(fy[n], A.dt, dif_cy, dif_u[n], dif_uym[n]);
      }
      if (MASK) {
        ok_ym = smask[((c + 3) % 3 * BY + tym) * BX + tx];
        const bool zy = ((okc | ok_ym) & CELL_REFINED) != 0;
#pragma unroll
        for (int n = 0; n < NF; n++) fy[n] = zy ? 0.0 : fy[n];
      }
      // the flux through this row's -y face is the +y face flux of row ty-1: into ITS slot
#pragma unroll
      for (int n = 0; n < NF; n++) M.v[n][tym - M0][tx] = fy[n];
    }
    if constexpr (r_fxz) {
      // plane c-1: its x part and own -y flux were kept in registers, the +y face flux was left
      // in this row's slot of the other buffer by row ty+1 before this iteration's barrier.
      // (The first two iterations of a chunk produce values from the not yet primed pipeline;
      // they are computed and dropped by the store's range check.)
      double un[NF], fyh[NF];
#pragma unroll
      for (int n = 0; n < NF; n++) {
        fyh[n] = Mprev.v[n][ty - M0][tx];
        const double pxn = PARK ? park[n][ty - 2][tx] : partx[n];
        const double fyn = y_give ? yduty[(c & 1) ^ 1][n][tx] : (PARK ? park[NF + n][ty - 2][tx] : fyown[n]);
        const double part = (LATE ? bcar[n < NV ? n : 0] + pxn : pxn) + (fyn - fyh[n]);
        un[n] = part + dz[n];
      }
      if (NV > 5 + NE && !MASK) {
        // set_uold's passive-scalar fix near the density floor
        // (hydro/godunov_fine.f90:176-190), fused: the kernel's output is the new uold
        // (MASK: the kernel's output is unew; set_uold of the resident level applies the fix, csrc/capi_amr.hip lvl_set_uold)
        if (rold < P.smallr && un[0] > rold) {
#pragma unroll
          for (int n = 5 + NE; n < NV; n++) un[n] = sold[n - 5] * dmaxd(un[0], P.smallr) / P.smallr;
        } else if (un[0] < P.smallr && rold > un[0]) {
#pragma unroll
          for (int n = 5 + NE; n < NV; n++) un[n] = sold[n - 5] * P.smallr / dmaxd(rold, P.smallr);
        }
        rold = rnew;
#pragma unroll
        for (int n = 5 + NE; n < NV; n++) sold[n - 5] = snew[n - 5];
      }
#pragma unroll
      for (int n = 0; n < NF; n++) {
        if (PARK) { park[n][ty - 2][tx] = px[n]; if (!y_give) park[NF + n][ty - 2][tx] = fy[n]; }
        else { partx[n] = px[n]; fyown[n] = fy[n]; }
      }
      {
        const unsigned pb = MASK ? zpart(c - 1) * 8u : plane_off(c - 1);
        const unsigned so = SO1 ? (colb_upd | so_oob)
                                : ((c >= z0 + 1) ? (MASK ? ((r_upd && (ok_zlo & CELL_OWNED)) ? tbp(c - 1) : BUF_OOB) : colb_upd) : BUF_OOB);
#pragma unroll
        for (int n = 0; n < NV; n++) {
          if (MASK) plane_store(unew + (long)(n & ~1) * A.pitch_var, pb + (n & 1) * odd_var, so, un[n]);
          else plane_store(unew + (long)n * A.pitch_var, pb, so, un[n]);
        }
        if constexpr (PFIX) { plane_store(X.divu, pb, so, un[NV]); plane_store(X.enew, pb, so, un[NV + 1]); }
      }
      // LATE: the state the update of plane c starts from (MASK: unew, in place -- another array, an HBM miss; else the plane of
      // uold this workgroup read two iterations ago), requested now and used in phase B of the next iteration: at the top of
      // phase A it was due at the x flux, and every wave of the workgroup sat at that wait together
      if constexpr (LATE) { if (MASK) load_base(c, bcar); else load_u(c, bcar); }
    }
    // rotate the ring
    if (RING == 3) { const int t = sa; sa = sb; sb = sc; sc = t; }
    else { const int t = sa; sa = sb; sb = t; }
    if (MASK) ok_zlo = okc;
    if (TRIM) rinv_c = rinv_n;
    if (SO1) so_oob = c >= z0 ? 0u : so_oob;
    if (LB) { q_cur ^= QSLOT; q_prev ^= QSLOT; }
#if SWEEP_CYCLE_PROBE
    pr_a += pr_t1 - pr_t0; pr_w += pr_t2 - pr_t1; pr_b += __builtin_readcyclecounter() - pr_t2; pr_n += 1;
#endif
  }
#if SWEEP_CYCLE_PROBE
  if (tx == 0 && blockIdx.x < PROBE_BLOCKS && ty < PROBE_ROWS) {
    unsigned long long *o = sweep_cycle_probe[blockIdx.x][ty];
    o[0] = pr_a; o[1] = pr_w; o[2] = pr_b; o[3] = pr_n; o[4] = (unsigned long long)ty;
    o[5] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);     // HW_ID
  }
#endif
}

template <int ST, int RS, int BY, bool GRAV, int SCHEME, int NV, bool MASK = false>
__global__ __launch_bounds__(BX *BY) void godunov_sweep_kernel(SweepArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int ty = threadIdx.y;   // wave-uniform
  // the full rows are the critical path between two barriers: let them win the issue
  // arbitration over the light rows (measured: -1.1 % at 512^3)
  if (ty >= 2 && ty <= BY - 3) __builtin_amdgcn_s_setprio(3);
  if (ty == 0) sweep_march<ST, RS, BY, GRAV, SCHEME, NV, ROLE_HALO, MASK>(A, smem_raw);
  else if (ty == BY - 1) sweep_march<ST, RS, BY, GRAV, SCHEME, NV, ROLE_HALO_HI, MASK>(A, smem_raw);
  else if (ty == 1) sweep_march<ST, RS, BY, GRAV, SCHEME, NV, ROLE_LOW, MASK>(A, smem_raw);
  else if (ty == BY - 2) sweep_march<ST, RS, BY, GRAV, SCHEME, NV, ROLE_HIGH, MASK>(A, smem_raw);
  else {
    if constexpr (y_duty<ST, RS, BY, GRAV, SCHEME, NV, MASK>()) {
      if (ty == 2) { sweep_march<ST, RS, BY, GRAV, SCHEME, NV, ROLE_FULL_LO, MASK>(A, smem_raw); return; }
    }
    sweep_march<ST, RS, BY, GRAV, SCHEME, NV, ROLE_FULL, MASK>(A, smem_raw);
  }
}

#ifndef RAMSES_AMD_FAST
// pressure_fix on a level in tiles (strict arithmetic only: scaled_interface_flux_tmp): muscl, the 8-row layout of the
// NV = 6, 7 kernels -- the two face quantities cost what two passive scalars cost -- or 6 rows where the LDS of 8 does not
// hold them (NV = 7 with the 27-point slope's third ring plane).  A kernel of its own so that the symbols and the code of the
// kernels without pressure_fix stay what they were.
template <int ST, int NV>
struct PfixRows {
  static constexpr int BY = (ST == 3 && NV == 7) ? 6 : 8;
};
template <int ST, int RS, int BY, bool GRAV, int NV>
__global__ __launch_bounds__(BX *BY) void godunov_sweep_pfix_kernel(SweepArgs A, SweepPfix X) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  static_assert(Lds<ST, BY, NV, true, GRAV, 2>::bytes <= 160 * 1024, "the pressure_fix sweep fits one workgroup's LDS");
  const int ty = threadIdx.y;   // wave-uniform
  if (ty >= 2 && ty <= BY - 3) __builtin_amdgcn_s_setprio(3);
  if (ty == 0) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_HALO, true, 0, true>(A, smem_raw, X);
  else if (ty == BY - 1) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_HALO_HI, true, 0, true>(A, smem_raw, X);
  else if (ty == 1) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_LOW, true, 0, true>(A, smem_raw, X);
  else if (ty == BY - 2) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_HIGH, true, 0, true>(A, smem_raw, X);
  else sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_FULL, true, 0, true>(A, smem_raw, X);
}
#endif

#ifndef RAMSES_AMD_FAST
// difmag > 0 on a level in tiles (strict arithmetic only: the term exists in the reference's operation order only): muscl, no
// pressure_fix, the 8-row layout with three ring planes for every slope type (sweep_march DIFMAG).  A kernel of its own so that
// the symbols and the code of the kernels without difmag stay what they were.
template <int ST, int RS, int BY, bool GRAV, int NV>
__global__ __launch_bounds__(BX *BY) void godunov_sweep_difmag_kernel(SweepArgs A, SweepDifmag D) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  static_assert(Lds<ST, BY, NV, true, GRAV, 0, false, true, dif_parked<RS, NV>()>::bytes <= 160 * 1024, "the difmag sweep fits one workgroup's LDS");
  const int ty = threadIdx.y;   // wave-uniform
  if (ty >= 2 && ty <= BY - 3) __builtin_amdgcn_s_setprio(3);
  if (ty == 0) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_HALO, true, 0, false, true>(A, smem_raw, SweepPfix(), D);
  else if (ty == BY - 1) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_HALO_HI, true, 0, false, true>(A, smem_raw, SweepPfix(), D);
  else if (ty == 1) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_LOW, true, 0, false, true>(A, smem_raw, SweepPfix(), D);
  else if (ty == BY - 2) sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_HIGH, true, 0, false, true>(A, smem_raw, SweepPfix(), D);
  else sweep_march<ST, RS, BY, GRAV, 0, NV, ROLE_FULL, true, 0, false, true>(A, smem_raw, SweepPfix(), D);
}
#endif

// NENER > 0 (the non-thermal energies in variables 5 .. 5+NE-1, passive scalars after them): the 8-row layout of the
// passive-scalar kernels of the same NV, muscl, no gravity, the plain brick (no tiles).  A kernel of its own so that the
// symbols and the code of the NE = 0 kernels stay what they were.
template <int ST, int RS, int NV, int NE>
__global__ __launch_bounds__(BX * 8) void godunov_sweep_nener_kernel(SweepArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int BY = 8;
  const int ty = threadIdx.y;
  if (ty >= 2 && ty <= BY - 3) __builtin_amdgcn_s_setprio(3);
  if (ty == 0) sweep_march<ST, RS, BY, false, 0, NV, ROLE_HALO, false, NE>(A, smem_raw);
  else if (ty == BY - 1) sweep_march<ST, RS, BY, false, 0, NV, ROLE_HALO_HI, false, NE>(A, smem_raw);
  else if (ty == 1) sweep_march<ST, RS, BY, false, 0, NV, ROLE_LOW, false, NE>(A, smem_raw);
  else if (ty == BY - 2) sweep_march<ST, RS, BY, false, 0, NV, ROLE_HIGH, false, NE>(A, smem_raw);
  else sweep_march<ST, RS, BY, false, 0, NV, ROLE_FULL, false, NE>(A, smem_raw);
}

// ---------------------------------------------------------------------------
// scalar pass: passive scalars beyond NVAR=7
// ---------------------------------------------------------------------------
// A passive scalar never feeds back into the hydro (hydro/umuscl.f90:680-700, the "passive scalars" blocks of
// hydro/godunov_utils.f90), so with NVAR > 7 the brick is swept in passes: the kernels above at NV = 5+NE sweep the hydro
// variables, then this kernel sweeps the scalars in groups of G.  It re-derives from uold what a scalar's flux needs -- the
// primitives, slopes and traced states of the 5+NE hydro variables, and the solver's face quantities (LLF: rho, u_n and
// cmax; HLL: SL, SR; HLLC, acoustic, exact: the mass flux and its upwind side) -- with the same functions on the same values
// as the hydro pass, hence the same bits, and updates its group's rows of unew only.  The Riemann routines are called
// whole: the hydro components of their flux are dead code the compiler removes.  set_uold's near-floor fix of the scalars
// (hydro/godunov_fine.f90:176-190) is fused as in the kernels above, with the new density read back from unew, which the
// hydro pass has just written on the same stream.
// Group g covers the variables s0 .. s0+nlive-1 in slots 5+NE .. 5+NE+nlive-1; the slots past nlive (a group of fewer than
// G scalars) load the group's last scalar and store nothing.
// LDS: RING + 2 planes of NV = 5+NE+G doubles per column of a 64 x 8 tile, 16 KB x NV (RING 2) or 20 KB x NV (slope type 3,
// RING 3), within 160 KB: NV = 10 or 8, the largest group that fits.  One 8-wave workgroup per CU, as the NV = 6, 7 kernels.
// The exact solver's Newton loop needs ~40 registers more: with it a group is two slots smaller (at NV = 10 / 8 it spills).
template <int ST, int RS, int NE>
struct ScalarGroup {
  static constexpr int RING = (ST == 3) ? 3 : 2;
  static constexpr int NH = 5 + NE;
  static constexpr int G = (ST == 3 ? 8 : 10) - (RS == RIEMANN_EXACT ? 2 : 0) - NH;
  static constexpr int NV = NH + G;
  static constexpr size_t m_off = RING * sizeof(Plane<8, NV>);
  static constexpr size_t bytes = m_off + 2 * sizeof(Plane<8, NV>);
  static_assert(G >= 1 && bytes <= 160 * 1024, "the scalar pass fits one workgroup's LDS");
};

template <int ST, int RS, bool GRAV, int NE, int ROLE>
__device__ __forceinline__ void scalar_march(const SweepArgs &A, int s0, int nlive, unsigned char *smem_raw) {
  typedef ScalarGroup<ST, RS, NE> SG;
  constexpr int BY = 8, RING = SG::RING, NH = SG::NH, G = SG::G, NV = SG::NV;
  const bool DXPOW2 = A.pow2 != 0;
  Plane<BY, NV> *qring = reinterpret_cast<Plane<BY, NV> *>(smem_raw);
  Plane<BY, NV> *mring = reinterpret_cast<Plane<BY, NV> *>(smem_raw + SG::m_off);
  const int tx = threadIdx.x, ty = threadIdx.y;
  const HydroConst &P = A.P;

  // tile decode: the plain brick's of sweep_march
  const int hb = blockIdx.x;
  int bi = 0;
#pragma unroll
  for (int i = 1; i < 6; i++)
    if (i < A.nbox && hb >= A.box[i].first) bi = i;
  const SweepBox &B = A.box[bi];
  int lb = hb - B.first;
  {
    const int nxcd = 8;
    const int cnt = (bi + 1 < A.nbox ? A.box[bi + 1].first : (int)gridDim.x) - B.first;
    if (cnt % nxcd == 0) {
      const int per = cnt / nxcd;
      lb = (lb % nxcd) * per + lb / nxcd;
    }
  }
  const int tix = B.tx0 + lb % B.ntx;
  const int tiy = B.ty0 + (lb / B.ntx) % B.nty;
  const int tiz = lb / (B.ntx * B.nty);
  const int x0 = tix * (BX - 4), y0 = tiy * (BY - 4);
  const int z0 = B.zlo + tiz * B.zchunk;
  const int z1 = min(z0 + B.zchunk, B.zhi);
  const int xu = x0 - 2 + tx, yu = y0 - 2 + ty;
  int xi, yi;
  if (A.ng == 0) {
    xi = xu < 0 ? xu + A.nx : (xu >= A.nx ? xu - A.nx : xu);
    xi = xi >= A.nx ? xi % A.nx : xi;
    yi = yu < 0 ? yu + A.ny : (yu >= A.ny ? yu - A.ny : yu);
    yi = yi >= A.ny ? yi % A.ny : yi;
  } else {
    xi = min(max(xu, -A.ng), A.nx + A.ng - 1) + A.ng;
    yi = min(max(yu, -A.ng), A.ny + A.ng - 1) + A.ng;
  }
  const unsigned colb = (unsigned)(xi + yi * (int)A.pitch_y) * 8u;
  const double *__restrict__ uold = A.uold;
  double *__restrict__ unew = A.unew;
  const double *__restrict__ grav = A.grav;

  constexpr bool r_trace = ROLE == ROLE_LOW || ROLE == ROLE_HIGH || ROLE == ROLE_FULL;
  constexpr bool r_fxz = ROLE == ROLE_FULL;
  const bool r_upd = r_fxz && (tx >= 2) && (tx <= BX - 3) && (xu < A.nx) && (yu < A.ny);
  const unsigned colb_upd = r_upd ? colb : BUF_OOB;
  const double dtdx = A.dt / A.dx;
  const double dtxhalf = A.dt * 0.5;

  auto plane_off = [&](int p) -> unsigned {
    int pz;
    if (A.ng == 0) { pz = p < 0 ? p + A.nz : (p >= A.nz ? p - A.nz : p); }
    else { pz = p + A.ng; }
    return (unsigned)pz * (unsigned)(A.pitch_z * 8);
  };
  // slot n of the group -> variable of the brick (wave-uniform)
  auto var_of = [&](int n) -> long { return n < NH ? n : s0 + min(n - NH, nlive - 1); };
  auto load_u = [&](int p, double (&u)[NV]) {
    const unsigned pb = plane_off(p);
#pragma unroll
    for (int n = 0; n < NV; n++) u[n] = plane_load(uold + var_of(n) * A.pitch_var, pb, colb);
  };
  auto load_g = [&](int p, double (&g)[3]) {
    if (GRAV) {
      const unsigned pb = plane_off(p);
#pragma unroll
      for (int d = 0; d < 3; d++) g[d] = plane_load(grav + (long)d * A.pitch_var, pb, colb);
    } else {
      g[0] = g[1] = g[2] = 0.0;
    }
  };

  double qmz[NV];                   // qm along z of plane c-1
  double fzlo[G];                   // z flux of the scalars through the -z face of plane c-1
  double upre[NV], gpre[3];         // prefetch: plane c+1
  double rold = 0.0, sold[G];       // uold density / scalars of plane c-1
  double rnew = 0.0;                // uold density of plane c
  double partx[G], fyown[G], dz[G], px[G], fy[G];
  int sa = 0, sb = 1, sc = 2;
  {
    double u[NV], g[3], q[NV];
    load_u(z0 - 2, u); load_g(z0 - 2, g);
    ctoprim_cell<NV, GRAV, NE>(u, g, dtxhalf, P, q);
#pragma unroll
    for (int n = 0; n < NV; n++) qring[sa].v[n][ty][tx] = q[n];
    load_u(z0 - 1, u); load_g(z0 - 1, g);
    ctoprim_cell<NV, GRAV, NE>(u, g, dtxhalf, P, q);
#pragma unroll
    for (int n = 0; n < NV; n++) qring[sb].v[n][ty][tx] = q[n];
    load_u(z0, upre); load_g(z0, gpre);
#pragma unroll
    for (int n = 0; n < NV; n++) qmz[n] = 1.0;
#pragma unroll
    for (int j = 0; j < G; j++) { fzlo[j] = 0.0; sold[j] = 0.0; partx[j] = 0.0; fyown[j] = 0.0; dz[j] = 0.0; px[j] = 0.0; }
  }
  __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0)
  __syncthreads();
  const int txm = tx - 1, txp = tx + 1;
  const int tym = ty - 1, typ = ty + 1;

  for (int c = z0 - 1; c <= z1; c++) {
    Plane<BY, NV> &M = mring[c & 1];
    Plane<BY, NV> &Mprev = mring[(c & 1) ^ 1];
    // ---- phase A: plane c+1 arrives; trace plane c; x and z fluxes of the scalars ----
    double qc[NV];
    ctoprim_cell<NV, GRAV, NE>(upre, gpre, dtxhalf, P, qc);
    if (RING == 3 || !r_trace) {
#pragma unroll
      for (int n = 0; n < NV; n++) qring[RING == 3 ? sc : sa].v[n][ty][tx] = qc[n];
    }
    double rnew_m = 0.0;            // the hydro pass's new density of plane c-1
    double ucur[G];
    if (r_fxz) {
      const unsigned pc = plane_off(c);
      rnew = plane_load(uold, pc, colb);
#pragma unroll
      for (int j = 0; j < G; j++) ucur[j] = plane_load(uold + var_of(NH + j) * A.pitch_var, pc, colb);
      rnew_m = plane_load(unew, plane_off(c - 1), colb);
    }
    double qpy[NV];
    if (ST == 3) __syncthreads();
    if constexpr (r_trace) {
      const Plane<BY, NV> &qs = qring[sb];
      const Plane<BY, NV> &qprev = qring[sa];
      double qb[NV], dq[3][NV];
      if (ST == 3) {
        const Plane<BY, NV> &qnext = qring[sc];
        const int xs[3] = {txm, tx, txp}, ys[3] = {tym, ty, typ};
#pragma unroll
        for (int n = 0; n < NV; n++) {
          double nb[27], d3[3];
#pragma unroll
          for (int dj = 0; dj < 3; dj++)
#pragma unroll
            for (int di = 0; di < 3; di++) {
              nb[di + 3 * dj] = qprev.v[n][ys[dj]][xs[di]];
              nb[di + 3 * dj + 9] = qs.v[n][ys[dj]][xs[di]];
              nb[di + 3 * dj + 18] = qnext.v[n][ys[dj]][xs[di]];
            }
          qb[n] = nb[13];
          slope3_var(nb, d3);
          dq[0][n] = d3[0]; dq[1][n] = d3[1]; dq[2][n] = d3[2];
        }
      } else {
#pragma unroll
        for (int n = 0; n < NV; n++) {
          qb[n] = qs.v[n][ty][tx];
          dq[0][n] = slope1<ST>(qs.v[n][ty][txm], qb[n], qs.v[n][ty][txp], P);
          dq[1][n] = slope1<ST>(qs.v[n][tym][tx], qb[n], qs.v[n][typ][tx], P);
          dq[2][n] = slope1<ST>(qprev.v[n][ty][tx], qb[n], qc[n], P);
        }
      }
      if (RING == 2) {
#pragma unroll
        for (int n = 0; n < NV; n++) qring[sa].v[n][ty][tx] = qc[n];
      }
      double qm[3][NV], qp[3][NV];
      trace3d_cell<NV, NE>(qb, dq, dtdx, dtdx, dtdx, P, qm, qp);
#pragma unroll
      for (int n = 0; n < NV; n++) M.v[n][ty][tx] = qm[1][n];
#pragma unroll
      for (int n = 0; n < NV; n++) qpy[n] = qp[1][n];
      if constexpr (r_fxz) {
        double qL[NV], fx[NV], fz[NV];
#pragma unroll
        for (int n = 0; n < NV; n++) qL[n] = wave_shr1(qm[0][n]);
        scaled_interface_flux<RS, NV, 0, true, NE>(qL, qp[0], P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, fx);
        scaled_interface_flux<RS, NV, 2, true, NE>(qmz, qp[2], P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, fz);
#pragma unroll
        for (int n = 0; n < NV; n++) qmz[n] = qm[2][n];
#pragma unroll
        for (int j = 0; j < G; j++) {
          dz[j] = fzlo[j] - fz[NH + j];
          fzlo[j] = fz[NH + j];
          px[j] = ucur[j] + (fx[NH + j] - wave_shl1(fx[NH + j]));
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    {
      const int pn = min(c + 2, z1 + 1);
      load_u(pn, upre); load_g(pn, gpre);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();

    // ---- phase B: y flux of plane c; finish plane c-1 ----
    if constexpr (ROLE == ROLE_FULL || ROLE == ROLE_HIGH) {
      double qL[NV], f[NV];
#pragma unroll
      for (int n = 0; n < NV; n++) qL[n] = M.v[n][tym][tx];
      scaled_interface_flux<RS, NV, 1, true, NE>(qL, qpy, P, A.dt, A.dx, A.rdx, dtdx, DXPOW2, f);
#pragma unroll
      for (int j = 0; j < G; j++) { fy[j] = f[NH + j]; M.v[NH + j][tym][tx] = fy[j]; }
    }
    if constexpr (r_fxz) {
      double un[G];
#pragma unroll
      for (int j = 0; j < G; j++) un[j] = (partx[j] + (fyown[j] - Mprev.v[NH + j][ty][tx])) + dz[j];
      // set_uold's passive-scalar fix near the density floor (hydro/godunov_fine.f90:176-190), as in sweep_march
      if (rold < P.smallr && rnew_m > rold) {
#pragma unroll
        for (int j = 0; j < G; j++) un[j] = sold[j] * dmaxd(rnew_m, P.smallr) / P.smallr;
      } else if (rnew_m < P.smallr && rold > rnew_m) {
#pragma unroll
        for (int j = 0; j < G; j++) un[j] = sold[j] * P.smallr / dmaxd(rold, P.smallr);
      }
      rold = rnew;
#pragma unroll
      for (int j = 0; j < G; j++) { sold[j] = ucur[j]; partx[j] = px[j]; fyown[j] = fy[j]; }
      const unsigned pb = plane_off(c - 1);
      const unsigned so = (c >= z0 + 1) ? colb_upd : BUF_OOB;
#pragma unroll
      for (int j = 0; j < G; j++)
        if (j < nlive) plane_store(unew + var_of(NH + j) * A.pitch_var, pb, so, un[j]);
    }
    if (RING == 3) { const int t = sa; sa = sb; sb = sc; sc = t; }
    else { const int t = sa; sa = sb; sb = t; }
  }
}

template <int ST, int RS, bool GRAV, int NE>
__global__ __launch_bounds__(BX * 8) void godunov_scalar_kernel(SweepArgs A, int s0, int nlive) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int BY = 8;
  const int ty = threadIdx.y;
  if (ty >= 2 && ty <= BY - 3) __builtin_amdgcn_s_setprio(3);
  if (ty == 0) scalar_march<ST, RS, GRAV, NE, ROLE_HALO>(A, s0, nlive, smem_raw);
  else if (ty == BY - 1) scalar_march<ST, RS, GRAV, NE, ROLE_HALO_HI>(A, s0, nlive, smem_raw);
  else if (ty == 1) scalar_march<ST, RS, GRAV, NE, ROLE_LOW>(A, s0, nlive, smem_raw);
  else if (ty == BY - 2) scalar_march<ST, RS, GRAV, NE, ROLE_HIGH>(A, s0, nlive, smem_raw);
  else scalar_march<ST, RS, GRAV, NE, ROLE_FULL>(A, s0, nlive, smem_raw);
}

// ---------------------------------------------------------------------------
// surface pass of a level in tiles (SurfArgs): the fluxes owed to the coarser level
// ---------------------------------------------------------------------------
// index (0-based) of cell (x, y, z) of the level in a cell vector; the layout gave every position this pass asks for a tile
__device__ __forceinline__ long surf_cell(const SurfArgs &A, int x, int y, int z) {
  // (the level's box is whole tiles, per axis: a coarse grid of several cells is not a cube; the pass asks for cells at most
  //  two beyond a face of the box)
  const int nx = 2 * TILE_OX * A.ntx, ny = 2 * TILE_OY * A.nty, nz = 2 * TILE_OZ * A.ntz;
  x = x < 0 ? x + nx : (x >= nx ? x - nx : x);
  y = y < 0 ? y + ny : (y >= ny ? y - ny : y);
  z = z < 0 ? z + nz : (z >= nz ? z - nz : z);
  const int ox = x >> 1, oy = y >> 1, oz = z >> 1;
  const int t = (ox / TILE_OX) + A.ntx * ((oy / TILE_OY) + A.nty * (oz / TILE_OZ));
  const long c0 = A.dir[t];
  const int ind = (x & 1) + 2 * (y & 1) + 4 * (z & 1);
  return c0 + (ox % TILE_OX) + TILE_OX * ((oy % TILE_OY) + TILE_OY * (oz % TILE_OZ)) + (long)ind * A.ngd;
}
// One interface of direction DIR between the cells lo (left) and hi = lo + e_DIR: the twelve cells the two traces read -- four
// along DIR (lo - 1 .. hi + 1), the four transverse neighbours of each of the two -- are addressed and requested FIRST (the kernel
// is a gather of isolated 8-byte words: what it costs is the latency of dependent loads, so nothing may wait between them), then
// converted (ctoprim), then the slopes and the two traces -- what a lane of the marching kernel does for its cell in phase A --
// and the Riemann flux, scaled like the marching kernel's.
// (slope type 3: the 3 x 3 x 3 neighbourhoods of the two cells -- 36 cells, four slabs of nine along DIR)
// (NF = NV + 2: pressure_fix -- fl[NV], fl[NV + 1] = the face velocity and the internal-energy flux, scaled like the fluxes)
template <int RS, int NV, bool GRAV, int SCHEME, int DIR, int NF = NV>
__device__ __forceinline__ void surf_interface27(const SurfArgs &A, const int (&lo)[3], double (&fl)[NF]) {
  constexpr int T0 = DIR == 0 ? 1 : 0, T1 = DIR == 2 ? 1 : 2;
  long c[36];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
      for (int v = 0; v < 3; v++) {
        int p[3] = {lo[0], lo[1], lo[2]};
        p[DIR] += a - 1; p[T0] += u - 1; p[T1] += v - 1;
        c[a * 9 + u * 3 + v] = surf_cell(A, p[0], p[1], p[2]);
      }
  double q[36][NV];
#pragma unroll
  for (int k = 0; k < 36; k++) {
    double u[NV], g[3];
#pragma unroll
    for (int n = 0; n < NV; n++) u[n] = A.uold[(long)n * A.ncell + c[k]];
#pragma unroll
    for (int d = 0; d < 3; d++) g[d] = GRAV ? A.grav[(long)d * A.ncell + c[k]] : 0.0;
    ctoprim_cell<NV, GRAV>(u, g, A.dt * 0.5, A.P, q[k]);
  }
  const double dtdx = A.dt / A.dx;
  double qL[NV], qR[NV];
#pragma unroll
  for (int w = 0; w < 2; w++) {
    double dq[3][NV], qm[3][NV], qp[3][NV];
#pragma unroll
    for (int n = 0; n < NV; n++) {
      double nb[27], d3[3];
#pragma unroll
      for (int dz = 0; dz < 3; dz++)
#pragma unroll
        for (int dy = 0; dy < 3; dy++)
#pragma unroll
          for (int dx = 0; dx < 3; dx++) {
            const int o[3] = {dx, dy, dz};
            nb[dx + 3 * dy + 9 * dz] = q[(w + o[DIR]) * 9 + o[T0] * 3 + o[T1]][n];
          }
      slope3_var(nb, d3);
      dq[0][n] = d3[0]; dq[1][n] = d3[1]; dq[2][n] = d3[2];
    }
    const double (&qb)[NV] = q[(1 + w) * 9 + 4];
    if (SCHEME == 0) trace3d_cell<NV>(qb, dq, dtdx, dtdx, dtdx, A.P, qm, qp);
    else tracexyz_cell<NV>(qb, dq, ctoprim_sound(qb[0], qb[4], A.P), dtdx, dtdx, dtdx, A.P, qm, qp);
#pragma unroll
    for (int n = 0; n < NV; n++) { if (w == 0) qL[n] = qm[DIR][n]; else qR[n] = qp[DIR][n]; }
  }
  if constexpr (NF == NV) {
  scaled_interface_flux<RS, NV, DIR, false>(qL, qR, A.P, A.dt, A.dx, A.rdx, dtdx, A.pow2 != 0, fl);   // (as the marching kernel of a level in tiles does)
  } else {
#ifndef RAMSES_AMD_FAST
    double f[NV], t[2];
    scaled_interface_flux_tmp<RS, NV, DIR>(qL, qR, A.P, A.dt, A.dx, A.rdx, A.pow2 != 0, f, t);
#pragma unroll
    for (int n = 0; n < NV; n++) fl[n] = f[n];
    fl[NV] = t[0]; fl[NV + 1] = t[1];
#endif
  }
}
template <int ST, int RS, int NV, bool GRAV, int SCHEME, int DIR, int NF = NV>
__device__ __forceinline__ void surf_interface(const SurfArgs &A, const int (&lo)[3], double (&fl)[NF]) {
  if constexpr (ST == 3) { surf_interface27<RS, NV, GRAV, SCHEME, DIR, NF>(A, lo, fl); return; }
  constexpr int T0 = DIR == 0 ? 1 : 0, T1 = DIR == 2 ? 1 : 2;
  long c[12];
  // 0..3: along DIR at lo-1, lo, hi, hi+1;  4..7: lo -T0, +T0, -T1, +T1;  8..11: the same of hi
#pragma unroll
  for (int k = 0; k < 4; k++) {
    int p[3] = {lo[0], lo[1], lo[2]};
    p[DIR] += k - 1;
    c[k] = surf_cell(A, p[0], p[1], p[2]);
  }
#pragma unroll
  for (int w = 0; w < 2; w++)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      int p[3] = {lo[0], lo[1], lo[2]};
      p[DIR] += w;
      p[k < 2 ? T0 : T1] += (k & 1) ? 1 : -1;
      c[4 + 4 * w + k] = surf_cell(A, p[0], p[1], p[2]);
    }
  double q[12][NV];
  {
    double u[12][NV], g[12][3];
#pragma unroll
    for (int k = 0; k < 12; k++) {
#pragma unroll
      for (int n = 0; n < NV; n++) u[k][n] = A.uold[(long)n * A.ncell + c[k]];
#pragma unroll
      for (int d = 0; d < 3; d++) g[k][d] = GRAV ? A.grav[(long)d * A.ncell + c[k]] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 12; k++) ctoprim_cell<NV, GRAV>(u[k], g[k], A.dt * 0.5, A.P, q[k]);
  }
  const double dtdx = A.dt / A.dx;
  double qL[NV], qR[NV];
#pragma unroll
  for (int w = 0; w < 2; w++) {
    double dq[3][NV], qm[3][NV], qp[3][NV];
#pragma unroll
    for (int n = 0; n < NV; n++) {
      dq[DIR][n] = slope1<ST>(q[w][n], q[1 + w][n], q[2 + w][n], A.P);
      dq[T0][n] = slope1<ST>(q[4 + 4 * w][n], q[1 + w][n], q[5 + 4 * w][n], A.P);
      dq[T1][n] = slope1<ST>(q[6 + 4 * w][n], q[1 + w][n], q[7 + 4 * w][n], A.P);
    }
    if (SCHEME == 0) trace3d_cell<NV>(q[1 + w], dq, dtdx, dtdx, dtdx, A.P, qm, qp);
    else tracexyz_cell<NV>(q[1 + w], dq, ctoprim_sound(q[1 + w][0], q[1 + w][4], A.P), dtdx, dtdx, dtdx, A.P, qm, qp);
#pragma unroll
    for (int n = 0; n < NV; n++) { if (w == 0) qL[n] = qm[DIR][n]; else qR[n] = qp[DIR][n]; }
  }
  if constexpr (NF == NV) {
  scaled_interface_flux<RS, NV, DIR, false>(qL, qR, A.P, A.dt, A.dx, A.rdx, dtdx, A.pow2 != 0, fl);   // (as the marching kernel of a level in tiles does)
  } else {
#ifndef RAMSES_AMD_FAST
    double f[NV], t[2];
    scaled_interface_flux_tmp<RS, NV, DIR>(qL, qR, A.P, A.dt, A.dx, A.rdx, A.pow2 != 0, f, t);
#pragma unroll
    for (int n = 0; n < NV; n++) fl[n] = f[n];
    fl[NV] = t[0]; fl[NV + 1] = t[1];
#endif
  }
}
#ifndef RAMSES_AMD_FAST
// difmag > 0: the diffusive term of the interface between lo and hi = lo + e_DIR (consup), added to the scaled flux fl.  The
// four corners of the face take the velocities of the 2 x 3 x 3 cells round it -- ctoprim_cell's, with the half kick of the
// gravity, exactly what the marching kernel's ring holds -- and the term the conserved pair lo, hi.  A gather of its own after
// the interface routine's (the cells of that one are cache hits here): the routines of the kernels without difmag stay as they are.
template <int NV, bool GRAV, int DIR>
__device__ __forceinline__ void surf_difmag_term(const SurfArgs &A, double coef_difmag, const int (&lo)[3], double (&fl)[NV]) {
  constexpr int T0 = DIR == 0 ? 1 : 0, T1 = DIR == 2 ? 1 : 2;
  long c[2][3][3];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
      for (int v = 0; v < 3; v++) {
        int p[3] = {lo[0], lo[1], lo[2]};
        p[DIR] += s; p[T0] += u - 1; p[T1] += v - 1;
        c[s][u][v] = surf_cell(A, p[0], p[1], p[2]);
      }
  double vel[2][3][3][3], ulo[NV], uhi[NV];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
      for (int v = 0; v < 3; v++) {
        double uc[NV], g[3], q[NV];
#pragma unroll
        for (int n = 0; n < NV; n++) uc[n] = A.uold[(long)n * A.ncell + c[s][u][v]];
#pragma unroll
        for (int d = 0; d < 3; d++) g[d] = GRAV ? A.grav[(long)d * A.ncell + c[s][u][v]] : 0.0;
        ctoprim_cell<NV, GRAV>(uc, g, A.dt * 0.5, A.P, q);
#pragma unroll
        for (int d = 0; d < 3; d++) vel[s][u][v][d] = q[1 + d];
        if (u == 1 && v == 1) {
#pragma unroll
          for (int n = 0; n < NV; n++) { if (s == 0) ulo[n] = uc[n]; else uhi[n] = uc[n]; }
        }
      }
  const double fdiv = 0.25 / A.dx;
  double cn[2][2];
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) {
      double w[3][2][2][2];
#pragma unroll
      for (int d = 0; d < 3; d++)
#pragma unroll
        for (int dk = 0; dk < 2; dk++)
#pragma unroll
          for (int dj = 0; dj < 2; dj++)
#pragma unroll
            for (int di = 0; di < 2; di++) {
              const int o[3] = {di, dj, dk};
              w[d][dk][dj][di] = vel[o[DIR]][a + o[T0]][b + o[T1]][d];
            }
      cn[a][b] = difmag::cmpdivu_corner(w, fdiv, fdiv, fdiv);
    }
  const double coef = difmag::consup_coef(coef_difmag, difmag::consup_div1<DIR>(cn));
#pragma unroll
  for (int n = 0; n < NV; n++) fl[n] = difmag::consup_term(fl[n], A.dt, coef, uhi[n], ulo[n]);
}
template <int NV, bool GRAV>
__device__ __forceinline__ void surf_difmag_add(const SurfArgs &A, double coef_difmag, int dirn, const int (&lo)[3], double (&fl)[NV]) {
  if (dirn == 0) surf_difmag_term<NV, GRAV, 0>(A, coef_difmag, lo, fl);
  else if (dirn == 1) surf_difmag_term<NV, GRAV, 1>(A, coef_difmag, lo, fl);
  else surf_difmag_term<NV, GRAV, 2>(A, coef_difmag, lo, fl);
}
#endif
// (NF = NV + 2: the records' last two slots are written too -- pressure_fix; NF = NV: they are neither written nor read)
// (the body as a macro, not a function of its own: through a function the compiler commutes the operands of 27 additions of
//  surface_flux_kernel -- harmless, but the kernels without pressure_fix are to stay the code they were, instruction for
//  instruction.  Events arrive sorted by device oct and face -- round 6, session T: 2.59 -> 2.38 ms strict on the shell level
//  against the (face, oct) order -- and the four fine faces of an event sit in neighbouring lanes.  The updated cell behind fine
//  face q of face f (q: the two transverse coordinates, lower axis first), the ghost cell beyond the face, lo = the left cell of
//  the interface; hydro/godunov_fine.f90:720-747: reset when the cell on either side is refined (a ghost cell never is))
// (POST: what a kernel does to the flux between the interface routine and the reset -- nothing, or the diffusive term of difmag)
#define SURFACE_FLUX_BODY(SCHEME, NF, POST) \
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x; \
  if (t >= (long)A.nevent * 4) return; \
  const int e = A.qminor ? (int)(t >> 2) : (int)(t % A.nevent), q = A.qminor ? (int)(t & 3) : (int)(t / A.nevent); \
  const int ev = A.events[e]; \
  const int io = ev / 6, f = ev % 6; \
  const int dirn = f >> 1, side = f & 1; \
  const long r = (long)A.ig[io] - A.base; \
  const int tl = A.tileid[r / TILE_OCTS], l = (int)(r % TILE_OCTS); \
  int p[3] = {2 * ((tl % A.ntx) * TILE_OX + l % TILE_OX), 2 * (((tl / A.ntx) % A.nty) * TILE_OY + (l / TILE_OX) % TILE_OY), \
              2 * ((tl / (A.ntx * A.nty)) * TILE_OZ + l / (TILE_OX * TILE_OY))}; \
  const int t0 = dirn == 0 ? 1 : 0, t1 = dirn == 2 ? 1 : 2; \
  p[dirn] += side; p[t0] += q & 1; p[t1] += q >> 1; \
  const bool zero = (A.stat[surf_cell(A, p[0], p[1], p[2])] & CELL_REFINED) != 0; \
  int lo[3] = {p[0], p[1], p[2]}; \
  if (!side) lo[dirn] -= 1; \
  double fl[NF]; \
  if (dirn == 0) surf_interface<ST, RS, NV, GRAV, SCHEME, 0, NF>(A, lo, fl); \
  else if (dirn == 1) surf_interface<ST, RS, NV, GRAV, SCHEME, 1, NF>(A, lo, fl); \
  else surf_interface<ST, RS, NV, GRAV, SCHEME, 2, NF>(A, lo, fl); \
  POST \
  double *dst = A.rec + ((long)e * 4 + q) * (NV + 2); \
  _Pragma("unroll") for (int n = 0; n < NF; n++) dst[n] = zero ? 0.0 : fl[n];
template <int ST, int RS, int NV, bool GRAV, int SCHEME = 0>
__global__ __launch_bounds__(128) void surface_flux_kernel(SurfArgs A) {
  SURFACE_FLUX_BODY(SCHEME, NV, )
}
#ifndef RAMSES_AMD_FAST
template <int ST, int RS, int NV, bool GRAV>
__global__ __launch_bounds__(128) void surface_flux_pfix_kernel(SurfArgs A) {
  SURFACE_FLUX_BODY(0, NV + 2, )
}
// difmag > 0: the flux of the interface WITH the diffusive term (the coarser level is owed what the fine cell exchanged)
template <int ST, int RS, int NV, bool GRAV>
__global__ __launch_bounds__(128) void surface_flux_difmag_kernel(SurfArgs A, SweepDifmag D) {
#define SURFACE_DIFMAG_POST surf_difmag_add<NV, GRAV>(A, D.difmag, dirn, lo, fl);
  SURFACE_FLUX_BODY(0, NV, SURFACE_DIFMAG_POST)
#undef SURFACE_DIFMAG_POST
}
#endif
#undef SURFACE_FLUX_BODY

// ---------------------------------------------------------------------------
// host-side dispatch
// ---------------------------------------------------------------------------
// The runtime options of a call -- slope type, solver, NVAR, scheme, gravity, tile rows, NENER, brick or tiles -- become template
// arguments in one way: pick(v, IntList<...>(), f) calls f(std::integral_constant<int, V>()) for the V of the list that equals v
// and returns hipErrorInvalidValue when there is none; pick(b, f) does the same for a bool.  The lists below are the option
// matrix -- a value that is in no list has no kernel -- and a family is its preconditions, its Lds<...> and its kernel.
// (tests/test_sweep_dispatch_host.py holds, from a CPU run, which kernel every combination of options launches)
template <int... V>
struct IntList {};
template <int... V, class F>
static hipError_t pick(int v, IntList<V...>, F &&f) {
  hipError_t e = hipErrorInvalidValue;
  (void)(... || (v == V && ((e = f(std::integral_constant<int, V>())), true)));
  return e;
}
template <class F>
static hipError_t pick(bool b, F &&f) {
  return b ? f(std::true_type()) : f(std::false_type());
}
template <int... A, int... B>
IntList<A..., B...> operator+(IntList<A...>, IntList<B...>);      // (two lists in a row; declared only, for decltype)

#ifndef SWEEP_FLAGSHIP_ONLY
using Slopes3D = IntList<1, 0, 2, 3, 7, 8>;
using Slopes1D = IntList<4, 5, 6>;                         // the NDIM=1 slope types: the plain sweep only
using Solvers = IntList<RIEMANN_LLF, RIEMANN_HLLC, RIEMANN_HLL, RIEMANN_ACOUSTIC, RIEMANN_EXACT>;
using Nvars = IntList<5, 6, 7>;
using Schemes = IntList<0, 1>;                             // muscl, plmde
#else
// (scripts/build_variant.sh, scripts/sweep_regs.sh, build_ab.py: minmod, LLF, NVAR 5, muscl only -- a one-minute compile)
using Slopes3D = IntList<1>;
using Slopes1D = IntList<>;
using Solvers = IntList<RIEMANN_LLF>;
using Nvars = IntList<5>;
using Schemes = IntList<0>;
#endif
constexpr bool is_1d(int st) { return st == 4 || st == 5 || st == 6; }
// (every family but the plain sweep picks its solver here: nothing for the NDIM=1 slope types)
template <int ST>
using SolversOf = std::conditional_t<is_1d(ST), IntList<>, Solvers>;
// the (solver, NVAR, gravity) of a call: f(RS, NV, GRAV)
template <class RSList, class F>
static hipError_t pick_variant(RSList, int rs, int nvar, bool grav, F &&f) {
  return pick(rs, RSList(), [&](auto r) { return pick(nvar, Nvars(), [&](auto nv) { return pick(grav, [&](auto g) { return f(r, nv, g); }); }); });
}

// Rows of the workgroup that sweeps a variant: 8 (two waves per SIMD, 256 VGPRs, smaller LDS planes) for the register/LDS-hungry
// ones -- the Newton solver, the 27-point slope, the PLMDE tracing, runs with passive scalars --, else 12 on the brick and
// TILE_SWEEP_BY on a level in tiles.  THE rule: the launchers choose kernels by it, the instantiations that exist follow from it
// (sweep_variant), and the plan of csrc/capi_amr.hip cuts the work items of a level by it (tile_sweep_rows).
constexpr int sweep_rows(int st, int rs, int nv, int scheme, bool tiles) {
  if (rs == RIEMANN_EXACT || st == 3 || scheme != 0 || nv != 5) return 8;
  if (tiles) return TILE_SWEEP_BY;
  return is_1d(st) ? 8 : 12;
}
// the godunov_sweep_kernel instantiations that exist
constexpr bool sweep_variant(int st, int rs, int by, bool grav, int scheme, int nv, bool tiles) {
  // NDIM=1 slope types: the plain configuration only (the reference's 1-D tests: NVAR=3 embedded as 5, muscl, no gravity)
  if (is_1d(st) && (grav || scheme != 0 || nv != 5 || tiles)) return false;
  if (scheme == 1 && nv != 5) return false;                // plmde: the hydro variables only
  return by == sweep_rows(st, rs, nv, scheme, tiles) || (by == 8 && !tiles);      // (the brick has every variant in 8 rows too)
}
// NENER > 0: LLF, HLL, HLLC
constexpr bool nener_solver(int rs) { return rs == RIEMANN_LLF || rs == RIEMANN_HLL || rs == RIEMANN_HLLC; }

template <class K, class... Args>
static hipError_t launch_kernel(K k, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args) {
  if (lds > 0) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k, grid, block, lds, s, args...);
  return hipGetLastError();
}
// the surface pass: one thread per (event, fine face)
template <class K, class... Args>
static hipError_t launch_surface(K k, hipStream_t s, const SurfArgs &A, const Args &...args) {
  return launch_kernel(k, dim3((unsigned)(((long)A.nevent * 4 + 127) / 128)), dim3(128), 0, s, A, args...);
}

// The entry points of one slope type.  One translation unit per slope type (ramses_amd/build.py compiles this file once without
// SWEEP_ST -- the dispatchers at the end -- and once per slope type with -DSWEEP_ST=<type>, 3 standing for 3, 4, 5 and 6, for
// each arithmetic: the instantiations of the option matrix build side by side instead of in two nine-minute compiles; the
// variant builds of scripts/build_variant.sh -- SWEEP_FLAGSHIP_ONLY -- keep one unit)
template <int ST>
struct SweepOf {
  static hipError_t sweep(SweepArgs &A, int rs, int by, int scheme, int nvar, bool grav, hipStream_t s);
  static hipError_t nener(SweepArgs &A, int rs, int nvar, int nener, hipStream_t s);
  static hipError_t scalars(SweepArgs &A, int rs, int by, int nvar, int nener, bool grav, hipStream_t s);
  static hipError_t surface(const SurfArgs &A, int rs, int nvar, int scheme, bool grav, hipStream_t s);
#ifndef RAMSES_AMD_FAST
  // pressure_fix, difmag > 0: a level in tiles, muscl, NVAR 5 .. 7, every solver
  static hipError_t pfix(SweepArgs &A, const SweepPfix &X, int rs, int nvar, bool grav, hipStream_t s);
  static hipError_t difmag(SweepArgs &A, const SweepDifmag &D, int rs, int nvar, bool grav, hipStream_t s);
  static hipError_t surface_pfix(const SurfArgs &A, int rs, int nvar, bool grav, hipStream_t s);
  static hipError_t surface_difmag(const SurfArgs &A, const SweepDifmag &D, int rs, int nvar, bool grav, hipStream_t s);
#endif
};

template <int ST>
hipError_t SweepOf<ST>::surface(const SurfArgs &A, int rs, int nvar, int scheme, bool grav, hipStream_t s) {
  return pick_variant(SolversOf<ST>(), rs, nvar, grav, [&](auto r, auto nv, auto g) {
    return pick(scheme, Schemes(), [&](auto sc) {
      constexpr int RS = decltype(r)::value, NV = decltype(nv)::value, SCHEME = decltype(sc)::value;
      if constexpr (SCHEME == 1 && NV != 5) return hipErrorInvalidValue;
      else return launch_surface(surface_flux_kernel<ST, RS, NV, decltype(g)::value, SCHEME>, s, A);
    });
  });
}
#ifndef RAMSES_AMD_FAST
template <int ST>
hipError_t SweepOf<ST>::surface_pfix(const SurfArgs &A, int rs, int nvar, bool grav, hipStream_t s) {
  return pick_variant(SolversOf<ST>(), rs, nvar, grav, [&](auto r, auto nv, auto g) {
    return launch_surface(surface_flux_pfix_kernel<ST, decltype(r)::value, decltype(nv)::value, decltype(g)::value>, s, A);
  });
}
template <int ST>
hipError_t SweepOf<ST>::surface_difmag(const SurfArgs &A, const SweepDifmag &D, int rs, int nvar, bool grav, hipStream_t s) {
  return pick_variant(SolversOf<ST>(), rs, nvar, grav, [&](auto r, auto nv, auto g) {
    return launch_surface(surface_flux_difmag_kernel<ST, decltype(r)::value, decltype(nv)::value, decltype(g)::value>, s, A, D);
  });
}
#endif

// tiles of the whole brick, then the boxes this launch covers (A.region); 0 = nothing to sweep, -1 = bad region
static int plan_boxes(SweepArgs &A, int by) {
  const int NTX = (A.nx + (BX - 4) - 1) / (BX - 4);
  const int NTY = (A.ny + (by - 4) - 1) / (by - 4);
  // Boundary shell / interior split used to overlap the halo exchange with the
  // interior sweep: shell = the tiles and planes that produce the cells within
  // 2 of a face (what the neighbours receive); zb planes at each z end.  The six
  // shell boxes go into ONE launch, cut into short z-chunks so that the thin
  // slabs still fill the chip.
  const int zb = 2;
  const bool splittable = NTX >= 3 && NTY >= 3 && A.nz >= 4 * zb;
  A.nbox = 0;
  int nblocks = 0;
  auto add_box = [&](int tx0, int tx1, int ty0, int ty1, int zlo, int zhi, int zchunk) {
    if (tx1 <= tx0 || ty1 <= ty0 || zhi <= zlo) return;
    SweepBox &B = A.box[A.nbox++];
    B.tx0 = tx0; B.ntx = tx1 - tx0; B.ty0 = ty0; B.nty = ty1 - ty0;
    B.zlo = zlo; B.zhi = zhi; B.zchunk = zchunk < (zhi - zlo) ? zchunk : (zhi - zlo);
    B.first = nblocks;
    nblocks += B.ntx * B.nty * ((zhi - zlo + B.zchunk - 1) / B.zchunk);
  };
  const int zc = A.zchunk;
  if (A.region == SWEEP_ALL || (A.region == SWEEP_SHELL && !splittable)) {
    add_box(0, NTX, 0, NTY, 0, A.nz, zc);
  } else if (A.region == SWEEP_INTERIOR) {
    if (splittable) add_box(1, NTX - 1, 1, NTY - 1, zb, A.nz - zb, zc);
  } else if (A.region == SWEEP_SHELL) {
    const int zs = 32;
    // (long blocks first, the 2-plane slabs fill the gaps at the end)
    add_box(0, 1, 1, NTY - 1, zb, A.nz - zb, zs);                       // x low tile column
    add_box(NTX - 1, NTX, 1, NTY - 1, zb, A.nz - zb, zs);               // x high tile column
    add_box(0, NTX, 0, 1, zb, A.nz - zb, zs);                           // y low tile row
    add_box(0, NTX, NTY - 1, NTY, zb, A.nz - zb, zs);                   // y high tile row
    add_box(0, NTX, 0, NTY, 0, zb, zs);                                 // z low slab
    add_box(0, NTX, 0, NTY, A.nz - zb, A.nz, zs);                       // z high slab
  } else {
    return -1;
  }
  if (nblocks == 0) return 0;
  A.nblocks = nblocks;
  return nblocks;
}

// a level of a resident AMR run in tiles: one workgroup per work item of the plan (the box decode runs, its result is replaced
// by the work item)
static bool tile_items(SweepArgs &A) {
  if (!A.stat || !A.dir || !A.work || A.ng != 0 || A.nwork <= 0) return false;
  A.nblocks = A.nwork;
  A.nbox = 1;
  return true;
}

template <int ST, int RS, int BY, bool GRAV, int SCHEME, int NV, bool MASK>
static hipError_t launch_sweep(const SweepArgs &A, hipStream_t s) {
  if constexpr (!sweep_variant(ST, RS, BY, GRAV, SCHEME, NV, MASK)) {
    return hipErrorInvalidValue;
  } else {
    typedef Lds<ST, BY, NV, MASK, GRAV, 0, y_duty<ST, RS, BY, GRAV, SCHEME, NV, MASK>()> L;
    static_assert(L::bytes <= 160 * 1024, "one workgroup's LDS");
    return launch_kernel(godunov_sweep_kernel<ST, RS, BY, GRAV, SCHEME, NV, MASK>, dim3(A.nblocks), dim3(BX, BY), L::bytes, s, A);
  }
}
// the brick (by = 8, 12 or 0: the rule's) or, with A.stat, a level in tiles (MASK; the plan's work items were cut for
// tile_sweep_rows(...) interior rows; anything that has no kernel: the caller keeps the tree-walking sweep)
template <int ST>
hipError_t SweepOf<ST>::sweep(SweepArgs &A, int rs, int by, int scheme, int nvar, bool grav, hipStream_t s) {
  return pick(rs, Solvers(), [&](auto r) {
    constexpr int RS = decltype(r)::value;
    const bool tiles = A.stat != nullptr;
    const int rows = sweep_rows(ST, RS, nvar, scheme, tiles);
    if (by == 0 || rows == 8) by = rows;
    const int planned = plan_boxes(A, by);
    if (planned < 0) return hipErrorInvalidValue;
    if (planned == 0) return hipSuccess;
    if (tiles) {
      if (!tile_items(A)) return hipErrorInvalidValue;
    } else if (!is_1d(ST) && nvar == 5 && scheme != 1) {
      // (a scheme that is neither 0 nor 1 -- the C ABI passes no other -- runs as muscl in the 8-row tiles planned above: the
      //  launcher has always taken it so, and the dispatch record holds it)
      scheme = 0;
    }
    return pick(by, IntList<8, 12, TILE_SWEEP_BY>(), [&](auto b) { return pick(nvar, Nvars(), [&](auto nv) { return pick(scheme, Schemes(), [&](auto sc) {
      return pick(grav, [&](auto g) { return pick(tiles, [&](auto m) {
        return launch_sweep<ST, RS, decltype(b)::value, decltype(g)::value, decltype(sc)::value, decltype(nv)::value, decltype(m)::value>(A, s);
      }); }); }); }); });
  });
}

#ifndef RAMSES_AMD_FAST
// pressure_fix on a level in tiles: the plan's work items were cut for tile_sweep_rows_pfix interior rows
template <int ST>
hipError_t SweepOf<ST>::pfix(SweepArgs &A, const SweepPfix &X, int rs, int nvar, bool grav, hipStream_t s) {
  if (!X.divu || !X.enew || !tile_items(A)) return hipErrorInvalidValue;
  A.box[0] = SweepBox{0, 1, 0, 1, 0, A.nz, A.nz, 0};
  return pick_variant(SolversOf<ST>(), rs, nvar, grav, [&](auto r, auto nv, auto g) {
    constexpr int RS = decltype(r)::value, NV = decltype(nv)::value, BY = PfixRows<ST, NV>::BY;
    constexpr bool GRAV = decltype(g)::value;
    return launch_kernel(godunov_sweep_pfix_kernel<ST, RS, BY, GRAV, NV>, dim3(A.nblocks), dim3(BX, BY), Lds<ST, BY, NV, true, GRAV, 2>::bytes, s, A, X);
  });
}
// difmag > 0 on a level in tiles: the plan's work items were cut for tile_sweep_rows_difmag interior rows
template <int ST>
hipError_t SweepOf<ST>::difmag(SweepArgs &A, const SweepDifmag &D, int rs, int nvar, bool grav, hipStream_t s) {
  if (!(D.difmag > 0.0) || !tile_items(A)) return hipErrorInvalidValue;
  A.box[0] = SweepBox{0, 1, 0, 1, 0, A.nz, A.nz, 0};
  return pick_variant(SolversOf<ST>(), rs, nvar, grav, [&](auto r, auto nv, auto g) {
    constexpr int RS = decltype(r)::value, NV = decltype(nv)::value, BY = 8;
    constexpr bool GRAV = decltype(g)::value;
    return launch_kernel(godunov_sweep_difmag_kernel<ST, RS, BY, GRAV, NV>, dim3(A.nblocks), dim3(BX, BY),
                         Lds<ST, BY, NV, true, GRAV, 0, false, true, dif_parked<RS, NV>()>::bytes, s, A, D);
  });
}
#endif

// NENER > 0: (NE, NV) = (1, 6), (1, 7) [one passive scalar], (2, 7); LLF, HLL, HLLC; muscl, no gravity, the plain brick
template <int ST>
hipError_t SweepOf<ST>::nener(SweepArgs &A, int rs, int nvar, int nener, hipStream_t s) {
  return pick(rs, SolversOf<ST>(), [&](auto r) {
    constexpr int RS = decltype(r)::value;
    if constexpr (!nener_solver(RS)) {
      return hipErrorInvalidValue;
    } else {
      if (A.stat) return hipErrorInvalidValue;
      const int planned = plan_boxes(A, 8);
      if (planned < 0) return hipErrorInvalidValue;
      if (planned == 0) return hipSuccess;
      return pick(nener, IntList<1, 2>(), [&](auto ne) { return pick(nvar, IntList<6, 7>(), [&](auto nv) {
        constexpr int NE = decltype(ne)::value, NV = decltype(nv)::value;
        if constexpr (NV < 5 + NE) return hipErrorInvalidValue;
        else return launch_kernel(godunov_sweep_nener_kernel<ST, RS, NV, NE>, dim3(A.nblocks), dim3(BX, 8), Lds<ST, 8, NV, false, false>::bytes, s, A);
      }); });
    }
  });
}

// The scalar pass updates exactly the cells that the hydro pass of the same region updated -- it reads their new density back
// from unew -- so its boxes are planned in the hydro pass's tiles (sweep()'s rows: 12 or 8; the NENER kernels: 8) and re-cut
// into its own 8-row tiles (4 interior rows; 8 = 2 x 4, so the cut is exact): a shell and an interior call each stand alone.
static int plan_boxes_scalar(SweepArgs &A, int hydro_by) {
  const int planned = plan_boxes(A, hydro_by);
  if (planned <= 0 || hydro_by == 8) return planned;
  const int f = (hydro_by - 4) / 4, NTY = (A.ny + 3) / 4;
  int nblocks = 0, k = 0;
  for (int i = 0; i < A.nbox; i++) {
    SweepBox B = A.box[i];
    const int ty0 = B.ty0 * f, ty1 = min((B.ty0 + B.nty) * f, NTY);
    if (ty1 <= ty0) continue;
    B.ty0 = ty0; B.nty = ty1 - ty0; B.first = nblocks;
    nblocks += B.ntx * B.nty * ((B.zhi - B.zlo + B.zchunk - 1) / B.zchunk);
    A.box[k++] = B;
  }
  A.nbox = k;
  A.nblocks = nblocks;
  return nblocks;
}
// NVAR > 7: the scalar passes that follow the hydro pass (godunov_scalar_kernel), ceil(nscalars / G) launches of the whole
// region; the last group may hold fewer than G scalars.  Gravity with nener = 0 only.
template <int ST>
hipError_t SweepOf<ST>::scalars(SweepArgs &A, int rs, int by, int nvar, int nener, bool grav, hipStream_t s) {
  if (A.stat || nener < 0 || nener > MAX_NENER || nvar <= 7 || nvar > MAX_NVAR) return hipErrorInvalidValue;
  const int rows = nener > 0 ? 8 : sweep_rows(ST, rs, 5, 0, false);          // of the hydro pass: sweep() at NV = 5, muscl; nener()
  const int hydro_by = (by == 0 || rows == 8) ? rows : by;
  if (hydro_by != 8 && hydro_by != 12) return hipErrorInvalidValue;
  const int planned = plan_boxes_scalar(A, hydro_by);
  if (planned < 0) return hipErrorInvalidValue;
  if (planned == 0) return hipSuccess;
  return pick(grav, [&](auto g) { return pick(rs, SolversOf<ST>(), [&](auto r) { return pick(nener, IntList<0, 1, 2>(), [&](auto ne) {
    constexpr int RS = decltype(r)::value, NE = decltype(ne)::value;
    constexpr bool GRAV = decltype(g)::value;
    if constexpr (NE > 0 && (GRAV || !nener_solver(RS))) {
      return hipErrorInvalidValue;
    } else {
      typedef ScalarGroup<ST, RS, NE> SG;
      for (int s0 = SG::NH; s0 < nvar; s0 += SG::G) {
        const int nlive = nvar - s0 < SG::G ? nvar - s0 : SG::G;
        const hipError_t e = launch_kernel(godunov_scalar_kernel<ST, RS, GRAV, NE>, dim3(A.nblocks), dim3(BX, 8), SG::bytes, s, A, s0, nlive);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    }
  }); }); });
}

#if defined(SWEEP_ST)
template struct SweepOf<SWEEP_ST>;
#if SWEEP_ST == 3
template struct SweepOf<4>;
template struct SweepOf<5>;
template struct SweepOf<6>;
#endif
#elif !defined(SWEEP_FLAGSHIP_ONLY)
extern template struct SweepOf<0>;
extern template struct SweepOf<1>;
extern template struct SweepOf<2>;
extern template struct SweepOf<3>;
extern template struct SweepOf<4>;
extern template struct SweepOf<5>;
extern template struct SweepOf<6>;
extern template struct SweepOf<7>;
extern template struct SweepOf<8>;
#endif

#ifndef SWEEP_ST
// the public launchers (csrc/sweep_args.hpp): what does not depend on the variant, then the slope type
// (lanes address a plane of the brick with a 32-bit byte offset; a cell vector of a level in tiles likewise)
static bool brick_offsets_fit(const SweepArgs &A) {
  return (unsigned long)A.pitch_z * 8ul < (1ul << 31) && (unsigned long)A.pitch_var * 8ul < (1ul << 32);
}
static bool tile_offsets_fit(const SweepArgs &A) { return (unsigned long)A.pitch_var * 8ul < (1ul << 31); }

hipError_t launch_godunov_sweep(SweepArgs &A, int slope_type, int riemann, int by, int scheme, int nvar,
                                bool grav, hipStream_t s) {
  if (!brick_offsets_fit(A)) return hipErrorInvalidValue;
  return pick(slope_type, decltype(Slopes3D() + Slopes1D())(), [&](auto st) { return SweepOf<decltype(st)::value>::sweep(A, riemann, by, scheme, nvar, grav, s); });
}
hipError_t launch_godunov_sweep_nener(SweepArgs &A, int slope_type, int riemann, int nvar, int nener, hipStream_t s) {
  if (!brick_offsets_fit(A)) return hipErrorInvalidValue;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::nener(A, riemann, nvar, nener, s); });
}
hipError_t launch_godunov_sweep_scalars(SweepArgs &A, int slope_type, int riemann, int by, int nvar, int nener, bool grav, hipStream_t s) {
  if (!brick_offsets_fit(A)) return hipErrorInvalidValue;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::scalars(A, riemann, by, nvar, nener, grav, s); });
}
hipError_t launch_surface_flux(const SurfArgs &A, int slope_type, int riemann, int nvar, int scheme, bool grav, hipStream_t s) {
  if (A.nevent <= 0) return hipSuccess;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::surface(A, riemann, nvar, scheme, grav, s); });
}
// interior rows of a work item of the sweep of a level in tiles (the plan of csrc/capi_amr.hip cuts the level accordingly)
int tile_sweep_rows(int riemann, int nvar, int slope_type, int scheme) { return sweep_rows(slope_type, riemann, nvar, scheme, true) - 4; }

#ifndef RAMSES_AMD_FAST
hipError_t launch_godunov_sweep_pfix(SweepArgs &A, const SweepPfix &X, int slope_type, int riemann, int nvar, bool grav, hipStream_t s) {
  if (!tile_offsets_fit(A)) return hipErrorInvalidValue;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::pfix(A, X, riemann, nvar, grav, s); });
}
hipError_t launch_godunov_sweep_difmag(SweepArgs &A, const SweepDifmag &D, int slope_type, int riemann, int nvar, bool grav, hipStream_t s) {
  if (!tile_offsets_fit(A)) return hipErrorInvalidValue;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::difmag(A, D, riemann, nvar, grav, s); });
}
hipError_t launch_surface_flux_pfix(const SurfArgs &A, int slope_type, int riemann, int nvar, bool grav, hipStream_t s) {
  if (A.nevent <= 0) return hipSuccess;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::surface_pfix(A, riemann, nvar, grav, s); });
}
hipError_t launch_surface_flux_difmag(const SurfArgs &A, const SweepDifmag &D, int slope_type, int riemann, int nvar, bool grav, hipStream_t s) {
  if (A.nevent <= 0) return hipSuccess;
  return pick(slope_type, Slopes3D(), [&](auto st) { return SweepOf<decltype(st)::value>::surface_difmag(A, D, riemann, nvar, grav, s); });
}
// interior rows of a work item of the pressure_fix sweep of a level in tiles (PfixRows), and of the difmag sweep: the 8-row
// kernels for every NVAR and slope type
int tile_sweep_rows_pfix(int nvar, int slope_type) { return ((slope_type == 3 && nvar == 7) ? 6 : 8) - 4; }
int tile_sweep_rows_difmag(int nvar, int slope_type) { (void)nvar; (void)slope_type; return 8 - 4; }
#endif
#endif   // SWEEP_ST

}  // namespace SWEEP_NS
}  // namespace ramses_amd

#if SWEEP_CYCLE_PROBE && defined(RAMSES_AMD_FAST) && defined(SWEEP_ST) && SWEEP_ST == 1
// the probe's sums of the last launches of this unit's kernels: PROBE_BLOCKS x PROBE_ROWS x PROBE_WORDS 64-bit words
extern "C" int ramses_amd_sweep_cycle_probe(unsigned long long *out, long nwords) {
  using namespace ramses_amd::fastmode;
  const long have = (long)PROBE_BLOCKS * PROBE_ROWS * PROBE_WORDS;
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sweep_cycle_probe), sizeof(unsigned long long) * (nwords < have ? nwords : have)) != hipSuccess) return -1;
  return 0;
}
#endif

// (the units of one slope type are not warmed up: a run uses one of the twelve, which loads with its first sweep)
#include "warm.hpp"
#if defined(SWEEP_ST)
#elif RAMSES_AMD_FAST
RAMSES_AMD_TU_WARM(hydro_sweep_fast)
#else
RAMSES_AMD_TU_WARM(hydro_sweep_strict)
#endif

// sweep_dispatch_dump.cpp -- walks a fixed grid of runtime options through the public launchers of csrc/hydro_sweep.hip (both
// arithmetic modes) on a CPU, linked against hip_stub.cpp, and writes what every call launched: the record that
// tests/test_sweep_dispatch_host.py compares with tests/golden/sweep_dispatch.json.gz.  The grid reaches one value beyond every
// accepted range, so the rejections are on record too.  Pointers are never dereferenced on the host: dummies.
//   A <mode> <family> <params> TAB <rc> <nbox> <nblocks> <8 ints per box> { TAB <kernel>|<grid> <bx> <by> <lds> <attr> }   accepted call
//   X ...                                                 a call that failed otherwise than hipErrorInvalidValue without a launch
//   V <mode> <function> <params> <value>                  tile_sweep_rows*
//   R <mode> <family> <rejected> <calls>                  end of a family
#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

#include "csrc/sweep_args.hpp"

struct StubLaunch { const std::string *name; unsigned grid, bx, by; size_t lds; int attr; };
extern std::vector<StubLaunch> stub_launches;
extern int stub_attr;

using namespace ramses_amd;

static double dummy_d[1];
static unsigned char dummy_b[1];
static int dummy_i[4];

// layouts of a SweepArgs: 0-2 a brick that splits into shell and interior (ALL, SHELL, INTERIOR), 3-5 one that does not, 6 a bad
// region, 7 pitches beyond the 32-bit offsets, 8 a level in tiles, 9-13 the same with one precondition missing (dir, work, nwork,
// ng, stat)
enum { NLAY = 14 };
static SweepArgs layout(int lay) {
  static const int region[3] = {SWEEP_ALL, SWEEP_SHELL, SWEEP_INTERIOR};
  SweepArgs A{};
  A.uold = dummy_d; A.unew = dummy_d;
  const bool tiles = lay >= 8, split = lay <= 2 || lay == 6 || lay == 7;
  A.nx = tiles ? 128 : split ? 180 : 64; A.ny = tiles ? 16 : split ? 24 : 32; A.nz = tiles ? 16 : split ? 40 : 16;
  A.ng = lay == 12 ? 2 : 0;
  A.pitch_y = A.nx; A.pitch_z = A.pitch_y * A.ny; A.pitch_var = A.pitch_z * A.nz;
  if (lay == 7) { A.pitch_z = 1L << 28; A.pitch_var = 1L << 29; }
  A.zchunk = 16;
  A.region = lay < 6 ? region[lay % 3] : lay == 6 ? 3 : SWEEP_ALL;
  A.nbox = -1; A.nblocks = -1;
  if (tiles) {
    A.stat = lay == 13 ? nullptr : dummy_b; A.dir = lay == 9 ? nullptr : dummy_i; A.work = lay == 10 ? nullptr : dummy_i;
    A.nwork = lay == 11 ? 0 : 7; A.ntx = A.nty = A.ntz = 2;
  }
  A.dt = 0.1; A.dx = 0.5; A.rdx = 2.0; A.pow2 = 1;
  return A;
}
static SurfArgs surf(int nevent) {
  SurfArgs A{};
  A.uold = dummy_d; A.stat = dummy_b; A.dir = A.tileid = A.events = A.ig = dummy_i; A.rec = dummy_d;
  A.nevent = nevent; A.ntx = A.nty = A.ntz = 2;
  return A;
}

static const char *g_mode, *g_family;
static long g_calls, g_rejected;
static void begin(const char *mode, const char *family) { g_mode = mode; g_family = family; g_calls = g_rejected = 0; }
static void end() { std::printf("R %s %s %ld %ld\n", g_mode, g_family, g_rejected, g_calls); }
static void reset() { stub_launches.clear(); stub_attr = -1; }
static void emit(std::initializer_list<int> params, hipError_t e, const SweepArgs *A) {
  g_calls++;
  if (e == hipErrorInvalidValue && stub_launches.empty()) { g_rejected++; return; }
  std::printf("%c %s %s", e == hipSuccess ? 'A' : 'X', g_mode, g_family);
  for (int p : params) std::printf(" %d", p);
  const int nbox = A ? A->nbox : 0;
  std::printf("\t%d %d %d", (int)e, nbox, A ? A->nblocks : 0);
  for (int i = 0; i < nbox && i < 6; i++) {
    const SweepBox &B = A->box[i];
    std::printf(" %d %d %d %d %d %d %d %d", B.tx0, B.ntx, B.ty0, B.nty, B.zlo, B.zhi, B.zchunk, B.first);
  }
  for (const StubLaunch &L : stub_launches) {
    char *d = abi::__cxa_demangle(L.name->c_str(), nullptr, nullptr, nullptr);
    std::printf("\t%s|%u %u %u %zu %d", d ? d : L.name->c_str(), L.grid, L.bx, L.by, L.lds, L.attr);
    std::free(d);
  }
  std::printf("\n");
}

// the families both arithmetic modes have (the declarations of the two namespaces are the same)
static void common(const char *mode, decltype(&strictmode::launch_godunov_sweep) sweep, decltype(&strictmode::launch_godunov_sweep_nener) nener,
                   decltype(&strictmode::launch_godunov_sweep_scalars) scalars, decltype(&strictmode::launch_surface_flux) surface,
                   decltype(&strictmode::tile_sweep_rows) rows) {
  begin(mode, "godunov_sweep");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int scheme = 0; scheme <= 2; scheme++)
    for (int grav = 0; grav <= 1; grav++) for (int by : {0, 8, 10, 12}) for (int lay = 0; lay < NLAY; lay++) {
      SweepArgs A = layout(lay);
      reset();
      emit({st, rs, nvar, scheme, grav, by, lay}, sweep(A, st, rs, by, scheme, nvar, grav != 0, nullptr), &A);
    }
  end();
  begin(mode, "godunov_sweep_nener");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int ne = 0; ne <= 3; ne++)
    for (int lay = 0; lay < NLAY; lay++) {
      SweepArgs A = layout(lay);
      reset();
      emit({st, rs, nvar, ne, lay}, nener(A, st, rs, nvar, ne, nullptr), &A);
    }
  end();
  begin(mode, "godunov_sweep_scalars");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar : {7, 8, 9, 16, 17}) for (int ne = 0; ne <= 3; ne++)
    for (int grav = 0; grav <= 1; grav++) for (int by : {0, 8, 10, 12}) for (int lay = 0; lay < NLAY; lay++) {
      SweepArgs A = layout(lay);
      reset();
      emit({st, rs, nvar, ne, grav, by, lay}, scalars(A, st, rs, by, nvar, ne, grav != 0, nullptr), &A);
    }
  end();
  begin(mode, "surface_flux");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int scheme = 0; scheme <= 2; scheme++)
    for (int grav = 0; grav <= 1; grav++) for (int nevent : {0, 5, 1000}) {
      const SurfArgs A = surf(nevent);
      reset();
      emit({st, rs, nvar, scheme, grav, nevent}, surface(A, st, rs, nvar, scheme, grav != 0, nullptr), nullptr);
    }
  end();
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int scheme = 0; scheme <= 2; scheme++)
    std::printf("V %s tile_sweep_rows %d %d %d %d %d\n", mode, st, rs, nvar, scheme, rows(rs, nvar, st, scheme));
}

int main() {
  common("strict", strictmode::launch_godunov_sweep, strictmode::launch_godunov_sweep_nener, strictmode::launch_godunov_sweep_scalars,
         strictmode::launch_surface_flux, strictmode::tile_sweep_rows);
  common("fast", fastmode::launch_godunov_sweep, fastmode::launch_godunov_sweep_nener, fastmode::launch_godunov_sweep_scalars,
         fastmode::launch_surface_flux, fastmode::tile_sweep_rows);
  // pressure_fix and difmag: strict arithmetic only; x / d: one more precondition missing (divu, enew; difmag = 0)
  begin("strict", "godunov_sweep_pfix");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int grav = 0; grav <= 1; grav++)
    for (int x = 0; x <= 2; x++) for (int lay = 0; lay < NLAY; lay++) {
      SweepArgs A = layout(lay);
      SweepPfix X;
      X.divu = x == 1 ? nullptr : dummy_d; X.enew = x == 2 ? nullptr : dummy_d;
      reset();
      emit({st, rs, nvar, grav, x, lay}, strictmode::launch_godunov_sweep_pfix(A, X, st, rs, nvar, grav != 0, nullptr), &A);
    }
  end();
  begin("strict", "godunov_sweep_difmag");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int grav = 0; grav <= 1; grav++)
    for (int d = 0; d <= 1; d++) for (int lay = 0; lay < NLAY; lay++) {
      SweepArgs A = layout(lay);
      SweepDifmag D;
      D.difmag = d ? 0.0 : 0.1;
      reset();
      emit({st, rs, nvar, grav, d, lay}, strictmode::launch_godunov_sweep_difmag(A, D, st, rs, nvar, grav != 0, nullptr), &A);
    }
  end();
  begin("strict", "surface_flux_pfix");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int grav = 0; grav <= 1; grav++)
    for (int nevent : {0, 5, 1000}) {
      const SurfArgs A = surf(nevent);
      reset();
      emit({st, rs, nvar, grav, nevent}, strictmode::launch_surface_flux_pfix(A, st, rs, nvar, grav != 0, nullptr), nullptr);
    }
  end();
  begin("strict", "surface_flux_difmag");
  for (int st = 0; st <= 9; st++) for (int rs = -1; rs <= 5; rs++) for (int nvar = 4; nvar <= 8; nvar++) for (int grav = 0; grav <= 1; grav++)
    for (int nevent : {0, 5, 1000}) {
      const SurfArgs A = surf(nevent);
      SweepDifmag D;
      D.difmag = 0.1;
      reset();
      emit({st, rs, nvar, grav, nevent}, strictmode::launch_surface_flux_difmag(A, D, st, rs, nvar, grav != 0, nullptr), nullptr);
    }
  end();
  for (int st = 0; st <= 9; st++) for (int nvar = 4; nvar <= 8; nvar++) {
    std::printf("V strict tile_sweep_rows_pfix %d %d %d\n", st, nvar, strictmode::tile_sweep_rows_pfix(nvar, st));
    std::printf("V strict tile_sweep_rows_difmag %d %d %d\n", st, nvar, strictmode::tile_sweep_rows_difmag(nvar, st));
  }
  return 0;
}

// eos_host_check.cpp -- the host side of csrc/eos_core.hpp under a plain host compiler with -fsanitize=address,undefined
// (tests/test_eos_checker.py).  Reads one record of the reference program as the test wrote it:
//   int64 n; double T2c, scale_nH, scale_T2, smallr, gamma; double rho[n], mx[n], my[n], mz[n], e_in[n], e_out[n]; int32 son[n]
// and checks, bit for bit, that eos_energy gives e_out in every leaf cell (son == 0) and that e_out == e_in in every split cell.
// No GPU is opened and nothing of the HIP runtime is linked.  Prints "ok <leaf cells> <split cells>" and returns 0 when every cell
// holds; the first that does not is named on stderr.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "csrc/eos_core.hpp"

namespace {
template <class T>
bool read(FILE *f, std::vector<T> &v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof(b));
  return b;
}
}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s RECORD\n", argv[0]); return 2; }
  FILE *f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int64_t n = 0;
  double par[5];
  std::vector<double> rho, mx, my, mz, ein, eout;
  std::vector<int32_t> son;
  bool ok = fread(&n, sizeof(n), 1, f) == 1 && n >= 0 && n < (1 << 28) && fread(par, sizeof(double), 5, f) == 5;
  ok = ok && read(f, rho, n) && read(f, mx, n) && read(f, my, n) && read(f, mz, n) && read(f, ein, n) && read(f, eout, n) && read(f, son, n);
  ok = ok && fgetc(f) == EOF;
  fclose(f);
  if (!ok) { fprintf(stderr, "%s: not a record of %lld cells\n", argv[1], (long long)n); return 2; }
  const ramses_amd::EosConst C{par[0], par[1], par[2]};
  long leaf = 0, split = 0;
  for (int64_t i = 0; i < n; i++) {
    if (son[i] == 0) {
      leaf++;
      const double e = ramses_amd::eos_energy(C, rho[i], mx[i], my[i], mz[i], par[3], par[4]);
      if (bits(e) != bits(eout[i])) { fprintf(stderr, "leaf cell %lld: %.17g, the reference has %.17g\n", (long long)i, e, eout[i]); return 1; }
    } else {
      split++;
      if (bits(ein[i]) != bits(eout[i])) { fprintf(stderr, "split cell %lld changed in the record\n", (long long)i); return 1; }
    }
  }
  printf("ok %ld %ld\n", leaf, split);
  return 0;
}

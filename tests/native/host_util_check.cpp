// host_util_check.cpp -- csrc/host_util.hpp under a plain host compiler with -fsanitize=address,undefined
// (tests/test_host_util_host.py): the growable buffers over counting stand-ins for the allocators of the HIP runtime, the
// error path into a stand-in for ramses_amd_set_error, the three regimes of grid_for.  No GPU is opened and nothing of the
// HIP runtime is linked.  Prints "ok" and returns 0 when every check holds; the first that does not is named on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "csrc/host_util.hpp"

namespace {

struct Heap {      // one allocator pair of the runtime
  int allocs = 0, frees = 0;
  bool fail_next = false;
  size_t last_bytes = 0;
  std::set<void *> live;
  hipError_t alloc(void **p, size_t bytes) {
    if (fail_next) { fail_next = false; return hipErrorOutOfMemory; }
    allocs++;
    last_bytes = bytes;
    *p = malloc(bytes);      // (the sanitizer watches every byte of it)
    live.insert(*p);
    return hipSuccess;
  }
  hipError_t free(void *p) {
    if (!live.erase(p)) return hipErrorInvalidValue;
    frees++;
    ::free(p);
    return hipSuccess;
  }
};
Heap g_dev, g_pin;
unsigned g_pin_flags = ~0u;
int g_code = 0, g_errors = 0;
std::string g_msg;

int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return g_dev.alloc(p, bytes); }
hipError_t hipFree(void *p) { return g_dev.free(p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int flags) { g_pin_flags = flags; return g_pin.alloc(p, bytes); }
hipError_t hipHostFree(void *p) { return g_pin.free(p); }
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "some error"; }
int ramses_amd_set_error(int code, const char *msg) {
  g_errors++;
  g_code = code;
  g_msg = msg;
  return code;
}
}

using namespace ramses_amd;

template <class B>
static void check_buffer(Heap &H) {
  {
    B b;
    CHECK(b.p == nullptr && b.cap == 0);
    // a first ensure(0): a pointer and one allocation of at least 8 bytes
    CHECK(b.ensure(0) == hipSuccess);
    CHECK(b.p != nullptr && b.cap >= 8 && H.last_bytes >= 8);
    CHECK(H.allocs == 1 && H.frees == 0);
    memset(b.p, 0x5a, 8);
    void *first = b.p;
    CHECK(b.ensure(0) == hipSuccess && b.ensure(8) == hipSuccess && b.p == first && H.allocs == 1 && H.frees == 0);
    // growing: one free, one allocation
    CHECK(b.ensure(1000) == hipSuccess);
    CHECK(b.p != nullptr && b.cap == 1000 && H.last_bytes == 1000);
    CHECK(H.allocs == 2 && H.frees == 1);
    memset(b.p, 0x5a, 1000);
    // smaller or equal: the same pointer and no call
    void *kept = b.p;
    CHECK(b.ensure(1000) == hipSuccess && b.ensure(999) == hipSuccess && b.ensure(1) == hipSuccess && b.ensure(0) == hipSuccess);
    CHECK(b.p == kept && b.cap == 1000 && H.allocs == 2 && H.frees == 1);
    CHECK(b.template as<double>() == reinterpret_cast<double *>(kept));
    const B &cb = b;
    CHECK(cb.template as<const int>() == reinterpret_cast<const int *>(kept));
    // the allocation fails: the old block is gone, the buffer is empty and says so
    H.fail_next = true;
    CHECK(b.ensure(2000) == hipErrorOutOfMemory);
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(H.allocs == 2 && H.frees == 2 && H.live.empty());
    // ... and recovers with the next request, however small
    CHECK(b.ensure(16) == hipSuccess && b.p != nullptr && b.cap == 16 && H.allocs == 3 && H.frees == 2);
    // release: one free, then nothing
    b.release();
    CHECK(b.p == nullptr && b.cap == 0 && H.allocs == 3 && H.frees == 3);
    b.release();
    CHECK(b.p == nullptr && b.cap == 0 && H.allocs == 3 && H.frees == 3);
    // a failure on an empty buffer
    H.fail_next = true;
    CHECK(b.ensure(0) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && H.allocs == 3 && H.frees == 3);
  }
  CHECK(H.live.empty() && H.allocs == H.frees);
}

static int leaves_through_hchk(hipError_t e, int *after) {
  HCHK(e, "the call");
  *after = 1;
  return 0;
}

int main() {
  check_buffer<DevBuf>(g_dev);
  CHECK(g_pin.allocs == 0 && g_pin.frees == 0);     // the device buffer never touched the pinned pair ...
  check_buffer<PinBuf>(g_pin);
  CHECK(g_dev.allocs == 3 && g_dev.frees == 3);     // ... nor the pinned buffer the device's
  CHECK(g_pin_flags == hipHostMallocDefault);

  // the error path
  CHECK(fail(RAMSES_AMD_EINVAL, "%s %d", "x", 3) == RAMSES_AMD_EINVAL);
  CHECK(g_errors == 1 && g_code == RAMSES_AMD_EINVAL && g_msg == "x 3");
  const std::string longmsg(2000, 'm');
  CHECK(fail(RAMSES_AMD_EUNSUPPORTED, "%s", longmsg.c_str()) == RAMSES_AMD_EUNSUPPORTED);
  CHECK(g_errors == 2 && g_code == RAMSES_AMD_EUNSUPPORTED && g_msg == std::string(511, 'm'));
  CHECK(hipfail(hipErrorOutOfMemory, "hipMalloc brick") == RAMSES_AMD_EHIP);
  CHECK(g_errors == 3 && g_code == RAMSES_AMD_EHIP && g_msg == "hipMalloc brick: out of memory");
  int after = 0;
  CHECK(leaves_through_hchk(hipErrorOutOfMemory, &after) == RAMSES_AMD_EHIP && after == 0);
  CHECK(g_errors == 4 && g_msg == "the call: out of memory");
  CHECK(leaves_through_hchk(hipSuccess, &after) == 0 && after == 1 && g_errors == 4);

  // grid_for: nothing to do, beyond the cap, an exact multiple (and one more)
  CHECK(grid_for(0) == 1 && grid_for(-5) == 1 && grid_for(1) == 1);
  CHECK(grid_for(4096L * 256 + 1) == 4096 && grid_for(4096L * 256) == 4096 && grid_for(4096L * 256 - 256) == 4095);
  CHECK(grid_for(10 * 256) == 10 && grid_for(10 * 256 + 1) == 11);
  CHECK(grid_for(8192L * 256 + 1, 8192) == 8192 && grid_for(8191L * 256 + 1, 8192) == 8192 && grid_for(8191L * 256, 8192) == 8191);
  CHECK(grid_for(65536L * 128 + 1, 65536, 128) == 65536 && grid_for(3 * 128, 65536, 128) == 3 && grid_for(3 * 128 + 1, 65536, 128) == 4);
  CHECK(grid_for(1L << 40) == 4096);

  CHECK(g_dev.live.empty() && g_pin.live.empty());
  if (g_failed) return 1;
  puts("ok");
  return 0;
}

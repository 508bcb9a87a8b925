// host_util.hpp -- the host-side helpers every unit of the C ABI shares: the error path behind ramses_amd_last_error(), the
// growable device and page-locked buffers, the block count of a one-dimensional launch.  Host code only: it includes no
// kernel header and a plain host compiler takes it (tests/native/host_util_check.cpp).  A new unit includes this header
// instead of defining its own copies.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>

#include "../../include/ramses_amd.h"

extern "C" int ramses_amd_set_error(int code, const char *msg);   // capi.hip: the thread's last error text

namespace ramses_amd {

static inline int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return ramses_amd_set_error(code, buf);
}
static inline int hipfail(hipError_t e, const char *what) {
  return fail(RAMSES_AMD_EHIP, "%s: %s", what, hipGetErrorString(e));
}
// leaves the enclosing function with the HIP error of `call` as the thread's last error
#define HCHK(call, what) do { hipError_t e_ = (call); if (e_ != hipSuccess) return ::ramses_amd::hipfail(e_, what); } while (0)

// A buffer that only grows: ensure() keeps pointer and contents while the request fits, else frees and allocates anew (the
// contents are lost), never fewer than 8 bytes, so that a buffer that was ensured is never null.
struct DevMem {
  static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void *p) { return hipFree(p); }
};
struct PinMem {     // page-locked host memory
  static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t free(void *p) { return hipHostFree(p); }
};
template <class Mem> struct GrowBuf {
  void *p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    release();
    if (bytes < 8) bytes = 8;
    hipError_t e = Mem::alloc(&p, bytes);
    if (e == hipSuccess) cap = bytes;
    else p = nullptr;
    return e;
  }
  void release() {
    if (p) (void)Mem::free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
using DevBuf = GrowBuf<DevMem>;
using PinBuf = GrowBuf<PinMem>;

// blocks of a one-dimensional launch over `work` items: enough to cover them once, at least 1, at most `cap` (the kernels
// behind it stride over the rest)
static inline int grid_for(long work, int cap = 4096, int block = 256) {
  const long g = (work + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace ramses_amd

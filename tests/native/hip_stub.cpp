// hip_stub.cpp -- a stand-in for the nine HIP runtime symbols the sweep objects need, which RECORDS the launches instead of
// making them: linked with the hydro_sweep_*.o objects and sweep_dispatch_dump.cpp only (tests/test_sweep_dispatch_host.py),
// never into anything that opens a GPU.
#include <cstddef>
#include <map>
#include <string>
#include <vector>

struct Dim3 { unsigned x, y, z; };
struct StubLaunch { const std::string *name; unsigned grid, bx, by; size_t lds; int attr; };
std::vector<StubLaunch> stub_launches;     // (read and cleared by the dump program)
int stub_attr = -1;                        // the last hipFuncSetAttribute value
static std::map<const void *, std::string> &names() { static std::map<const void *, std::string> m; return m; }
static Dim3 g_grid, g_block; static size_t g_shm; static void *g_stream;

extern "C" {
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host, char *, const char *dev, unsigned, void *, void *, void *, void *, int *) { names()[host] = dev; }
int __hipPushCallConfiguration(Dim3 grid, Dim3 block, size_t shm, void *stream) { g_grid = grid; g_block = block; g_shm = shm; g_stream = stream; return 0; }
int __hipPopCallConfiguration(Dim3 *grid, Dim3 *block, size_t *shm, void **stream) { *grid = g_grid; *block = g_block; *shm = g_shm; *stream = g_stream; return 0; }
int hipFuncSetAttribute(const void *, int, int v) { stub_attr = v; return 0; }
int hipGetLastError() { return 0; }
int hipLaunchKernel(const void *host, Dim3 grid, Dim3 block, void **, size_t shm, void *) {
  stub_launches.push_back(StubLaunch{&names()[host], grid.x, block.x, block.y, shm, stub_attr});
  return 0;
}
}

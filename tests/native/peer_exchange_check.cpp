// peer_exchange_check.cpp -- csrc/peer_exchange.hpp under a plain host compiler with -fsanitize=address,undefined
// (tests/test_peer_exchange_host.py): the halo protocol of the AMR, multigrid and CG units over stand-ins for the allocators, the
// copies and the stream of the HIP runtime and for ramses_amd_rccl_exchange, which copies message i of the send buffer to message
// i of the receive buffer and records its arguments.  No GPU is opened and nothing of the HIP runtime is linked.  Prints "ok" and
// returns 0 when every check holds; the first that does not is named on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "csrc/peer_exchange.hpp"

namespace {

struct Heap {      // one allocator pair of the runtime
  int allocs = 0, frees = 0;
  size_t last_bytes = 0;
  std::set<void *> live;
  hipError_t alloc(void **p, size_t bytes) {
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
int g_syncs = 0, g_errors = 0;
std::string g_msg;

struct RcclCall {
  int calls = 0;
  std::vector<int> peer;
  std::vector<int64_t> so, sc, ro, rcn;
  const double *send = nullptr;
  double *recv = nullptr;
  void *stream = &g_dev;
} g_rccl;

int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); g_failed++; } } while (0)

}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) { return g_dev.alloc(p, bytes); }
hipError_t hipFree(void *p) { return g_dev.free(p); }
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { return g_pin.alloc(p, bytes); }
hipError_t hipHostFree(void *p) { return g_pin.free(p); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipMemcpy(void *dst, const void *src, size_t bytes, hipMemcpyKind) { memcpy(dst, src, bytes); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { g_syncs++; return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "some error"; }
int ramses_amd_set_error(int code, const char *msg) {
  g_errors++;
  g_msg = msg;
  return code;
}
int ramses_amd_rccl_exchange(int npeer, const int *peer, const double *d_send, const int64_t *send_off, const int64_t *send_cnt, double *d_recv,
                             const int64_t *recv_off, const int64_t *recv_cnt, void *stream) {
  RcclCall &R = g_rccl;
  R.calls++;
  R.peer.assign(peer, peer + npeer);
  R.so.assign(send_off, send_off + npeer); R.sc.assign(send_cnt, send_cnt + npeer);
  R.ro.assign(recv_off, recv_off + npeer); R.rcn.assign(recv_cnt, recv_cnt + npeer);
  R.send = d_send; R.recv = d_recv; R.stream = stream;
  for (int k = 0; k < npeer; k++) {
    const int64_t n = send_cnt[k] < recv_cnt[k] ? send_cnt[k] : recv_cnt[k];
    if (n > 0) memcpy(d_recv + recv_off[k], d_send + send_off[k], sizeof(double) * (size_t)n);
  }
  return 0;
}
}

using namespace ramses_amd;
typedef std::vector<int> ivec;

// one exchange over both transports: em / rc = octs per peer in each direction, per = doubles per oct
static void check_exchange(PeerExchange &X, const ivec &sn, const ivec &rn, size_t per) {
  const int ncpu = (int)sn.size();
  ivec sf(ncpu + 1, 0), rf(ncpu + 1, 0);
  for (int c = 0; c < ncpu; c++) { sf[c + 1] = sf[c] + sn[c]; rf[c + 1] = rf[c] + rn[c]; }
  CHECK(X.plan(ncpu, sf.data(), rf.data(), per) == 0);
  CHECK(X.send_off.size() == (size_t)ncpu + 1 && X.recv_off.size() == (size_t)ncpu + 1);
  for (int c = 0; c <= ncpu; c++) CHECK(X.send_off[c] == (int64_t)per * sf[c] && X.recv_off[c] == (int64_t)per * rf[c]);
  const size_t ns = per * sf[ncpu], nr = per * rf[ncpu];
  CHECK(X.sendbuf.p && X.recvbuf.p && X.sendbuf.cap >= 8 * (ns > 0 ? ns : 1) && X.recvbuf.cap >= 8 * (nr > 0 ? nr : 1));   // both sides empty: still buffers
  CHECK(X.tag[0] == 0 && X.tag[2] == -1);
  double *s = X.sendbuf.as<double>(), *r = X.recvbuf.as<double>();
  for (size_t i = 0; i < ns; i++) s[i] = 0.5 * (double)(i + 1);
  for (size_t i = 0; i < nr; i++) r[i] = -1.0;

  // host transport
  int64_t hs = 0, hr = 0;
  std::vector<int64_t> so(ncpu + 1, -7), ro(ncpu + 1, -7);
  const int syncs = g_syncs, errors = g_errors;
  CHECK(X.stage_out(3, 2, 1, ncpu, &hs, &hr, so.data(), ro.data()) == 0);
  CHECK(g_syncs == syncs + 1);
  CHECK(hs != 0 && hr != 0 && hs == (int64_t)(intptr_t)X.h_send.p && hr == (int64_t)(intptr_t)X.h_recv.p);
  CHECK(so == X.send_off && ro == X.recv_off);
  CHECK(X.h_send.cap >= 8 * (ns > 0 ? ns : 1) && X.h_recv.cap >= 8 * (nr > 0 ? nr : 1));
  CHECK(ns == 0 || memcmp(X.h_send.p, s, 8 * ns) == 0);
  CHECK(X.tag[0] == 3 && X.tag[1] == 2 && X.tag[2] == 1);
  double *h = X.h_recv.as<double>();
  for (size_t i = 0; i < nr; i++) h[i] = 3.0 + (double)i;
  // a stage_in that does not close this exchange: refused with the caller's text, the exchange stays open
  CHECK(X.stage_in(3, 1, 1, ncpu, "wrong %s (%d)", "component", X.tag[1]) == RAMSES_AMD_EINVAL && g_msg == "wrong component (2)");
  CHECK(X.stage_in(3, 2, 0, ncpu, "%s", "wrong dir") == RAMSES_AMD_EINVAL && g_msg == "wrong dir");
  CHECK(X.stage_in(2, 2, 1, ncpu, "%s", "wrong level") == RAMSES_AMD_EINVAL && X.stage_in(3, 2, 1, ncpu + 1, "%s", "wrong ncpu") == RAMSES_AMD_EINVAL);
  CHECK(g_errors == errors + 4 && X.tag[0] == 3 && X.tag[1] == 2 && X.tag[2] == 1);
  for (size_t i = 0; i < nr; i++) CHECK(r[i] == -1.0);
  CHECK(X.stage_in(3, 2, 1, ncpu, "%s", "refused") == 0 && g_errors == errors + 4);
  CHECK(nr == 0 || memcmp(r, h, 8 * nr) == 0);
  CHECK(X.tag[0] == 0 && X.tag[2] == -1);
  CHECK(X.stage_in(3, 2, 1, ncpu, "%s", "closed already") == RAMSES_AMD_EINVAL && g_msg == "closed already");
  CHECK(g_syncs == syncs + 1);

  // RCCL transport: the peers with a message either way, in icpu order, on the null stream
  for (size_t i = 0; i < nr; i++) r[i] = -1.0;
  const int calls = g_rccl.calls;
  CHECK(X.rccl() == 0 && g_rccl.calls == calls + 1);
  ivec peers;
  for (int c = 0; c < ncpu; c++) if (sn[c] > 0 || rn[c] > 0) peers.push_back(c);
  CHECK(g_rccl.peer == peers && g_rccl.send == s && g_rccl.recv == r && g_rccl.stream == nullptr);
  for (size_t k = 0; k < peers.size() && k < g_rccl.so.size(); k++) {
    const int c = peers[k];
    CHECK(g_rccl.so[k] == (int64_t)per * sf[c] && g_rccl.sc[k] == (int64_t)per * sn[c]);
    CHECK(g_rccl.ro[k] == (int64_t)per * rf[c] && g_rccl.rcn[k] == (int64_t)per * rn[c]);
    const size_t n = per * (size_t)(sn[c] < rn[c] ? sn[c] : rn[c]);
    CHECK(n == 0 || memcmp(r + per * rf[c], s + per * sf[c], 8 * n) == 0);
  }
  CHECK(X.tag[0] == 0 && X.tag[2] == -1);
}

int main() {
  {
    PeerExchange X;
    CHECK(X.tag[0] == 0 && X.tag[2] == -1 && !X.sendbuf.p && !X.h_send.p);
    check_exchange(X, {4}, {4}, 8);                        // one rank, its own peer
    check_exchange(X, {3, 0, 2}, {2, 0, 0}, 8 * 5);        // the middle peer has nothing either way, the last one only sends
    check_exchange(X, {0, 0, 6}, {5, 0, 1}, 8 * 4);
    check_exchange(X, {0, 0, 0}, {0, 0, 0}, 8);            // both sides empty
    check_exchange(X, {1, 1, 1}, {0, 0, 0}, 8);            // nothing to receive at all
    X.release();
    CHECK(!X.sendbuf.p && !X.recvbuf.p && !X.h_send.p && !X.h_recv.p);
    CHECK(g_dev.live.empty() && g_pin.live.empty());
  }
  {
    // what stage_out refuses; (new with the shared protocol) a plan for other ranks between stage_out and stage_in closes the
    // exchange, and tables of another size never pass for those of `ncpu` ranks
    PeerExchange X;
    int64_t hs, hr, so[4], ro[4];
    const int one[2] = {0, 2}, three[4] = {0, 2, 2, 5};
    CHECK(X.stage_out(1, 0, 0, 1, &hs, &hr, so, ro) == RAMSES_AMD_EINVAL && g_msg == "ncpu mismatch");      // nothing planned yet
    CHECK(X.stage_out(1, 0, 0, -1, &hs, &hr, so, ro) == RAMSES_AMD_EINVAL && g_msg == "ncpu mismatch");
    CHECK(X.plan(1, one, one, 8) == 0);
    CHECK(X.stage_out(1, 0, 0, 1, nullptr, &hr, so, ro) == RAMSES_AMD_EINVAL && g_msg == "NULL argument");
    CHECK(X.stage_out(1, 0, 0, 1, &hs, &hr, so, nullptr) == RAMSES_AMD_EINVAL && g_msg == "NULL argument");
    CHECK(X.stage_out(1, 0, 0, 3, &hs, &hr, so, ro) == RAMSES_AMD_EINVAL && g_msg == "ncpu mismatch");
    CHECK(X.tag[0] == 0 && !X.h_send.p);
    CHECK(X.stage_out(1, 0, 0, 1, &hs, &hr, so, ro) == 0 && X.tag[0] == 1);
    CHECK(X.plan(3, three, three, 8) == 0);
    CHECK(X.tag[0] == 0 && X.stage_in(1, 0, 0, 3, "%s", "no exchange is open") == RAMSES_AMD_EINVAL && g_msg == "no exchange is open");
    X.tag[0] = 1; X.tag[1] = 0; X.tag[2] = 0;      // (as the three copies behaved before: the tag survives the new tables)
    CHECK(X.stage_in(1, 0, 0, 1, "%s", "tables of 3 ranks") == RAMSES_AMD_EINVAL && g_msg == "tables of 3 ranks" && X.tag[0] == 1);
    X.release();
  }
  {
    // the pinned twins: a request that fits allocates nothing, one that does not gets half as much again
    PeerExchange X;
    int64_t hs, hr, so[2], ro[2];
    auto out = [&](int nsend, int nrecv) {
      const int sf[2] = {0, nsend}, rf[2] = {0, nrecv};
      CHECK(X.plan(1, sf, rf, 8) == 0 && X.stage_out(1, 0, 0, 1, &hs, &hr, so, ro) == 0);
    };
    const int a0 = g_pin.allocs, f0 = g_pin.frees;
    out(100, 10);
    CHECK(g_pin.allocs == a0 + 2 && g_pin.frees == f0 && X.h_send.cap == 9600 && X.h_recv.cap == 960);
    const void *ps = X.h_send.p, *pr = X.h_recv.p;
    out(40, 1); out(0, 0); out(150, 15); out(100, 10);
    CHECK(g_pin.allocs == a0 + 2 && g_pin.frees == f0 && X.h_send.p == ps && X.h_recv.p == pr);
    out(151, 15);                                          // one double more than the headroom holds
    CHECK(g_pin.allocs == a0 + 3 && g_pin.frees == f0 + 1 && X.h_send.cap == 151 * 64 * 3 / 2 && X.h_recv.p == pr);
    out(150, 16);
    CHECK(g_pin.allocs == a0 + 4 && g_pin.frees == f0 + 2 && X.h_recv.cap == 16 * 64 * 3 / 2);
    X.release();
    CHECK(g_pin.allocs == g_pin.frees && g_dev.allocs == g_dev.frees);
  }
  {
    // the communicator lists: prefix tables, the lists on the "device" as they came, what is refused
    DevBuf d_em, d_rc;
    ivec ef, rf;
    const int em_n[3] = {2, 0, 3}, rc_n[3] = {1, 0, 0}, em[5] = {11, 12, 13, 14, 15}, rc[1] = {21};
    CHECK(peer_lists("x_comm_set", 3, em_n, em, rc_n, rc, ef, rf, d_em, d_rc) == 0);
    CHECK(ef == ivec({0, 2, 2, 5}) && rf == ivec({0, 1, 1, 1}));
    CHECK(memcmp(d_em.p, em, sizeof(em)) == 0 && memcmp(d_rc.p, rc, sizeof(rc)) == 0);
    const int none[3] = {0, 0, 0}, neg[3] = {1, -1, 0};
    CHECK(peer_lists("x_comm_set", 3, none, nullptr, none, nullptr, ef, rf, d_em, d_rc) == 0 && d_em.p && d_rc.p && ef == ivec(4, 0));
    CHECK(peer_lists("x_comm_set", 3, em_n, nullptr, rc_n, rc, ef, rf, d_em, d_rc) == RAMSES_AMD_EINVAL && g_msg == "x_comm_set: NULL list");
    CHECK(peer_lists("x_comm_set", 3, em_n, em, neg, rc, ef, rf, d_em, d_rc) == RAMSES_AMD_EINVAL && g_msg == "x_comm_set: negative list length");
    CHECK(peer_prefix("y", 3, neg, rc_n, ef, rf) == RAMSES_AMD_EINVAL && g_msg == "y: negative list length");
    d_em.release(); d_rc.release();
  }
  CHECK(g_dev.live.empty() && g_pin.live.empty() && g_dev.allocs == g_dev.frees && g_pin.allocs == g_pin.frees);
  if (g_failed) return 1;
  puts("ok");
  return 0;
}

// peer_exchange.hpp -- the protocol that moves a halo between MPI ranks, once, for every unit that keeps cell vectors on the
// device (capi_amr.hip: the resident AMR levels; capi_tree_poisson.hip: the levels of an AMR multigrid solve and the search
// direction of the CG loop).  One message per peer, the peers in icpu order, offsets in doubles.  The caller packs into sendbuf
// and unpacks from recvbuf with its own kernels; between the two the messages travel either over RCCL (rccl) or through
// page-locked host twins and the caller's own MPI (stage_out ... stage_in).  Host code only, like host_util.hpp
// (tests/native/peer_exchange_check.cpp compiles it with a plain host compiler).
#pragma once
#include <cstdint>
#include <vector>

#include "host_util.hpp"

// capi_mpi.hip: one grouped send/recv, message k with rank peer[k] (0-based)
extern "C" int ramses_amd_rccl_exchange(int npeer, const int *peer, const double *d_send, const int64_t *send_off, const int64_t *send_cnt,
                                        double *d_recv, const int64_t *recv_off, const int64_t *recv_cnt, void *stream);

namespace ramses_amd {

struct __attribute__((visibility("hidden"))) PeerExchange {      // (hidden: the library exports the C ABI, not this)
  DevBuf sendbuf, recvbuf;                    // the messages of all peers, one after the other
  PinBuf h_send, h_recv;                      // their host twins (host transport)
  std::vector<int64_t> send_off, recv_off;    // [ncpu+1], doubles, of the exchange that was planned last
  int tag[3] = {0, 0, -1};                    // the exchange stage_out has opened: (level, component, direction); level 0, direction -1: none

  void close() { tag[0] = 0; tag[2] = -1; }

  // offsets and device buffers of an exchange: send_first / recv_first = [ncpu+1] prefix tables in octs, per = doubles per oct.
  // Whatever exchange was open is gone with its tables.
  int plan(int ncpu, const int *send_first, const int *recv_first, size_t per) {
    close();
    send_off.assign((size_t)ncpu + 1, 0); recv_off.assign((size_t)ncpu + 1, 0);
    for (int c = 0; c <= ncpu; c++) { send_off[c] = (int64_t)(per * send_first[c]); recv_off[c] = (int64_t)(per * recv_first[c]); }
    const size_t ns = (size_t)send_off[ncpu], nr = (size_t)recv_off[ncpu];
    HCHK(sendbuf.ensure(sizeof(double) * (ns > 0 ? ns : 1)), "hipMalloc sendbuf");
    HCHK(recvbuf.ensure(sizeof(double) * (nr > 0 ? nr : 1)), "hipMalloc recvbuf");
    return 0;
  }

  // The exchange over RCCL (every rank on its own GPU), asynchronous on the null stream; peers with nothing either way drop out
  int rccl() const {
    std::vector<int> peer;
    std::vector<int64_t> so, sc, ro, rcn;
    for (int c = 0; c + 1 < (int)send_off.size(); c++) {
      const int64_t ns = send_off[c + 1] - send_off[c], nr = recv_off[c + 1] - recv_off[c];
      if (ns == 0 && nr == 0) continue;
      // a peer that is the rank itself (a communicator of the rank with itself) is legal: the grouped exchange matches the send to
      // self with the receive from self; build_comm never produces one, the single-rank execution test of the transport does
      peer.push_back(c); so.push_back(send_off[c]); sc.push_back(ns); ro.push_back(recv_off[c]); rcn.push_back(nr);
    }
    return ramses_amd_rccl_exchange((int)peer.size(), peer.data(), sendbuf.as<double>(), so.data(), sc.data(), recvbuf.as<double>(), ro.data(),
                                    rcn.data(), nullptr);
  }

  // The caller's own MPI as transport (several ranks on one GPU, or no RCCL): what was packed goes to h_send; the message for
  // peer icpu is at h_send + send_off[icpu-1], send_off[icpu] - send_off[icpu-1] doubles, likewise h_recv / recv_off.  Addresses as
  // integers for c_f_pointer.  The twins grow with 50 % headroom: a multigrid solve asks for many sizes, and every hipHostMalloc
  // synchronises the device.
  int stage_out(int t0, int t1, int t2, int ncpu, int64_t *h_send_addr, int64_t *h_recv_addr, int64_t *send_off_out, int64_t *recv_off_out) {
    if (!h_send_addr || !h_recv_addr || !send_off_out || !recv_off_out) return fail(RAMSES_AMD_EINVAL, "NULL argument");
    if (ncpu < 1 || send_off.size() != (size_t)ncpu + 1) return fail(RAMSES_AMD_EINVAL, "ncpu mismatch");
    const size_t ns = (size_t)send_off[ncpu], nr = (size_t)recv_off[ncpu];
    HCHK(grow(h_send, sizeof(double) * (ns > 0 ? ns : 1)), "hipHostMalloc"); HCHK(grow(h_recv, sizeof(double) * (nr > 0 ? nr : 1)), "hipHostMalloc");
    if (ns > 0) HCHK(hipMemcpyAsync(h_send.p, sendbuf.p, sizeof(double) * ns, hipMemcpyDeviceToHost, nullptr), "D2H halo");
    HCHK(hipStreamSynchronize(nullptr), "sync");
    *h_send_addr = (int64_t)(intptr_t)h_send.p; *h_recv_addr = (int64_t)(intptr_t)h_recv.p;
    for (int c = 0; c <= ncpu; c++) { send_off_out[c] = send_off[c]; recv_off_out[c] = recv_off[c]; }
    tag[0] = t0; tag[1] = t1; tag[2] = t2;
    return 0;
  }
  // what arrived in h_recv goes to recvbuf -- if (t0, t1, t2) is the exchange stage_out opened and its tables are those of `ncpu`
  // ranks; else the caller's message (printf style) is the error and the exchange stays open
  template <class... Args> int stage_in(int t0, int t1, int t2, int ncpu, const char *fmt, Args... args) {
    if (tag[0] != t0 || tag[1] != t1 || tag[2] != t2 || recv_off.size() != (size_t)ncpu + 1) return fail(RAMSES_AMD_EINVAL, fmt, args...);
    close();
    const size_t nr = (size_t)recv_off[ncpu];
    if (nr > 0) HCHK(hipMemcpyAsync(recvbuf.p, h_recv.p, sizeof(double) * nr, hipMemcpyHostToDevice, nullptr), "H2D halo");
    return 0;
  }

  void release() {
    sendbuf.release(); recvbuf.release(); h_send.release(); h_recv.release();
    close();
  }

 private:
  static hipError_t grow(PinBuf &b, size_t bytes) { return b.p && bytes <= b.cap ? hipSuccess : b.ensure(bytes + bytes / 2); }
};

// [ncpu+1] prefix tables of the per-peer counts em_n / rc_n [ncpu]
static inline int peer_prefix(const char *who, int ncpu, const int *em_n, const int *rc_n, std::vector<int> &em_first, std::vector<int> &rc_first) {
  em_first.assign((size_t)ncpu + 1, 0); rc_first.assign((size_t)ncpu + 1, 0);
  for (int c = 0; c < ncpu; c++) {
    if (em_n[c] < 0 || rc_n[c] < 0) return fail(RAMSES_AMD_EINVAL, "%s: negative list length", who);
    em_first[c + 1] = em_first[c] + em_n[c];
    rc_first[c + 1] = rc_first[c] + rc_n[c];
  }
  return 0;
}
// the communicators of a level as build_comm leaves them: em_n / rc_n [ncpu] octs per peer, em_ig / rc_ig the lists concatenated
// in icpu order, which go to the device as they are
static inline int peer_lists(const char *who, int ncpu, const int *em_n, const int *em_ig, const int *rc_n, const int *rc_ig,
                             std::vector<int> &em_first, std::vector<int> &rc_first, DevBuf &d_em, DevBuf &d_rc) {
  if (int rc = peer_prefix(who, ncpu, em_n, rc_n, em_first, rc_first)) return rc;
  const int nem = em_first[ncpu], nrc = rc_first[ncpu];
  if ((nem > 0 && !em_ig) || (nrc > 0 && !rc_ig)) return fail(RAMSES_AMD_EINVAL, "%s: NULL list", who);
  HCHK(d_em.ensure(sizeof(int) * (size_t)(nem > 0 ? nem : 1)), "hipMalloc"); HCHK(d_rc.ensure(sizeof(int) * (size_t)(nrc > 0 ? nrc : 1)), "hipMalloc");
  if (nem > 0) HCHK(hipMemcpy(d_em.p, em_ig, sizeof(int) * (size_t)nem, hipMemcpyHostToDevice), "H2D emission list");
  if (nrc > 0) HCHK(hipMemcpy(d_rc.p, rc_ig, sizeof(int) * (size_t)nrc, hipMemcpyHostToDevice), "H2D reception list");
  return 0;
}

}  // namespace ramses_amd

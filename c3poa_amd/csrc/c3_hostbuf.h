// c3_hostbuf.h -- growable host buffer of the reader's batch sets and of c3_host_alloc.  Header-only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

// ---- growable host buffer, page-locked when a GPU runtime is present (plain malloc otherwise: pinning is a transfer
//      optimisation, not a compute path) -------------------------------------------------------------------------
struct HostBuf {
  char* p = nullptr; size_t cap = 0; bool pinned = false;
  ~HostBuf() { release(); }
  void release() {
    if (!p) return;
    if (pinned) (void)hipHostFree(p); else free(p);
    p = nullptr; cap = 0;
  }
  bool reserve(size_t need, size_t keep) {
    if (need <= cap) return true;
    size_t ncap = cap ? cap : (size_t)1 << 20;
    while (ncap < need) ncap += ncap / 2;
    char* q = nullptr; bool pin = false;
    static int can_pin = -1;
    if (can_pin < 0) { int n = 0; can_pin = (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0; (void)hipGetLastError(); }
    if (can_pin && hipHostMalloc((void**)&q, ncap, hipHostMallocDefault) == hipSuccess) pin = true;
    else { (void)hipGetLastError(); q = (char*)malloc(ncap); }
    if (getenv("C3_DEBUG")) fprintf(stderr, "[c3_io] host buffer %zu MiB %s\n", ncap >> 20, pin ? "page-locked" : "pageable");
    if (!q) return false;
    if (keep) memcpy(q, p, keep);
    release();
    p = q; cap = ncap; pinned = pin;
    return true;
  }
};

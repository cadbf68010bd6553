// c3_gunzip.cpp -- host statement of the k_gunzip kernels (include/c3poa.h "gzip input"): find, decode with
// markers, chain, windows and resolve by plain loops on one thread, through the same procedure (c3_gunzip_run.h) and the same
// decoder (c3_gunzip.h) that c3_gunzip runs on the device.  No zlib here: the tests hold this against Python's zlib, and
// damaged input can be thrown at it under a sanitizer on the CPU.
#include "../../include/c3poa.h"
#include "c3_gunzip_run.h"

namespace {

struct HostBackend {
  const uint8_t* src; int64_t n;
  std::unique_ptr<uint16_t[]> arena; int64_t arena_n = 0, head_n = 0;
  std::vector<std::unique_ptr<uint16_t[]>> heads;           // the slabs of relaunched pieces, made when one is used
  C3InfTab T;

  int reserve(int64_t symbols, int64_t head, int n_heads) {
    arena.reset(new uint16_t[(size_t)std::max<int64_t>(symbols, 1)]);
    arena_n = symbols; head_n = head;
    heads.clear(); heads.resize((size_t)n_heads);
    return 0;
  }
  uint16_t* slab(int64_t at) {
    if (at < arena_n) return arena.get() + at;
    std::unique_ptr<uint16_t[]>& h = heads[(size_t)((at - arena_n) / head_n)];
    if (!h) h.reset(new uint16_t[(size_t)head_n]);
    return h.get();
  }
  // the 74 bits at bit q of the file (zero past its end)
  void bits_at(int64_t q, uint64_t* v0, uint64_t* v1) const {
    uint8_t b[16] = {0};
    const int64_t at = q >> 3;
    if (at < n) memcpy(b, src + at, (size_t)std::min<int64_t>(16, n - at));
    uint64_t lo, hi;
    memcpy(&lo, b, 8); memcpy(&hi, b + 8, 8);
    const int s = (int)(q & 7);
    *v0 = s ? lo >> s | hi << (64 - s) : lo;
    *v1 = hi >> s;
  }
  int find(int64_t s0, int64_t s1, int64_t piece, int64_t* cand) {
    const int64_t np = (s1 - s0 + piece - 1) / piece;
    for (int64_t k = 1; k < np; ++k) {
      const int64_t q0 = 8 * (s0 + k * piece), q1 = 8 * std::min(s1, s0 + (k + 1) * piece);
      cand[k] = -1;
      for (int64_t q = q0; q < q1; ++q) {
        uint64_t v0, v1;
        bits_at(q, &v0, &v1);
        if (!c3_gz_quick(v0, v1)) continue;
        const C3GzRel r = c3_gz_rel(q, 0, n);
        c3gz::HostIO io{src, n, r.base, nullptr};
        if (c3_gz_header_at(io, &T, r.sbit, r.total)) { cand[k] = q; break; }
      }
    }
    return 0;
  }
  int decode(const C3GzJob* jobs, int nj, C3GzRes* res) {
    for (int j = 0; j < nj; ++j) c3gz::host_decode(src, n, jobs[j], slab(jobs[j].slab), &T, &res[j]);
    return 0;
  }
  int begin_output(int64_t) { return 0; }
  int put(const char*, int64_t, int64_t) { return 0; }
  int finish(const C3GzSeg* segs, int ns, const uint8_t* win0, char* dst, int64_t, int64_t, uint32_t* crc, int* bad) {
    c3gz::host_finish(segs, ns, [&](const C3GzSeg& g) { return (const uint16_t*)slab(g.slab); }, win0, dst, crc, bad);
    return 0;
  }
};

thread_local int64_t g_stats[C3_GZS_N];

}  // namespace

int64_t* c3_gunzip_stats_slot() { return g_stats; }

extern "C" int c3_gunzip_stats(int64_t* v, int n) {
  if (!v || n < 0) { c3_set_host_error("c3_gunzip_stats: bad arguments"); return C3_E_ARG; }
  for (int i = 0; i < n; ++i) v[i] = i < C3_GZS_N ? g_stats[i] : 0;
  return C3_E_OK;
}

extern "C" int c3_gunzip_host(const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len, int64_t piece) {
  int rc = 0;
  if (!c3gz::check_args("c3_gunzip_host", src, n, dst, cap, out_len, &rc)) return rc;
  memset(g_stats, 0, sizeof g_stats);
  HostBackend be{(const uint8_t*)src, n};
  c3gz::Run<HostBackend> run{"c3_gunzip_host", be, (const uint8_t*)src, n, dst, cap, c3gz::options(piece), g_stats};
  return run.run(out_len);
}

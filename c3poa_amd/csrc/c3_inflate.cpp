// c3_inflate.cpp -- host statement of k_inflate (include/c3poa.h "BGZF input"): the members of a buffer
// inflated one after the other on one thread by the decoder of c3_inflate.h, which k_inflate runs as well.  No zlib here:
// the tests hold this against Python's zlib, and damaged input can be thrown at it under a sanitizer on the CPU.
#include "../../include/c3poa.h"
#include "c3_inflate.h"
#include "c3_checks.h"
#include <cstdio>
#include <cstring>

namespace {

struct HostIO {
  const uint8_t* src; uint32_t plen; uint8_t* out;
  uint32_t word(uint32_t i) const {
    const uint64_t at = 4ull * i;
    if (at >= plen) return 0;
    uint32_t v = 0;
    memcpy(&v, src + at, plen - at >= 4 ? 4 : (size_t)(plen - at));
    return v;
  }
  void lit(uint32_t b, uint32_t at) { out[at] = (uint8_t)b; }
  void match(uint32_t len, uint32_t dist, uint32_t at) { for (uint32_t i = 0; i < len; ++i) out[at + i] = out[at - dist + i]; }
  void stored(uint32_t pos, uint32_t len, uint32_t at) { memcpy(out + at, src + pos, len); }
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() {}
  static uint32_t uni(uint32_t v) { return v; }
};

int data_error(const char* who, int64_t member, int st) {
  char buf[160];
  snprintf(buf, sizeof buf, "%s: member %lld is damaged (%s)", who, (long long)member, c3_inflate_reason(st));
  c3_set_host_error(buf);
  return C3_E_DATA;
}

}  // namespace

int c3_bgzf_data_error(const char* who, int64_t member, int st) { return data_error(who, member, st); }

extern "C" int c3_bgzf_scan(const char* src, int64_t n, int64_t* n_members, int64_t* out_bytes) {
  if (n < 0 || (n > 0 && !src) || (!n_members && !out_bytes)) { c3_set_host_error("c3_bgzf_scan: bad arguments"); return C3_E_ARG; }
  int64_t nm = 0, ob = 0;
  for (int64_t at = 0; at < n;) {
    C3BgzfMember m;
    const uint32_t size = c3_bgzf_member_at((const unsigned char*)src, n, at, &m);
    if (!size) return data_error("c3_bgzf_scan", nm, C3_INF_HEADER);
    ++nm; ob += m.isize; at += size;
  }
  if (n_members) *n_members = nm;
  if (out_bytes) *out_bytes = ob;
  return C3_E_OK;
}

extern "C" int c3_bgzf_decompress_host(const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!out_len || n < 0 || (n > 0 && !src)) { c3_set_host_error("c3_bgzf_decompress_host: bad arguments"); return C3_E_ARG; }
  *out_len = 0;
  int64_t nm = 0, ob = 0;
  const int rc = c3_bgzf_scan(src, n, &nm, &ob);
  if (rc) return rc;
  if (cap < ob || (ob > 0 && !dst)) { c3_set_host_error("c3_bgzf_decompress_host: cap < inflated size (c3_bgzf_scan)"); return C3_E_ARG; }
  uint32_t tab[256];
  for (uint32_t t = 0; t < 256; ++t) tab[t] = bgzf_crc_entry(t);
  C3InfTab T;
  int64_t o = 0, at = 0;
  for (int64_t i = 0; i < nm; ++i) {
    C3BgzfMember m;
    const uint32_t size = c3_bgzf_member_at((const unsigned char*)src, n, at, &m);
    HostIO io{(const uint8_t*)src + at + m.poff, m.plen, (uint8_t*)dst + o};
    int st = c3_inflate_member(io, &T, m.plen, m.isize);
    if (st == C3_INF_OK) {
      uint32_t c = 0xFFFFFFFFu;
      for (uint32_t k = 0; k < m.isize; ++k) c = tab[(c ^ io.out[k]) & 0xFFu] ^ (c >> 8);
      if ((~c) != m.crc) st = C3_INF_CRC;
    }
    if (st != C3_INF_OK) return data_error("c3_bgzf_decompress_host", i, st);
    o += m.isize; at += size;
  }
  *out_len = o;
  return C3_E_OK;
}

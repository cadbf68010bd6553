// c3_bgzf.cpp -- host statement of k_bgzf (include/c3poa.h "BGZF output"): the same members, byte for byte,
// one member after the other on one thread.  Code lengths and codes come from c3_bgzf.h, which k_bgzf calls as well; the
// histogram, the bit packing, the stored fallback and the CRC are written out here independently of the kernel.
#include "../../include/c3poa.h"
#include "c3_bgzf.h"
#include "c3_checks.h"
#include <zlib.h>
#include <algorithm>
#include <cstring>

namespace {

struct Bits {                                      // LSB-first bit writer (RFC 1951 3.1.1)
  uint8_t* p; uint64_t acc = 0; int n = 0;
  void put(uint32_t v, int len) {
    acc |= (uint64_t)v << n; n += len;
    while (n >= 8) { *p++ = (uint8_t)acc; acc >>= 8; n -= 8; }
  }
  void flush() { if (n > 0) { *p++ = (uint8_t)acc; acc = 0; n = 0; } }
};

void put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); }
void put32(uint8_t* p, uint32_t v) { put16(p, v & 0xFFFFu); put16(p + 2, v >> 16); }

// code lengths of n symbols with counts cnt (0 = unused) under limit L: leaves sorted by (count, symbol), package-merge
void lengths_of(const uint32_t* cnt, int n, int L, uint8_t* len) {
  uint32_t sym[BGZF_NSYM], w[BGZF_NSYM], A[4 * BGZF_NSYM], bits[15 * BGZF_PM_WORDS];
  uint8_t depth[BGZF_NSYM];
  int k = 0;
  for (int s = 0; s < n; ++s) if (cnt[s]) sym[k++] = (uint32_t)s;
  std::sort(sym, sym + k, [&](uint32_t a, uint32_t b) { return cnt[a] != cnt[b] ? cnt[a] < cnt[b] : a < b; });
  for (int i = 0; i < k; ++i) w[i] = cnt[sym[i]];
  bgzf_pm_lengths(w, k, L, A, bits, depth);
  for (int s = 0; s < n; ++s) len[s] = 0;
  for (int i = 0; i < k; ++i) len[sym[i]] = depth[i];
}

// one member for in[0..n), 1 <= n <= BGZF_BLOCK; returns its size
size_t member(const uint8_t* in, int n, uint8_t* out) {
  static const int ORD[19] = BGZF_CL_ORDER;
  uint32_t cnt[BGZF_NSYM] = {0};
  for (int i = 0; i < n; ++i) cnt[in[i]]++;
  cnt[256] = 1;
  uint8_t len[BGZF_NSYM], cllen[19];
  uint32_t code[BGZF_NSYM], clcode[19], clc[19] = {0};
  lengths_of(cnt, BGZF_NSYM, 15, len);
  bgzf_canon_codes(len, BGZF_NSYM, code);
  for (int s = 0; s < BGZF_NSYM; ++s) clc[len[s]]++;
  clc[1]++;                                                    // the one distance code, length 1
  lengths_of(clc, 19, 7, cllen);
  bgzf_canon_codes(cllen, 19, clcode);
  int hclen = 19;
  while (hclen > 4 && cllen[ORD[hclen - 1]] == 0) --hclen;
  uint64_t bits = 3 + 14 + 3 * (uint64_t)hclen;
  for (int v = 0; v < 19; ++v) bits += (uint64_t)clc[v] * cllen[v];
  for (int s = 0; s < BGZF_NSYM; ++s) bits += (uint64_t)cnt[s] * len[s];
  const bool stored = bits >= 3 + 5 + 32 + 8 * (uint64_t)n;
  uint8_t* d = out + BGZF_HDR;
  size_t dlen;
  if (stored) {
    d[0] = 1;                                                  // BFINAL 1, BTYPE 00, padding
    put16(d + 1, (uint32_t)n); put16(d + 3, (uint32_t)n ^ 0xFFFFu);
    memcpy(d + 5, in, (size_t)n);
    dlen = 5 + (size_t)n;
  } else {
    Bits b{d};
    b.put(1 | (2 << 1), 3);                                    // BFINAL 1, BTYPE 10
    b.put(0, 5); b.put(0, 5); b.put((uint32_t)(hclen - 4), 4); // HLIT 257, HDIST 1
    for (int x = 0; x < hclen; ++x) b.put(cllen[ORD[x]], 3);
    for (int s = 0; s < BGZF_NSYM; ++s) b.put(clcode[len[s]], cllen[len[s]]);
    b.put(clcode[1], cllen[1]);                                // distance code length 1
    for (int i = 0; i < n; ++i) b.put(code[in[i]], len[in[i]]);
    b.put(code[256], len[256]);
    b.flush();
    dlen = (size_t)(b.p - d);
  }
  const size_t size = BGZF_HDR + dlen + 8;
  static const uint8_t H[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
  memcpy(out, H, 16);
  put16(out + 16, (uint32_t)(size - 1));
  put32(out + BGZF_HDR + dlen, (uint32_t)crc32(0L, in, (uInt)n));
  put32(out + BGZF_HDR + dlen + 4, (uint32_t)n);
  return size;
}

}  // namespace

extern "C" int64_t c3_bgzf_bound(int64_t n) {
  if (n <= 0) return 0;
  return (n + BGZF_BLOCK - 1) / BGZF_BLOCK * (int64_t)BGZF_MAX_MEMBER;
}

extern "C" int c3_bgzf_compress_host(const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!out_len || n < 0 || (n > 0 && (!src || !dst))) { c3_set_host_error("c3_bgzf_compress_host: bad arguments"); return C3_E_ARG; }
  if (cap < c3_bgzf_bound(n)) { c3_set_host_error("c3_bgzf_compress_host: cap < c3_bgzf_bound(n)"); return C3_E_ARG; }
  int64_t o = 0;
  for (int64_t at = 0; at < n; at += BGZF_BLOCK) {
    const int len = (int)std::min<int64_t>(BGZF_BLOCK, n - at);
    o += (int64_t)member((const uint8_t*)src + at, len, (uint8_t*)dst + o);
  }
  *out_len = o;
  return C3_E_OK;
}

// c3_bgzf.h -- the frozen BGZF member format of --bgzf, shared by the host statement (c3_bgzf.cpp) and
// k_bgzf (k_bgzf.hip): constants and the one procedure that turns counts into code lengths and codes.  Both sides call
// exactly these functions, so a length assignment can never differ between them where an optimal code has ties.
#ifndef C3_BGZF_H
#define C3_BGZF_H
#include <stdint.h>

#if defined(__HIP__) || defined(__HIPCC__)
#define C3_BGZF_HD __host__ __device__
#else
#define C3_BGZF_HD
#endif

#define BGZF_BLOCK 65280          // input bytes per member (the last member of a call holds the rest)
#define BGZF_SLOT 65536           // device slot per member; a member is at most BGZF_MAX_MEMBER bytes
#define BGZF_MAX_MEMBER 65311     // stored member: 18 header + 5 + 65280 + 8 trailer
#define BGZF_HDR 18
#define BGZF_NSYM 257             // literals 0..255 and end-of-block (HLIT = 257)
#define BGZF_PM_WORDS 17          // is-leaf bits of one package-merge level (2n - 2 <= 512 positions)

// RFC 1951 order of the code-length code lengths
#define BGZF_CL_ORDER {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}

// Package-merge (limit L) over n >= 1 leaves whose weights w[0..n) are sorted ascending by (count, symbol).  Level 1 is
// the leaves; level k (2..L) merges the leaves with the packages of level k-1 (pairs 2j, 2j+1 in order), ascending by
// weight, a leaf before a package of equal weight, keeping the first 2n - 2 items.  The first 2n - 2 items of level L are
// taken; going down, the packages among the m items taken at level k expand into the first 2 * packages items of level
// k-1.  depth[i] = number of levels at which leaf i is taken = its code length.  A: two lists of 2n - 2 weights (4n
// words), bits: L * BGZF_PM_WORDS words.  One thread; n <= 2^L.
C3_BGZF_HD inline void bgzf_pm_lengths(const uint32_t* w, int n, int L, uint32_t* A, uint32_t* bits, uint8_t* depth) {
  for (int i = 0; i < n; ++i) depth[i] = 0;
  if (n == 1) { depth[0] = 1; return; }
  const int cap = 2 * n - 2;
  const uint32_t* prev = w;
  int np = n;
  for (int k = 2; k <= L; ++k) {
    uint32_t* cur = A + ((k & 1) ? cap : 0);                 // levels alternate between the two lists
    uint32_t* bw = bits + (k - 1) * BGZF_PM_WORDS;
    for (int x = 0; x < BGZF_PM_WORDS; ++x) bw[x] = 0;
    const int npk = np / 2;
    int i = 0, j = 0, m = 0;
    while (m < cap && (i < n || j < npk)) {
      const uint32_t pw = j < npk ? prev[2 * j] + prev[2 * j + 1] : 0xFFFFFFFFu;
      if (i < n && (j >= npk || w[i] <= pw)) { cur[m] = w[i++]; bw[m >> 5] |= 1u << (m & 31); }
      else { cur[m] = pw; ++j; }
      ++m;
    }
    prev = cur; np = m;
  }
  int m = cap;
  for (int k = L; k >= 2; --k) {
    const uint32_t* bw = bits + (k - 1) * BGZF_PM_WORDS;
    int a = 0;
    for (int x = 0; x < (m >> 5); ++x) a += __builtin_popcount(bw[x]);
    if (m & 31) a += __builtin_popcount(bw[m >> 5] & ((1u << (m & 31)) - 1u));
    for (int i = 0; i < a; ++i) depth[i]++;
    m = 2 * (m - a);
  }
  for (int i = 0; i < m; ++i) depth[i]++;                      // level 1: leaves only
}

// Canonical codes of RFC 1951 3.2.2 from lengths len[0..n) (<= 15), bit-reversed for LSB-first output
C3_BGZF_HD inline void bgzf_canon_codes(const uint8_t* len, int n, uint32_t* rcode) {
  int bl[16];
  for (int b = 0; b < 16; ++b) bl[b] = 0;
  for (int s = 0; s < n; ++s) bl[len[s]]++;
  bl[0] = 0;
  uint32_t next[16], c = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) { c = (c + (uint32_t)bl[b - 1]) << 1; next[b] = c; }
  for (int s = 0; s < n; ++s) {
    const int l = len[s];
    if (!l) { rcode[s] = 0; continue; }
    const uint32_t v = next[l]++;
    uint32_t r = 0;
    for (int b = 0; b < l; ++b) r |= ((v >> b) & 1u) << (l - 1 - b);
    rcode[s] = r;
  }
}

// CRC-32 (zlib) algebra: multiplication modulo the reflected polynomial, and x^(2^k) mod p (zlib's crc32_combine)
C3_BGZF_HD inline uint32_t bgzf_multmodp(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0;
  for (;;) {
    if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
    m >>= 1;
    b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
  }
  return p;
}
// entry t of the byte-wise CRC table
C3_BGZF_HD inline uint32_t bgzf_crc_entry(uint32_t t) {
  for (int k = 0; k < 8; ++k) t = (t & 1) ? (t >> 1) ^ 0xEDB88320u : t >> 1;
  return t;
}
// x2n[k] = x^(2^k) mod p, k < 20
C3_BGZF_HD inline void bgzf_x2n_init(uint32_t* x2n) {
  uint32_t p = 1u << 30;                                       // x^1
  x2n[0] = p;
  for (int k = 1; k < 20; ++k) { p = bgzf_multmodp(p, p); x2n[k] = p; }
}
// the CRC of a piece moved in front of `after` < 65536 more bytes: multiplication by x^(8 * after)
C3_BGZF_HD inline uint32_t bgzf_crc_shift(const uint32_t* x2n, uint32_t after, uint32_t crc) {
  uint32_t p = 1u << 31;                                       // x^0
  for (int k = 0; k < 16; ++k) if ((after >> k) & 1u) p = bgzf_multmodp(x2n[k + 3], p);
  return bgzf_multmodp(p, crc);
}
#endif

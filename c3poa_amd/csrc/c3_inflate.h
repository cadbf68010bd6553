// c3_inflate.h -- the serial part of inflate (RFC 1951) for BGZF members, once, for the host statement (c3_inflate.cpp)
// and k_inflate (k_inflate.hip); DESIGN.md 5.4.  Block headers, code lengths, table building with zlib's validity rules,
// symbol decode, length / distance bases and every bounds check are here; what differs between the two sides -- where
// payload words come from, where bytes go, how many lanes share the loops that are plain data movement -- is the policy P:
//
//   uint32_t P::word(uint32_t i)                     little-endian dword i of the payload (anything past its end: the
//                                                    decoder notices that it consumed more bits than the payload has)
//   void P::lit(uint32_t b, uint32_t at)             out[at] = b
//   void P::match(uint32_t len, uint32_t dist, uint32_t at)     out[at + i] = out[at - dist + i], i < len, in order
//   void P::stored(uint32_t pos, uint32_t len, uint32_t at)     out[at + i] = payload byte pos + i
//   int P::lane(), int P::lanes()                    the loops marked "by all lanes" run i = lane(); i < n; i += lanes()
//   void P::sync()                                   table writes of all lanes visible to all lanes
//   static uint32_t P::uni(uint32_t)                 a value that is the same in every lane (device: readfirstlane)
//
// The decoder checks before it calls: at + len <= isize, dist <= at, pos + len <= payload length.  Everything outside the
// two "by all lanes" loops is the same instruction stream on the same values in every lane.
#ifndef C3_INFLATE_H
#define C3_INFLATE_H
#include <stdint.h>
#include "c3_bgzf.h"

// member status (c3_last_error names them: c3_inflate_reason)
enum {
  C3_INF_OK = 0,
  C3_INF_HEADER = 1,      // member header / sizes (host walk)
  C3_INF_BTYPE = 2,       // block type 3
  C3_INF_STORED = 3,      // stored block: LEN != ~NLEN
  C3_INF_LENS = 4,        // code lengths: counts, repeat codes, over-subscribed / incomplete set, no end-of-block code
  C3_INF_SYMBOL = 5,      // a bit pattern that is no code of the set, or a length / distance symbol beyond 285 / 29
  C3_INF_DIST = 6,        // distance beyond the output so far
  C3_INF_LONG = 7,        // output longer than ISIZE
  C3_INF_SHORT = 8,       // output shorter than ISIZE
  C3_INF_INPUT = 9,       // input exhausted
  C3_INF_CRC = 10
};

inline const char* c3_inflate_reason(int st) {
  static const char* const R[] = {"ok", "header", "block type", "stored block length", "code lengths", "symbol",
                                  "distance beyond the output so far", "output longer than ISIZE", "output shorter than ISIZE",
                                  "input exhausted", "CRC"};
  return st >= 0 && st <= C3_INF_CRC ? R[st] : "unknown status";
}

#define C3_INF_LBITS 10           // first-level table of the literal/length code
#define C3_INF_DBITS 8            // and of the distance code; longer codes take the canonical walk

struct C3InfTab {
  uint16_t lfast[1 << C3_INF_LBITS];        // symbol << 4 | length, 0 = no code this short
  uint16_t dfast[1 << C3_INF_DBITS];
  uint16_t lsym[288], dsym[32], csym[19];   // symbols in canonical order
  uint16_t lcnt[16], dcnt[16], ccnt[16];    // codes per length
  uint16_t first[16], offs[16];             // build scratch: first code / first canonical index per length
  uint8_t lens[320];                        // literal/length lengths, then the distance lengths
  uint8_t cl[19];
};

struct C3InfBits { uint64_t acc; int n; uint32_t wi; };

template <class P> C3_BGZF_HD inline void c3_inf_fill(P& p, C3InfBits& b) {       // afterwards >= 32 bits
  if (b.n <= 32) { b.acc |= (uint64_t)p.word(b.wi++) << b.n; b.n += 32; }
}
C3_BGZF_HD inline uint32_t c3_inf_take(C3InfBits& b, int k) {                     // k < 32
  const uint32_t v = (uint32_t)b.acc & ((1u << k) - 1u);
  b.acc >>= k; b.n -= k;
  return v;
}
C3_BGZF_HD inline uint32_t c3_inf_used(const C3InfBits& b) { return 32u * b.wi - (uint32_t)b.n; }

// Canonical code of len[0..n): cnt / sym for the walk, and (fast != null) the first-level table.  Returns 0, or 1 when the
// set is over-subscribed, or incomplete other than a single code of length 1 (zlib's inflate_table; strict: the
// code-length code, where every incomplete or empty set is refused).  An empty set is fine otherwise: nothing decodes.
template <class P>
C3_BGZF_HD inline int c3_inf_build(P& p, C3InfTab* T, const uint8_t* len, int n, uint16_t* cnt, uint16_t* sym, uint16_t* fast, int fbits, bool strict) {
  for (int l = 0; l < 16; ++l) cnt[l] = 0;
  for (int s = 0; s < n; ++s) cnt[len[s]]++;
  cnt[0] = 0;
  int left = 1, max = 0;
  uint32_t code = 0, at = 0;
  for (int l = 1; l < 16; ++l) {
    const int c = (int)P::uni(cnt[l]);
    left = (left << 1) - c;
    if (left < 0) return 1;
    if (c) max = l;
    T->first[l] = (uint16_t)code; T->offs[l] = (uint16_t)at;
    code = (code + (uint32_t)c) << 1; at += (uint32_t)c;
  }
  if (left > 0 && (strict || max > 1)) return 1;                // (max == 0: cnt is all zero and the table below all "no code")
  // canonical order = by length, then by symbol: a running index per length, kept in T->offs and restored afterwards
  for (int s = 0; s < n; ++s) {
    const int l = (int)P::uni(len[s]);
    if (l) { const uint32_t o = P::uni(T->offs[l]); sym[o] = (uint16_t)s; T->offs[l] = (uint16_t)(o + 1); }
  }
  for (int l = 15; l >= 1; --l) T->offs[l] = (uint16_t)(T->offs[l] - cnt[l]);
  if (!fast) return 0;
  p.sync();
  const int total = (int)at, size = 1 << fbits;
  for (int i = p.lane(); i < size; i += p.lanes()) fast[i] = 0;                 // by all lanes
  p.sync();
  for (int i = p.lane(); i < total; i += p.lanes()) {                            // by all lanes
    const uint32_t s = sym[i];
    const int l = len[s];
    if (l <= fbits) {
      const uint32_t c = (uint32_t)T->first[l] + ((uint32_t)i - T->offs[l]);
      uint32_t r = 0;
      for (int b = 0; b < l; ++b) r |= ((c >> b) & 1u) << (l - 1 - b);
      for (uint32_t x = r; x < (uint32_t)size; x += 1u << l) fast[x] = (uint16_t)(s << 4 | (uint32_t)l);
    }
  }
  p.sync();
  return 0;
}

// one symbol: first-level table, then the canonical walk bit by bit (puff); -1 when the bits are no code of the set
template <class P>
C3_BGZF_HD inline int c3_inf_sym(C3InfBits& b, const uint16_t* fast, int fbits, const uint16_t* cnt, const uint16_t* sym) {
  if (fast) {
    const uint32_t e = P::uni(fast[(uint32_t)b.acc & ((1u << fbits) - 1u)]);
    if (e) { b.acc >>= (e & 15u); b.n -= (int)(e & 15u); return (int)(e >> 4); }
  }
  int code = 0, first = 0, index = 0;
  uint32_t a = (uint32_t)b.acc;
  for (int l = 1; l < 16; ++l) {
    code |= (int)(a & 1u); a >>= 1;
    const int c = (int)P::uni(cnt[l]);
    if (code - c < first) { b.acc >>= l; b.n -= l; return (int)P::uni(sym[index + (code - first)]); }
    index += c; first += c; first <<= 1; code <<= 1;
  }
  return -1;
}

// RFC 1951 order of the code-length code lengths, five bits each
C3_BGZF_HD inline int c3_inf_clorder(int i) {
  const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
  const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
  return (int)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31u);
}

// The deflate stream of one member: plen payload bytes in, exactly isize bytes out.  Returns a C3_INF_ status (the CRC
// is the caller's).  Every loop ends by the payload's bit count or by isize.
template <class P>
C3_BGZF_HD inline int c3_inflate_member(P& p, C3InfTab* T, uint32_t plen, uint32_t isize) {
  C3InfBits b; b.acc = 0; b.n = 0; b.wi = 0;
  const uint32_t total = 8u * plen;
  uint32_t outn = 0;
  for (;;) {
    c3_inf_fill(p, b);
    const uint32_t bfinal = c3_inf_take(b, 1), btype = c3_inf_take(b, 2);
    if (c3_inf_used(b) > total) return C3_INF_INPUT;
    if (btype == 3) return C3_INF_BTYPE;
    if (btype == 0) {
      c3_inf_take(b, b.n & 7);
      c3_inf_fill(p, b);
      const uint32_t len = c3_inf_take(b, 16), nlen = c3_inf_take(b, 16);
      const uint32_t used = c3_inf_used(b);
      if (used > total) return C3_INF_INPUT;
      if ((len ^ nlen) != 0xFFFFu) return C3_INF_STORED;
      const uint32_t pos = used >> 3;
      if (len > plen - pos) return C3_INF_INPUT;
      if (len > isize - outn) return C3_INF_LONG;
      p.stored(pos, len, outn);
      outn += len;
      const uint32_t np = pos + len;
      b.acc = 0; b.n = 0; b.wi = np >> 2;
      c3_inf_fill(p, b);
      c3_inf_take(b, 8 * (int)(np & 3u));
    } else {
      int nl, nd;
      if (btype == 1) {
        nl = 288; nd = 32;
        for (int s = 0; s < 288; ++s) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        for (int s = 0; s < 32; ++s) T->lens[288 + s] = 5;
      } else {
        c3_inf_fill(p, b);
        nl = 257 + (int)c3_inf_take(b, 5); nd = 1 + (int)c3_inf_take(b, 5);
        const int nc = 4 + (int)c3_inf_take(b, 4);
        if (nl > 286 || nd > 30) return C3_INF_LENS;
        for (int i = 0; i < 19; ++i) T->cl[i] = 0;
        for (int i = 0; i < nc; ++i) { c3_inf_fill(p, b); T->cl[c3_inf_clorder(i)] = (uint8_t)c3_inf_take(b, 3); }
        if (c3_inf_used(b) > total) return C3_INF_INPUT;
        if (c3_inf_build(p, T, T->cl, 19, T->ccnt, T->csym, (uint16_t*)0, 0, true)) return C3_INF_LENS;
        int have = 0;
        while (have < nl + nd) {                               // each turn stores at least one length
          c3_inf_fill(p, b);
          const int s = c3_inf_sym<P>(b, (const uint16_t*)0, 0, T->ccnt, T->csym);
          if (s < 0) return C3_INF_LENS;
          if (s < 16) { T->lens[have++] = (uint8_t)s; continue; }
          int rep; uint8_t v = 0;
          if (s == 16) { if (have == 0) return C3_INF_LENS; v = (uint8_t)P::uni(T->lens[have - 1]); rep = 3 + (int)c3_inf_take(b, 2); }
          else if (s == 17) rep = 3 + (int)c3_inf_take(b, 3);
          else rep = 11 + (int)c3_inf_take(b, 7);
          if (have + rep > nl + nd) return C3_INF_LENS;
          for (int k = 0; k < rep; ++k) T->lens[have++] = v;
        }
        if (c3_inf_used(b) > total) return C3_INF_INPUT;
        if (P::uni(T->lens[256]) == 0) return C3_INF_LENS;
      }
      p.sync();
      if (c3_inf_build(p, T, T->lens, nl, T->lcnt, T->lsym, T->lfast, C3_INF_LBITS, false)) return C3_INF_LENS;
      if (c3_inf_build(p, T, T->lens + nl, nd, T->dcnt, T->dsym, T->dfast, C3_INF_DBITS, false)) return C3_INF_LENS;
      for (;;) {                                               // each turn consumes at least one bit
        c3_inf_fill(p, b);
        const int s = c3_inf_sym<P>(b, T->lfast, C3_INF_LBITS, T->lcnt, T->lsym);
        if (s < 0) return C3_INF_SYMBOL;
        if (c3_inf_used(b) > total) return C3_INF_INPUT;
        if (s < 256) {
          if (outn >= isize) return C3_INF_LONG;
          p.lit((uint32_t)s, outn);
          ++outn;
          continue;
        }
        if (s == 256) break;
        if (s > 285) return C3_INF_SYMBOL;
        uint32_t len;
        {
          const int k = s - 257;
          if (k < 8) len = 3u + (uint32_t)k;
          else if (k == 28) len = 258;
          else { const int e = (k >> 2) - 1; len = 3u + ((4u + (uint32_t)(k & 3)) << e) + c3_inf_take(b, e); }
        }
        c3_inf_fill(p, b);
        const int d = c3_inf_sym<P>(b, T->dfast, C3_INF_DBITS, T->dcnt, T->dsym);
        if (d < 0 || d > 29) return C3_INF_SYMBOL;
        uint32_t dist;
        if (d < 4) dist = 1u + (uint32_t)d;
        else { const int e = (d >> 1) - 1; dist = 1u + ((2u + (uint32_t)(d & 1)) << e) + c3_inf_take(b, e); }
        if (c3_inf_used(b) > total) return C3_INF_INPUT;
        if (dist > outn) return C3_INF_DIST;
        if (len > isize - outn) return C3_INF_LONG;
        p.match(len, dist, outn);
        outn += len;
      }
    }
    if (bfinal) break;
  }
  return outn == isize ? C3_INF_OK : C3_INF_SHORT;
}

// ---- member framing (host): what bgzf_next_stretch of c3_reader_bgzf.cpp checks, as one walk ------------------------------------
struct C3BgzfMember { uint32_t poff, plen, ooff, isize, crc; };   // payload offset / bytes, output offset, trailer

// member at src[at..n): fills m (poff counted from the member's first byte, ooff left alone) and returns its size, or 0
// when it is no whole BGZF member
inline uint32_t c3_bgzf_member_at(const unsigned char* src, int64_t n, int64_t at, C3BgzfMember* m) {
  if (n - at < 12 + 6 + 8) return 0;
  const unsigned char* p = src + at;
  if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return 0;
  const uint32_t xlen = (uint32_t)p[10] | (uint32_t)p[11] << 8;
  if (12 + (int64_t)xlen > n - at) return 0;
  uint32_t size = 0;
  for (uint32_t q = 12; q + 4 <= 12 + xlen;) {
    const uint32_t slen = (uint32_t)p[q + 2] | (uint32_t)p[q + 3] << 8;
    if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2 && q + 6 <= 12 + xlen) { size = ((uint32_t)p[q + 4] | (uint32_t)p[q + 5] << 8) + 1; break; }
    q += 4 + slen;
  }
  if (size < 12 + xlen + 8 || (int64_t)size > n - at) return 0;
  const unsigned char* t = p + size - 8;
  m->poff = 12 + xlen;
  m->plen = size - 12 - xlen - 8;
  m->crc = (uint32_t)t[0] | (uint32_t)t[1] << 8 | (uint32_t)t[2] << 16 | (uint32_t)t[3] << 24;
  m->isize = (uint32_t)t[4] | (uint32_t)t[5] << 8 | (uint32_t)t[6] << 16 | (uint32_t)t[7] << 24;
  if (m->isize > 65536u) return 0;
  return size;
}
#endif

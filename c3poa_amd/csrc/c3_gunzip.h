// c3_gunzip.h -- the parts of --gunzip gpu that the host statement (c3_gunzip.cpp) and the kernels (k_gunzip.hip) share
// (include/c3poa.h "gzip input"): the cheap reject and the full parse of a dynamic block header at any bit
// position, the decode of one piece into 16-bit symbols, and how a symbol becomes a byte.  Bit reader, code sets and the
// symbol walk are those of c3_inflate.h; the policy P is its policy with a sink of symbols instead of bytes:
//
//   uint32_t P::word(uint32_t i)                     little-endian dword i counted from the piece's base dword (zero past the file)
//   void P::lit(uint32_t b, uint32_t at)             sym[at] = b
//   void P::match(uint32_t len, uint32_t dist, uint32_t at)     sym[at + i] = at + i >= dist ? sym[at + i - dist]
//                                                                 : C3_GZ_MARK | (C3_GZ_WIN + at + i - dist), i < len, in order
//   void P::stored(uint32_t pos, uint32_t len, uint32_t at)     sym[at + i] = byte pos + i counted from the piece's base
//   lane(), lanes(), sync(), uni()                   as in c3_inflate.h
//
// A symbol below 256 is that byte; C3_GZ_MARK | p is byte p of the 32 KiB in front of the piece's first byte.  The decoder
// checks before it calls: at + len <= cap (the slab), dist <= 32768, pos + len inside the file.
#ifndef C3_GUNZIP_H
#define C3_GUNZIP_H
#include "c3_inflate.h"

#define C3_GZ_WIN 32768u
#define C3_GZ_MARK 0x8000u
#define C3_GZ_REL_MAX 0xF0000000u     // bits a piece may see counted from its base dword (the bit reader counts in 32 bits)

// how a piece stopped
enum {
  C3_GZ_LIMIT = 0,      // at the first block boundary at or past its limit
  C3_GZ_FINAL = 1,      // at a final block's end
  C3_GZ_FULL = 2,       // the slab is full: symbols [0, bb_nsym) up to the last block boundary bb are good
  C3_GZ_BAD = 3         // a C3_INF_ reason: damage if the piece began at a true block boundary, a false candidate otherwise
};

struct C3GzJob {        // one piece that decodes
  int64_t start;        // bit position (in the file) of its first block header
  int64_t limit;        // it stops at the first block boundary at or past this bit
  int64_t slab;         // first symbol of its slab in the arena
  uint32_t cap;         // symbols in the slab
  uint32_t pad;
};
struct C3GzRes {
  int32_t status, reason;
  uint32_t nsym, bb_nsym;   // symbols written; symbols written when the last block boundary was passed
  int64_t stop, bb;         // bit position where it stopped; of the last block boundary passed (start if none)
};
struct C3GzSeg {        // an accepted piece, for the window chain and the resolve
  int64_t slab;         // its symbols (arena index)
  int64_t out;          // where its bytes go, counted from the stretch's first output byte
  uint32_t nsym;
  uint32_t wlen;        // bytes of the 32 KiB in front of it that its member has written (a marker below 32768 - wlen is damage)
};
struct C3GzChunk { uint32_t seg, from, len, pad; };      // resolve work: symbols [from, from + len) of segment seg

// ---- find: does a dynamic-Huffman block header parse at this bit? ---------------------------------------------------------
// the cheap reject on the 74 bits at the position (v0 = bits 0..63, v1 = bits 64..): block type 2, HLIT and HDIST in
// range, and a code-length code whose Kraft sum is exactly 1 (c3_inf_build's strict rule)
C3_BGZF_HD inline bool c3_gz_quick(uint64_t v0, uint64_t v1) {
  if (((v0 >> 1) & 3u) != 2u) return false;
  if (((v0 >> 3) & 31u) > 29u || ((v0 >> 8) & 31u) > 29u) return false;
  const int nc = 4 + (int)((v0 >> 13) & 15u);
  const uint64_t cl = (v0 >> 17) | (v1 << 47);
  uint32_t kraft = 0;
  for (int i = 0; i < nc; ++i) { const uint32_t l = (uint32_t)(cl >> (3 * i)) & 7u; if (l) kraft += 128u >> l; }
  return kraft == 128u;
}

// the dynamic header behind BFINAL / BTYPE: HLIT, HDIST, HCLEN, the code-length code and the lengths into T->lens
// (c3_inflate_member's rules).  0 or a C3_INF_ reason.
template <class P>
C3_BGZF_HD inline int c3_gz_dyn_lens(P& p, C3InfTab* T, C3InfBits& b, uint32_t total, int* nl_out, int* nd_out) {
  c3_inf_fill(p, b);
  const int nl = 257 + (int)c3_inf_take(b, 5), nd = 1 + (int)c3_inf_take(b, 5);
  const int nc = 4 + (int)c3_inf_take(b, 4);
  if (nl > 286 || nd > 30) return C3_INF_LENS;
  for (int i = 0; i < 19; ++i) T->cl[i] = 0;
  for (int i = 0; i < nc; ++i) { c3_inf_fill(p, b); T->cl[c3_inf_clorder(i)] = (uint8_t)c3_inf_take(b, 3); }
  if (c3_inf_used(b) > total) return C3_INF_INPUT;
  if (c3_inf_build(p, T, T->cl, 19, T->ccnt, T->csym, (uint16_t*)0, 0, true)) return C3_INF_LENS;
  int have = 0;
  while (have < nl + nd) {                                   // each turn stores at least one length
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
  *nl_out = nl; *nd_out = nd;
  return C3_INF_OK;
}

C3_BGZF_HD inline void c3_gz_bits_at(C3InfBits& b, uint32_t bit) { b.acc = 0; b.n = 0; b.wi = bit >> 5; }

// the full test of a candidate: the header at bit `at` (counted from the policy's base) parses and both code sets are valid
template <class P>
C3_BGZF_HD inline bool c3_gz_header_at(P& p, C3InfTab* T, uint32_t at, uint32_t total) {
  C3InfBits b; c3_gz_bits_at(b, at);
  c3_inf_fill(p, b);
  c3_inf_take(b, (int)(at & 31u));
  c3_inf_fill(p, b);
  c3_inf_take(b, 1);
  if (c3_inf_take(b, 2) != 2u) return false;
  int nl = 0, nd = 0;
  if (c3_gz_dyn_lens(p, T, b, total, &nl, &nd)) return false;
  p.sync();
  if (c3_inf_build(p, T, T->lens, nl, T->lcnt, T->lsym, (uint16_t*)0, 0, false)) return false;
  if (c3_inf_build(p, T, T->lens + nl, nd, T->dcnt, T->dsym, (uint16_t*)0, 0, false)) return false;
  return true;
}

// ---- decode: one piece from a block header at bit `sbit` to its stop ------------------------------------------------------
// Positions are bits counted from the policy's base dword; r->stop and r->bb come back the same way (the caller adds the
// base).  Every loop ends by the bit count `total` or by the slab size `cap`.
template <class P>
C3_BGZF_HD inline void c3_gz_piece(P& p, C3InfTab* T, uint32_t sbit, uint32_t total, uint32_t limit, uint32_t cap, C3GzRes* r) {
  C3InfBits b; c3_gz_bits_at(b, sbit);
  c3_inf_fill(p, b);
  c3_inf_take(b, (int)(sbit & 31u));
  const uint32_t plen = total >> 3;
  uint32_t outn = 0;
  r->nsym = 0; r->bb_nsym = 0; r->bb = sbit; r->stop = sbit; r->reason = C3_INF_OK;
#define GZ_END(st, why) do { r->status = (st); r->reason = (why); r->nsym = outn; r->stop = c3_inf_used(b); return; } while (0)
  for (;;) {
    c3_inf_fill(p, b);
    const uint32_t bfinal = c3_inf_take(b, 1), btype = c3_inf_take(b, 2);
    if (c3_inf_used(b) > total) GZ_END(C3_GZ_BAD, C3_INF_INPUT);
    if (btype == 3) GZ_END(C3_GZ_BAD, C3_INF_BTYPE);
    if (btype == 0) {
      c3_inf_take(b, b.n & 7);
      c3_inf_fill(p, b);
      const uint32_t len = c3_inf_take(b, 16), nlen = c3_inf_take(b, 16);
      const uint32_t used = c3_inf_used(b);
      if (used > total) GZ_END(C3_GZ_BAD, C3_INF_INPUT);
      if ((len ^ nlen) != 0xFFFFu) GZ_END(C3_GZ_BAD, C3_INF_STORED);
      const uint32_t pos = used >> 3;
      if (len > plen - pos) GZ_END(C3_GZ_BAD, C3_INF_INPUT);
      if (len > cap - outn) GZ_END(C3_GZ_FULL, C3_INF_OK);
      p.stored(pos, len, outn);
      outn += len;
      const uint32_t np = pos + len;
      c3_gz_bits_at(b, 8u * np);
      c3_inf_fill(p, b);
      c3_inf_take(b, 8 * (int)(np & 3u));
    } else {
      int nl, nd;
      if (btype == 1) {
        nl = 288; nd = 32;
        for (int s = 0; s < 288; ++s) T->lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
        for (int s = 0; s < 32; ++s) T->lens[288 + s] = 5;
      } else {
        const int st = c3_gz_dyn_lens(p, T, b, total, &nl, &nd);
        if (st) GZ_END(C3_GZ_BAD, st);
      }
      p.sync();
      if (c3_inf_build(p, T, T->lens, nl, T->lcnt, T->lsym, T->lfast, C3_INF_LBITS, false)) GZ_END(C3_GZ_BAD, C3_INF_LENS);
      if (c3_inf_build(p, T, T->lens + nl, nd, T->dcnt, T->dsym, T->dfast, C3_INF_DBITS, false)) GZ_END(C3_GZ_BAD, C3_INF_LENS);
      for (;;) {                                             // each turn consumes at least one bit
        c3_inf_fill(p, b);
        const int s = c3_inf_sym<P>(b, T->lfast, C3_INF_LBITS, T->lcnt, T->lsym);
        if (s < 0) GZ_END(C3_GZ_BAD, C3_INF_SYMBOL);
        if (c3_inf_used(b) > total) GZ_END(C3_GZ_BAD, C3_INF_INPUT);
        if (s < 256) {
          if (outn >= cap) GZ_END(C3_GZ_FULL, C3_INF_OK);
          p.lit((uint32_t)s, outn);
          ++outn;
          continue;
        }
        if (s == 256) break;
        if (s > 285) GZ_END(C3_GZ_BAD, C3_INF_SYMBOL);
        uint32_t len;
        {
          const int k = s - 257;
          if (k < 8) len = 3u + (uint32_t)k;
          else if (k == 28) len = 258;
          else { const int e = (k >> 2) - 1; len = 3u + ((4u + (uint32_t)(k & 3)) << e) + c3_inf_take(b, e); }
        }
        c3_inf_fill(p, b);
        const int d = c3_inf_sym<P>(b, T->dfast, C3_INF_DBITS, T->dcnt, T->dsym);
        if (d < 0 || d > 29) GZ_END(C3_GZ_BAD, C3_INF_SYMBOL);
        uint32_t dist;
        if (d < 4) dist = 1u + (uint32_t)d;
        else { const int e = (d >> 1) - 1; dist = 1u + ((2u + (uint32_t)(d & 1)) << e) + c3_inf_take(b, e); }
        if (c3_inf_used(b) > total) GZ_END(C3_GZ_BAD, C3_INF_INPUT);
        if (len > cap - outn) GZ_END(C3_GZ_FULL, C3_INF_OK);
        p.match(len, dist, outn);                            // (dist <= 32768 by construction: nothing to refuse here)
        outn += len;
      }
    }
    const uint32_t pos = c3_inf_used(b);
    r->bb = pos; r->bb_nsym = outn;
    if (bfinal) GZ_END(C3_GZ_FINAL, C3_INF_OK);
    if (pos >= limit) GZ_END(C3_GZ_LIMIT, C3_INF_OK);
  }
#undef GZ_END
}

// the base dword of a piece that begins at file bit `start` in a file of n bytes, and its positions counted from there
struct C3GzRel { int64_t base; uint32_t sbit, total, limit; };     // base: byte offset of the base dword (a multiple of 4)
C3_BGZF_HD inline C3GzRel c3_gz_rel(int64_t start, int64_t limit, int64_t n) {
  C3GzRel q;
  q.base = (start >> 3) & ~(int64_t)3;
  q.sbit = (uint32_t)(start - 8 * q.base);
  const int64_t t = 8 * (n - q.base), l = limit - 8 * q.base;
  q.total = (uint32_t)(t < (int64_t)C3_GZ_REL_MAX ? t : (int64_t)C3_GZ_REL_MAX);
  q.limit = (uint32_t)(l < 0 ? 0 : l < (int64_t)0xFFFFFFFFu ? l : (int64_t)0xFFFFFFFFu);
  return q;
}

// ---- resolve: a symbol and the 32 KiB in front of its piece -----------------------------------------------------------------
// the byte, or -1 for a marker that points in front of what the member has written (wlen bytes of the window are real)
C3_BGZF_HD inline int c3_gz_byte(uint32_t s, const uint8_t* win, uint32_t wlen) {
  if (s < 256u) return (int)s;
  const uint32_t q = s & (C3_GZ_WIN - 1u);
  if ((s & C3_GZ_MARK) == 0u || q < C3_GZ_WIN - wlen) return -1;
  return (int)win[q];
}
// byte i of the window behind a piece of nsym symbols, from its symbols and the window in front of it
C3_BGZF_HD inline int c3_gz_next_window(const uint16_t* sym, uint32_t nsym, const uint8_t* win, uint32_t wlen, uint32_t i) {
  if (nsym >= C3_GZ_WIN) return c3_gz_byte(sym[nsym - C3_GZ_WIN + i], win, wlen);
  if (i + nsym >= C3_GZ_WIN) return c3_gz_byte(sym[i + nsym - C3_GZ_WIN], win, wlen);
  return (int)win[i + nsym];                                  // (bytes in front of the member are never looked at: wlen)
}

// x^(8 * len) applied to a CRC-32: the CRC of a run moved in front of len more bytes (any len; x2n[k] = x^(2^k), k < 36)
C3_BGZF_HD inline void c3_gz_x2n_init(uint32_t* x2n) {
  uint32_t p = 1u << 30;
  x2n[0] = p;
  for (int k = 1; k < 36; ++k) { p = bgzf_multmodp(p, p); x2n[k] = p; }
}
C3_BGZF_HD inline uint32_t c3_gz_crc_shift(const uint32_t* x2n, uint64_t len, uint32_t crc) {
  uint32_t p = 1u << 31;
  for (int k = 0; k < 33; ++k) if ((len >> k) & 1u) p = bgzf_multmodp(x2n[k + 3], p);
  return bgzf_multmodp(p, crc);
}
#endif

// c3_emit.h -- the record rule of the main CLI's writer (include/c3poa.h "Records formatted on the GPU"), once,
// for the host statement (c3_emit.cpp), the host writer (c3_writer.cpp: emit_of) and k_emit (k_emit.hip): which records a read
// produces (C3POa.py:115-132, determine_consensus.py:57-77,108-114), in which order, how long each is, and the text of the
// average quality in the consensus header (C3POa.py:168).  How the bytes are moved is what the two sides do each in their
// own way.
#ifndef C3_EMIT_H
#define C3_EMIT_H
#include <stdint.h>
#include "../../include/c3poa.h"
#include "c3_post.h"                    // C3_PO_HD, c3_post_digits, c3_post_digit

#define C3_EMIT_MAX_SPLINTS 64          // streams are scanned column by column: 3 * 64 columns at most
#define C3_EMIT_MAX_SUB 250             // C3_MAX_SUB of c3_dev.h: kept subreads of one read
#define C3_EMIT_KINDS 3
#define C3_EMIT_MAX_COLS (C3_EMIT_KINDS * C3_EMIT_MAX_SPLINTS + 1)      // + the record count
enum { C3_EMIT_CONS_FA = 0, C3_EMIT_SUB_FQ = 1, C3_EMIT_CONS_FQ = 2 };

// which records does a read produce?  any: its subread records; cons: the consensus record(s) too; ns = "repeats" as the
// header prints them; np = subread FASTQ records
struct C3EmitDec { int32_t any, cons, ns, np; };
C3_PO_HD inline C3EmitDec c3_emit_of(const c3_read_result& r, int s, int n_splints, int zero, int64_t clen) {
  C3EmitDec e = {0, 0, r.n_sub, 0};
  if (s < 0 || s >= n_splints) return e;
  if (r.status == C3_ST_NOT_ASSIGNED || r.status == C3_ST_NO_PEAKS || r.status == C3_ST_TOO_SHORT) return e;   // C3POa.py:115,125,131
  const int nd = (r.has_front ? 1 : 0) + (r.has_tail ? 1 : 0);
  if (r.n_sub == 0) { if (!(zero && nd == 2)) return e; }
  else if (r.status == C3_ST_LIMIT) return e;
  e.any = 1; e.cons = r.status == C3_ST_OK && clen > 0;
  const int nk = r.n_sub < 0 ? 0 : r.n_sub > C3_EMIT_MAX_SUB ? C3_EMIT_MAX_SUB : r.n_sub;
  e.np = r.n_sub == 0 ? 2 : nk + nd;
  return e;
}

// subread record j (0 .. np-1) of a read of L bases, in file order: kept subreads _1.._ns, then the front piece _0, then the tail
// piece _<ns+1> (_0 without a front piece); the zero-repeat pieces are _0 and _1.  The slice is clamped into the read: a no-op
// on records the callers have validated, and the device never reads outside a read whatever the record holds.
C3_PO_HD inline void c3_emit_piece(const c3_read_result& r, const C3EmitDec& d, int64_t L, int j, int32_t* idx, int64_t* beg, int64_t* end) {
  int64_t b, e;
  if (d.ns == 0) { *idx = j; if (j == 0) { b = 0; e = r.front_end; } else { b = r.tail_beg; e = L; } }
  else if (j < d.np - (r.has_front ? 1 : 0) - (r.has_tail ? 1 : 0)) { *idx = j + 1; b = r.sub_beg[j]; e = r.sub_end[j]; }
  else if (r.has_front && j == d.np - 1 - (r.has_tail ? 1 : 0)) { *idx = 0; b = 0; e = r.front_end; }
  else { *idx = r.has_front ? d.ns + 1 : 0; b = r.tail_beg; e = L; }
  b = b < 0 ? 0 : b > L ? L : b;
  e = e < b ? b : e > L ? L : e;
  *beg = b; *end = e;
}

// str(round(tot / L, 2)) of Python (C3POa.py:168; avg_qual_text of c3_writer.cpp prints "%.2f" and drops one trailing zero): the
// IEEE double d = tot / L, two decimals correctly rounded from d's binary value (ties of that value to even), by integers:
// |d| < 256, so d = m * 2^-sh with sh >= 45 and 100 * m < 2^60.  A sign whenever tot < 0.  At most 7 bytes; returns the length.
C3_PO_HD inline int c3_emit_avgq(int64_t tot, int64_t L, char* out) {
  const double d = (double)tot / (double)L;
  union { double f; uint64_t u; } cv; cv.f = d;
  const int ex = (int)((cv.u >> 52) & 0x7FFu);
  uint64_t m = cv.u & 0xFFFFFFFFFFFFFull;
  int sh;
  if (ex == 0) sh = 1074; else { m |= 1ull << 52; sh = 1075 - ex; }
  uint64_t q = 0;
  if (sh >= 1 && sh < 64) {             // (L == 0 has no quotient: the callers refuse a consensus record of an empty read)
    const uint64_t P = m * 100ull, half = 1ull << (sh - 1), rem = P & ((half << 1) - 1ull);
    q = P >> sh;
    if (rem > half || (rem == half && (q & 1ull))) ++q;
  }
  int n = 0;
  if (tot < 0) out[n++] = '-';
  const uint32_t ip = (uint32_t)(q / 100ull), fr = (uint32_t)(q % 100ull);
  const int nd = c3_post_digits(ip);
  for (int j = 0; j < nd; ++j) out[n++] = c3_post_digit(ip, nd, j);
  out[n++] = '.';
  out[n++] = (char)('0' + fr / 10u);
  if (fr % 10u) out[n++] = (char)('0' + fr % 10u);
  return n;
}

// lengths.  A subread record is @name_<idx>\nSEQ\n+\nQUAL\n; the consensus header is <c>name_<avgQ>_<L>_<ns>_<clen>\n
C3_PO_HD inline int c3_emit_dec_len(int32_t v) { return v < 0 ? 1 + c3_post_digits(0u - (uint32_t)v) : c3_post_digits((uint32_t)v); }
C3_PO_HD inline int64_t c3_emit_sub_len(int64_t nl, int32_t idx, int64_t len) { return nl + c3_emit_dec_len(idx) + 2 * len + 7; }
C3_PO_HD inline int c3_emit_head_tail_len(int aql, int64_t L, int32_t ns, int64_t clen) {
  return 5 + aql + c3_post_digits((uint32_t)L) + c3_emit_dec_len(ns) + c3_post_digits((uint32_t)clen);
}
C3_PO_HD inline char c3_emit_dec_char(int32_t v, int k) {
  if (v < 0) { if (k == 0) return '-'; const uint32_t u = 0u - (uint32_t)v; return c3_post_digit(u, c3_post_digits(u), k - 1); }
  return c3_post_digit((uint32_t)v, c3_post_digits((uint32_t)v), k);
}
// byte k of the header behind the name: _<avgQ>_<L>_<ns>_<clen>\n
C3_PO_HD inline char c3_emit_head_tail_char(int k, const char* aq, int aql, int64_t L, int32_t ns, int64_t clen) {
  if (k == 0) return '_';
  k -= 1; if (k < aql) return aq[k];
  k -= aql; if (k == 0) return '_';
  k -= 1; const int dl = c3_post_digits((uint32_t)L); if (k < dl) return c3_post_digit((uint32_t)L, dl, k);
  k -= dl; if (k == 0) return '_';
  k -= 1; const int dn = c3_emit_dec_len(ns); if (k < dn) return c3_emit_dec_char(ns, k);
  k -= dn; if (k == 0) return '_';
  k -= 1; const int dc = c3_post_digits((uint32_t)clen); if (k < dc) return c3_post_digit((uint32_t)clen, dc, k);
  return '\n';
}
C3_PO_HD inline int64_t c3_emit_cons_len(int kind, int64_t nl, int aql, int64_t L, int32_t ns, int64_t clen) {
  const int64_t h = 1 + nl + c3_emit_head_tail_len(aql, L, ns, clen);
  return kind == C3_EMIT_CONS_FA ? h + clen + 1 : h + 2 * clen + 4;
}

// k_emit (k_emit.hip): one group in structure-of-arrays form, its per-read records, the consensus (and QV) bytes of read i at
// cons[cons_at[i]], and what the passes hand each other.  cons_off != null: consensus length = cons_off[i+1] - cons_off[i]
// (the stand-alone call); null: status OK ? cons_len : 0 of the record (the resident batch, whose arena is indexed by off).
struct EmitHead { char aq[8]; int32_t aql, s, cons, np; };           // s: the read's splint, -1 when it writes nothing
struct EmitArgs {
  int n, n_splints, K, zero;
  const uint8_t* names; const int64_t* name_off; const uint8_t* seqs; const uint8_t* quals; const int64_t* off;
  const c3_read_result* info; const int16_t* sid;
  const uint8_t* cons; const uint8_t* qv; const int64_t* cons_at; const int64_t* cons_off;
  EmitHead* head;                       // [n]
  int64_t* len;                         // [n][C3_EMIT_KINDS] bytes the read adds to each kind of its splint
  long long* bsum;                      // [workgroups of 256 reads][S * K + 1] sums, then exclusive prefix sums; the last column counts records
  int64_t* stream_off;                  // [S * K + 2]: stream starts, total, records
  int64_t* roff;                        // [n][C3_EMIT_KINDS] arena offset of the read's bytes of each kind
  uint8_t* arena;
  int bam;                              // 1: BAM records (k_bamout.hip, c3_bamout.h; K = 2), 0: text
};

// argument and record rules shared by c3_emit_group and c3_emit_group_host (c3_emit.cpp); C3_E_OK = go on
int c3_emit_check_args(const char* who, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                       const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                       int64_t* stream_off, int64_t* n_records);

#endif

// c3_post.h -- the per-read rule of the post-processing step (include/c3poa.h "Post-processing on the GPU"),
// once, for the host statement (c3_post.cpp) and k_post (k_post.hip): which adapter hits count, where the read is cut, which
// way it is turned, where it goes, and what every record and PSL row looks like.  It states find_adapters_gpu -> PSL ->
// parse_blat -> write_fasta_file of c3poa_amd/postprocess.py.  A record is a short list of SEGMENTS (a literal, the name, a
// decimal number, a slice of the read forward or reverse-complemented, the same slice of the qualities forward or
// reversed); its length is the sum of the segment lengths.  How a segment's bytes are moved is what the two sides do each
// in their own way.  The rule is total: any int32 table entries give slices inside [0, L].
#ifndef C3_POST_H
#define C3_POST_H
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define C3_PO_HD __host__ __device__
#else
#define C3_PO_HD
#endif

#define C3_POST_MIN_SCORE 22          // MIN_SCORE of postprocess.py: a PSL row exists from this score on
#define C3_POST_MAX_IDX 16            // the limits of c3_match_index_batch
#define C3_POST_MAX_IDX_LEN 32
#define C3_POST_MAX_DEST (C3_POST_MAX_IDX + 1)
#define C3_POST_MAX_STREAMS (3 * C3_POST_MAX_DEST + 3)
#define C3_POST_REC 6                 // records of one read: main, left, right, 10x, TSV line, its PSL rows

// ---- match_index (C3POa_postprocessing.py:266-285) for one piece; k_match_index and c3_post_oligo call it --------------
// sliding Levenshtein distance against every index, the reference's quirks included (a slice that is too short for index k
// ends the loop over indexes at that position; stable order; the winner needs distance < 2 and a runner-up more than 1
// further away).  At most 16 indexes of at most 32 bases.  Same function as the host statement c3_match_index (c3_index.cpp).
template <class OFF> C3_PO_HD inline int c3_match_rule(const char* seq, int L, int n_idx, const char* idx_cat, const OFF* idx_off) {
  int best[C3_POST_MAX_IDX];
  for (int k = 0; k < C3_POST_MAX_IDX; ++k) best[k] = INT32_MAX;
  for (int p = 0; p < L; ++p) {
    for (int k = 0; k < n_idx; ++k) {
      const int len = (int)(idx_off[k + 1] - idx_off[k]);
      if (p + len > L) break;
      const char* b = idx_cat + idx_off[k];
      int prev[C3_POST_MAX_IDX_LEN + 1], cur[C3_POST_MAX_IDX_LEN + 1];
      for (int j = 0; j <= len; ++j) prev[j] = j;
      for (int i = 1; i <= len; ++i) {
        cur[0] = i;
        const char ca = seq[p + i - 1];
        for (int j = 1; j <= len; ++j) {
          int v = prev[j - 1] + (ca != b[j - 1]);
          v = v < prev[j] + 1 ? v : prev[j] + 1; v = v < cur[j - 1] + 1 ? v : cur[j - 1] + 1;
          cur[j] = v;
        }
        for (int j = 0; j <= len; ++j) prev[j] = cur[j];
      }
      best[k] = best[k] < prev[len] ? best[k] : prev[len];
    }
  }
  int i0 = -1, i1 = -1, res = -1; bool bad = false;
  for (int k = 0; k < n_idx; ++k) {
    if (best[k] == INT32_MAX) { bad = true; break; }
    if (i0 < 0 || best[k] < best[i0]) { i1 = i0; i0 = k; }
    else if (i1 < 0 || best[k] < best[i1]) i1 = k;
  }
  if (!bad && i0 >= 0 && i1 >= 0 && best[i0] < 2 && best[i1] - best[i0] > 1) res = i0;
  return res;
}

// ---- the rule ------------------------------------------------------------------------------------------------------------
struct C3PostOpt {
  int32_t n_ad, class5;                          // adapters; name class of "5Prime_adapter" (-1: absent)
  int32_t undirectional, trim, barcoded, quals;  // -u, -t, -b, --keep-quals
  int32_t has_index, n_idx, n_dest;              // -x given; index sequences; destinations (1 without -x; the last = no_index_found)
};
struct C3PostDec { int64_t p, m; int32_t kept, dir, dest, pad; };      // dir 0 = '+', 1 = '-'

// seq[a:b] of a string of length L as Python cuts it: a negative bound wraps once by +L, then both clamp to [0, L]
C3_PO_HD inline void c3_post_slice(int64_t a, int64_t b, int64_t L, int32_t* beg, int32_t* len) {
  if (a < 0) { a += L; if (a < 0) a = 0; } else if (a > L) a = L;
  if (b < 0) { b += L; if (b < 0) b = 0; } else if (b > L) b = L;
  *beg = (int32_t)a; *len = b > a ? (int32_t)(b - a) : 0;
}

// seqio._COMP: 28 characters have a complement, every other byte stays
C3_PO_HD inline uint8_t c3_post_comp(uint8_t c) {
  const char* from = "ACGTUNacgtunRYKMBDHVrykmbdhv";
  const char* to = "TGCAANtgcaanYRMKVHDByrmkvhdb";
  for (int k = 0; k < 28; ++k) if ((uint8_t)from[k] == c) return (uint8_t)to[k];
  return c;
}

// parse_blat + the adapter part of write_fasta_file: tab = this read's [n_ad][2][12] rows
C3_PO_HD inline void c3_post_adapters(const int32_t* tab, const int32_t* ad_len, const int32_t* ad_class, const C3PostOpt& o, C3PostDec* d) {
  int np = 0, nm = 0, cp = -1, cm = -1;
  int64_t p = 0, m = 0;
  for (int a = 0; a < o.n_ad; ++a)
    for (int rc = 0; rc < 2; ++rc) {
      const int32_t* e = tab + ((size_t)a * 2 + rc) * 12;
      if (e[0] < C3_POST_MIN_SCORE || e[7] >= 50 || e[5] <= 10) continue;
      const int64_t rest = (int64_t)ad_len[a] - e[4];
      if (rc == 0) { ++np; cp = ad_class[a]; p = (int64_t)e[2] + rest; }       // projected END of the adapter on the read
      else         { ++nm; cm = ad_class[a]; m = (int64_t)e[1] - rest; }       // projected START
    }
  d->p = p; d->m = m; d->dest = 0; d->pad = 0;
  d->kept = np == 1 && nm == 1 && m > p && (o.undirectional || cp != cm);
  d->dir = o.undirectional ? 0 : (cp == o.class5 ? 0 : 1);
}

// the oligo-dT part (-x): fwd = seq[p-4 : p+16], rev = revcomp(seq[m-16 : m+4]); both are at most 20 bytes
C3_PO_HD inline void c3_post_oligo(const char* seq, int32_t L, const C3PostOpt& o, const char* idx_cat, const int64_t* idx_off,
                                   const int32_t* idx_dest, C3PostDec* d) {
  char f[24], r[24];
  int32_t fb, fl, rb, rl;
  c3_post_slice(d->p - 4, d->p + 16, L, &fb, &fl);
  c3_post_slice(d->m - 16, d->m + 4, L, &rb, &rl);
  for (int j = 0; j < fl; ++j) f[j] = seq[fb + j];
  for (int j = 0; j < rl; ++j) r[j] = (char)c3_post_comp((uint8_t)seq[rb + rl - 1 - j]);
  const int kf = c3_match_rule(f, fl, o.n_idx, idx_cat, idx_off), kr = c3_match_rule(r, rl, o.n_idx, idx_cat, idx_off);
  d->dest = o.n_dest - 1;
  if (kf >= 0 && kr < 0) { d->dir = 1; d->dest = idx_dest[kf]; }
  if (kr >= 0 && kf < 0) { d->dir = 0; d->dest = idx_dest[kr]; }
}

// ---- records as segments -----------------------------------------------------------------------------------------------
enum { C3_SEG_LIT = 0, C3_SEG_NAME, C3_SEG_DEC, C3_SEG_SEQ_F, C3_SEG_SEQ_R, C3_SEG_QUAL_F, C3_SEG_QUAL_R };
enum { C3_LIT_GT = 0, C3_LIT_AT, C3_LIT_US, C3_LIT_NL, C3_LIT_PLUS, C3_LIT_MINUS, C3_LIT_SEP, C3_LIT_TAB };
struct C3PostSeg { int32_t kind, a, len; };      // a: literal number, value of the decimal, or first byte of the slice
#define C3_POST_MAX_SEG 9

C3_PO_HD inline const char* c3_post_lit(int id) {
  switch (id) {
    case C3_LIT_GT: return ">";
    case C3_LIT_AT: return "@";
    case C3_LIT_US: return "_";
    case C3_LIT_NL: return "\n";
    case C3_LIT_PLUS: return "plus\n";
    case C3_LIT_MINUS: return "minus\n";
    case C3_LIT_SEP: return "\n+\n";
    default: return "\t";
  }
}
C3_PO_HD inline int c3_post_lit_len(int id) { return id == C3_LIT_PLUS ? 5 : id == C3_LIT_MINUS ? 6 : id == C3_LIT_SEP ? 3 : 1; }
C3_PO_HD inline int c3_post_digits(uint32_t v) { int n = 1; while (v >= 10u) { v /= 10u; ++n; } return n; }
// digit j (0 = most significant) of v, which has nd digits
C3_PO_HD inline char c3_post_digit(uint32_t v, int nd, int j) { for (int k = nd - 1; k > j; --k) v /= 10u; return (char)('0' + v % 10u); }

// stream of record k of a read that goes to destination dest
C3_PO_HD inline int c3_post_stream(int k, int dest, int n_dest) { return k < 3 ? 3 * dest + k : 3 * n_dest + (k - 3); }

// segments of record k (0 main, 1 left, 2 right, 3 10x, 4 TSV line) of a read of L bytes with a name of nlen bytes;
// returns their number, 0 when the read has no such record (write_fasta_file, the lines after `seq = sequence[p_pos:m_pos]`)
C3_PO_HD inline int c3_post_plan(int k, const C3PostDec& d, int32_t L, int32_t nlen, const C3PostOpt& o, C3PostSeg* s, int64_t* total) {
  *total = 0;
  if (!d.kept || (k == 3 && !o.barcoded) || (k == 4 && !o.has_index)) return 0;
  int n = 0;
  int32_t b, l;
  if (k == 4) {                                                                  // name \t rev \t fwd \n
    s[n++] = {C3_SEG_NAME, 0, nlen};
    s[n++] = {C3_SEG_LIT, C3_LIT_TAB, 1};
    c3_post_slice(d.m - 16, d.m + 4, L, &b, &l); s[n++] = {C3_SEG_SEQ_R, b, l};
    s[n++] = {C3_SEG_LIT, C3_LIT_TAB, 1};
    c3_post_slice(d.p - 4, d.p + 16, L, &b, &l); s[n++] = {C3_SEG_SEQ_F, b, l};
    s[n++] = {C3_SEG_LIT, C3_LIT_NL, 1};
  } else {
    int32_t sb, sl;
    c3_post_slice(d.p, d.m, L, &sb, &sl);                                        // seq: its length names every record
    int rc = 0, lit = C3_LIT_NL;
    if (k == 0) {
      if (o.trim) { b = sb; l = sl; } else c3_post_slice(d.p - 40 > 0 ? d.p - 40 : 0, d.m + 40, L, &b, &l);
      rc = d.dir;
    } else if (k == 1) {                                                         // left splint file
      if (d.dir == 0) c3_post_slice(d.m, L, L, &b, &l); else { c3_post_slice(0, d.p + 40, L, &b, &l); rc = 1; }
    } else if (k == 2) {                                                         // right splint file
      if (d.dir == 0) { c3_post_slice(0, d.p, L, &b, &l); rc = 1; } else c3_post_slice(d.m, L, L, &b, &l);
    } else {                                                                     // 10x sequences
      if (d.dir == 0) { c3_post_slice(d.m - 40, d.m, L, &b, &l); rc = 1; lit = C3_LIT_PLUS; }
      else { c3_post_slice(d.p, d.p + 40, L, &b, &l); lit = C3_LIT_MINUS; }
    }
    const bool fq = o.quals && k < 3;
    s[n++] = {C3_SEG_LIT, fq ? C3_LIT_AT : C3_LIT_GT, 1};
    s[n++] = {C3_SEG_NAME, 0, nlen};
    s[n++] = {C3_SEG_LIT, C3_LIT_US, 1};
    s[n++] = {C3_SEG_DEC, sl, c3_post_digits((uint32_t)sl)};
    s[n++] = {C3_SEG_LIT, C3_LIT_NL, 1};
    s[n++] = {rc ? C3_SEG_SEQ_R : C3_SEG_SEQ_F, b, l};
    if (fq) {
      s[n++] = {C3_SEG_LIT, C3_LIT_SEP, 3};
      s[n++] = {rc ? C3_SEG_QUAL_R : C3_SEG_QUAL_F, b, l};
    }
    s[n++] = {C3_SEG_LIT, lit, c3_post_lit_len(lit)};
  }
  for (int j = 0; j < n; ++j) *total += s[j].len;
  return n;
}

// ---- PSL rows (psl_line of postprocess.py) -------------------------------------------------------------------------------
// a signed decimal at out (counted only when out is null); returns its length
C3_PO_HD inline int c3_post_put_dec(char* out, int64_t v) {
  char t[24];
  int n = 0;
  uint64_t u = v < 0 ? 0ull - (uint64_t)v : (uint64_t)v;
  do { t[n++] = (char)('0' + u % 10u); u /= 10u; } while (u);
  if (v < 0) t[n++] = '-';
  if (out) for (int j = 0; j < n; ++j) out[j] = t[n - 1 - j];
  return n;
}

// the row of table entry e (score >= C3_POST_MIN_SCORE) with its '\n'; out null: length only
C3_PO_HD inline int64_t c3_post_psl_row(char* out, const int32_t* e, const char* name, int32_t nlen, int32_t L,
                                        const char* ad, int32_t ad_nlen, int32_t ad_len, int rc) {
  int64_t n = 0;
#define C3_PSL_NUM(v) { n += c3_post_put_dec(out ? out + n : nullptr, (int64_t)(v)); }
#define C3_PSL_CH(c) { if (out) out[n] = (c); ++n; }
#define C3_PSL_STR(p, len) { if (out) for (int32_t j_ = 0; j_ < (len); ++j_) out[n + j_] = (p)[j_]; n += (len); }
  const int32_t blk = (int32_t)((uint32_t)e[2] - (uint32_t)e[1]);                // 32-bit arithmetic, as on the table's own type
  C3_PSL_NUM(e[5]) C3_PSL_CH('\t') C3_PSL_NUM(e[6]) C3_PSL_CH('\t') C3_PSL_NUM(0) C3_PSL_CH('\t') C3_PSL_NUM(0) C3_PSL_CH('\t')
  C3_PSL_NUM(e[9]) C3_PSL_CH('\t') C3_PSL_NUM(e[7]) C3_PSL_CH('\t') C3_PSL_NUM(e[10]) C3_PSL_CH('\t') C3_PSL_NUM(e[8]) C3_PSL_CH('\t')
  C3_PSL_CH(rc ? '-' : '+') C3_PSL_CH('\t') C3_PSL_STR(name, nlen) C3_PSL_CH('\t') C3_PSL_NUM(L) C3_PSL_CH('\t')
  C3_PSL_NUM(e[1]) C3_PSL_CH('\t') C3_PSL_NUM(e[2]) C3_PSL_CH('\t') C3_PSL_STR(ad, ad_nlen) C3_PSL_CH('\t') C3_PSL_NUM(ad_len) C3_PSL_CH('\t')
  C3_PSL_NUM(e[3]) C3_PSL_CH('\t') C3_PSL_NUM(e[4]) C3_PSL_CH('\t') C3_PSL_NUM(1) C3_PSL_CH('\t')
  C3_PSL_NUM(blk) C3_PSL_CH(',') C3_PSL_CH('\t') C3_PSL_NUM(e[1]) C3_PSL_CH(',') C3_PSL_CH('\t') C3_PSL_NUM(e[3]) C3_PSL_CH(',') C3_PSL_CH('\n')
#undef C3_PSL_NUM
#undef C3_PSL_CH
#undef C3_PSL_STR
  return n;
}

// k_post (k_post.hip): post-processing records.  One batch in structure-of-arrays form, its adapter table, the adapter and
// index descriptors (c3_post_args of c3poa.h, on the device), the rule's options, and what the passes hand each other.
struct PostArgs {
  int n, S; C3PostOpt o;
  const uint8_t* names; const int64_t* name_off; const uint8_t* seqs; const uint8_t* quals; const int64_t* off;
  const int32_t* table; const int32_t* ad_len; const int32_t* ad_class; const uint8_t* ad_names; const int64_t* ad_name_off;
  const uint8_t* idx_cat; const int64_t* idx_off; const int32_t* idx_dest;
  C3PostDec* dec;                       // [n] decisions
  int64_t* len;                         // [n][C3_POST_REC] record lengths: main, left, right, 10x, TSV line, PSL rows
  long long* bsum;                      // [workgroups of 256 reads][S + 1] sums, then exclusive prefix sums; column S = kept reads
  int64_t* stream_off;                  // [S + 2]: stream starts, total, kept reads
  int64_t* roff;                        // [n][C3_POST_REC] arena offset of every record
  uint8_t* arena;
};

// argument rules shared by c3_post_emit and c3_post_emit_host (c3_post.cpp); C3_E_OK = go on
struct c3_post_args;
int c3_post_check_args(const char* who, const c3_post_args* a, char* arena, int64_t cap, int64_t* stream_off, int64_t* n_kept);

#endif

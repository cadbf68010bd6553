// c3_bamout.h -- the record rule of --bam (include/c3poa.h "Records written as unaligned BAM"), once, for the host
// statement (c3_bamout.cpp) and k_bamout (k_bamout.hip).  Which reads write which records, in which order and from which slice is
// c3_emit.h (c3_emit_of, c3_emit_piece) and is not restated here; the text of a consensus record's name is the FASTA header's
// (c3_emit_avgq, c3_emit_head_tail_char).  This file says what one BAM record is made of and how long it is.
//
// Two kinds per splint, stream s * 2 + kind: C3_BAMOUT_CONS (= C3_EMIT_CONS_FA's slot) and C3_BAMOUT_SUB (= C3_EMIT_SUB_FQ's), so the
// scans of k_emit serve with K = 2.  One record, every field little-endian and none of them aligned:
//   block_size | refID -1 | pos -1 | l_read_name | mapq 0 | bin 4680 | n_cigar_op 0 | flag 4 | l_seq | next_refID -1 | next_pos -1 |
//   tlen 0 | read_name NUL | seq, two bases per byte, high nibble first | qual | tags (consensus only: np:i rl:i aq:f)
#ifndef C3_BAMOUT_H
#define C3_BAMOUT_H
#include "c3_emit.h"

enum { C3_BAMOUT_CONS = 0, C3_BAMOUT_SUB = 1 };
#define C3_BAMOUT_FIXED 36              // block_size .. tlen
#define C3_BAMOUT_TAGS 21               // three tags of 2 + 1 + 4 bytes
#define C3_BAMOUT_MAX_NAME 219          // 254 name bytes a record can hold - the longest suffix (_<avgQ>_<L>_<ns>_<clen>: 4 + 7 + 10 + 3 + 10 at most)
#define C3_BAMOUT_NOQUAL 0xFFu          // a consensus without QVs: l_seq bytes of 0xFF

// the 4-bit code of a base: its index in "=ACMGRSVTWYHKDBN", a lower-case letter as its upper-case form, any other byte 15 (N)
C3_PO_HD inline uint32_t c3_bamout_code(uint32_t c) {
  const char* t = "=ACMGRSVTWYHKDBN";
  if (c >= 'a' && c <= 'z') c -= 32u;
  for (uint32_t k = 0; k < 16u; ++k) if (c == (uint32_t)(uint8_t)t[k]) return k;
  return 15u;
}
// a quality byte of the text (phred + 33) as BAM stores it
C3_PO_HD inline uint32_t c3_bamout_qual(uint32_t b) { return b < 33u ? 0u : b > 126u ? 93u : b - 33u; }

// dword k (0 .. 8) of the 36 fixed bytes
C3_PO_HD inline uint32_t c3_bamout_fixed(int k, uint32_t block_size, uint32_t l_read_name, uint32_t l_seq) {
  return k == 0 ? block_size : k == 3 ? (l_read_name | 4680u << 16) : k == 4 ? 4u << 16 : k == 5 ? l_seq : k == 8 ? 0u : 0xFFFFFFFFu;
}

// record lengths (block_size + 4).  A subread's name is <name>_<idx>; a consensus's <name>_<avgQ>_<L>_<ns>_<clen>, whose bytes
// behind <name> are the FASTA header's without its newline (ht = c3_emit_head_tail_len counts that newline: here it is the NUL)
C3_PO_HD inline int64_t c3_bamout_sub_len(int64_t nl, int32_t idx, int64_t len) {
  return C3_BAMOUT_FIXED + nl + 1 + c3_emit_dec_len(idx) + 1 + (len + 1) / 2 + len;
}
C3_PO_HD inline int64_t c3_bamout_cons_len(int64_t nl, int ht, int64_t clen) {
  return C3_BAMOUT_FIXED + nl + ht + (clen + 1) / 2 + clen + C3_BAMOUT_TAGS;
}
// byte k (0 .. 20) of the tags: np:i = ns as the header prints it, rl:i = L, aq:f = (float)((double)tot / (double)L)
C3_PO_HD inline uint8_t c3_bamout_tag_byte(int k, int32_t ns, int64_t L, int64_t tot) {
  const int t = k / 7, b = k % 7;
  if (b < 3) return (uint8_t)("npirliaqf"[3 * t + b]);
  uint32_t v;
  if (t == 0) v = (uint32_t)ns;
  else if (t == 1) v = (uint32_t)L;
  else { union { float f; uint32_t u; } cv; cv.f = (float)((double)tot / (double)(L > 0 ? L : 1)); v = cv.u; }
  return (uint8_t)(v >> (8 * (b - 3)));
}

// names: at most C3_BAMOUT_MAX_NAME bytes (C3_E_LIMIT) and no NUL (C3_E_ARG), decided from the names alone before any launch, for
// every read of the group; the error text names the read.  C3_E_OK = go on.  (c3_bamout.cpp)
int c3_bamout_check_names(const char* who, const char* names, const int64_t* name_off, int n);

#endif

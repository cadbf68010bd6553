// c3_fastx.h -- the strict record rule of the post-processing input (include/c3poa.h "Strict FASTA / FASTQ records";
// DESIGN.md 5.9), once, for the host statement (c3_fastx.cpp) and whatever applies it on the device: a text is a sequence of
// records of KIND lines each, kind 4 being the four-line FASTQ of c3_fastq.h and kind 2 the two-line FASTA that C3POa.py
// writes.  The '\r' rule and the name rule are those of c3_fastq.h; finding the lines and moving the bytes is the caller's.
#ifndef C3_FASTX_H
#define C3_FASTX_H
#include "c3_fastq.h"
#include "c3_fasta.h"

// the kind a file's first byte announces; 0: neither, which is a departure
C3_FQ_HD inline int c3_fastx_kind_of(char first) { return first == '@' ? 4 : (first == '>' ? 2 : 0); }

// Is the record whose `kind` lines are [b[k], e[k]) ('\r' already stripped) strict?  Kind 4: c3_fastq_strict.  Kind 2: line 0
// begins with '>'; line 1 is not empty and does not begin with '>', '@' or '+'.
template <class I> C3_FQ_HD inline bool c3_fastx_strict(const char* t, int kind, const I* b, const I* e) {
  if (kind == 4) return c3_fastq_strict(t, b, e);
  if (e[0] == b[0] || t[b[0]] != '>') return false;
  if (e[1] == b[1]) return false;
  const char c = t[b[1]];
  return !(c == '>' || c == '@' || c == '+');
}

// a byte >= 0x80 in [b, e): such a record is no strict record of either kind (Python cuts characters, the device bytes)
template <class I> C3_FQ_HD inline bool c3_fastx_has_high(const char* t, I b, I e) {
  for (I k = b; k < e; ++k) if ((uint8_t)t[k] >= 0x80) return true;
  return false;
}

// the hash of c3_fasta_parse over the name bytes (line 0 after its first byte, up to the first blank or tab)
template <class I> C3_FQ_HD inline uint64_t c3_fastx_name_hash(const char* t, I name_begin, I name_len) {
  return c3_fasta_hash((const uint8_t*)t + name_begin, (int64_t)name_len);
}

#if defined(__HIPCC__)
// what k_fastx leaves for the host after its scans (c3_text.hip reads it back)
struct C3FxHdr {
  uint32_t first_bad;             // atomicMin of k_fastx_records: first candidate record that is not strict (UINT32_MAX: none)
  uint32_t first_high;            // atomicMin of k_fastx_high: first byte >= 0x80 of the text (UINT32_MAX: none)
  int32_t departed, max_len;      // max_len: longest sequence among the records
  int64_t n_records, consumed, name_bytes, base_bytes, words;      // words: 2-bit words of the pack k_adapter reads
};

// device pointers of one k_fastx pass (the launchers of k_fastx.hip take it by pointer; filled by c3_text.hip)
struct FxArgs {
  const uint8_t* buf; uint32_t hi; int32_t kind;        // the text is buf[0, hi), 256 bytes of slack behind it
  const int32_t* nl; int32_t L;                         // [L] positions of '\n' (k_fastq_lines); line L, if any, ends at hi
  int32_t n_full, partial;                              // whole candidate records; one more, incomplete, at the end of the file
  int32_t* slen; int32_t* nlen;                         // [n_full] sequence and name length of every candidate
  long long* bsum;                                      // [4 * (blocks + 1)] sums of the scans: bases, name bytes, words, longest
  C3FxHdr* hdr;
  int64_t* off; int64_t* name_off; int64_t* woff;       // [n_records + 1]; woff = word offsets of the 2-bit pack (c3_batch_stage)
  int4* src; uint64_t* hash;                            // [n_records] text positions of sequence, quality, name; FNV-1a of the name
  long long n_records;
  uint8_t* names; uint8_t* seqs; uint8_t* quals;        // the arenas of the gather; quals null: not gathered
};
#endif

#endif

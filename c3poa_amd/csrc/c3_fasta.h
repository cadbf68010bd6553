// c3_fasta.h -- the FASTA rule of the sample demultiplexer (include/c3poa.h "Sample demultiplexer, text in / file bytes out";
// DESIGN.md 5.7), once, for the host statements (c3_fasta.cpp) and k_fasta (k_fasta.hip): read_fasta of
// paper/Demultiplex_R2C2_reads.py / c3poa_amd/demux.py stated for ASCII bytes -- where a line ends, what is stripped, the kind
// of a line, the name hash, which records a text delivers and the length of an output record.  Finding the lines, the prefix
// sums and the byte moves are what the two sides do each in their own way.
#ifndef C3_FASTA_H
#define C3_FASTA_H
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define C3_FA_HD __host__ __device__
#else
#define C3_FA_HD
#endif

enum { C3_FA_BLANK = 0, C3_FA_HEADER = 1, C3_FA_SEQ = 2 };

// a line ends at every '\n' and at every '\r', each on its own (the empty line between "\r" and "\n" is blank)
C3_FA_HD inline bool c3_fasta_is_term(uint8_t c) { return c == '\n' || c == '\r'; }
// what str.rstrip() takes off an ASCII line: 9..13 and 28..32
C3_FA_HD inline bool c3_fasta_is_strip(uint8_t c) { return (c >= 9 && c <= 13) || (c >= 28 && c <= 32); }

// end of the line [b, e) after stripping (nothing is stripped at the front)
template <class I> C3_FA_HD inline I c3_fasta_strip_end(const uint8_t* t, I b, I e) {
  while (e > b && c3_fasta_is_strip(t[e - 1])) --e;
  return e;
}
// kind of the stripped line [b, se)
template <class I> C3_FA_HD inline int c3_fasta_kind(const uint8_t* t, I b, I se) {
  return se == b ? C3_FA_BLANK : (t[b] == '>' ? C3_FA_HEADER : C3_FA_SEQ);
}

// 64-bit FNV-1a of the name bytes
#define C3_FNV_BASIS 1469598103934665603ull
#define C3_FNV_PRIME 1099511628211ull
C3_FA_HD inline uint64_t c3_fasta_hash(const uint8_t* p, int64_t n) {
  uint64_t h = C3_FNV_BASIS;
  for (int64_t i = 0; i < n; ++i) { h ^= p[i]; h *= C3_FNV_PRIME; }
  return h;
}

// What a text of n bytes with H header lines delivers.  first_high: position of the first byte >= 0x80 (< 0: none);
// first_headless: first byte of the first non-blank sequence line in front of the first header (< 0: none);
// rec_of_high: number of the record (header line included) that holds first_high, -1 in front of the first header.
// The last record stays unconsumed unless at_eof; a departure delivers the records wholly in front of the offending byte.
struct C3FaVerdict { int64_t n_records; int32_t departed; };
C3_FA_HD inline C3FaVerdict c3_fasta_verdict(int64_t H, int at_eof, int64_t first_high, int64_t first_headless, int64_t rec_of_high) {
  C3FaVerdict v;
  v.n_records = at_eof ? H : (H > 0 ? H - 1 : 0);
  v.departed = 0;
  if (first_headless >= 0 && (first_high < 0 || first_headless <= first_high)) { v.departed = 2; v.n_records = 0; }
  else if (first_high >= 0) {
    v.departed = 1;
    const int64_t r = rec_of_high < 0 ? 0 : rec_of_high;
    if (r < v.n_records) v.n_records = r;
  }
  return v;
}
// bytes consumed: up to the header line of the first record that is not delivered (hb_next: its first byte; only read when
// n_records < H), everything when all is delivered at the end of the file
C3_FA_HD inline int64_t c3_fasta_consumed(const C3FaVerdict& v, int64_t H, int at_eof, int64_t n, int64_t hb_next) {
  if (v.departed == 2) return 0;
  if (v.n_records < H) return hb_next;
  return (at_eof && !v.departed) ? n : 0;
}

// '>' name '|' A '_' B '\n' sequence '\n'
C3_FA_HD inline int64_t c3_demux_rec_len(int64_t name_len, int64_t seq_len, int64_t a_len, int64_t b_len) {
  return 1 + name_len + 1 + a_len + 1 + b_len + 1 + seq_len + 1;
}
// ... and with qualities (C3_DEMUX_KEEP_QUALS): '@' name '|' A '_' B '\n' sequence '\n' '+' '\n' quality '\n'
C3_FA_HD inline int64_t c3_demux_rec_len(int64_t name_len, int64_t seq_len, int64_t a_len, int64_t b_len, int quals) {
  return c3_demux_rec_len(name_len, seq_len, a_len, b_len) + (quals ? 2 + seq_len + 1 : 0);
}

// what k_fasta leaves for the host after its scans (c3_scans.hip reads it back)
struct C3FaHdr {
  uint32_t first_high;            // atomicMin of k_fasta_count (UINT32_MAX: none)
  uint32_t first_headless;        // atomicMin of k_fasta_lfin (UINT32_MAX: none)
  int32_t rec_of_high;            // written by the lane whose line holds first_high
  int32_t n_term;                 // '\n' and '\r' in the text
  int32_t departed, pad;
  int64_t n_headers, n_records, consumed, name_bytes, base_bytes, n_kept, out_bytes;
};

// device pointers of one k_fasta pass (the launchers of k_fasta.hip take it by pointer; filled by c3_scans.hip)
struct FaArgs {
  const uint8_t* buf; uint32_t hi; int32_t at_eof;      // the text is buf[0, hi), 256 bytes of slack behind it
  int32_t* cnt;                                         // [4 * tiles] terminator counts per wave, then their exclusive sums
  int32_t* nl; int32_t T;                               // [T] terminator positions; lines 0 .. T (line T ends at hi)
  int32_t* lse; uint32_t* ldst;                         // [T + 1] stripped end of every line; place of a sequence line in seqs
  long long* bsum;                                      // [3 * (blocks + 1)] sums of the scans
  C3FaHdr* hdr;
  int64_t* off; int64_t* name_off; int32_t* rec_line; uint64_t* hash;      // [H + 1] per record; rec_line = its header line
  uint8_t* names; uint8_t* seqs;                        // the arenas of c3_fasta_parse
  // c3_demux_emit
  long long n_records, n_kept;
  int32_t* krec;                                        // [n_kept] record number of every kept record
  uint8_t* heads; const int32_t* win;                   // k_demux's slots and winners
  const uint8_t* a_names; const int64_t* a_no; const uint8_t* b_names; const int64_t* b_no;
  int64_t* roff; uint8_t* out;                          // [n_kept] place of every output record in out
};

#endif

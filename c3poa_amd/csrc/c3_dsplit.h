// c3_dsplit.h -- the stream rule of the demultiplexer's text path (include/c3poa.h "Sample demultiplexer, pieces of text in /
// per-sample streams out"), once, for the host statement (c3_dsplit.cpp) and k_dsplit (k_dsplit.hip): which
// records are written, into which stream, and how long an output record is (c3_demux_rec_len of c3_fasta.h).  The placement
// sums and the byte moves are what the two sides do each in their own way.
#ifndef C3_DSPLIT_H
#define C3_DSPLIT_H
#include "c3_fasta.h"

#define C3_DS_HEAD 300                  // C3_DEMUX_HEAD: a record is written when its sequence is longer
#define C3_DS_TILE 256                  // kept records per placement tile

C3_FA_HD inline bool c3_dsplit_kept(int64_t seq_len) { return seq_len > C3_DS_HEAD; }
// stream of a record whose winners are wa / wb (-1: none); one stream without split
C3_FA_HD inline int32_t c3_dsplit_stream(int32_t wa, int32_t wb, int32_t n_a, int32_t n_b, int split) {
  return split ? (wa < 0 ? n_a : wa) * (n_b + 1) + (wb < 0 ? n_b : wb) : 0;
}
C3_FA_HD inline int64_t c3_dsplit_index_len(const int64_t* no, int32_t w) { return w < 0 ? 0 : no[w + 1] - no[w]; }

#if defined(__HIPCC__)
// device pointers of one k_dsplit pass (the launchers of k_dsplit.hip take it by pointer; filled by c3_dtext.hip).  Every source
// array (names, seqs, quals, a_names, b_names) has at least 16 bytes of slack behind it.
struct DsArgs {
  long long n_records, n_kept;                          // parsed records; of them kept (k_dsplit_krec counts when it makes krec)
  const int64_t* off; const int64_t* name_off;          // [n_records + 1] into seqs / quals and names
  const uint8_t* names; const uint8_t* seqs; const uint8_t* quals;      // quals null: FASTA records out
  int32_t* krec;                                        // [n_kept] record number of every kept record, ascending
  long long* bsum; long long* n_kept_out;               // k_dsplit_krec: block sums [(n_records + 255) / 256 + 1]; the count
  const int32_t* win;                                   // [n_kept][2] winners of k_demux
  int32_t n_a, n_b, split, S;                           // S streams: 1, or (n_a + 1) * (n_b + 1)
  const uint8_t* a_names; const int64_t* a_no; const uint8_t* b_names; const int64_t* b_no;
  int32_t* key; int64_t* rank;                          // [n_kept] stream; bytes of earlier records of that stream in the tile
  int64_t* base; int32_t tiles;                         // [tiles][S] bytes per tile and stream, then their exclusive column sums
  int64_t* stream_off;                                  // [S + 1]
  uint8_t* out;
};
#endif

#endif

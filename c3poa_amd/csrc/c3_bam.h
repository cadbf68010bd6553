// c3_bam.h -- the rule of one unaligned BAM record (include/c3poa.h "Unaligned BAM records on the GPU"), once,
// for the host statement (c3_bam.cpp), the reader (c3_reader.cpp) and k_bam (k_bam.hip): the file header's extent, the strictness
// test of the record at a byte, the chain step, the name cut and the two byte maps.  Finding the record starts in parallel,
// the prefix sums and the byte moves are what the two sides do each in their own way.
#ifndef C3_BAM_H
#define C3_BAM_H
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define C3_BAM_HD __host__ __device__
#else
#define C3_BAM_HD
#endif

#ifndef C3_BAM_MAX_RECORD
#define C3_BAM_MAX_RECORD (1 << 28)
#endif
#ifndef C3_BAM_MAX_REFS
#define C3_BAM_MAX_REFS (1 << 20)      // references in the file header (an unaligned BAM has none); more is a departure (HEADER)
#endif
#define C3_BAM_MIN_BLOCK 34           // the 32 fixed bytes and two more; what a record needs beyond that is the FIELDS check

// why a record is not strict, in the order the checks are made (c3_bam_info.reason; 0 = strict)
enum { C3_BAM_OK = 0, C3_BAM_BLOCK = 1, C3_BAM_NAME = 2, C3_BAM_FIELDS = 3, C3_BAM_FLAG = 4, C3_BAM_EMPTY = 5, C3_BAM_NOQUAL = 6,
       C3_BAM_TRUNCATED = 7, C3_BAM_HEADER = 8,
       C3_BAM_INCOMPLETE = 100 };      // (internal: the record does not end inside the data; TRUNCATED once at_eof is set)

C3_BAM_HD inline uint32_t c3_bam_u16(const uint8_t* d, int64_t p) { return (uint32_t)d[p] | ((uint32_t)d[p + 1] << 8); }
C3_BAM_HD inline uint32_t c3_bam_u32(const uint8_t* d, int64_t p) {
  return (uint32_t)d[p] | ((uint32_t)d[p + 1] << 8) | ((uint32_t)d[p + 2] << 16) | ((uint32_t)d[p + 3] << 24);
}
C3_BAM_HD inline bool c3_bam_block_ok(uint32_t bs) { return bs >= C3_BAM_MIN_BLOCK && bs <= (uint32_t)C3_BAM_MAX_RECORD; }

// The file header at d[p0 .. end): magic, l_text, text, n_ref, per reference l_name, name, l_ref; skipped, not interpreted.
// Returns C3_BAM_OK with *next = the byte behind it, C3_BAM_INCOMPLETE when it does not end inside the data, C3_BAM_HEADER
// for a wrong magic, a negative length or n_ref > C3_BAM_MAX_REFS.  A reference takes 8 bytes at least, so a header whose
// n_ref exceeds an eighth of the bytes behind it cannot end inside the data: that is INCOMPLETE before any reference is looked
// at.  The reference loop (one dependent load per round, on one lane in k_bam_header) therefore runs only over a header the
// data can hold, and never more than C3_BAM_MAX_REFS rounds.
C3_BAM_HD inline int c3_bam_header(const uint8_t* d, int64_t p0, int64_t end, int64_t* next) {
  const int64_t have = end - p0;
  const uint8_t magic[4] = {'B', 'A', 'M', 1};
  for (int k = 0; k < 4 && k < have; ++k) if (d[p0 + k] != magic[k]) return C3_BAM_HEADER;
  if (have < 8) return C3_BAM_INCOMPLETE;
  const int32_t l_text = (int32_t)c3_bam_u32(d, p0 + 4);
  if (l_text < 0) return C3_BAM_HEADER;
  int64_t p = p0 + 8 + (int64_t)l_text;
  if (p + 4 > end) return C3_BAM_INCOMPLETE;
  const int32_t n_ref = (int32_t)c3_bam_u32(d, p);
  if (n_ref < 0 || n_ref > C3_BAM_MAX_REFS) return C3_BAM_HEADER;
  p += 4;
  if ((int64_t)n_ref > (end - p) / 8) return C3_BAM_INCOMPLETE;
  for (int64_t i = 0; i < (int64_t)n_ref; ++i) {
    if (p + 4 > end) return C3_BAM_INCOMPLETE;
    const int32_t l_name = (int32_t)c3_bam_u32(d, p);
    if (l_name < 0) return C3_BAM_HEADER;
    p += 4 + (int64_t)l_name + 4;
    if (p > end) return C3_BAM_INCOMPLETE;
  }
  *next = p;
  return C3_BAM_OK;
}

// what the rule says about the record at d[p]: where its parts lie (offsets into d) and how long they are
struct C3BamRec {
  int64_t next;                      // the next record: p + 4 + block_size (set whenever BLOCK passes)
  int64_t name, seq, qual;           // read_name, packed bases, qualities
  uint32_t l_seq, name_len;          // bases; bytes of the delivered name
};

// The record at d[p], with the data ending at `end`.  C3_BAM_OK: strict, every field of *r set.  C3_BAM_INCOMPLETE: it does
// not end inside the data (block_size itself cut, or p + 4 + block_size > end).  Otherwise the first check that fails, in
// the order BLOCK, NAME, FIELDS, FLAG, EMPTY, NOQUAL.  The name's last byte is looked at only where it lies inside the record
// (32 + l_read_name <= block_size); where it does not, FIELDS fails.  No byte outside [p, p + 4 + block_size) is read.
C3_BAM_HD inline int c3_bam_record(const uint8_t* d, int64_t p, int64_t end, C3BamRec* r) {
  if (p + 4 > end) return C3_BAM_INCOMPLETE;
  const uint32_t bs = c3_bam_u32(d, p);
  if (!c3_bam_block_ok(bs)) return C3_BAM_BLOCK;
  r->next = p + 4 + (int64_t)bs;
  if (r->next > end) return C3_BAM_INCOMPLETE;
  const uint32_t lrn = d[p + 12], nc = c3_bam_u16(d, p + 16), flag = c3_bam_u16(d, p + 18), ls = c3_bam_u32(d, p + 20);
  if (lrn == 0 || (32u + lrn <= bs && d[p + 36 + lrn - 1] != 0)) return C3_BAM_NAME;
  const uint64_t need = 32ull + lrn + 4ull * nc + ((uint64_t)ls + 1) / 2 + (uint64_t)ls;
  if (need > (uint64_t)bs) return C3_BAM_FIELDS;
  if (flag & (0x10u | 0x100u | 0x800u)) return C3_BAM_FLAG;
  if (ls == 0) return C3_BAM_EMPTY;
  r->name = p + 36;
  r->seq = r->name + lrn + 4 * (int64_t)nc;
  r->qual = r->seq + ((int64_t)ls + 1) / 2;
  if (d[r->qual] == 0xFF) return C3_BAM_NOQUAL;
  r->l_seq = ls;
  uint32_t k = 0;                    // the name: up to the first NUL, blank or tab (the cut of the FASTQ rule)
  while (k < lrn && d[r->name + k] != 0 && d[r->name + k] != ' ' && d[r->name + k] != '\t') ++k;
  r->name_len = k;
  return C3_BAM_OK;
}

// the two byte maps
C3_BAM_HD inline uint8_t c3_bam_base(uint32_t code) { return (uint8_t)"=ACMGRSVTWYHKDBN"[code & 15u]; }
C3_BAM_HD inline uint8_t c3_bam_qual(uint32_t q) { return (uint8_t)((q < 93u ? q : 93u) + 33u); }
// base i of the packed bases at s: high nibble first
C3_BAM_HD inline uint8_t c3_bam_base_at(const uint8_t* s, int64_t i) { const uint32_t b = s[i >> 1]; return c3_bam_base((i & 1) ? b : b >> 4); }

// what k_bam leaves for the host after its passes (c3_stream.hip reads it back; positions are buffer offsets, consumed and
// bad_at are relative to the data's first byte)
struct C3BamHdr {
  int32_t hstat;                     // the file header: C3_BAM_OK / _INCOMPLETE / _HEADER (OK without at_start)
  int32_t first_bad;                 // first record start that is not strict or not whole (INT32_MAX: none)
  int32_t departed, reason;
  int64_t start;                     // the first record's byte
  int64_t chain_end;                 // where the chain left the data (the byte behind the last whole record when all are strict)
  int64_t n_starts;                  // record starts in the data
  int64_t n_records, n_kept, n_short, consumed, name_bytes, base_bytes, bad_at;
};

// one chain tile of k_bam (C3_BAM_TILE bytes of the buffer): what the tile's wave found from its guess, and what the chain
// made of it.  Positions are 32-bit buffer offsets (C3_FASTQ_MAX_TEXT + one record stays below 2^32).
#define C3_BAM_NONE 0xFFFFFFFFu
struct C3BamTile {
  uint32_t guess, gexit;             // the first plausible record header of the tile (NONE: none) and where the walk from it left the tile
  int32_t gcnt, gstop;               // record starts on that walk; 1 when it ended at a start that has no whole, valid block_size
  uint32_t first;                    // the true first record start of the tile (NONE: it holds none)
  int32_t cnt, base, pad;            // true record starts in the tile; starts in the tiles in front of it
};

#endif

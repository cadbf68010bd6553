// c3_fastq.h -- the strict four-line FASTQ rule (include/c3poa.h "FASTQ records on the GPU"), once, for the
// host statement (c3_fastq.cpp) and k_fastq (k_fastq.hip): the strictness test of one record given its four line extents,
// the '\r' rule and the name rule.  Finding the lines, the prefix sums and the byte moves are what the two sides do each in
// their own way.
#ifndef C3_FASTQ_H
#define C3_FASTQ_H
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define C3_FQ_HD __host__ __device__
#else
#define C3_FQ_HD
#endif

// a line [b, e) as found between two '\n': one '\r' directly before the '\n' is not part of it
template <class I> C3_FQ_HD inline I c3_fastq_line_end(const char* t, I b, I e) { return (e > b && t[e - 1] == '\r') ? e - 1 : e; }

// Is the record whose four lines are [b[k], e[k]) ('\r' already stripped) strict?  Line 0 begins with '@'; line 1 is not
// empty and does not begin with '@', '>' or '+'; line 2 begins with '+'; line 3 is as long as line 1.
template <class I> C3_FQ_HD inline bool c3_fastq_strict(const char* t, const I* b, const I* e) {
  if (e[0] == b[0] || t[b[0]] != '@') return false;
  if (e[1] == b[1]) return false;
  const char c = t[b[1]];
  if (c == '@' || c == '>' || c == '+') return false;
  if (e[2] == b[2] || t[b[2]] != '+') return false;
  return e[3] - b[3] == e[1] - b[1];
}

// bytes of the name: line 0 after its '@', up to the first blank or tab
template <class I> C3_FQ_HD inline I c3_fastq_name_len(const char* t, I b, I e) {
  I k = b + 1;
  while (k < e && t[k] != ' ' && t[k] != '\t') ++k;
  return k - (b + 1);
}

// what k_fastq leaves for the host after its scans (c3_stream.hip reads it back; consumed is relative to the text's start)
struct C3FqHdr {
  int32_t n_lines;                // '\n' in the text
  int32_t n_lines_v;              // ... plus one when at_eof and the text does not end in '\n' (the unterminated last line)
  int32_t first_bad;              // first candidate record that is not strict (INT32_MAX: none)
  int32_t departed;
  int64_t n_records, n_kept, n_short, consumed, name_bytes, base_bytes;
};

#endif

// c3_fastq.cpp -- host statement of k_fastq (include/c3poa.h "FASTQ records on the GPU"): the longest prefix
// of whole strict records of a text, walked record by record on one thread with the rule of c3_fastq.h, which k_fastq
// applies as well.  The tests hold this against a parser of their own, and cut or edited text can be thrown at it under a
// sanitizer on the CPU.
#include "../../include/c3poa.h"
#include "c3_fastq.h"
#include "c3_checks.h"
#include <cstring>

// argument rules shared with c3_fastq_parse (c3_stream.hip); 0 = go on
int c3_fastq_check_args(const char* who, const char* text, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                        const char* seqs, const char* quals, int64_t bases_cap, const int64_t* off, int64_t max_records,
                        c3_fastq_info* info) {
  if (info) memset(info, 0, sizeof *info);
  char buf[96];
  if (!info || n < 0 || (n > 0 && !text) || !names || !name_off || !seqs || !quals || !off || names_cap < 0 || bases_cap < 0 || max_records < 0) {
    strcpy(buf, who); strcat(buf, ": bad arguments"); c3_set_host_error(buf); return C3_E_ARG;
  }
  if (n > C3_FASTQ_MAX_TEXT) { strcpy(buf, who); strcat(buf, ": text longer than C3_FASTQ_MAX_TEXT"); c3_set_host_error(buf); return C3_E_LIMIT; }
  return C3_E_OK;
}

extern "C" int c3_fastq_parse_host(const char* text, int64_t n, int at_eof, int min_len, char* names, int64_t names_cap,
                                   int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off,
                                   int64_t max_records, c3_fastq_info* info) {
  const int rc = c3_fastq_check_args("c3_fastq_parse_host", text, n, names, names_cap, name_off, seqs, quals, bases_cap, off, max_records, info);
  if (rc) return rc;
  // pass 0 counts, pass 1 (only when everything fits) writes: nothing is half written on C3_E_LIMIT
  for (int pass = 0; pass < 2; ++pass) {
    c3_fastq_info f; memset(&f, 0, sizeof f);
    int64_t p = 0;
    while (p < n || (at_eof && p == n)) {
      int64_t b[4], e[4], q = p;
      int have = 0;
      for (; have < 4; ++have) {
        const char* nl = q < n ? (const char*)memchr(text + q, '\n', (size_t)(n - q)) : nullptr;
        if (!nl && !(at_eof && q < n)) break;                 // (with at_eof the last line may lack its '\n')
        const int64_t end = nl ? (int64_t)(nl - text) : n;
        b[have] = q; e[have] = c3_fastq_line_end(text, q, end);
        q = nl ? end + 1 : n + 1;                              // n + 1: nothing follows the unterminated line
      }
      if (have < 4) {
        if (at_eof && have > 0) f.departed = 1;               // an incomplete record at the end of the file
        break;                                                // otherwise: left unconsumed
      }
      if (!c3_fastq_strict(text, b, e)) { f.departed = 1; break; }
      p = q > n ? n : q;
      ++f.n_records;
      const int64_t sl = e[1] - b[1];
      if (sl < (int64_t)min_len) { ++f.n_short; continue; }
      const int64_t nl = c3_fastq_name_len(text, b[0], e[0]);
      if (pass) {
        memcpy(names + f.name_bytes, text + b[0] + 1, (size_t)nl);
        memcpy(seqs + f.base_bytes, text + b[1], (size_t)sl);
        memcpy(quals + f.base_bytes, text + b[3], (size_t)sl);
        name_off[f.n_kept] = f.name_bytes; off[f.n_kept] = f.base_bytes;
      }
      ++f.n_kept; f.name_bytes += nl; f.base_bytes += sl;
      if (p == n && at_eof) break;
    }
    f.consumed = p;
    *info = f;
    if (f.n_kept > max_records || f.name_bytes > names_cap || f.base_bytes > bases_cap) {
      c3_set_host_error("c3_fastq_parse_host: capacity too small (needed sizes in info)");
      return C3_E_LIMIT;
    }
    if (pass) { name_off[f.n_kept] = f.name_bytes; off[f.n_kept] = f.base_bytes; }
  }
  return C3_E_OK;
}

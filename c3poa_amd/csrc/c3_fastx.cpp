// c3_fastx.cpp -- host statement of the strict record parser of the post-processing input (include/c3poa.h "Strict FASTA /
// FASTQ records"): the longest prefix of whole strict records of one kind, walked record by record on one
// thread with the rule of c3_fastx.h.  The tests hold it against seqio.fastx_read, and cut or edited text can be thrown at it
// under a sanitizer on the CPU (tools/post_text_fuzz_host.sh).
#include "../../include/c3poa.h"
#include "c3_fastx.h"
#include "c3_checks.h"
#include <cstring>

static int fx_bad(const char* what, int code) {
  char buf[128];
  strcpy(buf, "c3_fastx_strict_parse_host: "); strcat(buf, what); c3_set_host_error(buf);
  return code;
}

extern "C" int c3_fastx_strict_parse_host(const char* text, int64_t n, int at_eof, int kind, char* names, int64_t names_cap,
                                          int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off,
                                          uint64_t* name_hash, int64_t max_records, c3_fastx_info* info) {
  if (info) memset(info, 0, sizeof *info);
  if (!info || n < 0 || (n > 0 && !text) || (kind != 2 && kind != 4) || !names || !name_off || !seqs || (kind == 4 && !quals) || !off ||
      !name_hash || names_cap < 0 || bases_cap < 0 || max_records < 0)
    return fx_bad("bad arguments", C3_E_ARG);
  if (n > C3_FASTX_MAX_TEXT) return fx_bad("text longer than C3_FASTX_MAX_TEXT", C3_E_LIMIT);
  // pass 0 counts, pass 1 (only when everything fits) writes: nothing is half written on C3_E_LIMIT
  for (int pass = 0; pass < 2; ++pass) {
    c3_fastx_info f; memset(&f, 0, sizeof f);
    int64_t p = 0;
    while (p < n || (at_eof && p == n)) {
      int64_t b[4], e[4], q = p, raw_end = p;
      int have = 0;
      for (; have < kind; ++have) {
        const char* nl = q < n ? (const char*)memchr(text + q, '\n', (size_t)(n - q)) : nullptr;
        if (!nl && !(at_eof && q < n)) break;                 // (with at_eof the last line may lack its '\n')
        raw_end = nl ? (int64_t)(nl - text) : n;
        b[have] = q; e[have] = c3_fastq_line_end(text, q, raw_end);
        q = nl ? raw_end + 1 : n + 1;                          // n + 1: nothing follows the unterminated line
      }
      if (have < kind) {
        if (at_eof && have > 0) f.departed = 1;               // an incomplete record at the end of the file
        break;                                                // otherwise: left unconsumed
      }
      if (!c3_fastx_strict(text, kind, b, e) || c3_fastx_has_high(text, b[0], raw_end)) { f.departed = 1; break; }
      p = q > n ? n : q;
      const int64_t sl = e[1] - b[1], nl = c3_fastq_name_len(text, b[0], e[0]);
      if (pass) {
        memcpy(names + f.name_bytes, text + b[0] + 1, (size_t)nl);
        memcpy(seqs + f.base_bytes, text + b[1], (size_t)sl);
        if (kind == 4) memcpy(quals + f.base_bytes, text + b[3], (size_t)sl);
        name_off[f.n_records] = f.name_bytes; off[f.n_records] = f.base_bytes;
        name_hash[f.n_records] = c3_fastx_name_hash(text, b[0] + 1, nl);
      }
      ++f.n_records; f.name_bytes += nl; f.base_bytes += sl;
      if (p == n && at_eof) break;
    }
    f.consumed = p;
    *info = f;
    if (f.n_records > max_records || f.name_bytes > names_cap || f.base_bytes > bases_cap)
      return fx_bad("capacity too small (needed sizes in info)", C3_E_LIMIT);
    if (pass) { name_off[f.n_records] = f.name_bytes; off[f.n_records] = f.base_bytes; }
  }
  return C3_E_OK;
}

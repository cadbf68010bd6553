// c3_bam.cpp -- host statement of k_bam (include/c3poa.h "Unaligned BAM records on the GPU"): the file header
// and the longest prefix of whole strict records of a piece of inflated BAM, walked record by record on one thread with the
// rule of c3_bam.h, which k_bam and the reader apply as well.  The tests hold this against a parser of their own, and cut or
// edited data can be thrown at it under a sanitizer on the CPU (tools/bam_fuzz_host.sh).
#include "../../include/c3poa.h"
#include "c3_bam.h"
#include "c3_checks.h"
#include <cstring>

// argument rules shared with c3_bam_parse (c3_stream.hip); 0 = go on
int c3_bam_check_args(const char* who, const char* data, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                      const char* seqs, const char* quals, int64_t bases_cap, const int64_t* off, int64_t max_records,
                      c3_bam_info* info) {
  if (info) memset(info, 0, sizeof *info);
  char buf[96];
  if (!info || n < 0 || (n > 0 && !data) || !names || !name_off || !seqs || !quals || !off || names_cap < 0 || bases_cap < 0 || max_records < 0) {
    strcpy(buf, who); strcat(buf, ": bad arguments"); c3_set_host_error(buf); return C3_E_ARG;
  }
  if (n > C3_FASTQ_MAX_TEXT) { strcpy(buf, who); strcat(buf, ": data longer than C3_FASTQ_MAX_TEXT"); c3_set_host_error(buf); return C3_E_LIMIT; }
  return C3_E_OK;
}

const char* c3_bam_reason_text(int reason) {
  switch (reason) {
    case C3_BAM_BLOCK: return "block_size outside 34 .. C3_BAM_MAX_RECORD";
    case C3_BAM_NAME: return "read name empty or not NUL-terminated";
    case C3_BAM_FIELDS: return "name, cigar, bases and qualities do not fit in block_size";
    case C3_BAM_FLAG: return "a reverse-strand, secondary or supplementary record: the file is aligned; convert it with samtools fastq";
    case C3_BAM_EMPTY: return "a record without bases";
    case C3_BAM_NOQUAL: return "a record without qualities";
    case C3_BAM_TRUNCATED: return "the file ends inside a record or its header";
    case C3_BAM_HEADER: return "not a BAM header (magic, a negative length or more than C3_BAM_MAX_REFS references)";
  }
  return "strict";
}

extern "C" int c3_bam_parse_host(const char* data, int64_t n, int at_start, int at_eof, int min_len, char* names, int64_t names_cap,
                                 int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off,
                                 int64_t max_records, c3_bam_info* info) {
  const int rc = c3_bam_check_args("c3_bam_parse_host", data, n, names, names_cap, name_off, seqs, quals, bases_cap, off, max_records, info);
  if (rc) return rc;
  const uint8_t* d = (const uint8_t*)data;
  // pass 0 counts, pass 1 (only when everything fits) writes: nothing is half written on C3_E_LIMIT
  for (int pass = 0; pass < 2; ++pass) {
    c3_bam_info f; memset(&f, 0, sizeof f);
    int64_t p = 0;
    bool go = n > 0;
    if (go && at_start) {
      int64_t nx = 0;
      const int st = c3_bam_header(d, 0, n, &nx);
      if (st == C3_BAM_OK) { p = nx; f.header_bytes = nx; }
      else {
        go = false;
        if (st == C3_BAM_HEADER) { f.departed = 1; f.reason = C3_BAM_HEADER; }
        else if (at_eof) { f.departed = 1; f.reason = C3_BAM_TRUNCATED; }        // merely incomplete otherwise: consumed = 0
      }
    }
    while (go && p < n) {
      C3BamRec r;
      const int st = c3_bam_record(d, p, n, &r);
      if (st == C3_BAM_INCOMPLETE) { if (at_eof) { f.departed = 1; f.reason = C3_BAM_TRUNCATED; f.bad_at = p; } break; }
      if (st != C3_BAM_OK) { f.departed = 1; f.reason = st; f.bad_at = p; break; }
      p = r.next;
      ++f.n_records;
      if ((int64_t)r.l_seq < (int64_t)min_len) { ++f.n_short; continue; }
      if (pass) {
        memcpy(names + f.name_bytes, d + r.name, r.name_len);
        char* s = seqs + f.base_bytes; char* q = quals + f.base_bytes;
        for (int64_t i = 0; i < (int64_t)r.l_seq; ++i) { s[i] = (char)c3_bam_base_at(d + r.seq, i); q[i] = (char)c3_bam_qual(d[r.qual + i]); }
        name_off[f.n_kept] = f.name_bytes; off[f.n_kept] = f.base_bytes;
      }
      ++f.n_kept; f.name_bytes += r.name_len; f.base_bytes += r.l_seq;
    }
    f.consumed = p;
    *info = f;
    if (f.n_kept > max_records || f.name_bytes > names_cap || f.base_bytes > bases_cap) {
      c3_set_host_error("c3_bam_parse_host: capacity too small (needed sizes in info)");
      return C3_E_LIMIT;
    }
    if (pass) { name_off[f.n_kept] = f.name_bytes; off[f.n_kept] = f.base_bytes; }
  }
  return C3_E_OK;
}

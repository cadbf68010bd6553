// c3_bamout.cpp -- host statement of k_bamout (include/c3poa.h "Records written as unaligned BAM"): the rule of
// c3_emit.h (which records, which slices) and c3_bamout.h (what a record is made of) applied read by read, the records written
// one after the other into two streams per splint, uncompressed; and the file header.  Host code only; the tests decode its
// records and compare them with the text the existing writer makes of the same group, and the device with it byte for byte.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/c3poa.h"
#include "c3_bamout.h"
#include "c3_checks.h"

int c3_bamout_check_names(const char* who, const char* names, const int64_t* name_off, int n) {
  static thread_local char msg[200];
  for (int i = 0; i < n; ++i) {
    const int64_t nl = name_off[i + 1] - name_off[i];
    const char* nm = names + name_off[i];
    const bool nul = nl > 0 && memchr(nm, 0, (size_t)nl) != nullptr;
    if (nl <= C3_BAMOUT_MAX_NAME && !nul) continue;
    char shown[41];
    int k = 0;
    for (; k < 40 && k < nl && nm[k]; ++k) shown[k] = nm[k];
    shown[k] = 0;
    snprintf(msg, sizeof(msg), "%s: read %d (%s%s): %s", who, i, shown, k < nl ? "..." : "",
             nul ? "a NUL in the name" : "a name of more than 219 bytes does not fit a BAM record");
    c3_set_host_error(msg);
    return nul ? C3_E_ARG : C3_E_LIMIT;
  }
  return C3_E_OK;
}

static char* put32(char* o, uint32_t v) { for (int k = 0; k < 4; ++k) *o++ = (char)(v >> (8 * k)); return o; }
static char* put_fixed(char* o, int64_t total, int64_t l_read_name, int64_t l_seq) {
  for (int k = 0; k < 9; ++k) o = put32(o, c3_bamout_fixed(k, (uint32_t)(total - 4), (uint32_t)l_read_name, (uint32_t)l_seq));
  return o;
}
static char* put_bases(char* o, const char* s, int64_t n) {
  for (int64_t k = 0; k + 1 < n; k += 2) *o++ = (char)(c3_bamout_code((uint8_t)s[k]) << 4 | c3_bamout_code((uint8_t)s[k + 1]));
  if (n & 1) *o++ = (char)(c3_bamout_code((uint8_t)s[n - 1]) << 4);
  return o;
}
static char* put_quals(char* o, const char* q, int64_t n) {
  for (int64_t k = 0; k < n; ++k) *o++ = (char)c3_bamout_qual((uint8_t)q[k]);
  return o;
}

extern "C" int c3_emit_group_bam_host(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                      const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                                      int64_t* stream_off, int64_t* n_records) {
  int rc = c3_emit_check_args("c3_emit_group_bam_host", b, res, cons, cons_off, qv, splint_id, n_splints, zero, arena, cap, stream_off, n_records);
  if (rc == C3_E_OK) rc = c3_bamout_check_names("c3_emit_group_bam_host", b->names, b->name_off, b->n);
  if (rc != C3_E_OK) return rc;
  const int K = 2, S = n_splints * K;
  std::vector<int64_t> size((size_t)S, 0);
  int64_t records = 0;
  char aq[8];
  for (int pass = 0; pass < 2; ++pass) {                          // lengths, then (the streams placed) the bytes
    std::vector<int64_t> at(stream_off, stream_off + (pass ? S : 0));
    for (int i = 0; i < b->n; ++i) {
      const c3_read_result& r = res[i];
      const int s = splint_id[i];
      const int64_t clen = cons ? cons_off[i + 1] - cons_off[i] : 0;
      const C3EmitDec d = c3_emit_of(r, s, n_splints, zero, clen);
      if (!d.any) continue;
      const int64_t L = b->off[i + 1] - b->off[i], nl = b->name_off[i + 1] - b->name_off[i];
      const char* name = b->names + b->name_off[i];
      const char* seq = b->seqs + b->off[i];
      const char* qual = b->quals + b->off[i];
      for (int j = 0; j < d.np; ++j) {
        int32_t idx; int64_t pb, pe;
        c3_emit_piece(r, d, L, j, &idx, &pb, &pe);
        const int64_t len = pe - pb, total = c3_bamout_sub_len(nl, idx, len);
        const size_t x = (size_t)s * K + C3_BAMOUT_SUB;
        if (!pass) { size[x] += total; ++records; continue; }
        const int dn = c3_emit_dec_len(idx);
        char* o = put_fixed(arena + at[x], total, nl + 1 + dn + 1, len);
        memcpy(o, name, (size_t)nl); o += nl; *o++ = '_';
        for (int k = 0; k < dn; ++k) *o++ = c3_emit_dec_char(idx, k);
        *o++ = 0;
        o = put_bases(o, seq + pb, len);
        o = put_quals(o, qual + pb, len);
        at[x] += total;
      }
      if (!d.cons) continue;
      int64_t tot = 0;
      for (int64_t k = 0; k < L; ++k) tot += (uint8_t)qual[k];
      tot -= 33 * L;
      const int aql = c3_emit_avgq(tot, L, aq);
      const int ht = c3_emit_head_tail_len(aql, L, d.ns, clen);
      const size_t x = (size_t)s * K + C3_BAMOUT_CONS;
      const int64_t total = c3_bamout_cons_len(nl, ht, clen);
      if (!pass) { size[x] += total; ++records; continue; }
      char* o = put_fixed(arena + at[x], total, nl + ht, clen);
      memcpy(o, name, (size_t)nl); o += nl;
      for (int k = 0; k < ht - 1; ++k) *o++ = c3_emit_head_tail_char(k, aq, aql, L, d.ns, clen);
      *o++ = 0;                                                     // (where the FASTA header ends its line)
      o = put_bases(o, cons + cons_off[i], clen);
      if (qv) o = put_quals(o, qv + cons_off[i], clen);
      else { memset(o, (int)C3_BAMOUT_NOQUAL, (size_t)clen); o += clen; }
      for (int k = 0; k < C3_BAMOUT_TAGS; ++k) *o++ = (char)c3_bamout_tag_byte(k, d.ns, L, tot);
      at[x] += total;
    }
    if (pass) break;
    stream_off[0] = 0;
    for (int x = 0; x < S; ++x) stream_off[x + 1] = stream_off[x] + size[(size_t)x];
    *n_records = records;
    if (stream_off[S] > cap) { c3_set_host_error("c3_emit_group_bam_host: arena too small (bytes needed in stream_off[S])"); return C3_E_LIMIT; }
  }
  return C3_E_OK;
}

// BAM\1 | l_text | @HD, @PG | n_ref = 0
extern "C" int c3_bam_out_header(char* dst, int64_t cap, int64_t* len) {
  if (!len || cap < 0 || (cap > 0 && !dst)) { c3_set_host_error("c3_bam_out_header: null argument"); return C3_E_ARG; }
  char text[256];
  const int tl = snprintf(text, sizeof(text), "@HD\tVN:1.6\tSO:unknown\n@PG\tID:c3poa_amd\tPN:c3poa_amd\tVN:%s\n", c3_version());
  if (tl < 0 || tl >= (int)sizeof(text)) { c3_set_host_error("c3_bam_out_header: version text too long"); return C3_E_LIMIT; }
  *len = 12 + tl;
  if (*len > cap) { c3_set_host_error("c3_bam_out_header: dst too small (bytes needed in *len)"); return C3_E_LIMIT; }
  memcpy(dst, "BAM\1", 4);
  char* o = put32(dst + 4, (uint32_t)tl);
  memcpy(o, text, (size_t)tl);
  put32(o + tl, 0u);
  return C3_E_OK;
}

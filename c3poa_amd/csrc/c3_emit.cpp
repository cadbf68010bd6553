// c3_emit.cpp -- host statement of k_emit (include/c3poa.h "Records formatted on the GPU"): the rule of
// c3_emit.h applied read by read, the records written one after the other into K streams per splint.  Host code only; the
// tests compare it with the files c3_write_group / c3_write_consensus_fastq write, byte for byte, and the device with it.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/c3poa.h"
#include "c3_emit.h"
#include "c3_checks.h"

int c3_emit_check_args(const char* who, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                       const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                       int64_t* stream_off, int64_t* n_records) {
  static thread_local char msg[200];
  const char* why = nullptr;
  int rc = C3_E_ARG, bad = -1;
  (void)zero;
  if (!b || !stream_off || !n_records || cap < 0 || (cap > 0 && !arena)) why = "null argument";
  else if (b->n < 0 || n_splints <= 0) why = "negative count or no splint";
  else if (n_splints > C3_EMIT_MAX_SPLINTS) { why = "more than 64 splints"; rc = C3_E_LIMIT; }
  else if (qv && !cons) why = "qv without cons";
  else if (cons && !cons_off) why = "cons without cons_off";
  else if (b->n > 0 && (!res || !splint_id || !b->names || !b->name_off || !b->seqs || !b->quals || !b->off)) why = "batch arrays missing";
  if (!why && b->n > 0) {
    const int n = b->n;
    if (b->off[0] != 0 || b->name_off[0] != 0 || (cons && cons_off[0] != 0)) why = "offsets must start at 0";
    for (int i = 0; i < n && !why; ++i) {
      if (b->off[i + 1] < b->off[i] || b->name_off[i + 1] < b->name_off[i]) { why = "offsets not ascending"; bad = i; }
      else if (cons && cons_off[i + 1] < cons_off[i]) { why = "cons_off not ascending"; bad = i; }
    }
    // (a group may hold any number of bytes: every offset is 64-bit on both sides; one read, name or consensus stays below 2^31)
    for (int i = 0; i < n && !why; ++i)
      if (b->off[i + 1] - b->off[i] >= (1ll << 31) || b->name_off[i + 1] - b->name_off[i] >= (1ll << 31) || (cons && cons_off[i + 1] - cons_off[i] >= (1ll << 31))) {
        why = "a read, name or consensus of 2^31 bytes or more"; rc = C3_E_LIMIT; bad = i;
      }
    for (int i = 0; i < n && !why; ++i) {
      const c3_read_result& r = res[i];
      const int64_t L = b->off[i + 1] - b->off[i];
      const C3EmitDec d = c3_emit_of(r, splint_id[i], n_splints, zero, cons ? cons_off[i + 1] - cons_off[i] : 0);
      if (!d.any) continue;
      bad = i;
      if (r.n_sub < 0 || r.n_sub > C3_EMIT_MAX_SUB) { why = "n_sub outside 0 .. 250"; break; }
      if (d.cons && L == 0) { why = "consensus record of an empty read"; break; }
      if ((r.n_sub == 0 || r.has_front) && (r.front_end < 0 || r.front_end > L)) { why = "front_end outside the read"; break; }
      if ((r.n_sub == 0 || r.has_tail) && (r.tail_beg < 0 || r.tail_beg > L)) { why = "tail_beg outside the read"; break; }
      for (int k = 0; k < r.n_sub; ++k)
        if (r.sub_beg[k] < 0 || r.sub_end[k] < r.sub_beg[k] || r.sub_end[k] > L) { why = "subread outside 0 <= beg <= end <= L"; break; }
      if (why) break;
    }
  }
  if (!why) return C3_E_OK;
  if (bad >= 0) snprintf(msg, sizeof(msg), "%s: read %d: %s", who, bad, why);
  else snprintf(msg, sizeof(msg), "%s: %s", who, why);
  c3_set_host_error(msg);
  return rc;
}

extern "C" int c3_emit_group_host(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                  const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                                  int64_t* stream_off, int64_t* n_records) {
  const int rc = c3_emit_check_args("c3_emit_group_host", b, res, cons, cons_off, qv, splint_id, n_splints, zero, arena, cap, stream_off, n_records);
  if (rc != C3_E_OK) return rc;
  const int K = qv ? 3 : 2, S = n_splints * K;
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
        const int64_t len = pe - pb, total = c3_emit_sub_len(nl, idx, len);
        const size_t x = (size_t)s * K + C3_EMIT_SUB_FQ;
        if (!pass) { size[x] += total; ++records; continue; }
        char* o = arena + at[x];
        *o++ = '@'; memcpy(o, name, (size_t)nl); o += nl; *o++ = '_';
        const int dn = c3_emit_dec_len(idx);
        for (int k = 0; k < dn; ++k) *o++ = c3_emit_dec_char(idx, k);
        *o++ = '\n'; memcpy(o, seq + pb, (size_t)len); o += len;
        memcpy(o, "\n+\n", 3); o += 3; memcpy(o, qual + pb, (size_t)len); o += len; *o++ = '\n';
        at[x] += total;
      }
      if (!d.cons) continue;
      int64_t tot = 0;
      for (int64_t k = 0; k < L; ++k) tot += (uint8_t)qual[k];
      tot -= 33 * L;
      const int aql = c3_emit_avgq(tot, L, aq);
      const int ht = c3_emit_head_tail_len(aql, L, d.ns, clen);
      for (int kind = 0; kind < K; kind += 2) {                     // C3_EMIT_CONS_FA, and C3_EMIT_CONS_FQ with qv
        const size_t x = (size_t)s * K + kind;
        const int64_t total = c3_emit_cons_len(kind, nl, aql, L, d.ns, clen);
        if (!pass) { size[x] += total; ++records; continue; }
        char* o = arena + at[x];
        *o++ = kind == C3_EMIT_CONS_FA ? '>' : '@'; memcpy(o, name, (size_t)nl); o += nl;
        for (int k = 0; k < ht; ++k) *o++ = c3_emit_head_tail_char(k, aq, aql, L, d.ns, clen);
        memcpy(o, cons + cons_off[i], (size_t)clen); o += clen;
        if (kind == C3_EMIT_CONS_FQ) { memcpy(o, "\n+\n", 3); o += 3; memcpy(o, qv + cons_off[i], (size_t)clen); o += clen; }
        *o++ = '\n';
        at[x] += total;
      }
    }
    if (pass) break;
    stream_off[0] = 0;
    for (int x = 0; x < S; ++x) stream_off[x + 1] = stream_off[x] + size[(size_t)x];
    *n_records = records;
    if (stream_off[S] > cap) { c3_set_host_error("c3_emit_group_host: arena too small (bytes needed in stream_off[S])"); return C3_E_LIMIT; }
  }
  return C3_E_OK;
}

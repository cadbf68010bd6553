// c3_post.cpp -- host statement of k_post (include/c3poa.h "Post-processing on the GPU"): the rule of
// c3_post.h applied read by read, the records written one after the other.  Host code only; the tests compare it with the
// Python path byte for byte and the device with it.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../include/c3poa.h"
#include "c3_post.h"
#include "c3_checks.h"

int c3_post_check_args(const char* who, const c3_post_args* a, char* arena, int64_t cap, int64_t* stream_off, int64_t* n_kept) {
  static thread_local char msg[160];
  const char* why = nullptr;
  int rc = C3_E_ARG;
  if (!a || !stream_off || !n_kept || cap < 0 || (cap > 0 && !arena)) why = "null argument";
  else if (a->n < 0 || a->n_ad < 0 || a->n_idx < 0) why = "negative count";
  else if (a->n > 0 && (!a->names || !a->name_off || !a->seqs || !a->off || (a->n_ad > 0 && !a->table))) why = "batch arrays missing";
  else if (a->n_ad > 0 && (!a->ad_len || !a->ad_class || !a->ad_names || !a->ad_name_off)) why = "adapter descriptors missing";
  else if (a->has_index && a->n_idx > 0 && (!a->idx_cat || !a->idx_off || !a->idx_dest)) why = "index descriptors missing";
  else if (a->n_dest < 1 || (!a->has_index && a->n_dest != 1)) why = "n_dest must be 1 without an index set, at least 1 with one";
  else if (a->has_index && a->n_idx > C3_POST_MAX_IDX) { why = "more than 16 indexes"; rc = C3_E_LIMIT; }
  else if (a->n_dest > C3_POST_MAX_DEST) { why = "more than 17 destinations"; rc = C3_E_LIMIT; }
  if (!why && a->has_index)
    for (int k = 0; k < a->n_idx && !why; ++k) {
      const int64_t len = a->idx_off[k + 1] - a->idx_off[k];
      if (len < 0 || a->idx_off[0] != 0) why = "index offsets not ascending from 0";
      else if (len > C3_POST_MAX_IDX_LEN) { why = "index longer than 32 bases"; rc = C3_E_LIMIT; }
      else if (a->idx_dest[k] < 0 || a->idx_dest[k] >= a->n_dest) why = "idx_dest outside 0 .. n_dest-1";
    }
  if (!why && a->n > 0) {
    if (a->off[0] != 0 || a->name_off[0] != 0) why = "offsets must start at 0";
    for (int i = 0; i < a->n && !why; ++i)
      if (a->off[i + 1] < a->off[i] || a->name_off[i + 1] < a->name_off[i]) why = "offsets not ascending";
    if (!why && (a->off[a->n] >= (1ll << 31) || a->name_off[a->n] >= (1ll << 31))) { why = "batch of 2^31 bytes or more"; rc = C3_E_LIMIT; }
  }
  if (!why && a->n_ad > 0) {
    if (a->ad_name_off[0] != 0) why = "adapter name offsets must start at 0";
    for (int k = 0; k < a->n_ad && !why; ++k)
      if (a->ad_name_off[k + 1] < a->ad_name_off[k] || a->ad_class[k] < 0) why = "adapter name offsets not ascending or a negative class";
    if (!why && a->ad_name_off[a->n_ad] >= (1 << 20)) { why = "adapter names of 1 MiB or more"; rc = C3_E_LIMIT; }
  }
  if (!why) return C3_E_OK;
  snprintf(msg, sizeof(msg), "%s: %s", who, why);
  c3_set_host_error(msg);
  return rc;
}

namespace {
C3PostOpt make_opt(const c3_post_args* a) {
  C3PostOpt o;
  o.n_ad = a->n_ad; o.class5 = a->class5; o.undirectional = a->undirectional != 0; o.trim = a->trim != 0; o.barcoded = a->barcoded != 0;
  o.quals = a->quals != nullptr; o.has_index = a->has_index != 0; o.n_idx = a->has_index ? a->n_idx : 0; o.n_dest = a->n_dest;
  return o;
}

void put_segment(char* out, const C3PostSeg& s, const char* name, const char* seq, const char* qual) {
  switch (s.kind) {
    case C3_SEG_LIT: memcpy(out, c3_post_lit(s.a), (size_t)s.len); break;
    case C3_SEG_NAME: memcpy(out, name, (size_t)s.len); break;
    case C3_SEG_DEC: for (int j = 0; j < s.len; ++j) out[j] = c3_post_digit((uint32_t)s.a, s.len, j); break;
    case C3_SEG_SEQ_F: memcpy(out, seq + s.a, (size_t)s.len); break;
    case C3_SEG_QUAL_F: memcpy(out, qual + s.a, (size_t)s.len); break;
    case C3_SEG_SEQ_R: for (int j = 0; j < s.len; ++j) out[j] = (char)c3_post_comp((uint8_t)seq[s.a + s.len - 1 - j]); break;
    default: for (int j = 0; j < s.len; ++j) out[j] = qual[s.a + s.len - 1 - j]; break;
  }
}
}  // namespace

extern "C" int c3_post_emit_host(const c3_post_args* a, char* arena, int64_t cap, int64_t* stream_off, int64_t* n_kept) {
  const int rc = c3_post_check_args("c3_post_emit_host", a, arena, cap, stream_off, n_kept);
  if (rc != C3_E_OK) return rc;
  const C3PostOpt o = make_opt(a);
  const int S = 3 * o.n_dest + 3;
  const size_t row = (size_t)o.n_ad * 2 * 12;
  std::vector<C3PostDec> dec((size_t)a->n);
  std::vector<int64_t> size((size_t)S, 0);
  C3PostSeg seg[C3_POST_MAX_SEG];
  int64_t kept = 0, t;
  for (int pass = 0; pass < 2; ++pass) {                          // lengths, then (the streams placed) the bytes
    std::vector<int64_t> at(stream_off, stream_off + (pass ? S : 0));
    for (int i = 0; i < a->n; ++i) {
      const int32_t L = (int32_t)(a->off[i + 1] - a->off[i]), nlen = (int32_t)(a->name_off[i + 1] - a->name_off[i]);
      const char* seq = a->seqs + a->off[i];
      const char* name = a->names + a->name_off[i];
      const int32_t* tab = a->table + (size_t)i * row;
      C3PostDec& d = dec[(size_t)i];
      if (!pass) {
        c3_post_adapters(tab, a->ad_len, a->ad_class, o, &d);
        if (d.kept && o.has_index) c3_post_oligo(seq, L, o, a->idx_cat, a->idx_off, a->idx_dest, &d);
        kept += d.kept;
      }
      for (int k = 0; k < 5; ++k) {
        const int ns = c3_post_plan(k, d, L, nlen, o, seg, &t);
        if (!ns) continue;
        const int s = c3_post_stream(k, d.dest, o.n_dest);
        if (!pass) { size[(size_t)s] += t; continue; }
        for (int j = 0; j < ns; ++j) { put_segment(arena + at[(size_t)s], seg[j], name, seq, a->quals ? a->quals + a->off[i] : nullptr); at[(size_t)s] += seg[j].len; }
      }
      for (int e = 0; e < o.n_ad * 2; ++e) {
        const int32_t* r = tab + (size_t)e * 12;
        if (r[0] < C3_POST_MIN_SCORE) continue;
        const int ad = e >> 1;
        const char* an = a->ad_names + a->ad_name_off[ad];
        const int32_t anl = (int32_t)(a->ad_name_off[ad + 1] - a->ad_name_off[ad]);
        if (!pass) size[(size_t)S - 1] += c3_post_psl_row(nullptr, r, name, nlen, L, an, anl, a->ad_len[ad], e & 1);
        else at[(size_t)S - 1] += c3_post_psl_row(arena + at[(size_t)S - 1], r, name, nlen, L, an, anl, a->ad_len[ad], e & 1);
      }
    }
    if (pass) break;
    stream_off[0] = 0;
    for (int s = 0; s < S; ++s) stream_off[s + 1] = stream_off[s] + size[(size_t)s];
    *n_kept = kept;
    if (stream_off[S] > cap) { c3_set_host_error("c3_post_emit_host: arena too small (bytes needed in stream_off[S])"); return C3_E_LIMIT; }
  }
  return C3_E_OK;
}

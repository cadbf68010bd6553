// c3_dsplit.cpp -- host statement of the demultiplexer's text path (include/c3poa.h "Sample demultiplexer, pieces of text in /
// per-sample streams out"): one plain text of a stated kind parsed by c3_fasta_parse_host or
// c3_fastx_strict_parse_host, searched by c3_demux_host and written stream by stream with the rule of c3_dsplit.h, which
// k_dsplit applies as well; and the argument checks the device call shares.  Plain C++: the tests hold it against the Python
// path, and cut or edited text can be thrown at it under a sanitizer on the CPU (tools/demux_text_fuzz_host.sh).
#include "../../include/c3poa.h"
#include "c3_dsplit.h"
#include "c3_checks.h"
#include <cstring>
#include <string>
#include <vector>

static int ds_bad(const char* who, const char* what, int code) {
  const std::string m = std::string(who) + what;
  c3_set_host_error(m.c_str());
  return code;
}

// argument rules shared with c3_demux_emit_text (c3_dtext.hip); 0 = go on, with *S and the byte codes of the index sets
int c3_demux_text_check_args(const char* who, const char* src, int64_t n, int flags, const c3_demux_sets* sets, const char* arena,
                             int64_t cap, const int64_t* stream_off, const uint64_t* name_hash, int64_t max_records,
                             c3_demux_text_info* info, int* S, uint8_t* tab, int* n_codes) {
  if (info) memset(info, 0, sizeof *info);
  if (!info || n < 0 || (n > 0 && !src) || !sets || !arena || cap < 0 || !stream_off || !name_hash || max_records < 0 ||
      (flags & ~(C3_DEMUX_IN_BGZF | C3_DEMUX_OUT_BGZF | C3_DEMUX_KEEP_QUALS | C3_DEMUX_SPLIT)))
    return ds_bad(who, ": bad arguments", C3_E_ARG);
  c3_demux_info di;
  char one = 0;
  int rc = c3_demux_emit_check_args(who, &one, 0, sets->n_a, sets->a_names, sets->a_name_off, sets->n_b, sets->b_names, sets->b_name_off,
                                    &one, 0, name_hash, max_records, &di);
  if (rc != C3_E_OK) return rc;
  const char* msg = "";
  if ((rc = c3_demux_prepare(sets->n_a, sets->a_cat, sets->a_off, sets->n_b, sets->b_cat, sets->b_off, tab, n_codes, &msg)) != C3_E_OK) {
    c3_set_host_error(msg);
    return rc;
  }
  const int64_t s = (flags & C3_DEMUX_SPLIT) ? (int64_t)(sets->n_a + 1) * (sets->n_b + 1) : 1;
  if (s > C3_DEMUX_MAX_STREAMS) return ds_bad(who, ": more streams than C3_DEMUX_MAX_STREAMS", C3_E_LIMIT);
  *S = (int)s;
  info->n_streams = (int32_t)s;
  return C3_E_OK;
}

extern "C" int c3_demux_emit_text_host(const char* text, int64_t n, int at_eof, int kind, int flags, const c3_demux_sets* sets,
                                       char* arena, int64_t cap, int64_t* stream_off, uint64_t* name_hash, int64_t max_records,
                                       c3_demux_text_info* info) {
  static const char who[] = "c3_demux_emit_text_host";
  uint8_t tab[256]; int K = 0, S = 0;
  int rc = c3_demux_text_check_args(who, text, n, flags, sets, arena, cap, stream_off, name_hash, max_records, info, &S, tab, &K);
  if (rc) return rc;
  if ((flags & C3_DEMUX_IN_BGZF) || (kind != 2 && kind != 4)) return ds_bad(who, ": plain text of kind 2 or 4 only", C3_E_ARG);
  const bool keep_q = (flags & C3_DEMUX_KEEP_QUALS) != 0, split = (flags & C3_DEMUX_SPLIT) != 0, out_z = (flags & C3_DEMUX_OUT_BGZF) != 0;
  if (keep_q && kind == 2) return ds_bad(who, ": C3_DEMUX_KEEP_QUALS on a FASTA text", C3_E_ARG);
  if (n > C3_FASTX_MAX_TEXT) return ds_bad(who, ": text longer than C3_FASTX_MAX_TEXT", C3_E_LIMIT);
  for (int s = 0; s <= S; ++s) stream_off[s] = 0;
  info->text_bytes = n; info->kind = kind;
  if (n == 0) return C3_E_OK;

  // ---- parse: sizes first (a call with no room answers them), then the arrays ----
  int64_t R = 0, name_bytes = 0, base_bytes = 0;
  char none = 0; int64_t o1[1] = {0}, o2[1] = {0}; uint64_t h1[1];
  if (kind == 2) {
    c3_fasta_info f;
    rc = c3_fasta_parse_host(text, n, at_eof, &none, 0, o1, &none, 0, o2, h1, 0, &f);
    if (rc != C3_E_OK && rc != C3_E_LIMIT) return rc;
    R = f.n_records; name_bytes = f.name_bytes; base_bytes = f.base_bytes; info->consumed = f.consumed; info->departed = f.departed;
  } else {
    c3_fastx_info f;
    rc = c3_fastx_strict_parse_host(text, n, at_eof, 4, &none, 0, o1, &none, &none, 0, o2, h1, 0, &f);
    if (rc != C3_E_OK && rc != C3_E_LIMIT) return rc;
    R = f.n_records; name_bytes = f.name_bytes; base_bytes = f.base_bytes; info->consumed = f.consumed; info->departed = f.departed;
  }
  info->n_records = R;
  if (R > max_records) return ds_bad(who, ": more records than max_records (the need in info)", C3_E_LIMIT);
  if (R == 0) return C3_E_OK;
  std::vector<char> names((size_t)name_bytes + 1), seqs((size_t)base_bytes + 1), quals(kind == 4 ? (size_t)base_bytes + 1 : 1);
  std::vector<int64_t> name_off((size_t)R + 1), off((size_t)R + 1);
  std::vector<uint64_t> hash((size_t)R);
  if (kind == 2) {
    c3_fasta_info f;
    rc = c3_fasta_parse_host(text, n, at_eof, names.data(), name_bytes, name_off.data(), seqs.data(), base_bytes, off.data(), hash.data(), R, &f);
  } else {
    c3_fastx_info f;
    rc = c3_fastx_strict_parse_host(text, n, at_eof, 4, names.data(), name_bytes, name_off.data(), seqs.data(), quals.data(), base_bytes,
                                    off.data(), hash.data(), R, &f);
  }
  if (rc != C3_E_OK) return rc;

  // ---- search ----
  std::vector<int64_t> kept;
  for (int64_t r = 0; r < R; ++r) if (c3_dsplit_kept(off[(size_t)r + 1] - off[(size_t)r])) kept.push_back(r);
  const int64_t nk = (int64_t)kept.size();
  if (nk > INT32_MAX) return ds_bad(who, ": too many records in one text", C3_E_LIMIT);
  std::vector<char> heads((size_t)nk * C3_DEMUX_HEAD + 1);
  std::vector<int32_t> win((size_t)nk * 2 + 2);
  for (int64_t i = 0; i < nk; ++i) memcpy(&heads[(size_t)i * C3_DEMUX_HEAD], &seqs[(size_t)off[(size_t)kept[(size_t)i]]], C3_DEMUX_HEAD);
  rc = c3_demux_host((int)nk, heads.data(), sets->n_a, sets->a_cat, sets->a_off, sets->n_b, sets->b_cat, sets->b_off, win.data(), nullptr);
  if (rc != C3_E_OK) return rc;

  // ---- place: bytes per stream, then every record behind the earlier ones of its stream ----
  std::vector<int64_t> so((size_t)S + 1, 0), place((size_t)nk + 1);
  std::vector<int32_t> key((size_t)nk + 1);
  auto rec_len = [&](int64_t i) {
    const size_t r = (size_t)kept[(size_t)i];
    return c3_demux_rec_len(name_off[r + 1] - name_off[r], off[r + 1] - off[r], c3_dsplit_index_len(sets->a_name_off, win[2 * (size_t)i]),
                            c3_dsplit_index_len(sets->b_name_off, win[2 * (size_t)i + 1]), keep_q);
  };
  for (int64_t i = 0; i < nk; ++i) {
    key[(size_t)i] = c3_dsplit_stream(win[2 * (size_t)i], win[2 * (size_t)i + 1], sets->n_a, sets->n_b, split);
    so[(size_t)key[(size_t)i] + 1] += rec_len(i);
  }
  for (int s = 0; s < S; ++s) so[(size_t)s + 1] += so[(size_t)s];
  {
    std::vector<int64_t> fill(so.begin(), so.end() - 1);
    for (int64_t i = 0; i < nk; ++i) { place[(size_t)i] = fill[(size_t)key[(size_t)i]]; fill[(size_t)key[(size_t)i]] += rec_len(i); }
  }
  int64_t need = 0;
  for (int s = 0; s < S; ++s) {
    const int64_t len = so[(size_t)s + 1] - so[(size_t)s];
    stream_off[s] = need;
    need += (out_z && len) ? c3_bgzf_bound(len) : len;
  }
  stream_off[S] = need;
  info->n_kept = nk; info->out_bytes = need;
  if (need > cap) return ds_bad(who, ": arena too small (bytes needed in stream_off[S])", C3_E_LIMIT);

  // ---- write ----
  std::vector<char> plain;
  char* dst = arena;
  if (out_z) { plain.resize((size_t)so[(size_t)S] + 1); dst = plain.data(); }
  for (int64_t i = 0; i < nk; ++i) {
    const size_t r = (size_t)kept[(size_t)i];
    const int32_t wa = win[2 * (size_t)i], wb = win[2 * (size_t)i + 1];
    const int64_t nl = name_off[r + 1] - name_off[r], sl = off[r + 1] - off[r];
    const int64_t al = c3_dsplit_index_len(sets->a_name_off, wa), bl = c3_dsplit_index_len(sets->b_name_off, wb);
    char* o = dst + place[(size_t)i];
    *o++ = keep_q ? '@' : '>';
    if (nl) memcpy(o, &names[(size_t)name_off[r]], (size_t)nl);
    o += nl; *o++ = '|';
    if (al) memcpy(o, sets->a_names + sets->a_name_off[wa], (size_t)al);
    o += al; *o++ = '_';
    if (bl) memcpy(o, sets->b_names + sets->b_name_off[wb], (size_t)bl);
    o += bl; *o++ = '\n';
    memcpy(o, &seqs[(size_t)off[r]], (size_t)sl);
    o += sl; *o++ = '\n';
    if (keep_q) {
      *o++ = '+'; *o++ = '\n';
      memcpy(o, &quals[(size_t)off[r]], (size_t)sl);
      o += sl; *o++ = '\n';
    }
  }
  if (out_z) {
    int64_t out = 0;
    for (int s = 0; s < S; ++s) {
      const int64_t len = so[(size_t)s + 1] - so[(size_t)s];
      stream_off[s] = out;
      if (!len) continue;
      int64_t got = 0;
      if ((rc = c3_bgzf_compress_host(plain.data() + so[(size_t)s], len, arena + out, cap - out, &got)) != C3_E_OK) return rc;
      out += got;
    }
    stream_off[S] = out;
    info->out_bytes = out;
  }
  for (int64_t r = 0; r < R; ++r) name_hash[r] = hash[(size_t)r];
  return C3_E_OK;
}

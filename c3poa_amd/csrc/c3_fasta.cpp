// c3_fasta.cpp -- host statements of k_fasta (include/c3poa.h "Sample demultiplexer, text in / file bytes out"):
// the records of a FASTA text walked line by line on one thread with the rule of c3_fasta.h, which k_fasta applies as well, and
// the bytes of Indexed_reads.fasta made from them with c3_demux_host.  The tests hold both against the Python path, and cut or
// edited text can be thrown at them under a sanitizer on the CPU.
#include "../../include/c3poa.h"
#include "c3_fasta.h"
#include "c3_checks.h"
#include <algorithm>
#include <cstring>
#include <vector>

static int fa_bad(const char* who, const char* what, int code) {
  char buf[128];
  strcpy(buf, who); strcat(buf, what); c3_set_host_error(buf);
  return code;
}

// argument rules shared with c3_fasta_parse (c3_scans.hip); 0 = go on
int c3_fasta_check_args(const char* who, const char* text, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                        const char* seqs, int64_t bases_cap, const int64_t* off, const uint64_t* name_hash, int64_t max_records,
                        c3_fasta_info* info) {
  if (info) memset(info, 0, sizeof *info);
  if (!info || n < 0 || (n > 0 && !text) || !names || !name_off || !seqs || !off || !name_hash || names_cap < 0 || bases_cap < 0 || max_records < 0)
    return fa_bad(who, ": bad arguments", C3_E_ARG);
  if (n > C3_FASTA_MAX_TEXT) return fa_bad(who, ": text longer than C3_FASTA_MAX_TEXT", C3_E_LIMIT);
  return C3_E_OK;
}
// ... and with c3_demux_emit; the index sets are checked by c3_demux_prepare
int c3_demux_emit_check_args(const char* who, const char* text, int64_t n, int n_a, const char* a_names, const int64_t* a_name_off,
                             int n_b, const char* b_names, const int64_t* b_name_off, const char* out, int64_t cap,
                             const uint64_t* name_hash, int64_t max_records, c3_demux_info* info) {
  if (info) memset(info, 0, sizeof *info);
  if (!info || n < 0 || (n > 0 && !text) || !out || cap < 0 || !name_hash || max_records < 0 || !a_name_off || !b_name_off)
    return fa_bad(who, ": bad arguments", C3_E_ARG);
  if (n > C3_FASTA_MAX_TEXT) return fa_bad(who, ": text longer than C3_FASTA_MAX_TEXT", C3_E_LIMIT);
  const int ns[2] = {n_a, n_b}; const char* nm[2] = {a_names, b_names}; const int64_t* no[2] = {a_name_off, b_name_off};
  for (int s = 0; s < 2; ++s) {
    if (ns[s] < 0 || ns[s] > C3_DEMUX_MAX_IDX) continue;           // c3_demux_prepare refuses it with its own text
    if (no[s][0] != 0) return fa_bad(who, ": index name offsets not starting at 0", C3_E_ARG);
    for (int k = 0; k < ns[s]; ++k) if (no[s][k + 1] < no[s][k]) return fa_bad(who, ": index name offsets decrease", C3_E_ARG);
    if (ns[s] > 0 && no[s][ns[s]] > 0 && !nm[s]) return fa_bad(who, ": index names missing", C3_E_ARG);
  }
  return C3_E_OK;
}

namespace {
// f(b, e) for every line of the text, the unterminated last one included (it may be empty); stops when f returns false
template <class F> void fa_lines(const uint8_t* t, int64_t n, F f) {
  int64_t b = 0;
  for (int64_t i = 0; i < n; ++i)
    if (c3_fasta_is_term(t[i])) { if (!f(b, i)) return; b = i + 1; }
  (void)f(b, n);
}

struct FaParse { int64_t H = 0, consumed = 0, name_bytes = 0, base_bytes = 0; C3FaVerdict v{0, 0}; };

// which records the text delivers, and their byte totals
FaParse fa_measure(const uint8_t* t, int64_t n, int at_eof) {
  FaParse p;
  std::vector<int64_t> hb;
  int64_t first_high = -1, first_headless = -1;
  for (int64_t i = 0; i < n; ++i) if (t[i] >= 0x80) { first_high = i; break; }
  fa_lines(t, n, [&](int64_t b, int64_t e) {
    const int64_t se = c3_fasta_strip_end(t, b, e);
    const int kind = c3_fasta_kind(t, b, se);
    if (kind == C3_FA_HEADER) hb.push_back(b);
    else if (kind == C3_FA_SEQ && hb.empty() && first_headless < 0) first_headless = b;
    return true;
  });
  p.H = (int64_t)hb.size();
  const int64_t rec_of_high = first_high < 0 ? -1 : (int64_t)(std::upper_bound(hb.begin(), hb.end(), first_high) - hb.begin()) - 1;
  p.v = c3_fasta_verdict(p.H, at_eof, first_high, first_headless, rec_of_high);
  p.consumed = c3_fasta_consumed(p.v, p.H, at_eof, n, p.v.n_records < p.H ? hb[(size_t)p.v.n_records] : 0);
  int64_t rec = -1;
  fa_lines(t, n, [&](int64_t b, int64_t e) {
    const int64_t se = c3_fasta_strip_end(t, b, e);
    const int kind = c3_fasta_kind(t, b, se);
    if (kind == C3_FA_HEADER) { if (++rec >= p.v.n_records) return false; p.name_bytes += se - b - 1; }
    else if (kind == C3_FA_SEQ && rec >= 0) p.base_bytes += se - b;
    return true;
  });
  return p;
}

// the delivered records written out (everything fits)
void fa_write(const uint8_t* t, int64_t n, const FaParse& p, char* names, int64_t* name_off, char* seqs, int64_t* off, uint64_t* name_hash) {
  int64_t rec = -1, nb = 0, sb = 0;
  fa_lines(t, n, [&](int64_t b, int64_t e) {
    const int64_t se = c3_fasta_strip_end(t, b, e);
    const int kind = c3_fasta_kind(t, b, se);
    if (kind == C3_FA_HEADER) {
      if (++rec >= p.v.n_records) return false;
      name_off[rec] = nb; off[rec] = sb;
      name_hash[rec] = c3_fasta_hash(t + b + 1, se - b - 1);
      if (se - b - 1 > 0) memcpy(names + nb, t + b + 1, (size_t)(se - b - 1));
      nb += se - b - 1;
    } else if (kind == C3_FA_SEQ && rec >= 0) {
      memcpy(seqs + sb, t + b, (size_t)(se - b));
      sb += se - b;
    }
    return true;
  });
  name_off[p.v.n_records] = nb; off[p.v.n_records] = sb;
}
}  // namespace

extern "C" int c3_fasta_parse_host(const char* text, int64_t n, int at_eof, char* names, int64_t names_cap, int64_t* name_off,
                                   char* seqs, int64_t bases_cap, int64_t* off, uint64_t* name_hash, int64_t max_records,
                                   c3_fasta_info* info) {
  const int rc = c3_fasta_check_args("c3_fasta_parse_host", text, n, names, names_cap, name_off, seqs, bases_cap, off, name_hash, max_records, info);
  if (rc) return rc;
  const uint8_t* t = (const uint8_t*)text;
  const FaParse p = fa_measure(t, n, at_eof);
  info->n_records = p.v.n_records; info->consumed = p.consumed; info->name_bytes = p.name_bytes; info->base_bytes = p.base_bytes;
  info->departed = p.v.departed;
  if (p.v.n_records > max_records || p.name_bytes > names_cap || p.base_bytes > bases_cap)
    return fa_bad("c3_fasta_parse_host", ": capacity too small (needed sizes in info)", C3_E_LIMIT);
  fa_write(t, n, p, names, name_off, seqs, off, name_hash);
  return C3_E_OK;
}

extern "C" int c3_demux_emit_host(const char* text, int64_t n, int at_eof,
                                  int n_a, const char* a_cat, const int64_t* a_off, const char* a_names, const int64_t* a_name_off,
                                  int n_b, const char* b_cat, const int64_t* b_off, const char* b_names, const int64_t* b_name_off,
                                  char* out, int64_t cap, uint64_t* name_hash, int64_t max_records, c3_demux_info* info) {
  const int rc = c3_demux_emit_check_args("c3_demux_emit_host", text, n, n_a, a_names, a_name_off, n_b, b_names, b_name_off, out, cap, name_hash, max_records, info);
  if (rc) return rc;
  uint8_t tab[256]; int K = 0; const char* msg = "";
  const int rp = c3_demux_prepare(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, &K, &msg);
  if (rp != C3_E_OK) { c3_set_host_error(msg); return rp; }
  const uint8_t* t = (const uint8_t*)text;
  const FaParse p = fa_measure(t, n, at_eof);
  const int64_t R = p.v.n_records;
  info->n_records = R; info->consumed = p.consumed; info->departed = p.v.departed;
  if (R > max_records) return fa_bad("c3_demux_emit_host", ": more records than max_records (needed sizes in info)", C3_E_LIMIT);
  std::vector<char> names((size_t)p.name_bytes + 1), seqs((size_t)p.base_bytes + 1);
  std::vector<int64_t> name_off((size_t)R + 1), off((size_t)R + 1);
  std::vector<uint64_t> hash((size_t)R + 1);
  fa_write(t, n, p, names.data(), name_off.data(), seqs.data(), off.data(), hash.data());
  std::vector<int64_t> kept;
  for (int64_t r = 0; r < R; ++r) if (off[(size_t)r + 1] - off[(size_t)r] > C3_DEMUX_HEAD) kept.push_back(r);
  const int64_t nk = (int64_t)kept.size();
  if (nk > INT32_MAX) return fa_bad("c3_demux_emit_host", ": too many records in one text", C3_E_LIMIT);
  std::vector<char> heads((size_t)nk * C3_DEMUX_HEAD + 1);
  std::vector<int32_t> win((size_t)nk * 2 + 2);
  for (int64_t i = 0; i < nk; ++i) memcpy(&heads[(size_t)i * C3_DEMUX_HEAD], &seqs[(size_t)off[(size_t)kept[(size_t)i]]], C3_DEMUX_HEAD);
  const int rd = c3_demux_host((int)nk, heads.data(), n_a, a_cat, a_off, n_b, b_cat, b_off, win.data(), nullptr);
  if (rd != C3_E_OK) return rd;
  auto ilen = [](const int64_t* no, int32_t w) -> int64_t { return w < 0 ? 0 : no[w + 1] - no[w]; };
  int64_t need = 0;
  for (int64_t i = 0; i < nk; ++i) {
    const size_t r = (size_t)kept[(size_t)i];
    need += c3_demux_rec_len(name_off[r + 1] - name_off[r], off[r + 1] - off[r], ilen(a_name_off, win[2 * (size_t)i]), ilen(b_name_off, win[2 * (size_t)i + 1]));
  }
  info->n_kept = nk; info->out_bytes = need;
  if (need > cap) return fa_bad("c3_demux_emit_host", ": out too small (bytes needed in info)", C3_E_LIMIT);
  for (int64_t r = 0; r < R; ++r) name_hash[r] = hash[(size_t)r];
  char* o = out;
  for (int64_t i = 0; i < nk; ++i) {
    const size_t r = (size_t)kept[(size_t)i];
    const int32_t wa = win[2 * (size_t)i], wb = win[2 * (size_t)i + 1];
    const int64_t nl = name_off[r + 1] - name_off[r], sl = off[r + 1] - off[r], al = ilen(a_name_off, wa), bl = ilen(b_name_off, wb);
    *o++ = '>';
    if (nl) memcpy(o, &names[(size_t)name_off[r]], (size_t)nl);
    o += nl; *o++ = '|';
    if (al) memcpy(o, a_names + a_name_off[wa], (size_t)al);
    o += al; *o++ = '_';
    if (bl) memcpy(o, b_names + b_name_off[wb], (size_t)bl);
    o += bl; *o++ = '\n';
    memcpy(o, &seqs[(size_t)off[r]], (size_t)sl);
    o += sl; *o++ = '\n';
  }
  return C3_E_OK;
}

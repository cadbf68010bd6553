// c3_assign.cpp -- splint assignment from a PSL file, and the PSL rows of the GPU splint finder.  Host code only.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"

// ---- splint assignment from the PSL (bin/preprocess.py:22-45) without per-read Python objects ---------------------
// Rows with qBaseInsert (col 5) < 50 and matches (col 0) > 50 count; per read the row with the most matches wins, the
// earliest row on ties (Python's stable sort with reverse=True keeps the first of equal keys); every splint named by a
// counted row is "seen" (adapter_set).  Rows naming a splint that is not in the splint file are ignored.

struct c3_assign {
  // open-addressing table keyed by the read name: names live in one arena (no per-row allocation), rows are parsed by several
  // threads and inserted in file order (3 M rows: 2.1 s through std::unordered_map<std::string, ...>, ~0.4 s like this)
  struct Slot { uint64_t hash; uint32_t name_off, name_len; float matches; int16_t splint; char strand; char used; };
  std::vector<Slot> slots; size_t mask = 0, n_used = 0;
  std::vector<char> names;
  std::unordered_map<std::string, int> splint_of;
  std::vector<uint8_t> seen;
  int64_t rows_kept = 0;
  static uint64_t hash_of(const char* p, size_t n) { uint64_t h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ull; } return h | 1; }
  void grow() {
    std::vector<Slot> old; old.swap(slots);
    slots.assign(old.empty() ? (size_t)1 << 16 : old.size() * 2, Slot{0, 0, 0, 0.f, 0, 0, 0});
    mask = slots.size() - 1;
    for (const Slot& o : old) if (o.used) { size_t i = (size_t)o.hash & mask; while (slots[i].used) i = (i + 1) & mask; slots[i] = o; }
  }
  Slot* find(const char* p, size_t n, uint64_t h) {
    if (slots.empty()) return nullptr;
    for (size_t i = (size_t)h & mask;; i = (i + 1) & mask) {
      Slot& s = slots[i];
      if (!s.used) return nullptr;
      if (s.hash == h && s.name_len == n && memcmp(names.data() + s.name_off, p, n) == 0) return &s;
    }
  }
  void upsert(const char* p, size_t n, float matches, int16_t splint, char strand) {
    const uint64_t h = hash_of(p, n);
    if (Slot* s = find(p, n, h)) { if (matches > s->matches) { s->matches = matches; s->splint = splint; s->strand = strand; } return; }   // earliest row wins ties
    if ((n_used + 1) * 10 > slots.size() * 6) grow();
    size_t i = (size_t)h & mask;
    while (slots[i].used) i = (i + 1) & mask;
    slots[i] = Slot{h, (uint32_t)names.size(), (uint32_t)n, matches, splint, strand, 1};
    names.insert(names.end(), p, p + n);
    ++n_used;
  }
};

namespace {
struct PslRow { const char* name; uint32_t name_len; float matches; int16_t splint; char strand; };
// rows of [p, e) (whole lines) that count (bin/preprocess.py:32: qBaseInsert < 50 and matches > 50) and name a known splint
void parse_psl_chunk(const char* p, const char* e, const std::unordered_map<std::string, int>& splint_of, std::vector<PslRow>& out) {
  std::string key;
  while (p < e) {
    const char* nl = (const char*)memchr(p, '\n', (size_t)(e - p));
    const char* le = nl ? nl : e;
    const char* lend = le;
    while (lend > p && (lend[-1] == '\r' || lend[-1] == '\n')) --lend;
    if (lend > p) {
      const char* col[21]; size_t len[21]; int nc = 0;
      const char* q = p;
      while (nc < 21) {
        const char* t = (const char*)memchr(q, '\t', (size_t)(lend - q));
        col[nc] = q; len[nc] = t ? (size_t)(t - q) : (size_t)(lend - q); ++nc;
        if (!t) break;
        q = t + 1;
      }
      if (nc >= 14) {
        char tmp[64];
        auto num = [&](int c) { size_t l = std::min(len[c], sizeof(tmp) - 1); memcpy(tmp, col[c], l); tmp[l] = 0; return strtod(tmp, nullptr); };
        const double matches = num(0), gaps = num(5);
        if (gaps < 50 && matches > 50) {
          key.assign(col[13], len[13]);
          auto sp = splint_of.find(key);
          if (sp != splint_of.end()) out.push_back(PslRow{col[9], (uint32_t)len[9], (float)matches, (int16_t)sp->second, len[8] ? col[8][0] : '?'});
        }
      }
    }
    p = nl ? nl + 1 : e;
  }
}
}  // namespace

extern "C" int c3_assign_open(const char* psl_path, int n_splints, const char* const* splint_names, c3_assign** out) {
  if (!psl_path || n_splints <= 0 || !splint_names || !out) return C3_E_ARG;
  FILE* f = fopen(psl_path, "rb");
  if (!f) return C3_E_ARG;
  c3_assign* a = new c3_assign();
  for (int i = 0; i < n_splints; ++i) a->splint_of.emplace(splint_names[i], i);
  a->seen.assign((size_t)n_splints, 0);
  a->grow();
  // the file goes through in slabs of whole lines; every slab is cut at line boundaries into one chunk per thread
  const size_t SLAB = (size_t)256 << 20;
  std::vector<char> buf(SLAB + 1);
  size_t have = 0;
  int T = 8; if (const char* e = getenv("C3_PSL_THREADS")) T = std::max(1, std::min(64, atoi(e)));
  for (;;) {
    const size_t got = fread(buf.data() + have, 1, SLAB - have, f);
    const bool last = got == 0 || have + got < SLAB;
    size_t n = have + got;
    size_t use = n;
    if (!last) { while (use > 0 && buf[use - 1] != '\n') --use; if (use == 0) { buf.resize(buf.size() * 2); have = n; continue; } }   // (a line longer than the slab)
    if (use > 0) {
      std::vector<std::vector<PslRow>> rows((size_t)T);
      std::vector<size_t> cut((size_t)T + 1, use);
      cut[0] = 0;
      for (int k = 1; k < T; ++k) { size_t c = use * (size_t)k / (size_t)T; while (c < use && c > 0 && buf[c - 1] != '\n') ++c; cut[(size_t)k] = std::max(c, cut[(size_t)k - 1]); }
      std::vector<std::thread> th;
      for (int k = 0; k < T; ++k) {
        auto fn = [&, k]() { parse_psl_chunk(buf.data() + cut[(size_t)k], buf.data() + cut[(size_t)k + 1], a->splint_of, rows[(size_t)k]); };
        if (k + 1 < T) th.emplace_back(fn); else fn();
      }
      for (auto& x : th) x.join();
      for (int k = 0; k < T; ++k)                                            // file order: the earliest row keeps a tie
        for (const PslRow& r : rows[(size_t)k]) { a->seen[(size_t)r.splint] = 1; ++a->rows_kept; a->upsert(r.name, r.name_len, r.matches, r.splint, r.strand); }
    }
    if (last) break;
    memmove(buf.data(), buf.data() + use, n - use);
    have = n - use;
  }
  fclose(f);
  *out = a;
  return C3_E_OK;
}

extern "C" void c3_assign_close(c3_assign* a) { delete a; }

// splint row / strand of every read of the group: -1 / '?' when the read has no counted row.  Returns the number of
// assigned reads (>= 0) or a negative c3_err.
extern "C" int c3_assign_batch(const c3_assign* a, const c3_host_batch* b, int16_t* splint_id, char* strand) {
  if (!a || !b || !splint_id || !strand) return C3_E_ARG;
  int n_ok = 0;
  c3_assign* m = const_cast<c3_assign*>(a);                                 // (find() does not modify)
  for (int i = 0; i < b->n; ++i) {
    const char* p = b->names + b->name_off[i]; const size_t n = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const c3_assign::Slot* s = m->find(p, n, c3_assign::hash_of(p, n));
    if (!s) { splint_id[i] = -1; strand[i] = '?'; }
    else { splint_id[i] = s->splint; strand[i] = s->strand == '-' ? '-' : '+'; ++n_ok; }
  }
  return n_ok;
}

// adapter_set of bin/preprocess.py:34,43: flags[s] = 1 when a counted row names splint s
extern "C" int c3_assign_seen(const c3_assign* a, uint8_t* flags, int64_t* rows_kept) {
  if (!a || !flags) return C3_E_ARG;
  memcpy(flags, a->seen.data(), a->seen.size());
  if (rows_kept) *rows_kept = a->rows_kept;
  return C3_E_OK;
}

// ---- PSL rows of the GPU splint finder (c3_scan_splints) written natively ------------------------------------------
// One 21-column row per assigned read of the group, appended to `path`: col 0 = equivalent perfect-match length m of the
// track maximum (match*m*(m+1)/2 = max, capped at the splint length), col 5 = 0, strand, read name, read length, query
// span, splint name / length -- the row psl_row() of c3poa_amd/preprocess.py states in Python.
extern "C" int c3_write_splint_psl(const c3_host_batch* b, const int32_t* table, const int16_t* splint_id, const char* strand,
                                   int n_splints, const char* const* splint_names, const int32_t* splint_lens, int match,
                                   const char* path, int64_t* rows_written) {
  if (!b || !table || !splint_id || !strand || n_splints <= 0 || !splint_names || !splint_lens || match <= 0 || !path) return C3_E_ARG;
  std::string out;
  out.reserve((size_t)b->n * 96);
  int64_t rows = 0;
  char tmp[256];
  for (int i = 0; i < b->n; ++i) {
    const int s = splint_id[i];
    if (s < 0 || s >= n_splints) continue;
    const int rc = strand[i] == '-' ? 1 : 0;
    const int32_t* e = table + (((size_t)i * n_splints + s) * 2 + rc) * 4;
    const long long L = b->off[i + 1] - b->off[i];
    const int S = splint_lens[s];
    const long long score = e[0] > 0 ? e[0] : 0;
    long long m = (long long)((std::sqrt(1.0 + 8.0 * (double)score / (double)match) - 1.0) / 2.0);
    if (m > S) m = S;
    long long q0 = e[1]; if (q0 < 0) q0 = 0; if (q0 > L) q0 = L;
    long long q1 = q0 + S; if (q1 > L) q1 = L;
    int k = snprintf(tmp, sizeof(tmp), "%lld\t%lld\t0\t0\t0\t0\t0\t0\t%c\t", m, (long long)S - m, rc ? '-' : '+');
    out.append(tmp, (size_t)k);
    out.append(b->names + b->name_off[i], (size_t)(b->name_off[i + 1] - b->name_off[i]));
    k = snprintf(tmp, sizeof(tmp), "\t%lld\t%lld\t%lld\t", L, q0, q1);
    out.append(tmp, (size_t)k);
    out.append(splint_names[s]);
    k = snprintf(tmp, sizeof(tmp), "\t%d\t0\t%d\t1\t%d,\t%lld,\t0,\n", S, S, S, q0);
    out.append(tmp, (size_t)k);
    ++rows;
  }
  if (!out.empty()) {
    FILE* f = fopen(path, "ab");
    if (!f) return C3_E_ARG;
    size_t w = fwrite(out.data(), 1, out.size(), f);
    if (fclose(f) != 0 || w != out.size()) return C3_E_ARG;
  }
  if (rows_written) *rows_written = rows;
  return C3_E_OK;
}

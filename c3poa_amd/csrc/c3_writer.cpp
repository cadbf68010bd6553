// c3_writer.cpp -- the writer of the reference's two per-group output files, the consensus FASTQ beside them, their --bgzf
// forms and the appender of finished device streams.  Host code only: no kernels here, nothing here touches the oracle.
//
//   c3_write_group   replaces the file side effects of analyze_reads + determine_consensus
//                    (C3POa.py:141-173, bin/determine_consensus.py:57-77,108-114)
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"
#include "c3_emit.h"

// ---- writer ------------------------------------------------------------------------------------------------------
namespace {

// Output bytes are produced straight into slices of one pooled arena per call (kept across calls: after the first group no
// page of it is faulted in again, nothing grows by copying).  A slice is sized from an upper bound of its records, so the
// appender needs no capacity checks.
struct Out {
  char* p;
  inline void put(char c) { *p++ = c; }
  inline void app(const char* s, size_t n) { memcpy(p, s, n); p += n; }
  inline void num(long long v) {                 // decimal, no allocation
    char t[24]; int k = 0;
    unsigned long long u = v < 0 ? (unsigned long long)(-v) : (unsigned long long)v;
    do { t[k++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) *p++ = '-';
    while (k) *p++ = t[--k];
  }
};

// str(round(sum / n, 2)) of Python: correctly rounded to 2 decimals, then the shortest repr (trailing zeros dropped,
// one decimal kept) -- C3POa.py:168
void avg_qual_text(const char* q, int64_t n, Out& out) {
  unsigned long long sum = 0;
  const unsigned char* u = (const unsigned char*)q;
  for (int64_t i = 0; i < n; ++i) sum += u[i];                 // (vectorises; the -33 per base comes off afterwards)
  const long long tot = (long long)sum - 33LL * n;
  char tmp[64];
  int k = snprintf(tmp, sizeof(tmp), "%.2f", (double)tot / (double)n);
  while (k > 0 && tmp[k - 1] == '0' && k >= 2 && tmp[k - 2] != '.') --k;
  out.app(tmp, (size_t)k);
}

inline void fastq(Out& o, const char* name, size_t nl, long idx, const char* s, const char* q, int64_t b, int64_t e) {
  o.put('@'); o.app(name, nl); o.put('_'); o.num(idx); o.put('\n');
  o.app(s + b, (size_t)(e - b)); o.app("\n+\n", 3); o.app(q + b, (size_t)(e - b)); o.put('\n');
}
inline size_t fastq_bound(size_t nl, int64_t len) { return nl + 2 * (size_t)std::max<int64_t>(len, 0) + 32; }

// which records does read i produce?  (one place for the rules of C3POa.py:115-132 / determine_consensus.py:57-77,108-114)
// (the rule itself is c3_emit_of of c3_emit.h, which k_emit applies as well)
struct Emit { bool any, cons; int ns; };
inline Emit emit_of(const c3_read_result& r, int s, int n_splints, int zero, int64_t clen) {
  const C3EmitDec d = c3_emit_of(r, s, n_splints, zero, clen);
  return Emit{d.any != 0, d.cons != 0, d.ns};
}

}  // namespace

namespace {

// upper bound of the bytes reads [i0, i1) append to the consensus / subread file of every splint
void bound_range(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                 const int16_t* splint_id, int n_splints, int zero, int i0, int i1, size_t* bc, size_t* bs) {
  for (int i = i0; i < i1; ++i) {
    const c3_read_result& r = res[i];
    const int s = splint_id[i];
    const int64_t clen = cons ? cons_off[i + 1] - cons_off[i] : 0;
    const Emit e = emit_of(r, s, n_splints, zero, clen);
    if (!e.any) continue;
    const size_t nl = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const int64_t L = b->off[i + 1] - b->off[i];
    size_t q = 0;
    if (e.ns == 0) q = fastq_bound(nl, r.front_end) + fastq_bound(nl, L - r.tail_beg);
    else {
      for (int k = 0; k < e.ns; ++k) q += fastq_bound(nl, (int64_t)r.sub_end[k] - r.sub_beg[k]);
      if (r.has_front) q += fastq_bound(nl, r.front_end);
      if (r.has_tail) q += fastq_bound(nl, L - r.tail_beg);
    }
    bs[s] += q;
    if (e.cons) bc[s] += nl + (size_t)clen + 96;
  }
}

// records of reads [i0, i1) appended to oc[s] / os[s] (one slice pair per splint)
void format_range(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                  const int16_t* splint_id, int n_splints, int zero, int i0, int i1, Out* oc, Out* os) {
  for (int i = i0; i < i1; ++i) {
    const c3_read_result& r = res[i];
    const int s = splint_id[i];
    const int64_t clen = cons ? cons_off[i + 1] - cons_off[i] : 0;
    const Emit e = emit_of(r, s, n_splints, zero, clen);
    if (!e.any) continue;
    const char* name = b->names + b->name_off[i]; const size_t nl = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const char* seq = b->seqs + b->off[i]; const char* qual = b->quals + b->off[i];
    const int64_t L = b->off[i + 1] - b->off[i];
    const int ns = e.ns;
    Out& fq = os[s];
    if (ns == 0) {
      fastq(fq, name, nl, 0, seq, qual, 0, r.front_end);
      fastq(fq, name, nl, 1, seq, qual, r.tail_beg, L);
    } else {
      for (int k = 0; k < ns; ++k) fastq(fq, name, nl, k + 1, seq, qual, r.sub_beg[k], r.sub_end[k]);
      int j = 0;
      if (r.has_front) { fastq(fq, name, nl, 0, seq, qual, 0, r.front_end); ++j; }
      if (r.has_tail) fastq(fq, name, nl, j == 0 ? 0 : ns + 1, seq, qual, r.tail_beg, L);
    }
    if (e.cons) {
      Out& fa = oc[s];
      fa.put('>'); fa.app(name, nl); fa.put('_');
      avg_qual_text(qual, L, fa);
      fa.put('_'); fa.num((long long)L); fa.put('_'); fa.num(ns);
      fa.put('_'); fa.num((long long)clen); fa.put('\n');
      fa.app(cons + cons_off[i], (size_t)clen); fa.put('\n');
    }
  }
}

// pooled arenas: one per c3_write_group call in flight, grow-only, reused by later calls
struct Arena { char* p = nullptr; size_t cap = 0; };
std::mutex g_arena_mu;
std::vector<Arena> g_arena_free;
Arena arena_get(size_t need) {
  Arena a;
  {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    size_t best = (size_t)-1;
    for (size_t k = 0; k < g_arena_free.size(); ++k)
      if (g_arena_free[k].cap >= need && (best == (size_t)-1 || g_arena_free[k].cap < g_arena_free[best].cap)) best = k;
    if (best == (size_t)-1 && !g_arena_free.empty()) best = 0;                 // too small: take one and grow it
    if (best != (size_t)-1) { a = g_arena_free[best]; g_arena_free.erase(g_arena_free.begin() + (long)best); }
  }
  if (a.cap < need) { free(a.p); a.cap = need + need / 8 + 4096; a.p = (char*)malloc(a.cap); if (!a.p) a.cap = 0; }
  return a;
}
void arena_put(Arena a) { if (a.p) { std::lock_guard<std::mutex> lk(g_arena_mu); g_arena_free.push_back(a); } }

bool pwrite_all(int fd, const char* p, size_t n, off_t at) {
  while (n) {
    ssize_t w = pwrite(fd, p, n, at);
    if (w < 0) { if (errno == EINTR) continue; return false; }
    p += w; n -= (size_t)w; at += w;
  }
  return true;
}

}  // namespace

// Appends the records of one group to <cons_paths[s]> / <sub_paths[s]> (s = splint_id[i]; reads with splint_id < 0 or a
// status that produces no output are skipped).  Record formats and the subread naming asymmetry follow the reference:
// kept subreads _1.._n, first dangling piece _0, second _<n+1> (determine_consensus.py:57-62,69-77); zero-repeat pieces
// _0,_1 are written before the rescue is tried (:108-114); consensus header name_avgQ_rawLen_repeats_consLen (C3POa.py:168-171).
// The group is cut into contiguous read ranges that are formatted and written (pwrite at precomputed offsets) by a few
// threads: record order in the files is read order, exactly as with one thread.
namespace {
// Append reservations per output file: a group's bytes go to [at, at + total) of the file, where `at` is handed out under a
// lock, so the writer threads of several GPU workers can format and pwrite into ONE file concurrently (no part files, no
// merge pass).  c3_writer_reset forgets the table (the caller truncates its files at the start of a run).
std::mutex g_res_mu;
struct ResEntry { off_t next = 0; int inflight = 0; };
struct ResKey { dev_t dev; ino_t ino; bool operator==(const ResKey& o) const { return dev == o.dev && ino == o.ino; } };
struct ResKeyHash { size_t operator()(const ResKey& k) const { return std::hash<unsigned long long>()((unsigned long long)k.dev * 1000003ull ^ (unsigned long long)k.ino); } };
// keyed by the FILE (device, inode), not by the path string: two spellings of one path share one entry, a replaced file
// gets a new one.  An entry only lives while reservations are in flight: once the last writer of a file has finished, the
// next group starts again from the file's real end, so a file truncated between calls is not extended with a hole.
std::unordered_map<ResKey, ResEntry, ResKeyHash> g_res;
bool res_key(int fd, ResKey* k) { struct stat st; if (fstat(fd, &st) != 0) return false; k->dev = st.st_dev; k->ino = st.st_ino; return true; }
off_t reserve_append(int fd, size_t total) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  const off_t end = lseek(fd, 0, SEEK_END);
  ResKey k;
  if (!res_key(fd, &k)) return end;
  ResEntry& e = g_res[k];
  const off_t at = e.inflight > 0 ? std::max(end, e.next) : end;
  e.next = at + (off_t)total; e.inflight++;
  return at;
}
void release_append(int fd) {
  std::lock_guard<std::mutex> lk(g_res_mu);
  ResKey k;
  if (!res_key(fd, &k)) return;
  auto it = g_res.find(k);
  if (it != g_res.end() && --it->second.inflight <= 0) g_res.erase(it);
}
}  // namespace

extern "C" void c3_writer_reset(void) { std::lock_guard<std::mutex> lk(g_res_mu); g_res.clear(); }

namespace {
// phases 0 and 1 of a writer call: the group cut into T contiguous read ranges, each range's records formatted (in
// parallel) into its own (kind, splint) slices of one pooled arena.  Slice x = k * NS + s of thread k: consensus text
// [sc[x], oc[x].p), subread text [ss[x], os[x].p).
struct Formatted {
  int T = 1; size_t NS = 0; Arena ar;
  std::vector<char*> sc, ss; std::vector<Out> oc, os;
  template <class F> void run_all(F&& fn) const {
    std::vector<std::thread> th;
    for (int k = 0; k < T; ++k) { if (k + 1 < T) th.emplace_back(fn, k); else fn(k); }
    for (auto& x : th) x.join();
  }
  size_t len(int kind, size_t x) const { return kind ? (size_t)(os[x].p - ss[x]) : (size_t)(oc[x].p - sc[x]); }
  const char* txt(int kind, size_t x) const { return kind ? ss[x] : sc[x]; }
};
int format_group(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                 const int16_t* splint_id, int n_splints, int zero, Formatted& f) {
  int T = 1;
  if (b->n >= 4096) { T = 8; if (const char* e = getenv("C3_WRITER_THREADS")) T = std::max(1, std::min(64, atoi(e))); }
  f.T = T;
  const size_t NS = f.NS = (size_t)n_splints;
  auto range = [&](int k, int* i0, int* i1) { *i0 = (int)((int64_t)b->n * k / T); *i1 = (int)((int64_t)b->n * (k + 1) / T); };
  // phase 0: size of every (thread, kind, splint) slice from an upper bound of its records; one pooled arena holds them all
  std::vector<size_t> bc((size_t)T * NS, 0), bs((size_t)T * NS, 0);
  f.run_all([&](int k) { int i0, i1; range(k, &i0, &i1); bound_range(b, res, cons, cons_off, splint_id, n_splints, zero, i0, i1, &bc[(size_t)k * NS], &bs[(size_t)k * NS]); });
  size_t need = 64;
  for (size_t x : bc) need += x;
  for (size_t x : bs) need += x;
  f.ar = arena_get(need);
  if (!f.ar.p) return C3_E_NOMEM;
  f.sc.resize((size_t)T * NS); f.ss.resize((size_t)T * NS);             // slice starts
  { char* p = f.ar.p; for (size_t x = 0; x < (size_t)T * NS; ++x) { f.sc[x] = p; p += bc[x]; f.ss[x] = p; p += bs[x]; } }
  f.oc.resize((size_t)T * NS); f.os.resize((size_t)T * NS);
  for (size_t x = 0; x < (size_t)T * NS; ++x) { f.oc[x].p = f.sc[x]; f.os[x].p = f.ss[x]; }
  // phase 1: format (parallel), straight into the slices
  f.run_all([&](int k) { int i0, i1; range(k, &i0, &i1); format_range(b, res, cons, cons_off, splint_id, n_splints, zero, i0, i1, &f.oc[(size_t)k * NS], &f.os[(size_t)k * NS]); });
  return C3_E_OK;
}

// R2C2_Consensus.fastq text of splint s (the consensus records of c3_write_group, emit_of, same header, with the QV line)
size_t format_consensus_fastq(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                              const char* qv, const int16_t* splint_id, int n_splints, int zero, int s, char* buf) {
  Out o{buf};
  for (int i = 0; i < b->n; ++i) {
    if (splint_id[i] != s) continue;
    const int64_t clen = cons_off[i + 1] - cons_off[i];
    const Emit e = emit_of(res[i], s, n_splints, zero, clen);
    if (!e.cons) continue;
    const char* name = b->names + b->name_off[i]; const size_t nl = (size_t)(b->name_off[i + 1] - b->name_off[i]);
    const int64_t L = b->off[i + 1] - b->off[i];
    o.put('@'); o.app(name, nl); o.put('_');
    avg_qual_text(b->quals + b->off[i], L, o);
    o.put('_'); o.num((long long)L); o.put('_'); o.num(e.ns);
    o.put('_'); o.num((long long)clen); o.put('\n');
    o.app(cons + cons_off[i], (size_t)clen); o.app("\n+\n", 3);
    o.app(qv + cons_off[i], (size_t)clen); o.put('\n');
  }
  return (size_t)(o.p - buf);
}
std::vector<size_t> consensus_fastq_bounds(const c3_host_batch* b, const c3_read_result* res, const int64_t* cons_off,
                                           const int16_t* splint_id, int n_splints, int zero) {
  std::vector<size_t> bound((size_t)n_splints, 0);
  for (int i = 0; i < b->n; ++i) {
    const int64_t clen = cons_off[i + 1] - cons_off[i];
    const Emit e = emit_of(res[i], splint_id[i], n_splints, zero, clen);
    if (e.cons) bound[(size_t)splint_id[i]] += (size_t)(b->name_off[i + 1] - b->name_off[i]) + 2 * (size_t)clen + 96;
  }
  return bound;
}

// compressed bytes of one file: appended at a reserved range of the compressed file, by T threads (one contiguous piece each,
// as c3_write_group's phase 2 does)
bool append_file(const char* path, const char* p, size_t n, const Formatted* f = nullptr) {
  const int fd = open(path, O_WRONLY | O_CREAT, 0644);
  if (fd < 0) return false;
  const off_t at = reserve_append(fd, n);
  bool ok = true;
  if (f && f->T > 1 && n >= ((size_t)1 << 20)) {
    const int T = f->T;
    std::vector<char> good((size_t)T, 1);
    f->run_all([&](int k) {
      const size_t b = n * (size_t)k / (size_t)T, e = n * (size_t)(k + 1) / (size_t)T;
      if (!pwrite_all(fd, p + b, e - b, at + (off_t)b)) good[(size_t)k] = 0;
    });
    for (char g : good) ok = ok && g;
  } else {
    ok = pwrite_all(fd, p, n, at);
  }
  release_append(fd);
  if (close(fd) != 0) ok = false;
  return ok;
}
}  // namespace


extern "C" int c3_write_group(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                              const int16_t* splint_id, int n_splints, const char* const* cons_paths,
                              const char* const* sub_paths, int zero) {
  if (!b || !res || !cons_off || !splint_id || n_splints <= 0 || !cons_paths || !sub_paths) return C3_E_ARG;
  Formatted f;
  int rc = format_group(b, res, cons, cons_off, splint_id, n_splints, zero, f);
  if (rc) return rc;
  const int T = f.T; const size_t NS = f.NS;
  if (getenv("C3_WRITER_NO_IO")) { arena_put(f.ar); return C3_E_OK; }      // diagnostic (tools/formatter_throughput.py): the formatter alone
  // phase 2: one pwrite stream per (thread, file), offsets from the current file size
  struct Job { int fd; const char* txt; size_t len; off_t at; };
  std::vector<std::vector<Job>> jobs((size_t)T);
  std::vector<int> fds;
  bool ok = true;
  for (int s = 0; s < n_splints && ok; ++s) {
    for (int kind = 0; kind < 2 && ok; ++kind) {
      const char* path = kind ? sub_paths[s] : cons_paths[s];
      size_t total = 0;
      for (int k = 0; k < T; ++k) total += f.len(kind, (size_t)k * NS + (size_t)s);
      if (!total || !path) continue;
      int fd = open(path, O_WRONLY | O_CREAT, 0644);
      if (fd < 0) { ok = false; break; }
      fds.push_back(fd);
      off_t at = reserve_append(fd, total);                 // several writer threads (one per GPU worker) append to one file
      for (int k = 0; k < T; ++k) {
        const size_t x = (size_t)k * NS + (size_t)s;
        const size_t len = f.len(kind, x);
        if (len) { jobs[(size_t)k].push_back({fd, f.txt(kind, x), len, at}); at += (off_t)len; }
      }
    }
  }
  if (ok) {
    std::vector<char> good((size_t)T, 1);
    f.run_all([&](int k) { for (const Job& j : jobs[(size_t)k]) if (!pwrite_all(j.fd, j.txt, j.len, j.at)) good[(size_t)k] = 0; });
    for (char g : good) ok = ok && g;
  }
  arena_put(f.ar);
  for (int fd : fds) { release_append(fd); if (close(fd) != 0) ok = false; }
  return ok ? C3_E_OK : C3_E_ARG;
}

// --bgzf: the same slices; each file's text of the call (its T slices in record order) is compressed through z as one text
// (the slices land back to back on the device), so the members do not depend on C3_WRITER_THREADS
extern "C" int c3_write_group_bgzf(c3_bgzf* z, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                   const int16_t* splint_id, int n_splints, const char* const* cons_paths,
                                   const char* const* sub_paths, int zero) {
  if (!z || !b || !res || !cons_off || !splint_id || n_splints <= 0 || !cons_paths || !sub_paths) return C3_E_ARG;
  Formatted f;
  int rc = format_group(b, res, cons, cons_off, splint_id, n_splints, zero, f);
  if (rc) return rc;
  const int T = f.T; const size_t NS = f.NS;
  std::vector<const char*> pp((size_t)T);
  std::vector<int64_t> pl((size_t)T);
  Arena zb;
  for (int s = 0; s < n_splints && rc == C3_E_OK; ++s) {
    for (int kind = 0; kind < 2 && rc == C3_E_OK; ++kind) {
      const char* path = kind ? sub_paths[s] : cons_paths[s];
      int64_t total = 0;
      for (int k = 0; k < T; ++k) { const size_t x = (size_t)k * NS + (size_t)s; pp[(size_t)k] = f.txt(kind, x); pl[(size_t)k] = (int64_t)f.len(kind, x); total += pl[(size_t)k]; }
      if (!total || !path) continue;
      const int64_t cap = c3_bgzf_bound(total);
      if (zb.cap < (size_t)cap) { arena_put(zb); zb = arena_get((size_t)cap); if (!zb.p) { rc = C3_E_NOMEM; break; } }
      int64_t clen = 0;
      rc = c3_bgzf_compress_pieces(z, pp.data(), pl.data(), T, zb.p, (int64_t)zb.cap, &clen);
      if (rc == C3_E_OK && !append_file(path, zb.p, (size_t)clen, &f)) rc = C3_E_ARG;
    }
  }
  arena_put(zb);
  arena_put(f.ar);
  return rc;
}

// R2C2_Consensus.fastq beside the FASTA: the consensus records of c3_write_group (emit_of, same header) with the QV line.
// One formatting pass per splint file (the records are a small share of the group's bytes), then c3_write_group's
// reservation of the byte range at the end of the file and one pwrite.
extern "C" int c3_write_consensus_fastq(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                        const char* qv, const int16_t* splint_id, int n_splints, const char* const* fq_paths, int zero) {
  if (!b || !res || !cons || !cons_off || !qv || !splint_id || n_splints <= 0 || !fq_paths) return C3_E_ARG;
  const std::vector<size_t> bound = consensus_fastq_bounds(b, res, cons_off, splint_id, n_splints, zero);
  bool ok = true;
  for (int s = 0; s < n_splints && ok; ++s) {
    if (!bound[(size_t)s] || !fq_paths[s]) continue;
    std::vector<char> buf(bound[(size_t)s]);
    const size_t total = format_consensus_fastq(b, res, cons, cons_off, qv, splint_id, n_splints, zero, s, buf.data());
    if (!total) continue;
    const int fd = open(fq_paths[s], O_WRONLY | O_CREAT, 0644);
    if (fd < 0) { ok = false; break; }
    const off_t at = reserve_append(fd, total);
    if (!pwrite_all(fd, buf.data(), total, at)) ok = false;
    release_append(fd);
    if (close(fd) != 0) ok = false;
  }
  return ok ? C3_E_OK : C3_E_ARG;
}

extern "C" int c3_write_consensus_fastq_bgzf(c3_bgzf* z, const c3_host_batch* b, const c3_read_result* res, const char* cons,
                                             const int64_t* cons_off, const char* qv, const int16_t* splint_id, int n_splints,
                                             const char* const* fq_paths, int zero) {
  if (!z || !b || !res || !cons || !cons_off || !qv || !splint_id || n_splints <= 0 || !fq_paths) return C3_E_ARG;
  const std::vector<size_t> bound = consensus_fastq_bounds(b, res, cons_off, splint_id, n_splints, zero);
  int rc = C3_E_OK;
  for (int s = 0; s < n_splints && rc == C3_E_OK; ++s) {
    if (!bound[(size_t)s] || !fq_paths[s]) continue;
    std::vector<char> buf(bound[(size_t)s]);
    const int64_t total = (int64_t)format_consensus_fastq(b, res, cons, cons_off, qv, splint_id, n_splints, zero, s, buf.data());
    if (!total) continue;
    std::vector<char> zbuf((size_t)c3_bgzf_bound(total));
    int64_t clen = 0;
    rc = c3_bgzf_compress(z, buf.data(), total, zbuf.data(), (int64_t)zbuf.size(), &clen);
    if (rc == C3_E_OK && !append_file(fq_paths[s], zbuf.data(), (size_t)clen)) rc = C3_E_ARG;
  }
  return rc;
}

// --emit gpu: finished streams (c3_emit_group, c3_batch_emit_fetch) appended to their files with the writers' reservation
extern "C" int c3_append_streams(const char* const* paths, const char* arena, const int64_t* stream_off, int n_streams) {
  if (!paths || !stream_off || n_streams < 0) return C3_E_ARG;
  for (int x = 0; x < n_streams; ++x) if (stream_off[x + 1] < stream_off[x] || stream_off[0] < 0) return C3_E_ARG;
  if (n_streams > 0 && stream_off[n_streams] > stream_off[0] && !arena) return C3_E_ARG;
  for (int x = 0; x < n_streams; ++x) {
    const int64_t len = stream_off[x + 1] - stream_off[x];
    if (!len || !paths[x]) continue;
    if (!append_file(paths[x], arena + stream_off[x], (size_t)len)) {      // (the code c3_write_group and its kin return for I/O errors, with the reason)
      const int err = errno;
      char msg[512];
      snprintf(msg, sizeof msg, "c3_append_streams: stream %d: cannot append %lld bytes to %s: %s", x, (long long)len, paths[x], strerror(err));
      c3_set_host_error(msg);
      return C3_E_ARG;
    }
  }
  return C3_E_OK;
}

// c3_gunzip_run.h -- the rule of --gunzip gpu as one host procedure over a backend: member headers and
// trailers, stretches, the chain over the pieces, relaunches, the serial fallback and the CRC bookkeeping.  c3_gunzip_host
// (c3_gunzip.cpp) runs it over plain loops, c3_gunzip (c3_gunzip_dev.hip) over the kernels of k_gunzip.hip, so which piece
// is accepted, relaunched or handed to the fallback can never differ between the two.  Host only.
//
// A backend B gives:
//   int reserve(int64_t symbols, int64_t head, int heads)                the symbol arena of one stretch: symbols for the
//                                                                        first launch, then `heads` slabs of `head` symbols
//   int find(int64_t s0, int64_t s1, int64_t piece, int64_t* cand)      cand[k], k >= 1: the first bit in piece k of [s0, s1)
//                                                                        where a dynamic header parses, or -1
//   int decode(const C3GzJob* jobs, int nj, C3GzRes* res)
//   int begin_output(int64_t bytes)                                      the stretch will deliver this many bytes
//   int finish(const C3GzSeg* segs, int ns, const uint8_t* win0, char* dst, int64_t base, int64_t bytes, uint32_t* crc, int* bad)
//   int put(const char* src, int64_t at, int64_t len)                    bytes the serial fallback made, at byte `at` of the stretch
//              the windows down the chain, then every segment's bytes at dst + seg.out, its CRC-32, and whether a marker
//              of it points in front of its member (bad); base: where the batch begins in the stretch's output (dst is there).
//              A backend that keeps the text elsewhere must still leave the last 32 KiB of the batch at dst.
// Each returns 0 or a c3_err code with the text set.
#pragma once
#include "c3_gunzip.h"
#include "c3_checks.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#define C3_GUNZIP_PIECE_DEFAULT 4096           // compressed bytes per piece (C3_GUNZIP_PIECE, >= 64)
#define C3_GUNZIP_STRETCH_DEFAULT (32 << 20)   // compressed bytes per stretch (C3_GUNZIP_STRETCH)
#define C3_GUNZIP_RELAUNCH_DEFAULT 16          // relaunches per stretch before the serial fallback (C3_GUNZIP_RELAUNCH)
#define C3_GUNZIP_MIN_CAND 1                   // a stretch with fewer candidates goes to the serial fallback whole
#define C3_GUNZIP_SLAB_PER_BYTE 16             // slab symbols per compressed byte between two candidates ...
#define C3_GUNZIP_SLAB_MIN 1024                // ... plus this
#define C3_GUNZIP_FINISH_SEGS 2048             // accepted pieces per window chain + resolve: 64 MiB of windows at most
#define C3_GUNZIP_HEAD_SLAB (4 << 20)          // slab of a relaunched piece (C3_GUNZIP_SLAB caps every slab: test hook)

enum { C3_GZ_AGAIN = 1000 };                   // (internal) the stretch needs more of the file than the caller has brought
enum { C3_GZS_PIECES, C3_GZS_CANDIDATES, C3_GZS_ACCEPTED, C3_GZS_REJECTED, C3_GZS_RELAUNCHES, C3_GZS_FULL_SLABS,
       C3_GZS_FALLBACK_BYTES, C3_GZS_STRETCHES, C3_GZS_N };

int64_t* c3_gunzip_stats_slot();               // c3_gunzip.cpp: the calling thread's counters of its last call

namespace c3gz {

struct Options { int64_t piece, stretch, slab; int relaunch, finish; };
inline int64_t env_num(const char* name, int64_t lo, int64_t hi, int64_t def) {
  const char* e = getenv(name);
  if (!e || !*e) return def;
  const long long v = atoll(e);
  return v < lo ? lo : v > hi ? hi : v;
}
inline Options options(int64_t piece) {
  Options o;
  o.piece = piece > 0 ? std::max<int64_t>(64, piece) : env_num("C3_GUNZIP_PIECE", 64, 1 << 26, C3_GUNZIP_PIECE_DEFAULT);
  o.stretch = env_num("C3_GUNZIP_STRETCH", 64, 1 << 26, C3_GUNZIP_STRETCH_DEFAULT);
  o.slab = env_num("C3_GUNZIP_SLAB", 16, 1 << 24, 1 << 24);
  o.relaunch = (int)env_num("C3_GUNZIP_RELAUNCH", 0, 1024, C3_GUNZIP_RELAUNCH_DEFAULT);
  o.finish = (int)env_num("C3_GUNZIP_FINISH", 1, C3_GUNZIP_FINISH_SEGS, C3_GUNZIP_FINISH_SEGS);      // test hook: batches of a few segments
  return o;
}

// the host policy of c3_gz_piece / c3_gz_header_at: plain loops over the file in memory
struct HostIO {
  const uint8_t* src; int64_t n, base; uint16_t* sym;
  uint32_t word(uint32_t i) const {
    const int64_t at = base + 4ll * i;
    if (at >= n) return 0;
    uint32_t v = 0;
    memcpy(&v, src + at, n - at >= 4 ? 4 : (size_t)(n - at));
    return v;
  }
  void lit(uint32_t b, uint32_t at) { sym[at] = (uint16_t)b; }
  void match(uint32_t len, uint32_t dist, uint32_t at) {
    for (uint32_t i = 0; i < len; ++i) sym[at + i] = at + i >= dist ? sym[at + i - dist] : (uint16_t)(C3_GZ_MARK | (C3_GZ_WIN + at + i - dist));
  }
  void stored(uint32_t pos, uint32_t len, uint32_t at) { for (uint32_t i = 0; i < len; ++i) sym[at + i] = src[base + pos + i]; }
  int lane() const { return 0; }
  int lanes() const { return 1; }
  void sync() {}
  static uint32_t uni(uint32_t v) { return v; }
};

inline void host_decode(const uint8_t* src, int64_t n, const C3GzJob& j, uint16_t* sym, C3InfTab* T, C3GzRes* r) {
  const C3GzRel q = c3_gz_rel(j.start, j.limit, n);
  HostIO io{src, n, q.base, sym};
  c3_gz_piece(io, T, q.sbit, q.total, q.limit, j.cap, r);
  r->stop += 8 * q.base; r->bb += 8 * q.base;
}

// the windows and bytes of segments whose symbols lie in host memory (sym_of(seg) = its first symbol)
template <class SymOf>
inline void host_finish(const C3GzSeg* segs, int ns, SymOf sym_of, const uint8_t* win0, char* dst, uint32_t* crc, int* bad) {
  uint32_t tab[256];
  for (uint32_t t = 0; t < 256; ++t) tab[t] = bgzf_crc_entry(t);
  std::vector<uint8_t> win(win0, win0 + C3_GZ_WIN), nxt(C3_GZ_WIN);
  for (int s = 0; s < ns; ++s) {
    const C3GzSeg& g = segs[s];
    const uint16_t* sym = sym_of(g);
    uint32_t c = 0xFFFFFFFFu; int b = 0;
    for (uint32_t i = 0; i < g.nsym; ++i) {
      const int v = c3_gz_byte(sym[i], win.data(), g.wlen);
      if (v < 0) { b = 1; continue; }
      dst[g.out + i] = (char)v;
      c = tab[(c ^ (uint32_t)v) & 0xFFu] ^ (c >> 8);
    }
    crc[s] = ~c; bad[s] = b;
    if (s + 1 < ns) {
      for (uint32_t i = 0; i < C3_GZ_WIN; ++i) { const int v = c3_gz_next_window(sym, g.nsym, win.data(), g.wlen, i); nxt[i] = (uint8_t)(v < 0 ? 0 : v); }
      win.swap(nxt);
    }
  }
}

// ---- gzip member framing (RFC 1952, zlib's rules) ---------------------------------------------------------------------------
// the header at byte `at`: *data = first byte of the deflate stream.  0, C3_INF_HEADER, or C3_INF_INPUT when the file ends in it
inline int member_header(const uint8_t* s, int64_t n, int64_t at, int64_t* data) {
  if (n - at < 10) return C3_INF_INPUT;
  if (s[at] != 0x1f || s[at + 1] != 0x8b || s[at + 2] != 8 || (s[at + 3] & 0xE0)) return C3_INF_HEADER;
  const int flg = s[at + 3];
  int64_t p = at + 10;
  if (flg & 4) {
    if (n - p < 2) return C3_INF_INPUT;
    const int64_t xlen = (int64_t)s[p] | (int64_t)s[p + 1] << 8;
    p += 2;
    if (n - p < xlen) return C3_INF_INPUT;
    p += xlen;
  }
  for (int f = 8; f <= 16; f <<= 1) if (flg & f) {
    while (p < n && s[p]) ++p;
    if (p >= n) return C3_INF_INPUT;
    ++p;
  }
  if (flg & 2) {
    if (n - p < 2) return C3_INF_INPUT;
    uint32_t c = 0xFFFFFFFFu;
    for (int64_t i = at; i < p; ++i) { c ^= s[i]; for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1; }
    if (((~c) & 0xFFFFu) != ((uint32_t)s[p] | (uint32_t)s[p + 1] << 8)) return C3_INF_HEADER;
    p += 2;
  }
  *data = p;
  return C3_INF_OK;
}

inline int data_error(const char* who, int64_t member, int64_t offset, int reason) {
  char buf[200];
  snprintf(buf, sizeof buf, "%s: member %lld at offset %lld is damaged (%s)", who, (long long)member, (long long)offset, c3_inflate_reason(reason));
  c3_set_host_error(buf);
  return C3_E_DATA;
}

template <class B>
struct Run {
  const char* who; B& be; const uint8_t* src; int64_t n; char* dst; int64_t cap; Options opt; int64_t* st;
  int64_t o = 0;                                             // bytes delivered
  int64_t member = 0, member_at = 0; uint64_t mlen = 0; uint32_t mcrc = 0;      // the open member: index, offset, bytes and CRC so far
  uint32_t x2n[36];
  bool more = false;                                         // [src, src + n) is the front of a longer file: running out of it is C3_GZ_AGAIN, not damage
  std::vector<char>* grow = nullptr;                         // the reader's stream: dst is this buffer and grows with the stretch
  struct End { int seg; uint32_t crc, isize; int64_t member, at; };             // a member ends behind segment seg

  int short_input() { return more ? (int)C3_GZ_AGAIN : data_error(who, member, member_at, C3_INF_INPUT); }
  int too_small() { c3_set_host_error((std::string(who) + ": cap < inflated size").c_str()); return C3_E_ARG; }
  void window_at(int64_t end, uint8_t* win) const {          // the 32 KiB in front of output byte `end`
    const int64_t k = std::min<int64_t>(C3_GZ_WIN, end);
    memset(win, 0, C3_GZ_WIN - (size_t)k);
    memcpy(win + C3_GZ_WIN - k, dst + end - k, (size_t)k);
  }
  // the trailer behind a final block that ended at bit `stop`, and the next member's header: *pos = the next true bit
  // position, -1 at the end of the file
  int member_end(int64_t stop, End* e, int64_t* pos) {
    const int64_t t = (stop + 7) >> 3;
    if (n - t < 8 || (more && t + 8 == n)) return short_input();
    e->crc = (uint32_t)src[t] | (uint32_t)src[t + 1] << 8 | (uint32_t)src[t + 2] << 16 | (uint32_t)src[t + 3] << 24;
    e->isize = (uint32_t)src[t + 4] | (uint32_t)src[t + 5] << 8 | (uint32_t)src[t + 6] << 16 | (uint32_t)src[t + 7] << 24;
    e->member = member; e->at = member_at;
    ++member; member_at = t + 8;
    if (t + 8 == n) { *pos = -1; return 0; }
    int64_t data = 0;
    const int why = member_header(src, n, t + 8, &data);
    if (why) return why == C3_INF_INPUT ? short_input() : data_error(who, member, member_at, why);
    *pos = 8 * data;
    return 0;
  }
  // segments [s0, s1) are resolved: their CRCs into the members' running CRCs, the trailers of the members that ended
  int settle(const std::vector<C3GzSeg>& segs, int s0, int s1, const uint32_t* crc, const int* bad, const std::vector<End>& ends, size_t* ei,
             const std::vector<int64_t>& seg_member, const std::vector<int64_t>& seg_member_at) {
    for (int s = s0; s < s1; ++s) {
      if (bad[s - s0]) return data_error(who, seg_member[s], seg_member_at[s], C3_INF_DIST);
      mcrc = c3_gz_crc_shift(x2n, segs[s].nsym, mcrc) ^ (segs[s].nsym ? crc[s - s0] : 0u);
      mlen += segs[s].nsym;
      while (*ei < ends.size() && ends[*ei].seg == s) {
        const End& e = ends[*ei];
        if (mcrc != e.crc) return data_error(who, e.member, e.at, C3_INF_CRC);
        if ((uint32_t)mlen != e.isize) return data_error(who, e.member, e.at, mlen < e.isize ? C3_INF_SHORT : C3_INF_LONG);
        mcrc = 0; mlen = 0; ++*ei;
      }
    }
    return 0;
  }

  // one stretch from the true bit position *pos (inside a member's deflate data): on return *pos is the next stretch's, -1 at the end
  // (C3_GZ_AGAIN: nothing has changed; the caller brings more of the file and calls again)
  int stretch(int64_t* pos) {
    const int64_t m0 = member, a0 = member_at;
    int64_t st0[C3_GZS_N];
    memcpy(st0, st, sizeof st0);
    const int rc = stretch_once(pos);
    if (rc == C3_GZ_AGAIN) { member = m0; member_at = a0; memcpy(st, st0, sizeof st0); }
    return rc;
  }
  int stretch_once(int64_t* pos) {
    if (*pos >= 8 * n) return short_input();                 // the file ends where deflate data must follow
    const int64_t s0 = *pos >> 3, s1 = std::min(n, s0 + opt.stretch), end_bit = 8 * s1;
    const int64_t np = (s1 - s0 + opt.piece - 1) / opt.piece;
    st[C3_GZS_STRETCHES]++; st[C3_GZS_PIECES] += np;
    std::vector<int64_t> cand((size_t)np, -1);
    if (np > 1) { const int rc = be.find(s0, s1, opt.piece, cand.data()); if (rc) return rc; }
    std::vector<C3GzJob> jobs;
    jobs.push_back(C3GzJob{*pos, 0, 0, 0, 0});
    for (int64_t k = 1; k < np; ++k) if (cand[(size_t)k] >= 0) { jobs.push_back(C3GzJob{cand[(size_t)k], 0, 0, 0, 0}); st[C3_GZS_CANDIDATES]++; }      // (in piece k, so behind *pos and ascending)
    const int nc = (int)jobs.size();                         // job 0 and the candidates
    bool fallback = nc - 1 < C3_GUNZIP_MIN_CAND;
    auto slab_of = [&](int64_t bits, int64_t least) { return (uint32_t)std::min<int64_t>(opt.slab, std::max<int64_t>(least, (bits >> 3) * C3_GUNZIP_SLAB_PER_BYTE + C3_GUNZIP_SLAB_MIN)); };
    int64_t arena = 0;
    for (int j = 0; j < nc; ++j) {
      jobs[j].limit = j + 1 < nc ? jobs[j + 1].start : end_bit;
      jobs[j].cap = slab_of(jobs[j].limit - jobs[j].start, 0);
      jobs[j].slab = arena; arena += jobs[j].cap;
    }
    const uint32_t head_cap = slab_of(0, C3_GUNZIP_HEAD_SLAB);
    std::vector<C3GzRes> res((size_t)nc);
    std::vector<C3GzSeg> segs; std::vector<End> ends; std::vector<int64_t> seg_member, seg_member_at;
    std::vector<std::unique_ptr<uint16_t[]>> serial;         // symbols of the fallback's segments
    std::vector<const uint16_t*> seg_host;                   // a segment's symbols if the fallback made it, else null
    int64_t bytes = 0, true_pos = *pos; int n_dev = 0;
    uint32_t wlen = (uint32_t)std::min<uint64_t>(C3_GZ_WIN, mlen);
    bool done = false;                                       // the stretch (or the file) is through
    auto accept = [&](int64_t slab, const uint16_t* host, uint32_t nsym) {
      segs.push_back(C3GzSeg{slab, bytes, nsym, wlen}); seg_host.push_back(host); seg_member.push_back(member); seg_member_at.push_back(member_at);
      bytes += nsym; wlen = (uint32_t)std::min<uint64_t>(C3_GZ_WIN, (uint64_t)wlen + nsym);
    };
    // a piece that was reached by the chain: what it gives, and where the true position goes.  1: go on, 0: stretch done
    auto take = [&](const C3GzJob& j, const C3GzRes& r, const uint16_t* host, int* rc) -> int {
      *rc = 0;
      if (r.status == C3_GZ_BAD) { *rc = r.reason == C3_INF_INPUT ? short_input() : data_error(who, member, member_at, r.reason); return 0; }
      const bool full = r.status == C3_GZ_FULL;
      accept(j.slab, host, full ? r.bb_nsym : r.nsym);
      true_pos = full ? r.bb : r.stop;
      if (r.status == C3_GZ_FINAL) {
        End e; e.seg = (int)segs.size() - 1;
        int64_t nxt = 0;
        if ((*rc = member_end(r.stop, &e, &nxt)) != 0) return 0;
        ends.push_back(e);
        wlen = 0;
        if (nxt < 0) { true_pos = -1; return 0; }
        true_pos = nxt;
      }
      return true_pos < end_bit ? 1 : 0;
    };
    if (!fallback) {
      int rc = be.reserve(arena, head_cap, opt.relaunch + 1);
      if (rc) return rc;
      if ((rc = be.decode(jobs.data(), nc, res.data())) != 0) return rc;
      int nxt = 1, relaunches = 0;
      C3GzJob head = jobs[0]; C3GzRes hres = res[0];        // the piece the chain stands on
      for (;;) {
        if (hres.status == C3_GZ_FULL) st[C3_GZS_FULL_SLABS]++;
        const bool stuck = hres.status == C3_GZ_FULL && hres.bb_nsym == 0 && hres.bb == head.start;
        if (stuck && head.cap >= head_cap) { fallback = true; break; }       // not one block fits the largest slab
        if (!stuck) {
          const int go = take(head, hres, nullptr, &rc);
          if (rc) return rc;
          n_dev = (int)segs.size();
          if (!go) { done = true; break; }
        }
        while (nxt < nc && jobs[nxt].start < true_pos) { st[C3_GZS_REJECTED]++; ++nxt; }
        if (!stuck && nxt < nc && jobs[nxt].start == true_pos) {             // the chain holds: bit for bit
          st[C3_GZS_ACCEPTED]++;
          head = jobs[nxt]; hres = res[nxt]; ++nxt;
          continue;
        }
        if (relaunches >= opt.relaunch) { fallback = true; break; }
        ++relaunches; st[C3_GZS_RELAUNCHES]++;
        head = C3GzJob{true_pos, nxt < nc ? jobs[nxt].start : end_bit, arena, head_cap, 0};
        arena += head_cap;
        if ((rc = be.decode(&head, 1, &hres)) != 0) return rc;
      }
      for (; nxt < nc; ++nxt) st[C3_GZS_REJECTED]++;          // what the chain never reached
    } else {
      st[C3_GZS_REJECTED] += nc - 1;
    }
    if (fallback && !done) {                                 // the rest of the stretch, serially, from the true position
      C3InfTab T;
      uint32_t fcap = 1u << 22;
      while (true_pos >= 0 && true_pos < end_bit) {
        std::unique_ptr<uint16_t[]> sym(new uint16_t[fcap]);
        C3GzJob j{true_pos, end_bit, 0, fcap, 0}; C3GzRes r;
        host_decode(src, n, j, sym.get(), &T, &r);
        if (r.status == C3_GZ_FULL && r.bb_nsym == 0 && r.bb == true_pos) {
          if (fcap >= (1u << 30)) return data_error(who, member, member_at, C3_INF_LONG);
          fcap <<= 1;
          continue;
        }
        int rc = 0;
        const size_t before = segs.size();
        const int go = take(j, r, sym.get(), &rc);
        if (rc) return rc;
        st[C3_GZS_FALLBACK_BYTES] += segs.size() > before ? segs.back().nsym : 0;
        serial.push_back(std::move(sym));
        if (!go) break;
      }
    }
    if (bytes > cap - o) {
      if (!grow) return too_small();
      grow->resize((size_t)(o + bytes)); dst = grow->data(); cap = (int64_t)grow->size();
    }
    { const int rc = be.begin_output(bytes); if (rc) return rc; }
    // resolve: the device's segments through the backend, the fallback's here; windows come from the bytes already delivered
    const int ns = (int)segs.size();
    std::vector<uint32_t> crc((size_t)std::max(ns, 1)); std::vector<int> bad((size_t)std::max(ns, 1));
    std::vector<uint8_t> win(C3_GZ_WIN);
    size_t ei = 0;
    // (at most C3_GUNZIP_FINISH_SEGS segments per finish: a window of 32 KiB per segment bounds what the backend holds)
    std::vector<C3GzSeg> part;
    for (int b0 = 0; b0 < n_dev; b0 += opt.finish) {
      const int nb = std::min(opt.finish, n_dev - b0);
      const int64_t base = segs[b0].out;
      part.assign(segs.begin() + b0, segs.begin() + b0 + nb);
      for (C3GzSeg& g : part) g.out -= base;
      window_at(o + base, win.data());                      // the batches before this one have been delivered
      int rc = be.finish(part.data(), nb, win.data(), dst + o + base, base, part[nb - 1].out + part[nb - 1].nsym, crc.data() + b0, bad.data() + b0);
      if (rc) return rc;
    }
    if (n_dev) {
      const int rc = settle(segs, 0, n_dev, crc.data(), bad.data(), ends, &ei, seg_member, seg_member_at);
      if (rc) return rc;
    }
    for (int s = n_dev; s < ns; ++s) {                       // (one at a time: each one's window is the text in front of it)
      window_at(o + segs[s].out, win.data());
      host_finish(&segs[s], 1, [&](const C3GzSeg&) { return seg_host[s]; }, win.data(), dst + o, &crc[0], &bad[0]);
      int rc = settle(segs, s, s + 1, crc.data(), bad.data(), ends, &ei, seg_member, seg_member_at);
      if (rc == 0) rc = be.put(dst + o + segs[s].out, segs[s].out, segs[s].nsym);
      if (rc) return rc;
    }
    o += bytes;
    *pos = true_pos;
    return 0;
  }

  int run(int64_t* out_len) {
    c3_gz_x2n_init(x2n);
    int64_t data = 0;
    const int why = member_header(src, n, 0, &data);
    if (why) return data_error(who, 0, 0, why);
    int64_t pos = 8 * data;
    while (pos >= 0) { const int rc = stretch(&pos); if (rc) return rc; }
    *out_len = o;
    return C3_E_OK;
  }
};

// the argument checks both calls apply before anything runs; 1 = go on, otherwise *rc is the answer
inline int check_args(const char* who, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len, int* rc) {
  if (!out_len || n < 0 || cap < 0 || (n > 0 && !src) || (cap > 0 && !dst)) { c3_set_host_error((std::string(who) + ": bad arguments").c_str()); *rc = C3_E_ARG; return 0; }
  *out_len = 0;
  *rc = C3_E_OK;
  if (n == 0) return 0;
  if (n >= 18) {                                             // the last member's ISIZE, where the file could reach it (1032 : 1 at most)
    const uint8_t* t = (const uint8_t*)src + n - 4;
    const int64_t isize = (int64_t)t[0] | (int64_t)t[1] << 8 | (int64_t)t[2] << 16 | (int64_t)t[3] << 24;
    if (isize <= 1032 * n && cap < isize) { c3_set_host_error((std::string(who) + ": cap < inflated size").c_str()); *rc = C3_E_ARG; return 0; }
  }
  return 1;
}

}  // namespace c3gz

// bam_out_fuzz_host.cpp -- stand-alone sanitizer check of the host statement of k_bamout (c3_emit_group_bam_host,
// c3_bamout.cpp) against the writer whose records it restates as BAM (c3_write_group, c3_write_consensus_fastq, c3_writer.cpp).
// Random groups with random and hostile record tables (as tools/emit_fuzz_host.cpp makes them), names up to and beyond the
// 219-byte limit and names that hold a NUL go through the call; each is either refused (C3_E_ARG or C3_E_LIMIT, with a text)
// or written into an arena of exactly the stated size.  Every record is then decoded by the plain decoder below and walked in
// step with the writer's files of the same arguments: the name is the header text, the bases are the file's bases mapped to
// "=ACMGRSVTWYHKDBN", the qualities are the file's clamped to 0 .. 93 (0xFF without QVs), the tags hold what the name prints.
// Every input array and the arena are heap blocks of exactly the stated size, so AddressSanitizer sees any read or write
// outside them, and the arena must come back completely written.  tools/bam_out_fuzz_host.sh builds and runs it with
// -fsanitize=address,undefined; nothing here touches a GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <random>
#include <string>
#include <vector>
#include "../include/c3poa.h"

static std::string g_err;
void c3_set_host_error(const char* msg) { g_err = msg; }      // the library's c3_handle.hip holds these in the real build
extern "C" const char* c3_last_error(const c3_handle*) { return g_err.c_str(); }
extern "C" const char* c3_version(void) { return "fuzz"; }
// the writer unit also holds the --bgzf writers, which call into the stream unit: never reached here
extern "C" {
int64_t c3_bgzf_bound(int64_t n) { return n + 64; }
int c3_bgzf_compress(c3_bgzf*, const char*, int64_t, char*, int64_t, int64_t*) { return C3_E_NO_DEVICE; }
int c3_bgzf_compress_pieces(c3_bgzf*, const char* const*, const int64_t*, int, char*, int64_t, int64_t*) { return C3_E_NO_DEVICE; }
}

template <class T> static T* exact(const std::vector<T>& v) {  // a heap block of exactly v.size() elements (never null)
  T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
static std::string slurp(const std::string& path) {
  std::string s;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return s;
  char buf[1 << 16];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, k);
  fclose(f);
  return s;
}

// ---- the plain decoder: nothing of the code under test
struct Rec { std::string name, seq, qual, tags; };
static char letter_of(unsigned char c) {
  if (c >= 'a' && c <= 'z') c = (unsigned char)(c - 32);
  return c < 128 && c != 0 && strchr("=ACMGRSVTWYHKDBN", c) ? (char)c : 'N';
}
static int32_t le32(const unsigned char* p) { return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24); }
static const char* decode(const unsigned char* d, int64_t n, std::vector<Rec>& out) {
  int64_t p = 0;
  while (p < n) {
    if (p + 36 > n) return "fixed fields cross the end of the stream";
    const int64_t bs = le32(d + p), end = p + 4 + bs;
    if (bs < 32 || end > n) return "block_size does not chain";
    if (le32(d + p + 4) != -1 || le32(d + p + 8) != -1 || d[p + 13] != 0 || (d[p + 14] | d[p + 15] << 8) != 4680 || (d[p + 16] | d[p + 17]) != 0 ||
        (d[p + 18] | d[p + 19] << 8) != 4 || le32(d + p + 24) != -1 || le32(d + p + 28) != -1 || le32(d + p + 32) != 0) return "a fixed field";
    const int64_t lrn = d[p + 12], ls = le32(d + p + 20), nb = (ls + 1) / 2;
    if (lrn < 1 || ls < 0 || p + 36 + lrn + nb + ls > end) return "fields longer than block_size";
    Rec r;
    r.name.assign((const char*)d + p + 36, (size_t)lrn - 1);
    if (d[p + 36 + lrn - 1] != 0 || memchr(r.name.data(), 0, r.name.size())) return "name not NUL-terminated once";
    const unsigned char* s = d + p + 36 + lrn;
    for (int64_t k = 0; k < ls; ++k) r.seq.push_back("=ACMGRSVTWYHKDBN"[k & 1 ? s[k / 2] & 15 : s[k / 2] >> 4]);
    if ((ls & 1) && (s[nb - 1] & 15)) return "unused low nibble not 0";
    r.qual.assign((const char*)s + nb, (size_t)ls);
    r.tags.assign((const char*)s + nb + ls, (size_t)(end - (p + 36 + lrn + nb + ls)));
    out.push_back(r);
    p = end;
  }
  return nullptr;
}

// record r against the text at *at of a writer's file: <first>name\nSEQ\n[+\nQUAL\n]
static const char* step(const Rec& r, const std::string& text, size_t* at, char first, bool with_qual, bool want_ff) {
  size_t p = *at;
  const size_t n = r.seq.size();
  if (p + 1 + r.name.size() + 1 + n + 1 > text.size() || text[p] != first || text.compare(p + 1, r.name.size(), r.name) != 0 || text[p + 1 + r.name.size()] != '\n') return "name differs from the header";
  p += 2 + r.name.size();
  for (size_t k = 0; k < n; ++k) if (letter_of((unsigned char)text[p + k]) != r.seq[k]) return "a base";
  if (text[p + n] != '\n') return "sequence length";
  p += n + 1;
  if (with_qual) {
    if (p + 2 + n + 1 > text.size() || text[p] != '+' || text[p + 1] != '\n' || text[p + 2 + n] != '\n') return "quality line";
    for (size_t k = 0; k < n; ++k) {
      const int b = (unsigned char)text[p + 2 + k], q = b < 33 ? 0 : b - 33 > 93 ? 93 : b - 33;
      if ((unsigned char)r.qual[k] != q) return "a quality";
    }
    p += n + 3;
  } else if (want_ff) {
    for (size_t k = 0; k < n; ++k) if ((unsigned char)r.qual[k] != 0xFF) return "a quality that is not 0xFF";
  }
  *at = p;
  return nullptr;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 4000;
  const std::string dir = argc > 2 ? argv[2] : ".";
  std::mt19937_64 rng(20261021);
  auto U = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  const int32_t extreme[] = {INT32_MIN, INT32_MIN + 1, -65536, -2, -1, 0, 1, 2, 249, 250, 251, 255, 256, 257, 65536, INT32_MAX - 1, INT32_MAX};
  const int NX = (int)(sizeof(extreme) / sizeof(extreme[0]));
  int64_t bytes = 0, records = 0, refused = 0, refused_names = 0, formatted = 0, differences = 0;
  for (int r = 0; r < rounds; ++r) {
    const int n = (int)U(0, 10), n_splints = (int)U(1, 3), zero = (int)U(0, 1), with_qv = (int)U(0, 1), with_cons = with_qv || U(0, 5);
    const int hostile = (int)U(0, 2);                              // 0: every record inside its read; 1: a few fields spoilt; 2: anything
    const int names_bad = U(0, 9) == 0;                            // a name beyond the limit or with a NUL somewhere in the group
    bool long_name = false, nul_name = false;
    std::vector<char> names, seqs, quals, cons, qv;
    std::vector<int64_t> name_off{0}, off{0}, cons_off{0};
    std::vector<c3_read_result> res((size_t)n);
    std::vector<int16_t> sid;
    for (int i = 0; i < n; ++i) {
      const int L = U(0, 9) == 0 ? 0 : (int)U(1, U(0, 3) ? 80 : 900);
      int nl = U(0, 7) ? (int)U(0, 12) : (int)U(200, 219);
      if (names_bad && U(0, 2) == 0) { nl = (int)U(220, 300); long_name = true; }
      for (int j = 0; j < L; ++j) { seqs.push_back((char)U(0, 255)); const int64_t q = U(0, 254); quals.push_back((char)(q >= 10 ? q + 1 : q)); }      // (any quality byte but '\n')
      for (int j = 0; j < nl; ++j) names.push_back((char)U(0, 3) ? (char)U('!', '~') : (char)U(128, 255));
      if (names_bad && nl > 0 && U(0, 2) == 0) { names[names.size() - 1 - (size_t)U(0, nl - 1)] = 0; nul_name = true; }
      off.push_back((int64_t)seqs.size()); name_off.push_back((int64_t)names.size());
      sid.push_back((int16_t)(U(0, 7) ? U(0, n_splints - 1) : U(-2, n_splints + 1)));
      c3_read_result& x = res[(size_t)i];
      int32_t* w = (int32_t*)&x;
      for (size_t k = 0; k < sizeof(x) / 4; ++k) w[k] = (int32_t)rng();           // the array tails hold anything
      x.status = U(0, 3) ? C3_ST_OK : (int32_t)U(0, 5);
      x.n_sub = U(0, 4) ? (int32_t)U(0, 12) : U(0, 1) ? 0 : (int32_t)U(240, 250);
      x.has_front = (int32_t)U(0, 1); x.has_tail = (int32_t)U(0, 1);
      x.front_end = (int32_t)U(0, L); x.tail_beg = (int32_t)U(0, L);
      for (int k = 0; k < x.n_sub; ++k) { const int64_t b = U(0, L), e = U(b, L); x.sub_beg[k] = (int32_t)b; x.sub_end[k] = (int32_t)e; }
      int clen = x.status == C3_ST_OK && U(0, 5) ? (int)U(0, 300) : 0;
      if (L == 0 && hostile == 0) clen = 0;
      x.cons_len = clen;
      for (int j = 0; j < clen; ++j) { cons.push_back((char)U(0, 255)); const int64_t q = U(0, 254); qv.push_back((char)(q >= 10 ? q + 1 : q)); }
      cons_off.push_back((int64_t)cons.size());
      if (hostile == 0) continue;
      for (int k = (int)U(1, hostile == 2 ? 6 : 2); k > 0; --k) {
        const int32_t v = U(0, 1) ? extreme[U(0, NX - 1)] : (int32_t)U(-3, L + 3);
        switch ((int)U(0, 6)) {
          case 0: x.n_sub = v; break;
          case 1: x.front_end = v; break;
          case 2: x.tail_beg = v; break;
          case 3: x.sub_beg[U(0, 11)] = v; break;
          case 4: x.sub_end[U(0, 11)] = v; break;
          case 5: x.status = v; break;
          default: x.has_front = v; x.has_tail = (int32_t)U(-1, 2); break;
        }
      }
    }
    if (hostile == 2 && n > 1 && U(0, 3) == 0) std::swap(cons_off[(size_t)U(0, n)], cons_off[(size_t)U(0, n)]);      // (may leave it as it was)
    c3_host_batch b;
    memset(&b, 0, sizeof(b));
    b.n = n; b.names = exact(names); b.name_off = exact(name_off); b.seqs = exact(seqs); b.quals = exact(quals); b.off = exact(off);
    c3_read_result* R = exact(res);
    char* C = with_cons ? exact(cons) : nullptr;
    char* Q = with_qv ? exact(qv) : nullptr;
    int64_t* CO = exact(cons_off);
    int16_t* SID = exact(sid);
    const int S = n_splints * 2, KT = with_qv ? 3 : 2;
    std::vector<int64_t> so((size_t)S + 1, -1), so2((size_t)S + 1, -1);
    int64_t nrec = -1, nrec2 = -1;
    g_err.clear();
    int rc = c3_emit_group_bam_host(&b, R, C, CO, Q, SID, n_splints, zero, nullptr, 0, so.data(), &nrec);
    const std::string bam_err = g_err;
    // the text statement refuses what the BAM statement refuses for the record tables (the same check), and nothing else
    std::vector<int64_t> tso((size_t)n_splints * KT + 1, -1);
    int64_t trec = -1;
    const int trc = c3_emit_group_host(&b, R, C, CO, Q, SID, n_splints, zero, nullptr, 0, tso.data(), &trec);
    if (trc == C3_E_ARG) {
      if (rc != C3_E_ARG || hostile == 0 || bam_err.empty()) { fprintf(stderr, "round %d: the text form refuses, the BAM form returns %d (%s)\n", r, rc, bam_err.c_str()); return 1; }
      ++refused;
    } else if (long_name || nul_name) {
      if ((rc != C3_E_LIMIT && rc != C3_E_ARG) || (rc == C3_E_LIMIT && !long_name) || (rc == C3_E_ARG && !nul_name) || bam_err.find("read ") == std::string::npos) {
        fprintf(stderr, "round %d: a bad name returns %d (%s)\n", r, rc, bam_err.c_str()); return 1;
      }
      ++refused_names;
    } else {
      const int64_t need = so[(size_t)S];
      if (rc != (need > 0 ? C3_E_LIMIT : C3_E_OK) || need < 0 || so[0] != 0 || nrec < 0) { fprintf(stderr, "round %d: sizing call rc %d need %lld (%s)\n", r, rc, (long long)need, g_err.c_str()); return 1; }
      unsigned char* arena = (unsigned char*)malloc((size_t)need + (need ? 0 : 1));
      // a sentinel no written byte can be told from is avoided by writing twice with two sentinels and comparing
      unsigned char* arena2 = (unsigned char*)malloc((size_t)need + (need ? 0 : 1));
      memset(arena, 0x5A, (size_t)need); memset(arena2, 0xA5, (size_t)need);
      rc = c3_emit_group_bam_host(&b, R, C, CO, Q, SID, n_splints, zero, (char*)arena, need, so2.data(), &nrec2);
      const int rc2 = c3_emit_group_bam_host(&b, R, C, CO, Q, SID, n_splints, zero, (char*)arena2, need, so2.data(), &nrec2);
      if (rc != C3_E_OK || rc2 != C3_E_OK || so2 != so || nrec2 != nrec) { fprintf(stderr, "round %d: emit call rc %d (%s)\n", r, rc, g_err.c_str()); return 1; }
      if (memcmp(arena, arena2, (size_t)need) != 0) { fprintf(stderr, "round %d: a byte of the arena was not written\n", r); return 1; }
      if (need > 1 && c3_emit_group_bam_host(&b, R, C, CO, Q, SID, n_splints, zero, (char*)arena, need - 1, so2.data(), &nrec2) != C3_E_LIMIT) { fprintf(stderr, "round %d: short arena accepted\n", r); return 1; }
      // the writer, into empty files
      std::vector<std::string> path((size_t)n_splints * KT);
      std::vector<const char*> cp, sp, fp;
      for (size_t x = 0; x < path.size(); ++x) {
        path[x] = dir + "/bam_out_fuzz_" + std::to_string(x / KT) + "_" + std::to_string(x % KT);
        FILE* f = fopen(path[x].c_str(), "wb");
        if (!f) { fprintf(stderr, "cannot create %s\n", path[x].c_str()); return 1; }
        fclose(f);
      }
      for (int s = 0; s < n_splints; ++s) { cp.push_back(path[(size_t)s * KT].c_str()); sp.push_back(path[(size_t)s * KT + 1].c_str()); if (KT == 3) fp.push_back(path[(size_t)s * KT + 2].c_str()); }
      rc = c3_write_group(&b, R, C, CO, SID, n_splints, cp.data(), sp.data(), zero);
      if (rc == C3_E_OK && KT == 3) rc = c3_write_consensus_fastq(&b, R, C, CO, Q, SID, n_splints, fp.data(), zero);
      if (rc != C3_E_OK) { fprintf(stderr, "round %d: the writer failed (%d)\n", r, rc); return 1; }
      int64_t decoded = 0;
      for (int s = 0; s < n_splints; ++s) {
        std::vector<Rec> cr, sr;
        const char* why = decode(arena + so[(size_t)s * 2], so[(size_t)s * 2 + 1] - so[(size_t)s * 2], cr);
        if (!why) why = decode(arena + so[(size_t)s * 2 + 1], so[(size_t)s * 2 + 2] - so[(size_t)s * 2 + 1], sr);
        const std::string fa = slurp(path[(size_t)s * KT]), fq = slurp(path[(size_t)s * KT + 1]), cq = KT == 3 ? slurp(path[(size_t)s * KT + 2]) : std::string();
        size_t a = 0, q = 0, c = 0;
        for (size_t k = 0; k < sr.size() && !why; ++k) { why = step(sr[k], fq, &q, '@', true, false); if (!why && !sr[k].tags.empty()) why = "a subread record with tags"; }
        for (size_t k = 0; k < cr.size() && !why; ++k) {
          why = step(cr[k], fa, &a, '>', false, KT == 2);
          if (!why && KT == 3) why = step(cr[k], cq, &c, '@', true, false);
          if (why) break;
          // the tags against what the name prints: _<avgQ>_<L>_<ns>_<clen>
          const std::string& nm = cr[k].name;
          size_t u3 = nm.rfind('_'), u2 = nm.rfind('_', u3 - 1), u1 = nm.rfind('_', u2 - 1), u0 = nm.rfind('_', u1 - 1);
          const unsigned char* t = (const unsigned char*)cr[k].tags.data();
          if (cr[k].tags.size() != 21 || memcmp(t, "npi", 3) || memcmp(t + 7, "rli", 3) || memcmp(t + 14, "aqf", 3)) { why = "tag layout"; break; }
          float aq; memcpy(&aq, t + 17, 4);
          const double shown = atof(nm.substr(u0 + 1, u1 - u0 - 1).c_str());
          if (le32(t + 3) != atoi(nm.c_str() + u2 + 1) || le32(t + 10) != atoi(nm.c_str() + u1 + 1) || !(aq - shown < 0.00501 && shown - aq < 0.00501)) why = "a tag value";
          if (atoi(nm.c_str() + u3 + 1) != (int)cr[k].seq.size()) why = "clen of the name";
        }
        if (!why && (a != fa.size() || q != fq.size() || c != cq.size())) why = "fewer records than the writer wrote";
        if (why) { fprintf(stderr, "round %d splint %d: %s\n", r, s, why); ++differences; }
        decoded += (int64_t)(cr.size() + sr.size());
      }
      if (decoded != nrec) { fprintf(stderr, "round %d: %lld records decoded, n_records says %lld\n", r, (long long)decoded, (long long)nrec); ++differences; }
      bytes += need; records += nrec; ++formatted;
      free(arena); free(arena2);
    }
    for (const void* p : {(const void*)b.names, (const void*)b.name_off, (const void*)b.seqs, (const void*)b.quals, (const void*)b.off,
                          (const void*)R, (const void*)C, (const void*)Q, (const void*)CO, (const void*)SID}) free((void*)p);
  }
  for (int s = 0; s < 3; ++s) for (int k = 0; k < 3; ++k) unlink((dir + "/bam_out_fuzz_" + std::to_string(s) + "_" + std::to_string(k)).c_str());
  // the header: magic, text length, text, no references
  char hd[256];
  int64_t hl = 0;
  if (c3_bam_out_header(hd, 8, &hl) != C3_E_LIMIT || hl < 12 || c3_bam_out_header(hd, hl, &hl) != C3_E_OK || memcmp(hd, "BAM\1", 4) != 0 ||
      le32((unsigned char*)hd + 4) != hl - 12 || le32((unsigned char*)hd + hl - 4) != 0 || !strstr(std::string(hd + 8, (size_t)hl - 12).c_str(), "VN:fuzz\n")) { fprintf(stderr, "header\n"); ++differences; }
  printf("bam_out_fuzz_host: %d groups, %lld refused for their tables, %lld for a name, %lld decoded and equal to the writer's text (%lld records, %lld bytes), %lld differences\n",
         rounds, (long long)refused, (long long)refused_names, (long long)formatted, (long long)records, (long long)bytes, (long long)differences);
  return differences ? 1 : 0;
}

// emit_fuzz_host.cpp -- stand-alone sanitizer check of the host statement of k_emit (c3_emit_group_host, c3_emit.cpp) against
// the writer it states (c3_write_group, c3_write_consensus_fastq, c3_writer.cpp).  Random groups with random and hostile record
// tables (begins and ends outside the read, negative lengths, n_sub above 250, any int32, falling cons_off) go through the
// call; each is either refused with C3_E_ARG and a text, or formatted into an arena of exactly the stated size whose streams
// equal the files the writer makes of the same arguments.  Every input array and the arena are heap blocks of exactly the
// stated size, so AddressSanitizer sees any read or write outside them, and the arena must come back completely written (a sentinel byte no input holds).
// tools/emit_fuzz_host.sh builds and runs it with -fsanitize=address,undefined; nothing here touches a GPU.
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

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 4000;
  const std::string dir = argc > 2 ? argv[2] : ".";
  std::mt19937_64 rng(20241019);
  auto U = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  const char alpha[] = "ACGTNacgtn*-\x80\xff";
  const int32_t extreme[] = {INT32_MIN, INT32_MIN + 1, -65536, -2, -1, 0, 1, 2, 249, 250, 251, 255, 256, 257, 65536, INT32_MAX - 1, INT32_MAX};
  const int NX = (int)(sizeof(extreme) / sizeof(extreme[0]));
  int64_t bytes = 0, records = 0, refused = 0, formatted = 0;
  for (int r = 0; r < rounds; ++r) {
    const int n = (int)U(0, 10), n_splints = (int)U(1, 3), zero = (int)U(0, 1), with_qv = (int)U(0, 1), with_cons = with_qv || U(0, 5);
    const int hostile = (int)U(0, 2);                              // 0: every record inside its read; 1: a few fields spoilt; 2: anything
    std::vector<char> names, seqs, quals, cons, qv;
    std::vector<int64_t> name_off{0}, off{0}, cons_off{0};
    std::vector<c3_read_result> res((size_t)n);
    std::vector<int16_t> sid;
    for (int i = 0; i < n; ++i) {
      const int L = U(0, 9) == 0 ? 0 : (int)U(1, U(0, 3) ? 80 : 900), nl = (int)U(0, 12);
      for (int j = 0; j < L; ++j) { seqs.push_back(alpha[U(0, (int64_t)sizeof(alpha) - 2)]); const int64_t q = U(0, 254); quals.push_back((char)(q >= 1 ? q + 1 : q)); }      // (any byte but the arena's sentinel)
      for (int j = 0; j < nl; ++j) names.push_back((char)U('a', 'z'));
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
      for (int j = 0; j < clen; ++j) { cons.push_back("ACGT"[U(0, 3)]); qv.push_back((char)U(33, 93)); }
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
    const int K = with_qv ? 3 : 2, S = n_splints * K;
    std::vector<int64_t> so((size_t)S + 1, -1), so2((size_t)S + 1, -1);
    int64_t nrec = -1, nrec2 = -1;
    g_err.clear();
    int rc = c3_emit_group_host(&b, R, C, CO, Q, SID, n_splints, zero, nullptr, 0, so.data(), &nrec);
    if (rc == C3_E_ARG) {
      if (hostile == 0 || g_err.empty()) { fprintf(stderr, "round %d: refused without cause or text (%s)\n", r, g_err.c_str()); return 1; }
      ++refused;
    } else {
      const int64_t need = so[(size_t)S];
      if (rc != (need > 0 ? C3_E_LIMIT : C3_E_OK) || need < 0 || so[0] != 0 || nrec < 0) { fprintf(stderr, "round %d: sizing call rc %d need %lld (%s)\n", r, rc, (long long)need, g_err.c_str()); return 1; }
      char* arena = (char*)malloc((size_t)need + (need ? 0 : 1));
      memset(arena, 1, (size_t)need);
      rc = c3_emit_group_host(&b, R, C, CO, Q, SID, n_splints, zero, arena, need, so2.data(), &nrec2);
      if (rc != C3_E_OK || so2 != so || nrec2 != nrec) { fprintf(stderr, "round %d: emit call rc %d (%s)\n", r, rc, g_err.c_str()); return 1; }
      if (memchr(arena, 1, (size_t)need)) { fprintf(stderr, "round %d: a byte of the arena was not written\n", r); return 1; }
      if (need > 1 && c3_emit_group_host(&b, R, C, CO, Q, SID, n_splints, zero, arena, need - 1, so2.data(), &nrec2) != C3_E_LIMIT) { fprintf(stderr, "round %d: short arena accepted\n", r); return 1; }
      // the writer, into empty files
      std::vector<std::string> path((size_t)S);
      std::vector<const char*> cp, sp, fp;
      for (int s = 0; s < n_splints; ++s)
        for (int k = 0; k < K; ++k) {
          path[(size_t)s * K + k] = dir + "/emit_fuzz_" + std::to_string(s) + "_" + std::to_string(k);
          FILE* f = fopen(path[(size_t)s * K + k].c_str(), "wb");
          if (!f) { fprintf(stderr, "cannot create %s\n", path[(size_t)s * K + k].c_str()); return 1; }
          fclose(f);
        }
      for (int s = 0; s < n_splints; ++s) { cp.push_back(path[(size_t)s * K].c_str()); sp.push_back(path[(size_t)s * K + 1].c_str()); if (K == 3) fp.push_back(path[(size_t)s * K + 2].c_str()); }
      rc = c3_write_group(&b, R, C, CO, SID, n_splints, cp.data(), sp.data(), zero);
      if (rc == C3_E_OK && K == 3) rc = c3_write_consensus_fastq(&b, R, C, CO, Q, SID, n_splints, fp.data(), zero);
      if (rc != C3_E_OK) { fprintf(stderr, "round %d: the writer failed (%d)\n", r, rc); return 1; }
      for (int x = 0; x < S; ++x) {
        const std::string want = slurp(path[(size_t)x]);
        const int64_t len = so[(size_t)x + 1] - so[(size_t)x];
        if ((int64_t)want.size() != len || memcmp(want.data(), arena + so[(size_t)x], (size_t)len) != 0) {
          fprintf(stderr, "round %d: stream %d differs from the writer's file (%lld bytes against %zu)\n", r, x, (long long)len, want.size());
          return 1;
        }
      }
      bytes += need; records += nrec; ++formatted;
      free(arena);
    }
    for (const void* p : {(const void*)b.names, (const void*)b.name_off, (const void*)b.seqs, (const void*)b.quals, (const void*)b.off,
                          (const void*)R, (const void*)C, (const void*)Q, (const void*)CO, (const void*)SID}) free((void*)p);
  }
  for (int s = 0; s < 3; ++s) for (int k = 0; k < 3; ++k) unlink((dir + "/emit_fuzz_" + std::to_string(s) + "_" + std::to_string(k)).c_str());
  printf("emit_fuzz_host: %d groups, %lld refused, %lld formatted like the writer (%lld records, %lld bytes), clean\n", rounds,
         (long long)refused, (long long)formatted, (long long)records, (long long)bytes);
  return 0;
}

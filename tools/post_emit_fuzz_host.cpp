// post_emit_fuzz_host.cpp -- stand-alone sanitizer check of the host statement of k_post (c3_post_emit_host, c3_post.cpp).
// Random batches with random and hostile adapter tables (any int32, the extremes included) go through the call; every input
// array and the arena are heap blocks of exactly the stated size, so AddressSanitizer sees any read or write outside them,
// and the arena must come back completely written (a sentinel byte no input holds).  tools/post_emit_fuzz_host.sh builds and
// runs it with -fsanitize=address,undefined; nothing here touches a GPU.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <string>
#include <vector>
#include "../include/c3poa.h"

static std::string g_err;
void c3_set_host_error(const char* msg) { g_err = msg; }      // the library's c3_handle.hip holds this in the real build

template <class T> static T* exact(const std::vector<T>& v) {  // a heap block of exactly v.size() elements (never null)
  T* p = (T*)malloc(v.size() * sizeof(T) + (v.empty() ? 1 : 0));
  if (!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 3000;
  std::mt19937_64 rng(20240229);
  auto U = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1))); };
  const char alpha[] = "ACGTNacgtnRYKMBDHVUu*-";
  const int32_t extreme[] = {INT32_MIN, INT32_MIN + 1, -65536, -41, -40, -17, -16, -5, -4, -1, 0, 1, 3, 4, 15, 16, 39, 40, 41, 49, 50, 65536, INT32_MAX - 1, INT32_MAX};
  int64_t bytes = 0, kept_total = 0;
  for (int r = 0; r < rounds; ++r) {
    const int n = (int)U(0, 12), n_ad = (int)U(0, 4), has_index = (int)U(0, 1), n_idx = has_index ? (int)U(0, 6) : 0;
    const int n_dest = has_index ? (int)U(1, n_idx + 1) : 1;
    std::vector<char> names, seqs, quals, ad_names, idx_cat;
    std::vector<int64_t> name_off{0}, off{0}, ad_name_off{0}, idx_off{0};
    std::vector<int32_t> table, ad_len, ad_class, idx_dest;
    for (int i = 0; i < n; ++i) {
      const int L = U(0, 9) == 0 ? 0 : (int)U(1, U(0, 3) ? 60 : 700), nl = (int)U(0, 12);
      for (int j = 0; j < L; ++j) { seqs.push_back(alpha[U(0, (int64_t)sizeof(alpha) - 2)]); quals.push_back((char)U(33, 126)); }
      for (int j = 0; j < nl; ++j) names.push_back((char)U('a', 'z'));
      off.push_back((int64_t)seqs.size()); name_off.push_back((int64_t)names.size());
      for (int e = 0; e < n_ad * 2; ++e) {
        const int mode = (int)U(0, 3);
        for (int k = 0; k < 12; ++k) {
          int32_t v;
          if (mode == 0) v = (int32_t)rng();                                           // anything
          else if (mode == 1) v = extreme[U(0, (int64_t)(sizeof(extreme) / sizeof(extreme[0])) - 1)];
          else v = (int32_t)U(-50, L + 90);                                            // near the read
          if (mode >= 2 && k == 0) v = (int32_t)U(15, 90);
          if (mode >= 2 && k == 5) v = (int32_t)U(8, 40);
          if (mode >= 2 && k == 7) v = (int32_t)U(0, 60);
          table.push_back(v);
        }
      }
    }
    for (int a = 0; a < n_ad; ++a) {
      ad_len.push_back(U(0, 5) ? (int32_t)U(0, 60) : extreme[U(0, 23)]);
      ad_class.push_back((int32_t)U(0, 2));
      for (int j = (int)U(0, 14); j > 0; --j) ad_names.push_back((char)U('A', 'Z'));
      ad_name_off.push_back((int64_t)ad_names.size());
    }
    for (int k = 0; k < n_idx; ++k) {
      for (int j = (int)U(0, 32); j > 0; --j) idx_cat.push_back("ACGT"[U(0, 3)]);
      idx_off.push_back((int64_t)idx_cat.size());
      idx_dest.push_back((int32_t)U(0, n_dest - 1));
    }
    c3_post_args a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.names = exact(names); a.name_off = exact(name_off); a.seqs = exact(seqs); a.off = exact(off);
    a.quals = U(0, 1) ? exact(quals) : nullptr;
    a.table = exact(table); a.n_ad = n_ad; a.ad_len = exact(ad_len); a.ad_class = exact(ad_class); a.class5 = (int32_t)U(-1, 2);
    a.ad_names = exact(ad_names); a.ad_name_off = exact(ad_name_off);
    a.has_index = has_index; a.n_idx = n_idx; a.idx_cat = exact(idx_cat); a.idx_off = exact(idx_off); a.idx_dest = exact(idx_dest); a.n_dest = n_dest;
    a.undirectional = (int32_t)U(0, 1); a.trim = (int32_t)U(0, 1); a.barcoded = (int32_t)U(0, 1);
    const int S = 3 * n_dest + 3;
    std::vector<int64_t> so((size_t)S + 1, -1), so2((size_t)S + 1, -1);
    int64_t kept = -1, kept2 = -1;
    int rc = c3_post_emit_host(&a, nullptr, 0, so.data(), &kept);
    const int64_t need = so[(size_t)S];
    if (rc != (need > 0 ? C3_E_LIMIT : C3_E_OK) || need < 0 || so[0] != 0 || kept < 0 || kept > n) { fprintf(stderr, "round %d: sizing call rc %d need %lld (%s)\n", r, rc, (long long)need, g_err.c_str()); return 1; }
    for (int s = 0; s < S; ++s) if (so[(size_t)s + 1] < so[(size_t)s]) { fprintf(stderr, "round %d: stream_off not ascending\n", r); return 1; }
    char* arena = (char*)malloc((size_t)need + (need ? 0 : 1));
    memset(arena, 1, (size_t)need);
    rc = c3_post_emit_host(&a, arena, need, so2.data(), &kept2);
    if (rc != C3_E_OK || so2 != so || kept2 != kept) { fprintf(stderr, "round %d: emit call rc %d (%s)\n", r, rc, g_err.c_str()); return 1; }
    if (memchr(arena, 1, (size_t)need)) { fprintf(stderr, "round %d: a byte of the arena was not written\n", r); return 1; }
    if (need > 1 && c3_post_emit_host(&a, arena, need - 1, so2.data(), &kept2) != C3_E_LIMIT) { fprintf(stderr, "round %d: short arena accepted\n", r); return 1; }
    bytes += need; kept_total += kept;
    free(arena);
    for (const void* p : {(const void*)a.names, (const void*)a.name_off, (const void*)a.seqs, (const void*)a.off, (const void*)a.quals, (const void*)a.table,
                          (const void*)a.ad_len, (const void*)a.ad_class, (const void*)a.ad_names, (const void*)a.ad_name_off, (const void*)a.idx_cat,
                          (const void*)a.idx_off, (const void*)a.idx_dest}) free((void*)p);
  }
  printf("post_emit_fuzz_host: %d batches, %lld reads kept, %lld bytes written, clean\n", rounds, (long long)kept_total, (long long)bytes);
  return 0;
}

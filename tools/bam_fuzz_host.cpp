// Driver of tools/bam_fuzz_host.sh: c3_bam_parse_host (c3poa_amd/csrc/c3_bam.cpp) under AddressSanitizer / UBSan on the cases
// of a file written by the script -- BAM bytes with random cuts and edits (the fixed fields above all) and what the tests' own
// Python statement of the rule makes of each.  The data and every output array are heap blocks of exactly the size the case
// needs, so one byte too many, read or written, is an error.
// case: int64 n, at_start, at_eof, min_len; data; int64 n_records, n_kept, n_short, consumed, name_bytes, base_bytes,
//       header_bytes, bad_at, departed, reason; names, seqs, quals; name_off[n_kept + 1], off[n_kept + 1]
#include "../include/c3poa.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

void c3_set_host_error(const char*) {}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool eq(const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: fuzz CASES\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long n_cases = 0, n_departed = 0, n_limit = 0, by_reason[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (;;) {
    int64_t hd[4];
    if (fread(hd, sizeof hd, 1, f) != 1) break;
    std::vector<char> data((size_t)hd[0]);
    int64_t want[10];
    if (!rd(f, data.data(), data.size()) || !rd(f, want, sizeof want)) { fprintf(stderr, "short case file\n"); return 2; }
    const int64_t nk = want[1], nb = want[4], bb = want[5];
    std::vector<char> wn((size_t)nb), ws((size_t)bb), wq((size_t)bb);
    std::vector<int64_t> wno((size_t)nk + 1), wo((size_t)nk + 1);
    if (!rd(f, wn.data(), wn.size()) || !rd(f, ws.data(), ws.size()) || !rd(f, wq.data(), wq.size()) ||
        !rd(f, wno.data(), wno.size() * 8) || !rd(f, wo.data(), wo.size() * 8)) { fprintf(stderr, "short case file\n"); return 2; }
    // exact-size heap blocks (never a null pointer: a zero-size result still gets a block of one byte)
    char* names = (char*)malloc((size_t)nb + (nb == 0)); char* seqs = (char*)malloc((size_t)bb + (bb == 0)); char* quals = (char*)malloc((size_t)bb + (bb == 0));
    int64_t* name_off = (int64_t*)malloc(((size_t)nk + 1) * 8); int64_t* off = (int64_t*)malloc(((size_t)nk + 1) * 8);
    char* t = (char*)malloc(data.size() + (data.empty() ? 1 : 0));
    if (!data.empty()) memcpy(t, data.data(), data.size());
    c3_bam_info info;
    int rc = c3_bam_parse_host(t, hd[0], (int)hd[1], (int)hd[2], (int)hd[3], names, nb, name_off, seqs, quals, bb, off, nk, &info);
    const int64_t got[10] = {info.n_records, info.n_kept, info.n_short, info.consumed, info.name_bytes, info.base_bytes,
                             info.header_bytes, info.bad_at, info.departed, info.reason};
    bool ok = rc == 0 && eq(got, want, sizeof want) && eq(names, wn.data(), wn.size()) && eq(seqs, ws.data(), ws.size()) &&
              eq(quals, wq.data(), wq.size()) && eq(name_off, wno.data(), wno.size() * 8) && eq(off, wo.data(), wo.size() * 8);
    if (ok && nk > 0) {                                  // one record too few of room: refused, with the same needs
      c3_bam_info lim;
      ok = c3_bam_parse_host(t, hd[0], (int)hd[1], (int)hd[2], (int)hd[3], names, nb, name_off, seqs, quals, bb, off, nk - 1, &lim) == C3_E_LIMIT && lim.n_kept == nk;
      ++n_limit;
    }
    if (!ok) {
      fprintf(stderr, "case %ld differs from the reference (rc %d): got", n_cases, rc);
      for (int k = 0; k < 10; ++k) fprintf(stderr, " %lld/%lld", (long long)got[k], (long long)want[k]);
      fprintf(stderr, "\n");
      return 1;
    }
    n_departed += info.departed;
    if (info.reason >= 0 && info.reason < 9) ++by_reason[info.reason];
    free(names); free(seqs); free(quals); free(name_off); free(off); free(t);
    ++n_cases;
  }
  printf("bam fuzz: %ld cases equal to the reference parser (%ld departures: BLOCK %ld NAME %ld FIELDS %ld FLAG %ld EMPTY %ld NOQUAL %ld TRUNCATED %ld HEADER %ld; "
         "%ld capacity refusals), no sanitizer report\n", n_cases, n_departed, by_reason[1], by_reason[2], by_reason[3], by_reason[4], by_reason[5],
         by_reason[6], by_reason[7], by_reason[8], n_limit);
  return 0;
}

// Driver of tools/demux_emit_fuzz_host.sh: c3_fasta_parse_host and c3_demux_emit_host (c3poa_amd/csrc/c3_fasta.cpp) under
// AddressSanitizer / UBSan on the cases of a file written by the script -- texts with random cuts and byte edits and what the
// tests' own Python parser makes of each.  Every output array is a heap block of exactly the size the result needs, so one
// byte too many is an error.  The index search is not under test here (tests/test_demux_host.py holds c3_demux_host against
// the reference): this program supplies a stand-in with a rule the script applies as well -- the winner of set A is
// head[0] % (n_a + 1) - 1, of set B head[1] % (n_b + 1) - 1 -- so that every index name and the empty field get written.
// case: int64 n, at_eof; text; int64 n_records, consumed, name_bytes, base_bytes, departed; names, seqs;
//       name_off[n_records + 1], off[n_records + 1], hash[n_records]; int64 n_kept, out_bytes; out
#include "../include/c3poa.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

void c3_set_host_error(const char*) {}
int c3_demux_prepare(int, const char*, const int64_t*, int, const char*, const int64_t*, uint8_t*, int* n_codes, const char**) { *n_codes = 0; return C3_E_OK; }
extern "C" int c3_demux_host(int n, const char* heads, int n_a, const char*, const int64_t*, int n_b, const char*, const int64_t*, int32_t* win, uint8_t*) {
  for (int r = 0; r < n; ++r) {
    const unsigned char* h = (const unsigned char*)heads + (size_t)r * C3_DEMUX_HEAD;
    win[2 * r] = (int)(h[0] % (unsigned)(n_a + 1)) - 1; win[2 * r + 1] = (int)(h[1] % (unsigned)(n_b + 1)) - 1;
  }
  return C3_E_OK;
}

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool eq(const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }
template <class T> static T* block(size_t n) { return (T*)malloc(n * sizeof(T) + (n == 0)); }      // never null, never larger than asked

// the index sets of the script (names only matter here)
static const char A_NAMES[] = "xNextera_7";   static const int64_t A_NO[] = {0, 0, 1, 10};
static const std::string B_STR = std::string("T1a name of sixty-four bytes") + std::string(38, '.');
static const char* const B_NAMES = B_STR.c_str(); static const int64_t B_NO[] = {0, 2, 2, 66};
static const char CAT[] = "ACGTGGCCTTAA";     static const int64_t OFF[] = {0, 4, 8, 12};

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: fuzz CASES\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  long n_cases = 0, n_dep[3] = {0, 0, 0}, n_limit = 0, n_kept_all = 0;
  for (;;) {
    int64_t hd[2];
    if (fread(hd, sizeof hd, 1, f) != 1) break;
    std::vector<char> text((size_t)hd[0]);
    int64_t want[5];
    if (!rd(f, text.data(), text.size()) || !rd(f, want, sizeof want)) { fprintf(stderr, "short case file\n"); return 2; }
    const int64_t R = want[0], nb = want[2], bb = want[3];
    std::vector<char> wn((size_t)nb), ws((size_t)bb);
    std::vector<int64_t> wno((size_t)R + 1), wo((size_t)R + 1), we(2);
    std::vector<uint64_t> wh((size_t)R);
    if (!rd(f, wn.data(), wn.size()) || !rd(f, ws.data(), ws.size()) || !rd(f, wno.data(), wno.size() * 8) || !rd(f, wo.data(), wo.size() * 8) ||
        !rd(f, wh.data(), wh.size() * 8) || !rd(f, we.data(), 16)) { fprintf(stderr, "short case file\n"); return 2; }
    std::vector<char> wout((size_t)we[1]);
    if (!rd(f, wout.data(), wout.size())) { fprintf(stderr, "short case file\n"); return 2; }
    char* names = block<char>((size_t)nb); char* seqs = block<char>((size_t)bb);
    int64_t* name_off = block<int64_t>((size_t)R + 1); int64_t* off = block<int64_t>((size_t)R + 1);
    uint64_t* hash = block<uint64_t>((size_t)R);
    char* t = block<char>(text.size());
    if (!text.empty()) memcpy(t, text.data(), text.size());
    c3_fasta_info info;
    int rc = c3_fasta_parse_host(t, hd[0], (int)hd[1], names, nb, name_off, seqs, bb, off, hash, R, &info);
    const int64_t got[5] = {info.n_records, info.consumed, info.name_bytes, info.base_bytes, info.departed};
    bool ok = rc == 0 && eq(got, want, sizeof want) && eq(names, wn.data(), wn.size()) && eq(seqs, ws.data(), ws.size()) &&
              eq(name_off, wno.data(), wno.size() * 8) && eq(off, wo.data(), wo.size() * 8) && eq(hash, wh.data(), wh.size() * 8);
    if (ok && R > 0) {                                   // one record too few of room: refused, with the same needs
      c3_fasta_info lim;
      ok = c3_fasta_parse_host(t, hd[0], (int)hd[1], names, nb, name_off, seqs, bb, off, hash, R - 1, &lim) == C3_E_LIMIT && lim.n_records == R;
      ++n_limit;
    }
    if (!ok) { fprintf(stderr, "case %ld: parse differs from the reference (rc %d)\n", n_cases, rc); return 1; }
    char* out = block<char>(wout.size());
    uint64_t* hash2 = block<uint64_t>((size_t)R);
    c3_demux_info di;
    rc = c3_demux_emit_host(t, hd[0], (int)hd[1], 3, CAT, OFF, A_NAMES, A_NO, 3, CAT, OFF, B_NAMES, B_NO, out, (int64_t)wout.size(), hash2, R, &di);
    ok = rc == 0 && di.n_records == R && di.consumed == want[1] && di.departed == want[4] && di.n_kept == we[0] && di.out_bytes == we[1] &&
         eq(out, wout.data(), wout.size()) && eq(hash2, wh.data(), wh.size() * 8);
    if (ok && !wout.empty()) {                           // one byte too few of room: refused, with the need
      c3_demux_info lim;
      ok = c3_demux_emit_host(t, hd[0], (int)hd[1], 3, CAT, OFF, A_NAMES, A_NO, 3, CAT, OFF, B_NAMES, B_NO, out, (int64_t)wout.size() - 1, hash2, R, &lim) == C3_E_LIMIT &&
           lim.out_bytes == we[1];
      ++n_limit;
    }
    if (!ok) { fprintf(stderr, "case %ld: emit differs from the reference (rc %d)\n", n_cases, rc); return 1; }
    n_dep[info.departed] += 1; n_kept_all += we[0];
    free(names); free(seqs); free(name_off); free(off); free(hash); free(t); free(out); free(hash2);
    ++n_cases;
  }
  printf("demux emit fuzz: %ld cases equal to the reference parser (%ld / %ld departures of kind 1 / 2, %ld records written, %ld capacity refusals), no sanitizer report\n",
         n_cases, n_dep[1], n_dep[2], n_kept_all, n_limit);
  return 0;
}

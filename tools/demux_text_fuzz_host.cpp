// Driver of tools/demux_text_fuzz_host.sh: c3_demux_emit_text_host (c3poa_amd/csrc/c3_dsplit.cpp) under AddressSanitizer / UBSan on
// the cases of a file written by the script -- FASTA and FASTQ texts with random cuts and byte edits, a flag combination, and
// what the tests' own Python models make of each.  Every output array is a heap block of exactly the size the result needs, so
// one byte too many is an error.  The index search is not under test here (tests/test_demux_host.py holds c3_demux_host against
// the reference): this program supplies the stand-in of tools/demux_emit_fuzz_host.cpp, whose rule the script applies as well --
// the winner of set A is head[0] % (n_a + 1) - 1, of set B head[1] % (n_b + 1) - 1 -- so that every stream gets records.  With
// C3_DEMUX_OUT_BGZF the expected streams are c3_bgzf_compress_host of the script's plain ones.
// case: int64 n, at_eof, kind, flags; text; int64 n_records, consumed, departed, n_kept, S; hash[n_records]; int64 len[S]; streams
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
int c3_bgzf_data_error(const char*, int64_t, int) { return C3_E_DATA; }

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }
static bool eq(const void* a, const void* b, size_t n) { return n == 0 || memcmp(a, b, n) == 0; }
template <class T> static T* block(size_t n) { return (T*)malloc(n * sizeof(T) + (n == 0)); }      // never null, never larger than asked

// the index sets of the script (names only matter here)
static const char A_NAMES[] = "xNextera_7";   static const int64_t A_NO[] = {0, 0, 1, 10};
static const std::string B_STR = std::string("T1a name of sixty-four bytes") + std::string(38, '.');
static const int64_t B_NO[] = {0, 2, 2, 66};
static const char CAT[] = "ACGTGGCCTTAA";     static const int64_t OFF[] = {0, 4, 8, 12};

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: fuzz CASES\n"); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  const c3_demux_sets sets = {3, CAT, OFF, A_NAMES, A_NO, 3, CAT, OFF, B_STR.c_str(), B_NO};
  long n_cases = 0, n_kind[5] = {0, 0, 0, 0, 0}, n_dep = 0, n_rec = 0, n_kept_all = 0, n_limit = 0, n_split = 0, n_z = 0, n_arg = 0;
  for (;;) {
    int64_t hd[4];
    if (fread(hd, sizeof hd, 1, f) != 1) break;
    const int kind = (int)hd[2], flags = (int)hd[3];
    std::vector<char> text((size_t)hd[0]);
    int64_t want[5];
    if (!rd(f, text.data(), text.size()) || !rd(f, want, sizeof want)) { fprintf(stderr, "short case file\n"); return 2; }
    const int64_t R = want[0], S = want[4];
    std::vector<uint64_t> wh((size_t)R);
    std::vector<int64_t> wlen((size_t)S);
    if (!rd(f, wh.data(), wh.size() * 8) || !rd(f, wlen.data(), wlen.size() * 8)) { fprintf(stderr, "short case file\n"); return 2; }
    std::vector<std::vector<char>> ws((size_t)S);
    int64_t need = 0, bound = 0;
    for (int64_t s = 0; s < S; ++s) {
      ws[(size_t)s].resize((size_t)wlen[(size_t)s]);
      if (!rd(f, ws[(size_t)s].data(), ws[(size_t)s].size())) { fprintf(stderr, "short case file\n"); return 2; }
      if ((flags & C3_DEMUX_OUT_BGZF) && wlen[(size_t)s]) {                 // the members the statement has to deliver
        const int64_t b = c3_bgzf_bound(wlen[(size_t)s]);
        std::vector<char> z((size_t)b);
        int64_t got = 0;
        if (c3_bgzf_compress_host(ws[(size_t)s].data(), wlen[(size_t)s], z.data(), b, &got) != C3_E_OK) { fprintf(stderr, "case %ld: compressor failed\n", n_cases); return 1; }
        z.resize((size_t)got);
        ws[(size_t)s] = z;
        bound += b;
      }
      need += (int64_t)ws[(size_t)s].size();
    }
    const int64_t cap = (flags & C3_DEMUX_OUT_BGZF) ? bound : need;
    char* t = block<char>(text.size());
    if (!text.empty()) memcpy(t, text.data(), text.size());
    char* arena = block<char>((size_t)cap);
    int64_t* so = block<int64_t>((size_t)S + 1);
    uint64_t* hash = block<uint64_t>((size_t)R);
    c3_demux_text_info info;
    int rc = c3_demux_emit_text_host(t, hd[0], (int)hd[1], kind, flags, &sets, arena, cap, so, hash, R, &info);
    bool ok = rc == 0 && info.n_records == R && info.consumed == want[1] && info.departed == want[2] && info.n_kept == want[3] &&
              info.n_streams == S && info.text_bytes == hd[0] && info.kind == kind && info.out_bytes == need && so[0] == 0 && so[S] == need &&
              eq(hash, wh.data(), wh.size() * 8);
    for (int64_t s = 0; ok && s < S; ++s)
      ok = so[s + 1] - so[s] == (int64_t)ws[(size_t)s].size() && eq(arena + so[s], ws[(size_t)s].data(), ws[(size_t)s].size());
    if (!ok) { fprintf(stderr, "case %ld (kind %d, flags %d): differs from the reference (rc %d)\n", n_cases, kind, flags, rc); return 1; }
    if (cap > 0) {                                       // one byte too few of room: refused, with the need
      c3_demux_text_info lim;
      ok = c3_demux_emit_text_host(t, hd[0], (int)hd[1], kind, flags, &sets, arena, cap - 1, so, hash, R, &lim) == C3_E_LIMIT && so[S] == cap && lim.n_kept == want[3];
      ++n_limit;
    }
    if (ok && R > 0) {                                   // one record too few of room
      c3_demux_text_info lim;
      ok = c3_demux_emit_text_host(t, hd[0], (int)hd[1], kind, flags, &sets, arena, cap, so, hash, R - 1, &lim) == C3_E_LIMIT && lim.n_records == R;
      ++n_limit;
    }
    if (ok && kind == 2) {                               // qualities of a FASTA text: refused
      c3_demux_text_info bad;
      ok = c3_demux_emit_text_host(t, hd[0], (int)hd[1], kind, flags | C3_DEMUX_KEEP_QUALS, &sets, arena, cap, so, hash, R, &bad) == C3_E_ARG;
      ++n_arg;
    }
    if (!ok) { fprintf(stderr, "case %ld (kind %d, flags %d): a refusal differs\n", n_cases, kind, flags); return 1; }
    n_kind[kind] += 1; n_dep += info.departed != 0; n_rec += R; n_kept_all += want[3];
    n_split += (flags & C3_DEMUX_SPLIT) != 0; n_z += (flags & C3_DEMUX_OUT_BGZF) != 0;
    free(t); free(arena); free(so); free(hash);
    ++n_cases;
  }
  printf("demux text fuzz: %ld cases equal to the reference models (%ld FASTA, %ld FASTQ; %ld split, %ld compressed; %ld departures, %ld records parsed, "
         "%ld written; %ld capacity and %ld argument refusals), no sanitizer report\n",
         n_cases, n_kind[2], n_kind[4], n_split, n_z, n_dep, n_rec, n_kept_all, n_limit, n_arg);
  return 0;
}

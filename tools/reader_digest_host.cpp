// reader_digest_host.cpp -- stand-alone digest of what the streaming reader (c3_reader.cpp, c3_reader_bgzf.cpp, c3_bam.cpp) hands
// out: for every input file on the command line (range3:PATH = three byte ranges that tile PATH, through c3_reader_open_range)
// and every point of the grid max_reads {1, 7, 1000} x max_bases {0, one read's length, three reads' lengths} x min_len {0, the
// corpus' fifth-shortest length} x n_sets {1, 3} x names_only {0, 1} it takes one line per c3_reader_next call: n, n_short, a
// hash of the group's five arrays, c3_reader_reserved_bytes, c3_reader_noqual, and at a failure the return code and the
// reader's text.  With -v as the first argument it prints those lines (some ten thousand).  Without, it folds them: one line per
// input and (max_reads, max_bases, min_len) that holds, for n_sets, names_only = (1,0) (1,1) (3,0) (3,1), the number of calls, a hash
// over the calls' lines, the reserved bytes at the end and the last return code; then the input's distinct error texts.
// Two builds of the reader that hand out the same groups from the same buffer sizes print the same bytes either way.
// tools/reader_digest_host.sh builds and runs it with -fsanitize=address,undefined; nothing here touches a GPU: the device calls
// are stand-ins that answer C3_E_NO_DEVICE.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../include/c3poa.h"

static std::string g_err;
void c3_set_host_error(const char* msg) { g_err = msg; }      // the library's c3_handle.hip holds these in the real build
extern "C" const char* c3_last_error(const c3_handle*) { return g_err.c_str(); }
extern "C" {
int c3_bgzf_create(int, c3_bgzf**) { return C3_E_NO_DEVICE; }
void c3_bgzf_destroy(c3_bgzf*) {}
int c3_bgzf_decompress(c3_bgzf*, const char*, int64_t, char*, int64_t, int64_t*) { return C3_E_NO_DEVICE; }
struct c3_fq_stretch;
int c3_bgzf_stretch_parse(c3_bgzf*, int, const char*, int64_t, int64_t, int64_t, int, c3_fq_stretch*) { return C3_E_NO_DEVICE; }
int c3_bgzf_stretch_parse_bam(c3_bgzf*, int, const char*, int64_t, int64_t, int64_t, int, int, c3_fq_stretch*) { return C3_E_NO_DEVICE; }
int c3_bgzf_stretch_fetch(c3_bgzf*, int, int64_t, int64_t, char*, char*, char*) { return C3_E_NO_DEVICE; }
int c3_bgzf_stretch_text(c3_bgzf*, int, int64_t, int64_t, char*) { return C3_E_NO_DEVICE; }
int c3_bgzf_sets_create(c3_bgzf*, int) { return C3_E_NO_DEVICE; }
int c3_bgzf_set_reserve(c3_bgzf*, int, int64_t, int64_t) { return C3_E_NO_DEVICE; }
int c3_bgzf_stretch_stage(c3_bgzf*, int, int64_t, int64_t, char*, int, int64_t) { return C3_E_NO_DEVICE; }
int c3_bgzf_set_get(const c3_bgzf*, int, const char**, const char**, int*) { return C3_E_NO_DEVICE; }
struct c3_gunzip_stream;
int c3_gunzip_stream_open(c3_bgzf*, const char*, c3_gunzip_stream**) { return C3_E_NO_DEVICE; }
int c3_gunzip_stream_next(c3_gunzip_stream*, const char**, int64_t*, int*) { return C3_E_NO_DEVICE; }
int c3_gunzip_stream_next_parse(c3_gunzip_stream*, int, int64_t, int64_t, int*, int64_t*, c3_fq_stretch*) { return C3_E_NO_DEVICE; }
void c3_gunzip_stream_stats(const c3_gunzip_stream*, int64_t*, int) {}
void c3_gunzip_stream_close(c3_gunzip_stream*) {}
}

static uint64_t fnv(uint64_t h, const void* p, size_t n) {
  const unsigned char* u = (const unsigned char*)p;
  for (size_t i = 0; i < n; ++i) { h ^= u[i]; h *= 1099511628211ull; }
  return h;
}
static uint64_t group_hash(const c3_host_batch& b, bool names_only) {
  uint64_t h = 1469598103934665603ull;
  const size_t nn = (size_t)b.name_off[b.n], nb = (size_t)b.off[b.n];
  h = fnv(h, b.name_off, sizeof(int64_t) * ((size_t)b.n + 1));
  h = fnv(h, b.off, sizeof(int64_t) * ((size_t)b.n + 1));
  if (nn) h = fnv(h, b.names, nn);
  if (!names_only && nb) { h = fnv(h, b.seqs, nb); h = fnv(h, b.quals, nb); }
  return h;
}

struct Part { std::string path; int64_t beg, end; bool range; };
static int open_part(const Part& p, int n_sets, c3_reader** r) {
  return p.range ? c3_reader_open_range(p.path.c_str(), n_sets, p.beg, p.end, r) : c3_reader_open(p.path.c_str(), n_sets, r);
}

int main(int argc, char** argv) {
  const bool verbose = argc > 1 && strcmp(argv[1], "-v") == 0;
  for (int a = verbose ? 2 : 1; a < argc; ++a) {
    std::vector<Part> parts;
    std::string arg = argv[a];
    if (arg.rfind("range3:", 0) == 0) {
      const std::string path = arg.substr(7);
      struct stat st;
      if (stat(path.c_str(), &st) != 0) { fprintf(stderr, "cannot stat %s\n", path.c_str()); return 1; }
      const int64_t z = (int64_t)st.st_size;
      for (int k = 0; k < 3; ++k) parts.push_back(Part{path, z * k / 3, k == 2 ? -1 : z * (k + 1) / 3, true});
    } else parts.push_back(Part{arg, 0, -1, false});
    for (const Part& p : parts) {
      const char* base = strrchr(p.path.c_str(), '/');
      base = base ? base + 1 : p.path.c_str();
      // the lengths of the part's reads, in file order, one read per call (so that the reads in front of a failure count)
      std::vector<int64_t> lens;
      {
        c3_reader* r = nullptr;
        if (open_part(p, 1, &r) != C3_E_OK) { fprintf(stderr, "cannot open %s\n", p.path.c_str()); return 1; }
        c3_reader_names_only(r, 1);
        c3_host_batch b;
        while (c3_reader_next(r, 1, 0, 0, &b) == C3_E_OK && b.n == 1) lens.push_back(b.off[1]);
        c3_reader_close(r);
      }
      const int64_t one = lens.empty() ? 1 : lens[0];
      int64_t three = 0;
      for (size_t i = 0; i < lens.size() && i < 3; ++i) three += lens[i];
      std::vector<int64_t> sorted = lens;
      std::sort(sorted.begin(), sorted.end());
      const int64_t fifth = sorted.empty() ? 0 : sorted[std::min<size_t>(4, sorted.size() - 1)];
      const int mrs[3] = {1, 7, 1000};
      const int64_t mbs[3] = {0, one, std::max<int64_t>(three, 1)};
      const int64_t mls[2] = {0, fifth};
      std::vector<std::string> errors;                           // the part's distinct error texts, in order of appearance
      for (int mr : mrs) for (int64_t mb : mbs) for (int64_t ml : mls) {
        if (!verbose) printf("%s [%lld,%lld) %d %lld %lld |", base, (long long)p.beg, (long long)p.end, mr, (long long)mb, (long long)ml);
        for (int n_sets : {1, 3}) for (int names_only : {0, 1}) {
          if (verbose) printf("# %s [%lld,%lld) max_reads %d max_bases %lld min_len %lld n_sets %d names_only %d\n", base, (long long)p.beg,
                              (long long)p.end, mr, (long long)mb, (long long)ml, n_sets, names_only);
          c3_reader* r = nullptr;
          if (open_part(p, n_sets, &r) != C3_E_OK) { fprintf(stderr, "cannot open %s\n", p.path.c_str()); return 1; }
          c3_reader_names_only(r, names_only);
          uint64_t h = 1469598103934665603ull;                   // over the calls' lines, as -v prints them
          int calls = 0, rc = C3_E_OK;
          int64_t reserved = 0;
          char line[1024];
          for (bool more = true; more; ++calls) {
            c3_host_batch b;
            rc = c3_reader_next(r, mr, mb, (int)ml, &b);
            reserved = c3_reader_reserved_bytes(r);
            if (rc != C3_E_OK) {
              snprintf(line, sizeof line, "rc %d reserved %lld noqual %lld lost %d: %s\n", rc, (long long)reserved, (long long)c3_reader_noqual(r),
                       c3_reader_range_lost(r), c3_reader_error(r));
              if (std::find(errors.begin(), errors.end(), c3_reader_error(r)) == errors.end()) errors.push_back(c3_reader_error(r));
            } else snprintf(line, sizeof line, "%d %lld %016llx %lld %lld\n", b.n, (long long)b.n_short,
                            (unsigned long long)group_hash(b, names_only != 0), (long long)reserved, (long long)c3_reader_noqual(r));
            h = fnv(h, line, strlen(line));
            if (verbose) fputs(line, stdout);
            more = rc == C3_E_OK && b.n > 0;
          }
          if (!verbose) printf(" %d %016llx %lld %d", calls, (unsigned long long)h, (long long)reserved, rc);
          c3_reader_close(r);
        }
        if (!verbose) printf("\n");
      }
      if (!verbose) for (const std::string& e : errors) printf("! %s: %s\n", base, e.c_str());
    }
  }
  return 0;
}

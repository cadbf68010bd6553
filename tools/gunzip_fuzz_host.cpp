// gunzip_fuzz_host.cpp -- driver of tools/gunzip_fuzz_host.sh: the host statement of the k_gunzip kernels (c3_gunzip.cpp: the
// procedure of c3_gunzip_run.h over the decoder of c3_gunzip.h) under AddressSanitizer / UBSan on cut and edited gzip files
// at random piece sizes, verdict and bytes held against zlib linked into the same program.  Host code only.
//   gunzip_fuzz_host N_CASES SEED FILE.gz [FILE.gz ...]
#include "../include/c3poa.h"
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_err;
void c3_set_host_error(const char* msg) { g_err = msg; }

// gzread's rule with zlib: members back to back, each with a checked header and trailer, nothing else.  out = what zlib wrote
static bool reference(const std::vector<unsigned char>& m, std::vector<unsigned char>& out) {
  out.clear();
  if (m.empty()) return true;
  z_stream z; memset(&z, 0, sizeof z);
  if (inflateInit2(&z, 15 + 16) != Z_OK) abort();
  z.next_in = const_cast<unsigned char*>(m.data()); z.avail_in = (uInt)m.size();
  unsigned char buf[1 << 16];
  bool ok = false;
  for (;;) {
    z.next_out = buf; z.avail_out = sizeof buf;
    const int rc = inflate(&z, Z_NO_FLUSH);
    out.insert(out.end(), buf, buf + (sizeof buf - z.avail_out));
    if (rc == Z_STREAM_END) {
      if (z.avail_in == 0) { ok = true; break; }
      if (inflateReset(&z) != Z_OK) abort();
      continue;
    }
    if (rc != Z_OK || (z.avail_in == 0 && z.avail_out != 0)) break;      // an error, or the file ends inside a member
  }
  inflateEnd(&z);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s N_CASES SEED FILE.gz [FILE.gz ...]\n", argv[0]); return 2; }
  const long cases = atol(argv[1]);
  std::mt19937_64 rng((unsigned long long)atoll(argv[2]));
  std::vector<std::vector<unsigned char>> files;
  for (int a = 3; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { perror(argv[a]); return 2; }
    files.emplace_back();
    unsigned char buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) files.back().insert(files.back().end(), buf, buf + k);
    fclose(f);
  }
  long accepted = 0, refused = 0, differ = 0, small = 0;
  std::vector<unsigned char> want;
  for (long k = 0; k < cases; ++k) {
    std::vector<unsigned char> m = files[(size_t)k % files.size()];
    const int kind = (int)(rng() % 8);
    if (kind >= 1) {                                                              // (kind 0: the file as it is)
      const int n_flip = kind >= 6 ? 0 : 1 + (int)(rng() % 3);
      for (int j = 0; j < n_flip; ++j) m[(size_t)(rng() % m.size())] ^= (unsigned char)(1 + rng() % 255);
      if (kind == 6) m.resize((size_t)(rng() % m.size()));                       // cut at the end
      if (kind == 7 && m.size() > 64) {                                           // cut out of the middle
        const size_t at = (size_t)(rng() % (m.size() - 32)), len = 1 + (size_t)(rng() % 32);
        m.erase(m.begin() + (long)at, m.begin() + (long)(at + len));
      }
    }
    const bool ref_ok = reference(m, want);
    const int64_t piece = rng() % 4 == 0 ? 64 + (int64_t)(rng() % 64) : 64 + (int64_t)(rng() % 40000);
    // exactly sized heap copies, so that a read past the file or a write past cap is the sanitizer's business
    std::vector<unsigned char> exact(m);
    std::vector<char> dst(ref_ok ? want.size() : want.size() + (1 << 20));
    int64_t n = -1;
    const int rc = c3_gunzip_host((const char*)exact.data(), (int64_t)exact.size(), dst.data(), (int64_t)dst.size(), &n, piece);
    const bool ok = rc == C3_E_OK;
    if (!ok && rc == C3_E_ARG && !ref_ok) { ++small; ++refused; continue; }      // damage that ran past the slack: refused either way
    if (!ok && rc != C3_E_DATA) { fprintf(stderr, "case %ld: rc %d (%s)\n", k, rc, g_err.c_str()); return 1; }
    if (ok != ref_ok || (ok && (n != (int64_t)want.size() || memcmp(dst.data(), want.data(), (size_t)n) != 0))) {
      fprintf(stderr, "case %ld (file %zu, kind %d, piece %lld): zlib %s, host statement %s (%s)\n", k, (size_t)k % files.size(), kind, (long long)piece,
              ref_ok ? "accepts" : "refuses", ok ? "accepts" : "refuses", g_err.c_str());
      ++differ;
    }
    if (ok) ++accepted; else ++refused;
  }
  printf("gunzip_fuzz_host: %ld cases over %zu files: %ld accepted, %ld refused (%ld of them beyond the output slack), %ld differ from zlib\n",
         cases, files.size(), accepted, refused, small, differ);
  return differ ? 1 : 0;
}

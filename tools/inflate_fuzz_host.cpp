// inflate_fuzz_host.cpp -- driver of tools/inflate_fuzz_host.sh: the host statement of k_inflate (c3_inflate.cpp, the decoder
// of c3_inflate.h) under AddressSanitizer / UBSan on damaged members, its verdict held against zlib's.  Host code only.
//   inflate_fuzz_host FILE.gz N_FLIPS [SEED]     FILE.gz: BGZF; every member takes its share of the flips
#include "../include/c3poa.h"
#include "../c3poa_amd/csrc/c3_inflate.h"
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

static std::string g_err;
void c3_set_host_error(const char* msg) { g_err = msg; }

// the contract of include/c3poa.h "BGZF input" with zlib: accepted, and the bytes
static bool reference(const std::vector<unsigned char>& m, std::vector<unsigned char>& out) {
  C3BgzfMember d;
  if (!c3_bgzf_member_at(m.data(), (int64_t)m.size(), 0, &d) || d.poff + d.plen + 8 != m.size()) return false;
  out.assign(65537, 0);
  z_stream z; memset(&z, 0, sizeof z);
  if (inflateInit2(&z, -15) != Z_OK) abort();
  z.next_in = const_cast<unsigned char*>(m.data()) + d.poff; z.avail_in = d.plen;
  z.next_out = out.data(); z.avail_out = 65537;
  const int rc = inflate(&z, Z_FINISH);
  const size_t n = 65537 - z.avail_out;
  inflateEnd(&z);
  out.resize(n);
  return rc == Z_STREAM_END && n == d.isize && crc32(0L, out.data(), (uInt)n) == d.crc;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s FILE.gz N_FLIPS [SEED]\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  std::vector<unsigned char> file;
  unsigned char buf[1 << 16];
  for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) file.insert(file.end(), buf, buf + k);
  fclose(f);
  const long flips = atol(argv[2]);
  std::mt19937_64 rng(argc > 3 ? (unsigned long long)atoll(argv[3]) : 1);
  std::vector<std::vector<unsigned char>> members;
  for (int64_t at = 0; at < (int64_t)file.size();) {
    C3BgzfMember d;
    const uint32_t size = c3_bgzf_member_at(file.data(), (int64_t)file.size(), at, &d);
    if (!size) { fprintf(stderr, "not BGZF at %lld\n", (long long)at); return 2; }
    members.emplace_back(file.begin() + at, file.begin() + at + size);
    at += size;
  }
  long accepted = 0, refused = 0, differ = 0;
  std::vector<unsigned char> want, got(65536 + 1);
  for (long k = 0; k < flips; ++k) {
    std::vector<unsigned char> m = members[(size_t)k % members.size()];
    const int n_flip = 1 + (int)(rng() % 3);
    for (int j = 0; j < n_flip; ++j) m[(size_t)(rng() % m.size())] ^= (unsigned char)(1 + rng() % 255);      // framing bytes included
    if (rng() % 16 == 0 && m.size() > 40) {                                     // sometimes a truncated payload, BSIZE rewritten
      C3BgzfMember d;
      if (c3_bgzf_member_at(m.data(), (int64_t)m.size(), 0, &d) && d.plen > 2) {
        const size_t cut = 1 + rng() % std::min<size_t>(d.plen - 1, 200);
        m.erase(m.end() - 8 - cut, m.end() - 8);
        for (uint32_t q = 12; q + 6 <= d.poff; ++q)
          if (m[q] == 'B' && m[q + 1] == 'C' && m[q + 2] == 2 && m[q + 3] == 0) { m[q + 4] = (unsigned char)((m.size() - 1) & 255); m[q + 5] = (unsigned char)((m.size() - 1) >> 8); break; }
      }
    }
    const bool ref_ok = reference(m, want);
    int64_t n = -1;
    // an exactly sized heap copy, so that a read past the member is the sanitizer's business
    std::vector<unsigned char> exact(m);
    std::vector<char> dst(65536);
    const int rc = c3_bgzf_decompress_host((const char*)exact.data(), (int64_t)exact.size(), dst.data(), (int64_t)dst.size(), &n);
    const bool ok = rc == C3_E_OK;
    if (!ok && rc != C3_E_DATA) { fprintf(stderr, "case %ld: rc %d (%s)\n", k, rc, g_err.c_str()); return 1; }
    if (ok != ref_ok || (ok && (n != (int64_t)want.size() || memcmp(dst.data(), want.data(), (size_t)n) != 0))) {
      fprintf(stderr, "case %ld: zlib %s, host statement %s (%s)\n", k, ref_ok ? "accepts" : "refuses", ok ? "accepts" : "refuses", g_err.c_str());
      ++differ;
    }
    if (ok) ++accepted; else ++refused;
  }
  printf("inflate_fuzz_host: %ld cases over %zu members: %ld accepted, %ld refused, %ld verdicts differ from zlib\n", flips, members.size(), accepted, refused, differ);
  return differ ? 1 : 0;
}

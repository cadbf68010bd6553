// Driver of tools/post_text_fuzz_host.sh: c3_fastx_strict_parse_host (c3poa_amd/csrc/c3_fastx.cpp) under AddressSanitizer / UBSan
// on strict texts of both kinds with random cuts and byte edits (line ends, '>', '@', '+', blanks, bytes >= 0x80 put in or taken
// out), every result held against the plain reimplementation below: the text split into lines first, then records taken `kind`
// lines at a time.  Every buffer, the text included, is a heap block of exactly the size the result needs, so one byte too many
// in either direction is an error.  Nothing here runs on a GPU.
//   post_text_fuzz_host [N_CASES=20000] [SEED=1]
#include "../include/c3poa.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

void c3_set_host_error(const char*) {}

struct Ref { std::vector<std::string> names, seqs, quals; int64_t consumed = 0; int departed = 0; };

static Ref ref_parse(const std::string& t, bool at_eof, int kind) {
  struct Line { std::string s; size_t next; bool high; };
  std::vector<Line> lines;
  size_t at = 0;
  while (at < t.size()) {
    const size_t nl = t.find('\n', at);
    if (nl == std::string::npos && !at_eof) break;
    const size_t end = nl == std::string::npos ? t.size() : nl;
    std::string s = t.substr(at, end - at);
    bool high = false;
    for (unsigned char c : s) high = high || c >= 0x80;
    if (!s.empty() && s.back() == '\r') s.pop_back();
    lines.push_back({s, nl == std::string::npos ? t.size() : nl + 1, high});
    at = lines.back().next;
  }
  Ref r;
  const char lead = kind == 4 ? '@' : '>';
  size_t k = 0;
  for (; k + kind <= lines.size(); k += kind) {
    const std::string &h = lines[k].s, &s = lines[k + 1].s;
    bool ok = !h.empty() && h[0] == lead && !s.empty() && s[0] != '>' && s[0] != '@' && s[0] != '+';
    if (kind == 4) ok = ok && !lines[k + 2].s.empty() && lines[k + 2].s[0] == '+' && lines[k + 3].s.size() == s.size();
    for (int j = 0; j < kind; ++j) ok = ok && !lines[k + j].high;
    if (!ok) { r.departed = 1; return r; }
    r.names.push_back(h.substr(1, h.find_first_of(" \t", 1) == std::string::npos ? std::string::npos : h.find_first_of(" \t", 1) - 1));
    r.seqs.push_back(s);
    r.quals.push_back(kind == 4 ? lines[k + 3].s : std::string());
    r.consumed = (int64_t)lines[k + kind - 1].next;
  }
  if (at_eof && k < lines.size()) r.departed = 1;                   // an incomplete record at the end of the file
  return r;
}

static uint64_t fnv(const std::string& s) {
  uint64_t h = 1469598103934665603ull;
  for (unsigned char c : s) { h ^= c; h *= 1099511628211ull; }
  return h;
}

template <class T> static T* block(size_t n) { return (T*)malloc((n ? n : 1) * sizeof(T)); }      // never null; a zero-size result gets one element

int main(int argc, char** argv) {
  const long n_cases = argc > 1 ? atol(argv[1]) : 20000;
  std::mt19937_64 rng(argc > 2 ? (uint64_t)atoll(argv[2]) : 1);
  auto pick = [&](size_t n) { return (size_t)(rng() % n); };
  const char* edits[] = {"\n", "\r", "\r\n", ">", "@", "+", " ", "\t", "A", "\n\n", "", "\x80", "\xc3\xa9"};
  long n_departed = 0, n_limit = 0, n_records = 0;
  for (long c = 0; c < n_cases; ++c) {
    const int kind = pick(2) ? 4 : 2;
    std::string t;
    const size_t nrec = pick(5);
    const bool crlf = pick(4) == 0;
    for (size_t r = 0; r < nrec; ++r) {
      std::string name = "r" + std::to_string(rng() % 1000), seq, qual;
      if (pick(3) == 0) name += pick(2) ? " a comment" : "\tx=1";
      const size_t L = 1 + pick(pick(6) == 0 ? 300 : 20);
      for (size_t i = 0; i < L; ++i) { seq += "ACGTN"[pick(5)]; qual += (char)(33 + pick(60)); }
      const char* eol = crlf ? "\r\n" : "\n";
      t += (kind == 4 ? "@" : ">") + name + eol + seq + eol;
      if (kind == 4) t += std::string("+") + eol + qual + eol;
    }
    if (!t.empty() && pick(3) == 0) t.pop_back();                   // no final newline
    for (size_t k = pick(4); k > 0; --k) {
      const size_t at = pick(t.size() + 1);
      const std::string e = edits[pick(sizeof edits / sizeof *edits)];
      if (pick(2)) t.insert(at, e); else t.replace(at, at < t.size() ? 1 : 0, e);
    }
    if (pick(3) == 0) t.resize(pick(t.size() + 1));                 // cut
    const bool at_eof = pick(2);
    const Ref want = ref_parse(t, at_eof, kind);
    const size_t R = want.names.size();
    std::string wn, ws, wq;
    std::vector<int64_t> wno(R + 1, 0), wo(R + 1, 0);
    for (size_t r = 0; r < R; ++r) { wn += want.names[r]; ws += want.seqs[r]; wq += want.quals[r]; wno[r + 1] = (int64_t)wn.size(); wo[r + 1] = (int64_t)ws.size(); }
    char* text = block<char>(t.size()); memcpy(text, t.data(), t.size());
    char* names = block<char>(wn.size()); char* seqs = block<char>(ws.size()); char* quals = kind == 4 ? block<char>(ws.size()) : nullptr;
    int64_t* name_off = block<int64_t>(R + 1); int64_t* off = block<int64_t>(R + 1); uint64_t* hash = block<uint64_t>(R);
    c3_fastx_info info;
    const int rc = c3_fastx_strict_parse_host(text, (int64_t)t.size(), at_eof, kind, names, (int64_t)wn.size(), name_off, seqs, quals, (int64_t)ws.size(), off,
                                              hash, (int64_t)R, &info);
    bool ok = rc == 0 && info.n_records == (int64_t)R && info.consumed == want.consumed && info.departed == want.departed &&
              info.name_bytes == (int64_t)wn.size() && info.base_bytes == (int64_t)ws.size() && !memcmp(names, wn.data(), wn.size()) &&
              !memcmp(seqs, ws.data(), ws.size()) && (kind == 2 || !memcmp(quals, wq.data(), wq.size())) &&
              !memcmp(name_off, wno.data(), 8 * (R + 1)) && !memcmp(off, wo.data(), 8 * (R + 1));
    for (size_t r = 0; ok && r < R; ++r) ok = hash[r] == fnv(want.names[r]);
    if (ok && R > 0) {                                              // one record too few of room: refused, with the same needs
      c3_fastx_info lim;
      ok = c3_fastx_strict_parse_host(text, (int64_t)t.size(), at_eof, kind, names, (int64_t)wn.size(), name_off, seqs, quals, (int64_t)ws.size(), off, hash,
                                      (int64_t)R - 1, &lim) == C3_E_LIMIT && lim.n_records == (int64_t)R;
      ++n_limit;
    }
    if (ok && !info.departed && !at_eof)                            // what stays unconsumed holds no whole record
      ok = ref_parse(t.substr((size_t)info.consumed), false, kind).names.empty();
    if (!ok) { fprintf(stderr, "case %ld (kind %d, at_eof %d, %zu bytes) differs from the reference (rc %d)\n", c, kind, (int)at_eof, t.size(), rc); return 1; }
    n_departed += info.departed; n_records += (long)R;
    free(text); free(names); free(seqs); free(quals); free(name_off); free(off); free(hash);
  }
  printf("post text fuzz: %ld cases equal to the reference parser (%ld records, %ld departures, %ld capacity refusals), no sanitizer report\n",
         n_cases, n_records, n_departed, n_limit);
  return 0;
}

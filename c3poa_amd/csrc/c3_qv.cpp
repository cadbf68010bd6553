// c3_qv.cpp -- host statement of the per-base consensus quality values (include/c3poa.h, "per-base consensus quality
// values"; DESIGN.md "Consensus quality values").  Plain C++, no kernels: c3_consensus_qv_host computes the whole band DP of
// every piece with int32 cells and walks the traceback from the H values themselves.  k_qv (k_qv.hip) must match it byte
// for byte.  c3_qv_check holds the refusals both entry points share.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"

namespace {
const int NEG = -(1 << 28);                     // a cell outside the band or the matrix
const int HB = C3_QV_BAND / 2;                  // the band of row i is c(i) - 64 .. c(i) + 63

inline int code_of(char c) {
  switch (c) { case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 0; }
}
inline int q_of(char c) { return std::min(93, std::max(0, (int)(unsigned char)c - 33)); }

// band centre of row i
inline int64_t centre(int mode, int64_t i, int64_t m, int64_t n) { return mode == C3_QV_GLOBAL ? (i * n + m / 2) / m : i; }

// one piece (already reversed for mode 2) against one consensus (likewise): adds its contributions to S[0..n)
void align_piece(const std::vector<int>& C, const std::vector<int>& P, const std::vector<int>& Q, int mode, std::vector<int>& S) {
  const int64_t n = (int64_t)C.size(), m = (int64_t)P.size();
  std::vector<int> H((size_t)(m + 1) * C3_QV_BAND, NEG);
  std::vector<int64_t> lo((size_t)m + 1);
  auto cell = [&](int64_t i, int64_t j) -> int {           // H[i][j], -inf outside the band or the matrix
    if (i < 0 || j < 0 || j > n) return NEG;
    const int64_t t = j - lo[(size_t)i];
    return (t < 0 || t >= C3_QV_BAND) ? NEG : H[(size_t)i * C3_QV_BAND + (size_t)t];
  };
  for (int64_t i = 0; i <= m; ++i) {
    lo[(size_t)i] = centre(mode, i, m, n) - HB;
    for (int t = 0; t < C3_QV_BAND; ++t) {
      const int64_t j = lo[(size_t)i] + t;
      if (j < 0 || j > n) continue;
      int h;
      if (i == 0 && j == 0) h = 0;
      else {
        h = NEG;
        if (i > 0 && j > 0) h = std::max(h, cell(i - 1, j - 1) + (P[(size_t)i - 1] == C[(size_t)j - 1] ? C3_QV_MATCH : C3_QV_MISMATCH));
        if (j > 0) h = std::max(h, cell(i, j - 1) + C3_QV_GAP);
        if (i > 0) h = std::max(h, cell(i - 1, j) + C3_QV_GAP);
        h = std::max(h, NEG);
      }
      H[(size_t)i * C3_QV_BAND + t] = h;
    }
  }
  int64_t ei = m, ej = n;
  if (mode != C3_QV_GLOBAL) {                                 // the band cell of largest H, smallest i, then smallest j
    int best = NEG - 1;
    for (int64_t i = 0; i <= m; ++i)
      for (int t = 0; t < C3_QV_BAND; ++t) {
        const int64_t j = lo[(size_t)i] + t;
        if (j < 0 || j > n) continue;
        const int h = H[(size_t)i * C3_QV_BAND + t];
        if (h > best) { best = h; ei = i; ej = j; }
      }
  }
  // traceback, end cell -> (0,0): record the path as forward-order steps
  enum { DIAG, DEL, INS };
  struct Step { int kind; int64_t i, j; };                    // the cell the step enters
  std::vector<Step> path;
  for (int64_t i = ei, j = ej; i > 0 || j > 0;) {
    const int h = cell(i, j);
    if (i > 0 && j > 0 && h == cell(i - 1, j - 1) + (P[(size_t)i - 1] == C[(size_t)j - 1] ? C3_QV_MATCH : C3_QV_MISMATCH)) { path.push_back({DIAG, i, j}); --i; --j; }
    else if (j > 0 && h == cell(i, j - 1) + C3_QV_GAP) { path.push_back({DEL, i, j}); --j; }
    else { path.push_back({INS, i, j}); --i; }
  }
  std::reverse(path.begin(), path.end());
  const int64_t J = mode == C3_QV_GLOBAL ? n : ej;           // columns 0 .. J-1 are covered
  if (J == 0) return;
  int run = -1;                                               // max q of the insertion run in progress, -1 = none
  int64_t run_j = 0;
  auto flush = [&]() { if (run >= 0) { S[(size_t)std::min(run_j, J - 1)] -= run; run = -1; } };
  for (const Step& s : path) {
    if (s.kind == INS) { run = std::max(run, Q[(size_t)s.i - 1]); run_j = s.j; continue; }
    flush();
    const int64_t p = s.j - 1;
    if (s.kind == DIAG) S[(size_t)p] += P[(size_t)s.i - 1] == C[(size_t)p] ? Q[(size_t)s.i - 1] : -Q[(size_t)s.i - 1];
    else S[(size_t)p] -= Q[(size_t)(s.i > 0 ? s.i - 1 : 0)];
  }
  flush();
}
}  // namespace

// refusals shared by c3_consensus_qv and c3_consensus_qv_host
int c3_qv_check(const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat, const int64_t* piece_off,
                const int32_t* modes, const char* qv_out, const char** msg) {
  if (!cons || !qv_out || n <= 0) { *msg = "empty consensus"; return C3_E_ARG; }
  if (n_pieces < 0) { *msg = "negative piece count"; return C3_E_ARG; }
  if (n_pieces > C3_QV_MAX_PIECES) { *msg = "more than 252 pieces"; return C3_E_LIMIT; }
  if (n_pieces == 0) return C3_E_OK;
  if (!seq_cat || !qual_cat || !piece_off || !modes || piece_off[0] != 0) { *msg = "pieces missing or piece_off[0] != 0"; return C3_E_ARG; }
  for (int k = 0; k < n_pieces; ++k) {
    const int64_t m = piece_off[k + 1] - piece_off[k];
    if (m <= 0) { *msg = "empty piece"; return C3_E_ARG; }
    if (m > (1 << 30)) { *msg = "piece longer than 2^30"; return C3_E_LIMIT; }
    if (modes[k] < C3_QV_GLOBAL || modes[k] > C3_QV_ANCHOR_END) { *msg = "unknown alignment mode"; return C3_E_ARG; }
    if (modes[k] == C3_QV_GLOBAL && std::max<int64_t>(m, n) > (int64_t)C3_QV_SKEW * std::min<int64_t>(m, n)) {
      *msg = "mode-0 piece / consensus lengths beyond the skew limit (max > 4 * min)"; return C3_E_LIMIT;
    }
  }
  return C3_E_OK;
}

extern "C" int c3_consensus_qv_host(const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat,
                                    const int64_t* piece_off, const int32_t* modes, char* qv_out) {
  const char* msg = "";
  const int rc = c3_qv_check(cons, n, n_pieces, seq_cat, qual_cat, piece_off, modes, qv_out, &msg);
  if (rc != C3_E_OK) { c3_set_host_error(msg); return rc; }
  std::vector<int> S((size_t)n, 0), Sr;
  std::vector<int> C((size_t)n), Cr((size_t)n);
  for (int j = 0; j < n; ++j) { C[(size_t)j] = code_of(cons[j]); Cr[(size_t)(n - 1 - j)] = C[(size_t)j]; }
  for (int k = 0; k < n_pieces; ++k) {
    const int64_t b = piece_off[k], m = piece_off[k + 1] - b;
    std::vector<int> P((size_t)m), Q((size_t)m);
    const bool rev = modes[k] == C3_QV_ANCHOR_END;
    for (int64_t x = 0; x < m; ++x) {
      const int64_t y = rev ? m - 1 - x : x;
      P[(size_t)x] = code_of(seq_cat[b + y]); Q[(size_t)x] = q_of(qual_cat[b + y]);
    }
    if (!rev) { align_piece(C, P, Q, modes[k], S); continue; }
    Sr.assign((size_t)n, 0);
    align_piece(Cr, P, Q, C3_QV_ANCHOR_START, Sr);            // mode 2 = mode 1 in the reversed frame, mapped back
    for (int j = 0; j < n; ++j) S[(size_t)j] += Sr[(size_t)(n - 1 - j)];
  }
  for (int j = 0; j < n; ++j) qv_out[j] = (char)(33 + std::min(C3_QV_MAX, std::max(0, S[(size_t)j])));
  return C3_E_OK;
}

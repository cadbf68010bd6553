// c3_index.cpp -- host statements of the index matchers: c3_match_index (k_adapter's oligo-dT index step) and c3_demux_host
// (k_demux), with the checks c3_demux_prepare that the device call shares.  Host code only.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/c3poa.h"
#include "c3_checks.h"

// ---- oligo-dT index matcher of the post-processing step (C3POa_postprocessing.py:266-285, match_index) ----------
// seq is slid over every index (file order); the Levenshtein distance of seq[p : p+len(idx)] to idx is taken for every
// position where the slice has the full length (at a position where it is too short for index k the reference breaks
// out of the loop over indexes, so k+1.. are skipped there as well); per index the minimum counts.  Stable sort by
// distance; the best index wins when its distance is < 2 and the runner-up is more than 1 further away.  Returns the
// winning index number, -1 for '-'.  (The reference raises on an index that never fits and on fewer than two indexes;
// both cases return -1 here.)
namespace {
int edit_distance(const char* a, const char* b, int n) {
  int prev[256], cur[256];
  if (n > 255) return n;
  for (int j = 0; j <= n; ++j) prev[j] = j;
  for (int i = 1; i <= n; ++i) {
    cur[0] = i;
    for (int j = 1; j <= n; ++j) {
      int v = prev[j - 1] + (a[i - 1] != b[j - 1]);
      v = std::min(v, prev[j] + 1); v = std::min(v, cur[j - 1] + 1);
      cur[j] = v;
    }
    memcpy(prev, cur, sizeof(int) * (size_t)(n + 1));
  }
  return prev[n];
}
}  // namespace

extern "C" int c3_match_index(const char* seq, int n, int n_idx, const char* idx_cat, const int64_t* idx_off) {
  if (!seq || n_idx < 2 || !idx_cat || !idx_off) return -1;
  std::vector<int> best((size_t)n_idx, INT32_MAX);
  for (int p = 0; p < n; ++p) {
    for (int k = 0; k < n_idx; ++k) {
      const int len = (int)(idx_off[k + 1] - idx_off[k]);
      if (p + len > n) break;                                   // the reference's `break` (not `continue`)
      best[(size_t)k] = std::min(best[(size_t)k], edit_distance(seq + p, idx_cat + idx_off[k], len));
    }
  }
  int i0 = -1, i1 = -1;                                         // first and second entry of the stable sort
  for (int k = 0; k < n_idx; ++k) {
    if (best[(size_t)k] == INT32_MAX) return -1;
    if (i0 < 0 || best[(size_t)k] < best[(size_t)i0]) { i1 = i0; i0 = k; }
    else if (i1 < 0 || best[(size_t)k] < best[(size_t)i1]) i1 = k;
  }
  if (best[(size_t)i0] < 2 && best[(size_t)i1] - best[(size_t)i0] > 1) return i0;
  return -1;
}

// ---- sample demultiplexer (paper/Demultiplex_R2C2_reads.py, demultiplex) ------------------------------------------
// c3_demux_prepare checks the two index sets for both entry points and builds the byte -> code table of k_demux: the
// distinct bytes of all indexes get codes 1..K in byte order, every other byte 0 (which matches no index position).
int c3_demux_prepare(int n_a, const char* a_cat, const int64_t* a_off, int n_b, const char* b_cat, const int64_t* b_off,
                     uint8_t* tab, int* n_codes, const char** msg) {
  const int ns[2] = {n_a, n_b}; const char* cats[2] = {a_cat, b_cat}; const int64_t* offs[2] = {a_off, b_off};
  bool seen[256] = {};
  for (int s = 0; s < 2; ++s) {
    if (ns[s] < 2) { *msg = "an index set needs at least 2 indexes (the reference compares the best with the runner-up)"; return C3_E_ARG; }
    if (ns[s] > C3_DEMUX_MAX_IDX) { *msg = "more than 128 indexes in one set"; return C3_E_LIMIT; }
    if (!offs[s] || offs[s][0] != 0) { *msg = "index offsets missing or not starting at 0"; return C3_E_ARG; }
    for (int k = 0; k < ns[s]; ++k) {
      const int64_t len = offs[s][k + 1] - offs[s][k];
      if (len < 0) { *msg = "index offsets decrease"; return C3_E_ARG; }
      if (len > C3_DEMUX_MAX_LEN) { *msg = "index longer than 32 bytes"; return C3_E_LIMIT; }
      if (len > 0 && !cats[s]) { *msg = "index bytes missing"; return C3_E_ARG; }
      for (int64_t j = 0; j < len; ++j) seen[(uint8_t)cats[s][offs[s][k] + j]] = true;
    }
  }
  int K = 0;
  for (int b = 0; b < 256; ++b) tab[b] = seen[b] ? (uint8_t)++K : 0;
  if (K > C3_DEMUX_MAX_BYTES) { *msg = "more than 31 distinct bytes over the index sets"; return C3_E_LIMIT; }
  *n_codes = K;
  return C3_E_OK;
}

// Host statement of k_demux: textbook DP for every window (head[i : i+m], i < 300 - m) of every index.
extern "C" int c3_demux_host(int n, const char* heads, int n_a, const char* a_cat, const int64_t* a_off,
                             int n_b, const char* b_cat, const int64_t* b_off, int32_t* win, uint8_t* dist) {
  if (n < 0 || (n > 0 && (!heads || !win))) { c3_set_host_error("heads / win missing"); return C3_E_ARG; }
  uint8_t tab[256]; int K = 0; const char* msg = "";
  const int rc = c3_demux_prepare(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, &K, &msg);
  if (rc != C3_E_OK) { c3_set_host_error(msg); return rc; }
  const int ns[2] = {n_a, n_b}; const char* cats[2] = {a_cat, b_cat}; const int64_t* offs[2] = {a_off, b_off};
  std::vector<int> d((size_t)std::max(n_a, n_b));
  for (int r = 0; r < n; ++r) {
    const char* head = heads + (size_t)r * C3_DEMUX_HEAD;
    for (int s = 0; s < 2; ++s) {
      for (int k = 0; k < ns[s]; ++k) {
        const int m = (int)(offs[s][k + 1] - offs[s][k]);
        int best = m;                                           // an empty index: distance 0
        for (int i = 0; i < C3_DEMUX_HEAD - m; ++i) best = std::min(best, edit_distance(cats[s] + offs[s][k], head + i, m));
        d[(size_t)k] = best;
        if (dist) dist[(size_t)r * (n_a + n_b) + (s ? n_a : 0) + k] = (uint8_t)best;
      }
      int i0 = 0;                                               // first entry of the stable sort; the runner-up's distance
      for (int k = 1; k < ns[s]; ++k) if (d[(size_t)k] < d[(size_t)i0]) i0 = k;
      int d1 = INT32_MAX;
      for (int k = 0; k < ns[s]; ++k) if (k != i0) d1 = std::min(d1, d[(size_t)k]);
      win[2 * (size_t)r + s] = (d[(size_t)i0] < 4 && d[(size_t)i0] < d1 - 1) ? i0 : -1;
    }
  }
  return C3_E_OK;
}

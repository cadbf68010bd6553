// k_qv.hip -- per-base consensus quality values (include/c3poa.h "per-base consensus quality values"; DESIGN.md "Consensus
// quality values").  Same function as the host statement c3_consensus_qv_host (c3_qv.cpp), byte for byte.
//
// One workgroup of four waves takes one consensus (grid-stride over the reads); the waves take its pieces round-robin and
// share its support array S.  Where S lives: a consensus of at most lds_n columns keeps S (int32) and its 2-bit codes (one
// byte each) in LDS -- lds_n = min(longest read of the batch, QV_LDS_N = 8192), so at most 40 KiB per workgroup; a longer
// one uses the workgroup's slot in global memory (gS / gcodes, allocated only when the batch has such reads).  S is
// updated with atomics (LDS or device scope), so the result does not depend on which wave takes which piece.
//
// One wave aligns one piece.  Lane l holds the band cells 2l and 2l+1 of the 128-cell row in int32 (pieces are up to read
// length: 32 kb x 2 x 4 does not fit int16).  Per row:
//   - the band moves right by d = lo(i) - lo(i-1) (1 in modes 1 / 2; floor(n/m) or one more in mode 0, <= 5 under the skew
//     limit): the up and diagonal neighbours are the previous row's cells at band offsets t + d and t + d - 1, fetched with
//     two or three ds_bpermute lane rotates;
//   - the horizontal gap is a wave max-scan of D + 4t (D = best of diagonal and up), H = scan - 4t;
//   - 2 direction bits per cell (0 matching diagonal, 3 mismatching diagonal, 1 deletion, 2 insertion, in the traceback's
//     priority order), 4 per lane per row, 8 rows per dword: one 256-byte store per 8 rows into the wave's slot.
// The piece's bases come 64 rows at a time (one load per lane, readlane per row), the consensus codes of the row's two
// cells per lane from LDS (or the global slot).  Modes 1 / 2 stop at row min(m, n + 64), past which the band holds no cell.
// The traceback is wave-uniform (scalar): it walks the slot backwards a 256-byte group at a time (the next group and its
// 8 quality bytes are prefetched), reads its cell with readlane and adds each step's contribution to S from lane 0.
// Per piece it counts into cnt[]: pieces, band cells (128 per computed row, row 0 included), and a band edge hit when the
// path touched band offset 0 with j > 0 or offset 127 with j < n (a band-adequacy diagnostic, not an error).
//
// Resources (hipcc -O3 gfx950, -Rpass-analysis=kernel-resource-usage): 69 VGPRs, 0 AGPRs, 106 SGPRs (8 SGPR spills, which go
// to VGPR lanes), ScratchSize 0; occupancy 7 waves/SIMD by registers; dynamic LDS 5 * lds_n + 16 bytes (cfg2: 6.5 KiB, at most
// 40 KiB = 4 workgroups per CU).
// Measured (MI355X, profiles/qv_throughput.json, profiles/qv_kernel_stats_cfg2_100k.txt): 193 ms per 100 k cfg2 reads
// (63 G band cells, 329 G cells/s), 4.8x the 40 ms target: each row is a serial chain of lane rotates, a 6-step DPP scan and
// flat loads for one wave, and the traceback is a scalar loop; the row chain is what a next version would shorten.
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_launch.h"

#define QV_LDS_N 8192
#define QV_NEG (-(1 << 28))

__device__ __forceinline__ int qv_code(uint8_t b) {
  switch (b) { case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 0; }
}
__device__ __forceinline__ int qv_q(uint8_t b) { return min(93, max(0, (int)b - 33)); }
// value of `v` in lane `src`, QV_NEG when src is outside the wave
__device__ __forceinline__ int qv_fetch(int v, int src) {
  const int x = __builtin_amdgcn_ds_bpermute((src & 63) << 2, v);
  return (src >= 0 && src < 64) ? x : QV_NEG;
}

struct QvPiece { const uint32_t* pk; int64_t start; const uint8_t* q; int m; int mode; };

// one piece against the consensus codes Cc[0..n) (forward frame); adds its contributions to S
__device__ void qv_piece(const QvArgs& a, const QvPiece& P, const uint8_t* Cc, int* S, int n, uint32_t* dslot) {
  const int lane = wave_lane();
  const int m = P.m;
  if (P.mode == C3_QV_GLOBAL && max(m, n) > C3_QV_SKEW * min(m, n)) { if (lane == 0) atomicAdd(a.cnt + 2, 1ull); return; }
  const bool rev = P.mode == C3_QV_ANCHOR_END, glob = P.mode == C3_QV_GLOBAL;
  const int rows = glob ? m : min(m, n + 64);
  auto pcode = [&](int x) -> int { const int xx = rev ? m - 1 - x : x; return c3_code_at(P.pk, P.start + xx); };
  auto pq = [&](int x) -> int { return qv_q(P.q[rev ? m - 1 - x : x]); };
  auto ccode = [&](int j) -> int { return (j >= 1 && j <= n) ? Cc[rev ? n - j : j - 1] : 4; };   // code of column j-1 (4: none)
  // band centre c(i): mode 0 steps floor(n/m) or one more per row (c(i) = (i*n + m/2) / m), modes 1 / 2 step 1
  const int cq = glob ? n / m : 1, cr = glob ? n % m : 0;
  int c = 0, crem = glob ? m / 2 : 0;
  int lo = -64;
  const int t0 = 2 * lane;
  int j0 = lo + t0;
  int h0 = (j0 >= 0 && j0 <= n) ? C3_QV_GAP * j0 : QV_NEG;
  int h1 = (j0 + 1 >= 0 && j0 + 1 <= n) ? C3_QV_GAP * (j0 + 1) : QV_NEG;
  int bv = lane == 32 ? 0 : QV_NEG, bi = 0, bj = 0;          // best cell of this lane (modes 1 / 2); (0,0) is lane 32's cell 0
  int pcv = lane < m ? pcode(lane) : 0, pcn = 64 + lane < m ? pcode(64 + lane) : 0;
  uint32_t word = 0;
  // consensus codes of row 1
  int nc = cq, nrem = crem + cr; if (nrem >= m && glob) { nrem -= m; ++nc; }
  int c0 = ccode(nc - 64 + t0), c1 = ccode(nc - 64 + t0 + 1);
  for (int i = 1; i <= rows; ++i) {
    const int r = i - 1;
    c += cq; crem += cr; if (glob && crem >= m) { crem -= m; ++c; }
    const int lo_new = c - 64, d = lo_new - lo;
    lo = lo_new;
    j0 = lo + t0;
    if ((r & 63) == 0 && r > 0) { pcv = pcn; pcn = r + 64 + lane < m ? pcode(r + 64 + lane) : 0; }
    const int pb = __builtin_amdgcn_readlane(pcv, r & 63);
    const int e = d >> 1;
    const int X0 = qv_fetch(h0, lane + e), X1 = qv_fetch(h1, lane + e);
    int G0, U0, G1, U1;
    if (d & 1) { const int Y = qv_fetch(h0, lane + e + 1); G0 = X0; U0 = X1; G1 = X1; U1 = Y; }
    else { const int Y = qv_fetch(h1, lane + e - 1); G0 = Y; U0 = X0; G1 = X0; U1 = X1; }
    const bool m0 = pb == c0, m1 = pb == c1;
    const int dg0 = G0 + (m0 ? C3_QV_MATCH : C3_QV_MISMATCH), dg1 = G1 + (m1 ? C3_QV_MATCH : C3_QV_MISMATCH);
    // prefetch the next row's consensus codes (the centre of row i+1 is known now)
    {
      int c2 = c + cq, r2 = crem + cr; if (glob && r2 >= m) { r2 -= m; ++c2; }
      c0 = ccode(c2 - 64 + t0); c1 = ccode(c2 - 64 + t0 + 1);
    }
    const int D0 = max(dg0, U0 + C3_QV_GAP), D1 = max(dg1, U1 + C3_QV_GAP);
    const int a0 = D0 + 8 * lane, a1 = max(a0, D1 + 8 * lane + 4);
    const int E = wave_shr1(wave_scan_max(a1), C3_NEG2);
    int H0 = max(E, a0) - 8 * lane, H1 = max(E, a1) - 8 * lane - 4;
    if (!(j0 >= 0 && j0 <= n)) H0 = QV_NEG;
    if (!(j0 + 1 >= 0 && j0 + 1 <= n)) H1 = QV_NEG;
    const int L0 = wave_shr1(H1, QV_NEG);
    const int dir0 = H0 == dg0 ? (m0 ? 0 : 3) : (H0 == L0 + C3_QV_GAP ? 1 : 2);
    const int dir1 = H1 == dg1 ? (m1 ? 0 : 3) : (H1 == H0 + C3_QV_GAP ? 1 : 2);
    word |= (uint32_t)(dir0 | (dir1 << 2)) << ((r & 7) * 4);
    if ((r & 7) == 7 || i == rows) { dslot[(size_t)(r >> 3) * 64 + lane] = word; word = 0; }
    if (!glob) {
      if (H0 > bv) { bv = H0; bi = i; bj = j0; }
      if (H1 > bv) { bv = H1; bi = i; bj = j0 + 1; }
    }
    h0 = H0; h1 = H1;
  }
  __threadfence_block();                                     // the slot's stores land before the traceback reads them
  int ei = m, ej = n;
  if (!glob) {
    const int best = wave_max(bv);
    ei = wave_min(bv == best ? bi : INT32_MAX);
    ej = wave_min(bv == best && bi == ei ? bj : INT32_MAX);
  }
  // traceback (wave-uniform), end cell -> (0,0)
  const int J = glob ? n : ej;                               // covered columns 0 .. J-1
  int i = ei, j = ej;
  int tc, trem;                                              // centre of row i
  if (glob) { const int64_t num = (int64_t)i * n + m / 2; tc = (int)(num / m); trem = (int)(num % m); } else { tc = i; trem = 0; }
  const int q0 = pq(0);
  int g = i >= 1 ? (i - 1) >> 3 : 0;
  uint32_t dv = i >= 1 ? dslot[(size_t)g * 64 + lane] : 0u;
  int qv = (i >= 1 && lane < 8 && 8 * g + lane < m) ? pq(8 * g + lane) : 0;
  uint32_t dn = g >= 1 ? dslot[(size_t)(g - 1) * 64 + lane] : 0u;
  int qn = (g >= 1 && lane < 8) ? pq(8 * (g - 1) + lane) : 0;
  int run = -1, run_j = 0;
  bool edge = false;
  auto add = [&](int p, int v) { if (lane == 0) atomicAdd(S + (rev ? n - 1 - p : p), v); };
  auto up = [&]() {                                          // i -> i-1: centre and direction group follow
    --i;
    tc -= cq; trem -= cr; if (glob && trem < 0) { trem += m; --tc; }
    if (i >= 1 && ((i - 1) >> 3) != g) {
      --g; dv = dn; qv = qn;
      dn = g >= 1 ? dslot[(size_t)(g - 1) * 64 + lane] : 0u;
      qn = (g >= 1 && lane < 8) ? pq(8 * (g - 1) + lane) : 0;
    }
  };
  while (i > 0 || j > 0) {
    const int t = j - (tc - 64);
    if ((t == 0 && j > 0) || (t == C3_QV_BAND - 1 && j < n)) edge = true;
    int kind;
    if (i == 0) kind = 1;
    else if (j == 0) kind = 2;
    else {
      const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)dv, t >> 1);
      kind = (int)((w >> (((i - 1) & 7) * 4 + (t & 1) * 2)) & 3u);
    }
    if (kind == 2) {                                         // insertion: piece base i-1
      run = max(run, __builtin_amdgcn_readlane(qv, (i - 1) & 7)); run_j = j;
      up();
      continue;
    }
    if (run >= 0) { add(min(run_j, J - 1), -run); run = -1; }
    if (kind == 1) {                                         // deletion of column j-1
      add(j - 1, -(i > 0 ? __builtin_amdgcn_readlane(qv, (i - 1) & 7) : q0));
      --j;
    } else {                                                 // diagonal
      const int qb = __builtin_amdgcn_readlane(qv, (i - 1) & 7);
      add(j - 1, kind == 0 ? qb : -qb);
      --j; up();
    }
  }
  if (run >= 0 && J > 0) add(min(run_j, J - 1), -run);
  if (lane == 0) {
    atomicAdd(a.cnt + 1, 1ull);
    atomicAdd(a.cnt + 3, (unsigned long long)(rows + 1) * C3_QV_BAND);
    if (edge) atomicAdd(a.cnt + 4, 1ull);
  }
}

__global__ __launch_bounds__(256) void k_qv(QvArgs a) {
  extern __shared__ int qv_smem[];
  const int wv = threadIdx.x >> 6;
  uint32_t* dslot = a.dirs + (size_t)(blockIdx.x * 4 + wv) * (size_t)a.dir_words;
  const bool sa = a.sa_np >= 0;
  const int nr = sa ? 1 : a.n_reads;
  for (int r = blockIdx.x; r < nr; r += gridDim.x) {
    int n, np;
    const C3Info* I = nullptr;
    if (sa) { n = a.sa_n; np = a.sa_np; }
    else {
      I = a.info + r;
      if (I->status != C3_ST_OK || I->cons_len <= 0) continue;
      n = I->cons_len; np = I->n_sub + (I->has_tail ? 1 : 0) + (I->has_front ? 1 : 0);
    }
    const char* cons = a.cons + (sa ? 0 : a.off[r]);
    char* out = a.qv + (sa ? 0 : a.off[r]);
    const bool s_lds = n <= a.lds_n;
    if (!s_lds && n > a.gcap) { for (int p = threadIdx.x; p < n; p += blockDim.x) out[p] = 33; continue; }   // (cons_len <= read length: not reached)
    int* S = s_lds ? qv_smem : a.gS + (size_t)blockIdx.x * (size_t)a.gcap;
    uint8_t* Cc = s_lds ? (uint8_t*)(qv_smem + a.lds_n) : a.gcodes + (size_t)blockIdx.x * (size_t)a.gcap;
    for (int p = threadIdx.x; p < n; p += blockDim.x) { S[p] = 0; Cc[p] = (uint8_t)qv_code((uint8_t)cons[p]); }
    __syncthreads();
    for (int k = wv; k < np; k += 4) {
      QvPiece P;
      if (sa) {
        P.pk = a.pk + a.sa_woff[k]; P.start = 0; P.q = a.qual + a.sa_off[k]; P.m = (int)(a.sa_off[k + 1] - a.sa_off[k]); P.mode = a.sa_mode[k];
      } else {
        const int64_t L = a.off[r + 1] - a.off[r];
        int beg, end, mode;
        if (k < I->n_sub) { beg = I->sub_beg[k]; end = I->sub_end[k]; mode = C3_QV_GLOBAL; }
        else if (k == I->n_sub && I->has_tail) { beg = I->tail_beg; end = (int)L; mode = C3_QV_ANCHOR_START; }
        else { beg = 0; end = I->front_end; mode = C3_QV_ANCHOR_END; }
        if (end <= beg) continue;
        P.pk = a.pk + a.woff[r]; P.start = beg; P.q = a.qual + a.off[r] + beg; P.m = end - beg; P.mode = mode;
      }
      qv_piece(a, P, Cc, S, n, dslot);
    }
    __syncthreads();
    for (int p = threadIdx.x; p < n; p += blockDim.x) out[p] = (char)(33 + min(C3_QV_MAX, max(0, S[p])));
    if (!sa && threadIdx.x == 0) atomicAdd(a.cnt, 1ull);
    __syncthreads();                                         // S / Cc are reused by the next read
  }
}

extern "C" int c3k_qv_lds_max(void) { return QV_LDS_N; }
extern "C" void c3k_launch_qv(const QvArgs* a, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_qv, dim3(grid), dim3(256), (size_t)a->lds_n * 5 + 16, s, *a);
}

// k_zero.hip -- zero-repeat rescue: overlap of the two dangling pieces of a read with a single splint.
//
// Replaces bin/determine_consensus.py:106-136 (zero_repeats; mappy overlap + 2-row abPOA + pairwise merge).
// Spec: DESIGN.md 4.7, restated by oracle/c3o_zero.c (bit-exact).  k_zero finds the best forward local
// alignment of d1 = read[tail_beg:] (rows) against d0 = read[:front_end] (columns) with affine gaps and
// turns the read into a 2-"subread" POA job (the two overlap slices); k_zero_finish stitches
// d1[:q_st] + overlap consensus + d0[r_en:] after k_poa.  Rare path: one wave per read, previous
// H/E row in LDS, direction bytes in global memory, scalar traceback.
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_launch.h"

#define ZW 4096           // columns kept in the LDS row buffers
#define WSYNC() __syncthreads()

__global__ __launch_bounds__(64) void k_zero(ZeroArgs a) {
  __shared__ int Hrow[ZW + 1];
  __shared__ int Erow[ZW + 1];
  const int lane = wave_lane();
  const int go = a.p.zr_gapo, ge = a.p.zr_gape, ma = a.p.zr_match, mb = -a.p.zr_mismatch;
  const int NEGZ = INT32_MIN / 2;
  for (int wi = blockIdx.x; wi < a.n_work; wi += gridDim.x) {
    const int rid = a.work[wi];
    C3Info* info = &a.info[rid];
    const int64_t off = a.b.off[rid];
    const int L = (int)(a.b.off[rid + 1] - off);
    const uint32_t* pk = a.b.pk + a.b.woff[rid];
    const int n0 = info->front_end, t0 = info->tail_beg, n1 = L - t0;
    uint8_t* D = a.D + (size_t)blockIdx.x * a.dcap;
    int4 z; z.x = z.y = z.z = z.w = 0;
    bool ok = n0 > 0 && n1 > 0 && n0 <= ZW && (long long)n0 * n1 <= a.p.zr_max_cells && (long long)(n0 + 1) * (n1 + 1) <= a.dcap;
    if (ok) {
      const int W = n0 + 1;
      for (int j = lane; j <= n0; j += 64) { Hrow[j] = 0; Erow[j] = NEGZ; }
      int best = 0, bi = 0, bj = 0;
      for (int i = 1; i <= n1; ++i) {
        const int qc = c3_code_at(pk, t0 + i - 1);
        int carry_old = 0;            // H[i-1][c0]   (column left of the chunk; column 0 is always 0)
        int carry_f = NEGZ;           // max over previous chunks of Ht[k] + ge*k
        int carry_h = 0;              // H[i][c0]      (full H of the column left of the chunk)
        for (int c0 = 0; c0 < n0; c0 += 64) {
          const int j = c0 + lane + 1;
          const bool act = j <= n0;
          const int hpj = act ? Hrow[j] : 0;
          const int epj = act ? Erow[j] : NEGZ;
          const int hpm = wave_shr1(hpj, carry_old);
          carry_old = wave_bcast(hpj, 63);
          const int eo = hpj - go - ge, ee = epj - ge;
          const int ex = ee > eo;
          const int e = ex ? ee : eo;
          const int rc = act ? c3_code_at(pk, j - 1) : 0;
          const int dg = hpm + (qc == rc ? ma : mb);
          int ht = 0, src = 0;
          if (dg > ht) { ht = dg; src = 1; }
          if (e > ht) { ht = e; src = 2; }
          // F[j] = max_{k<j} Ht[k] - go - ge*(j-k)   (gap opened after an F cell is dominated)
          const int x = act ? ht + ge * j : NEGZ;
          const int sc = wave_scan_max(x);
          const int px = max(wave_shr1(sc, NEGZ), carry_f);
          // column 0 of the row (H = 0) can also open a gap
          const int f = max(px, 0 + ge * 0) - go - ge * j;
          carry_f = max(carry_f, wave_bcast(sc, 63));
          int h = ht;
          if (f > h) { h = f; src = 3; }
          // F extended?  oracle: fe > fo with fo = H[i][j-1] - go - ge  <=>  F != fo
          const int hleft = wave_shr1(act ? h : 0, carry_h);
          carry_h = wave_bcast(act ? h : 0, 63);
          const int fx = f != hleft - go - ge;
          if (act) {
            Hrow[j] = h; Erow[j] = e;
            D[(size_t)i * W + j] = (uint8_t)(src | (ex << 2) | (fx << 3));
            if (h > best) { best = h; bi = i; bj = j; }
          }
        }
      }
      WSYNC();
      const int gb = wave_max(best);
      const int gi = wave_min(best == gb ? bi : INT32_MAX / 2);
      const int gj = wave_min((best == gb && bi == gi) ? bj : INT32_MAX / 2);
      if (gb >= a.p.zr_min_score) {
        int i = gi, j = gj, st = 0;
        for (;;) {
          if (i == 0 || j == 0) break;                 // border cells are 0 and never stored
          const int d = D[(size_t)i * W + j];                 // border cells are 0 and never stored
          if (st == 0) { const int src = d & 3; if (src == 0) break; if (src == 1) { --i; --j; } else st = src; }
          else if (st == 2) { st = (d & 4) ? 2 : 0; --i; }
          else { st = (d & 8) ? 3 : 0; --j; }
        }
        z.x = j; z.y = gj; z.z = i; z.w = gi;           // r_st, r_en, q_st, q_en
        ok = gj > j && gi > i;
      } else ok = false;
      if (lane == 0) atomicAdd(&a.cnt->zero_cells, (unsigned long long)n0 * n1);
    }
    if (lane == 0) {
      a.zinfo[rid] = z;
      a.zflag[rid] = ok ? 1 : 0;
      if (ok) {       // hand the two overlap slices to k_poa as a 2-subread job
        info->n_sub = 2; info->status = C3_ST_OK;
        info->sub_beg[0] = z.x; info->sub_end[0] = z.y;
        info->sub_beg[1] = t0 + z.z; info->sub_end[1] = t0 + z.w;
      }
    }
    WSYNC();
  }
}

// ---- k_zero_long ---------------------------------------------------------------------------------------------------------
// The same alignment for reads k_zero cannot hold (d0 longer than ZW, or more cells than its direction matrix takes), with
// O(rows / K * columns) scratch instead of one byte per cell.  One workgroup of ZL_WAVES waves per read.  The columns of d0
// are cut into stripes of 64 * ZL_C; a wave keeps its stripe's H / E row in VGPRs (ZL_C consecutive columns per lane), and
// the waves run a row pipeline over ZL_WAVES adjacent stripes (a sweep): in step t wave w does row t - w of its stripe, with
// the carries of that row from wave w - 1 (LDS ring, one barrier per step); the last wave of a sweep leaves them in a per-row
// array for wave 0 of the next sweep.  The cell recurrence is k_zero's.
//   scores pass: first maximum in row-major order; H / E of every K-th row kept as checkpoints
//   traceback:   the block of rows (r0, i] above the current cell (i, j) is recomputed from the checkpoint at r0, columns
//                1 .. j only (j never grows), into a direction block, and walked with k_zero's state machine; a path that
//                leaves the block at its top (an E run included) continues in the block above
#define ZL_WAVES 4
#define ZL_C 8
#define ZL_SW (64 * ZL_C)
#define ZL_SWEEP (ZL_WAVES * ZL_SW)

struct ZlCarry { int old, h, f; };   // column c0 left of a stripe, row i: H[i-1][c0], H[i][c0], max_{1<=k<=c0} Ht[i][k] + ge*k

// rows r0+1 .. r1, columns 1 .. jl, from row r0 (ck: its H / E; nullptr: the zero row).
// TB = false: best cell per lane, and H / E of every row i % K == 0, i < r1, into ckw[(i / K) * (n0 + 1) + j].
// TB = true: direction bytes (encoding of k_zero's D) into D[(i - r0 - 1) * (jl + 1) + j].
template <bool TB>
__device__ __forceinline__ void zl_rows(const uint32_t* pk, int t0, int n0, int r0, int r1, int jl, int K, const int2* ck,
                                        int2* ckw, uint8_t* D, ZlCarry* car, ZlCarry (*ring)[2],
                                        int go, int ge, int ma, int mb, int& best, int& bi, int& bj) {
  const int NEGZ = INT32_MIN / 2;
  const int lane = wave_lane(), w = wave_first((int)threadIdx.x >> 6);
  __syncthreads();                                   // every wave is done with the scratch of the previous call
  for (int s0 = 0; s0 < jl; s0 += ZL_SWEEP) {
    const int c0 = s0 + w * ZL_SW;
    const bool live = c0 < jl;
    const bool to_next = s0 + ZL_SWEEP < jl;         // a next sweep follows (this one is then full width)
    const int jb = c0 + lane * ZL_C + 1;
    int hv[ZL_C], ev[ZL_C];
    uint32_t rcode = 0;
#pragma unroll
    for (int k = 0; k < ZL_C; ++k) {
      const int j = jb + k;
      const bool act = live && j <= jl;
      if (act && ck) { const int2 v = ck[j]; hv[k] = v.x; ev[k] = v.y; } else { hv[k] = 0; ev[k] = NEGZ; }
      rcode |= (uint32_t)(act ? c3_code_at(pk, j - 1) : 0) << (2 * k);
    }
    const int nst = r1 - r0 + ZL_WAVES - 1;
    for (int t = 0; t < nst; ++t) {
      const int i = r0 + 1 + t - w;
      if (live && i > r0 && i <= r1) {
        ZlCarry cin;
        if (w > 0) cin = ring[w - 1][(t - 1) & 1];
        else if (s0 > 0) cin = car[i - 1];
        else { cin.old = 0; cin.h = 0; cin.f = NEGZ; }     // column 0
        const int c_old = wave_first(cin.old), c_h = wave_first(cin.h), c_f = wave_first(cin.f);
        const int qc = c3_code_at(pk, t0 + i - 1);
        int ht[ZL_C], sr[ZL_C], lp[ZL_C];
        const int hpm0 = wave_shr1(hv[ZL_C - 1], c_old);
        int run = NEGZ;
#pragma unroll
        for (int k = 0; k < ZL_C; ++k) {
          const int j = jb + k;
          const int hpm = k ? hv[k - 1] : hpm0;
          const int eo = hv[k] - go - ge, ee = ev[k] - ge;
          const int ex = ee > eo;
          const int e = ex ? ee : eo;
          const int dg = hpm + ((int)((rcode >> (2 * k)) & 3) == qc ? ma : mb);
          int h = 0, src = 0;
          if (dg > h) { h = dg; src = 1; }
          if (e > h) { h = e; src = 2; }
          ht[k] = h; sr[k] = src | (ex << 2); ev[k] = e;
          run = max(run, j <= jl ? h + ge * j : NEGZ);
          lp[k] = run;                                  // max over the lane's columns <= j of Ht + ge*col
        }
        // F[j] = max_{k<j} Ht[k] - go - ge*(j-k), column 0 (H = 0) included
        const int sc = wave_scan_max(run);
        const int pl = max(wave_shr1(sc, NEGZ), c_f);      // columns left of the lane
        ZlCarry co;
        co.old = wave_bcast(hv[ZL_C - 1], 63);
        co.f = max(c_f, wave_bcast(sc, 63));
        int fv[ZL_C];
#pragma unroll
        for (int k = 0; k < ZL_C; ++k) {
          const int j = jb + k;
          const int px = k ? max(pl, lp[k - 1]) : pl;
          const int f = max(px, 0) - go - ge * j;
          fv[k] = f;
          if (f > ht[k]) { ht[k] = f; sr[k] = (sr[k] & 4) | 3; }
        }
        const int hl0 = wave_shr1(ht[ZL_C - 1], c_h);
        co.h = wave_bcast(ht[ZL_C - 1], 63);
#pragma unroll
        for (int k = 0; k < ZL_C; ++k) {
          const int j = jb + k;
          if (TB) {
            // F extended?  oracle: fe > fo with fo = H[i][j-1] - go - ge  <=>  F != fo
            const int fx = fv[k] != (k ? ht[k - 1] : hl0) - go - ge;
            if (j <= jl) D[(size_t)(i - r0 - 1) * (jl + 1) + j] = (uint8_t)(sr[k] | (fx << 3));
          } else if (j <= jl && (ht[k] > best || (ht[k] == best && i < bi))) { best = ht[k]; bi = i; bj = j; }
          hv[k] = ht[k];
        }
        if (!TB && i % K == 0 && i < r1) {
          int2* row = ckw + (size_t)(i / K) * (n0 + 1);
#pragma unroll
          for (int k = 0; k < ZL_C; ++k) if (jb + k <= jl) row[jb + k] = make_int2(hv[k], ev[k]);
        }
        if (w < ZL_WAVES - 1) { if (lane == 0) ring[w][t & 1] = co; }
        else if (to_next && lane == 0) car[i - 1] = co;
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(64 * ZL_WAVES) void k_zero_long(ZeroArgs a) {
  __shared__ ZlCarry ring[ZL_WAVES][2];
  __shared__ int red[ZL_WAVES][3];
  const int lane = wave_lane(), w = wave_first((int)threadIdx.x >> 6);
  const int go = a.p.zr_gapo, ge = a.p.zr_gape, ma = a.p.zr_match, mb = -a.p.zr_mismatch, K = a.zk;
  for (int wi = blockIdx.x; wi < a.n_work; wi += gridDim.x) {
    const int rid = a.work[wi];
    C3Info* info = &a.info[rid];
    const int64_t off = a.b.off[rid];
    const int L = (int)(a.b.off[rid + 1] - off);
    const uint32_t* pk = a.b.pk + a.b.woff[rid];
    const int n0 = info->front_end, t0 = info->tail_beg, n1 = L - t0;
    const ZlLayout lay = c3_zl_layout(n0, n1, K);
    uint8_t* S = a.S + (size_t)blockIdx.x * a.scap;
    int2* ck = (int2*)(S + lay.ck);
    uint8_t* D = S + lay.dir;
    ZlCarry* car = (ZlCarry*)(S + lay.car);
    int4 z; z.x = z.y = z.z = z.w = 0;
    bool ok = n0 > 0 && n1 > 0 && K > 0 && (long long)n0 * n1 <= a.p.zr_max_cells && lay.total <= a.scap;
    if (ok) {
      int best = 0, bi = 0, bj = 0;
      zl_rows<false>(pk, t0, n0, 0, n1, n0, K, nullptr, ck, nullptr, car, ring, go, ge, ma, mb, best, bi, bj);
      {   // max score, then min row, then min column
        const int b = wave_max(best);
        const int r = wave_min(best == b ? bi : INT32_MAX / 2);
        const int c = wave_min((best == b && bi == r) ? bj : INT32_MAX / 2);
        if (lane == 0) { red[w][0] = b; red[w][1] = r; red[w][2] = c; }
      }
      __syncthreads();
      int gb = red[0][0], gi = red[0][1], gj = red[0][2];
      for (int v = 1; v < ZL_WAVES; ++v) {
        const int b = red[v][0], r = red[v][1], c = red[v][2];
        if (b > gb || (b == gb && (r < gi || (r == gi && c < gj)))) { gb = b; gi = r; gj = c; }
      }
      if (gb >= a.p.zr_min_score) {
        int i = gi, j = gj, st = 0;
        bool stop = false;
        while (!stop && i > 0 && j > 0) {                 // border cells are 0 and never stored
          const int r0 = (i - 1) / K * K, jl = j;
          zl_rows<true>(pk, t0, n0, r0, i, jl, K, r0 ? ck + (size_t)(r0 / K) * (n0 + 1) : nullptr, nullptr, D, car, ring,
                        go, ge, ma, mb, best, bi, bj);
          while (i > r0 && j > 0) {
            const int d = D[(size_t)(i - r0 - 1) * (jl + 1) + j];
            if (st == 0) { const int src = d & 3; if (src == 0) { stop = true; break; } if (src == 1) { --i; --j; } else st = src; }
            else if (st == 2) { st = (d & 4) ? 2 : 0; --i; }
            else { st = (d & 8) ? 3 : 0; --j; }
          }
        }
        z.x = j; z.y = gj; z.z = i; z.w = gi;           // r_st, r_en, q_st, q_en
        ok = gj > j && gi > i;
      } else ok = false;
      // counted cells = the oracle's (n0 * n1); the traceback's recomputed rows are not counted
      if (threadIdx.x == 0) atomicAdd(&a.cnt->zero_cells, (unsigned long long)n0 * n1);
    }
    if (threadIdx.x == 0) {
      a.zinfo[rid] = z;
      a.zflag[rid] = ok ? 1 : 0;
      if (ok) {       // the same 2-subread job as k_zero's
        info->n_sub = 2; info->status = C3_ST_OK;
        info->sub_beg[0] = z.x; info->sub_end[0] = z.y;
        info->sub_beg[1] = t0 + z.z; info->sub_end[1] = t0 + z.w;
      }
    }
    __syncthreads();
  }
}

// after k_poa: consensus = d1[:q_st] + overlap consensus + d0[r_en:]; accepted when >= mdistcutoff
__global__ __launch_bounds__(64) void k_zero_finish(ZeroArgs a) {
  const int lane = wave_lane();
  for (int wi = blockIdx.x; wi < a.n_work; wi += gridDim.x) {
    const int rid = a.work[wi];
    if (!a.zflag[rid]) continue;
    C3Info* info = &a.info[rid];
    const int64_t off = a.b.off[rid];
    const uint32_t* pk = a.b.pk + a.b.woff[rid];
    const int4 z = a.zinfo[rid];
    const int n0 = info->front_end, t0 = info->tail_beg;
    const int C = info->draft_len;
    const uint8_t* draft = a.draft + off;
    char* cons = a.cons + off;
    const int total = z.z + C + (n0 - z.y);
    const bool good = info->status == C3_ST_OK && C > 0 && total >= a.p.mdist;
    if (good) {
      for (int k = lane; k < z.z; k += 64) cons[k] = "ACGT"[c3_code_at(pk, t0 + k)];
      for (int k = lane; k < C; k += 64) cons[z.z + k] = "ACGT"[draft[k] & 3];
      for (int k = lane; k < n0 - z.y; k += 64) cons[z.z + C + k] = "ACGT"[c3_code_at(pk, z.y + k)];
    }
    if (lane == 0) {
      info->n_sub = 0;                       // repeats == 0 (determine_consensus.py:18)
      info->draft_len = 0;                   // no polish on this path (:16-18)
      info->cons_len = good ? total : 0;
      info->status = good ? C3_ST_OK : C3_ST_NO_CONSENSUS;
      if (!good) a.zflag[rid] = 0;
    }
  }
}

extern "C" void c3k_launch_zero(const ZeroArgs* a, int grid, hipStream_t s) { hipLaunchKernelGGL(k_zero, dim3(grid), dim3(64), 0, s, *a); }
extern "C" void c3k_launch_zero_long(const ZeroArgs* a, int grid, hipStream_t s) { hipLaunchKernelGGL(k_zero_long, dim3(grid), dim3(64 * ZL_WAVES), 0, s, *a); }
extern "C" void c3k_launch_zero_finish(const ZeroArgs* a, int grid, hipStream_t s) { hipLaunchKernelGGL(k_zero_finish, dim3(grid), dim3(64), 0, s, *a); }

// k_demux.hip -- sample demultiplexer (paper/Demultiplex_R2C2_reads.py, demultiplex) for a batch of read heads.
// Per read and per index k (length m <= 32): the minimum over the windows head[i : i+m], i in 0 .. 299-m, of the global
// Levenshtein distance index <-> window; then per set (A = Nextera, B = TSO) the stable-sort decision: the first index
// of minimum distance wins when that distance is < 4 and the runner-up's is more than 1 further away.  Same function as
// the host statement c3_demux_host (c3_index.cpp), which the golden cases of the reference pin.
//
// One workgroup of 256 lanes takes DMX_R reads.  Lane work item = (read, index, window chunk): DMX_C chunks of ~37
// windows per (read, index), chunk fastest, so neighbouring lanes share one index (one m, equal trip counts) and one
// head (LDS reads of the same byte broadcast).  Every window is one global edit distance by the bit-parallel Myers /
// Hyyro recurrence on a 32-bit word (score starts at m, a 1 is shifted into Ph each text step); the chunk minimum goes
// to the LDS minimum of (read, index) by ds_min.  Bytes are matched through codes: the host gives every distinct index
// byte a code 1..K (K <= 31) and every other byte 0, so Peq is n_idx x (K+1) words in LDS and code 0 matches nothing;
// heads are translated to codes while they are staged into LDS.  No runtime-indexed private array.
// Resources (hipcc -O3 gfx950, -Rpass-analysis=kernel-resource-usage): 50 VGPRs, 38 SGPRs, no scratch
// (.private_segment_fixed_size 0), dynamic LDS 4.2 KiB with the paper sets (20 + 8 indexes, K = 4), at most 44 KiB with
// 2 x 128 indexes and K = 31; occupancy 8 waves/SIMD (the 32-waves/CU cap) up to 20 KiB of LDS per workgroup, 3 at 44 KiB.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "c3_launch.h"

#define DMX_HEAD 300    // bases searched per read (C3_DEMUX_HEAD)
#define DMX_R 8         // reads per workgroup
#define DMX_C 8         // window chunks per (read, index)
#define DMX_T 256       // lanes per workgroup

__global__ __launch_bounds__(DMX_T) void k_demux(const uint8_t* __restrict__ heads, int n, const uint8_t* __restrict__ meta,
                                                 int n_a, int n_b, int K1, int32_t* __restrict__ win, uint8_t* __restrict__ dist) {
  // meta (host-built, 4-byte aligned): peq[I * K1] words, len[I] words, tab[256] bytes
  extern __shared__ uint32_t smem[];
  const int I = n_a + n_b, tid = threadIdx.x, r0 = blockIdx.x * DMX_R;
  const int nr = min(DMX_R, n - r0);                           // reads of this workgroup
  uint32_t* peq_s = smem;                                      // [I][K1]
  int* len_s = (int*)(peq_s + I * K1);                         // [I]
  int* min_s = len_s + I;                                      // [DMX_R][I]
  uint8_t* tab_s = (uint8_t*)(min_s + DMX_R * I);              // [256]
  uint8_t* head_s = tab_s + 256;                               // [DMX_R][DMX_HEAD] codes

  const uint32_t* meta_w = (const uint32_t*)meta;
  for (int t = tid; t < I * K1 + I + 64; t += DMX_T) {         // peq and len are contiguous in meta and in LDS, tab follows min_s
    if (t < I * K1 + I) smem[t] = meta_w[t];
    else ((uint32_t*)tab_s)[t - I * K1 - I] = meta_w[t];
  }
  for (int t = tid; t < DMX_R * I; t += DMX_T) min_s[t] = DMX_HEAD;
  __syncthreads();
  const uint32_t* hw = (const uint32_t*)(heads + (size_t)r0 * DMX_HEAD);   // slots of 300 bytes: word aligned
  for (int t = tid; t < nr * (DMX_HEAD / 4); t += DMX_T) {
    const uint32_t w = hw[t];
    ((uint32_t*)head_s)[t] = (uint32_t)tab_s[w & 255] | ((uint32_t)tab_s[(w >> 8) & 255] << 8) |
                             ((uint32_t)tab_s[(w >> 16) & 255] << 16) | ((uint32_t)tab_s[w >> 24] << 24);
  }
  __syncthreads();

  for (int t = tid; t < nr * I * DMX_C; t += DMX_T) {
    const int c = t % DMX_C, rk = t / DMX_C, k = rk % I, rr = rk / I;
    const int m = len_s[k], W = DMX_HEAD - m;
    const int w0 = c * W / DMX_C, w1 = (c + 1) * W / DMX_C;
    const uint8_t* hd = head_s + rr * DMX_HEAD;
    const uint32_t* pq = peq_s + k * K1;
    const uint32_t hb = 1u << ((m - 1) & 31);
    int best = m;                                              // an empty index: distance 0 (no steps)
    for (int i = w0; i < w1; ++i) {                            // i + m - 1 <= 298: inside the head
      uint32_t Pv = ~0u, Mv = 0u;
      int sc = m;
      for (int j = 0; j < m; ++j) {
        const uint32_t Eq = pq[hd[i + j]];
        const uint32_t Xv = Eq | Mv;
        const uint32_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
        uint32_t Ph = Mv | ~(Xh | Pv);
        uint32_t Mh = Pv & Xh;
        sc += (int)((Ph & hb) != 0) - (int)((Mh & hb) != 0);
        Ph = (Ph << 1) | 1u;                                   // global: the top row grows by 1 per text step
        Mh <<= 1;
        Pv = Mh | ~(Xv | Ph);
        Mv = Ph & Xv;
      }
      best = min(best, sc);
    }
    atomicMin(&min_s[rk], best);
  }
  __syncthreads();

  if (dist)
    for (int t = tid; t < nr * I; t += DMX_T) dist[(size_t)r0 * I + t] = (uint8_t)min_s[t];
  if (tid < 2 * nr) {
    const int rr = tid >> 1, s = tid & 1, k0 = s ? n_a : 0, ns = s ? n_b : n_a;
    const int* d = min_s + rr * I + k0;
    int i0 = 0;                                                // first entry of the stable sort
    for (int k = 1; k < ns; ++k) if (d[k] < d[i0]) i0 = k;
    int d1 = 1 << 30;                                          // the runner-up's distance
    for (int k = 0; k < ns; ++k) if (k != i0) d1 = min(d1, d[k]);
    win[2 * (size_t)(r0 + rr) + s] = (d[i0] < 4 && d[i0] < d1 - 1) ? i0 : -1;
  }
}

// LDS bytes of one workgroup for I indexes and K1 codes
extern "C" size_t c3k_demux_lds(int I, int K1) { return sizeof(uint32_t) * ((size_t)I * K1 + I + (size_t)DMX_R * I) + 256 + DMX_R * DMX_HEAD; }

extern "C" void c3k_launch_demux(const uint8_t* heads, int n, const uint8_t* meta, int n_a, int n_b, int K1, int32_t* win,
                                 uint8_t* dist, hipStream_t s) {
  hipLaunchKernelGGL(k_demux, dim3((n + DMX_R - 1) / DMX_R), dim3(DMX_T), c3k_demux_lds(n_a + n_b, K1), s, heads, n, meta,
                     n_a, n_b, K1, win, dist);
}

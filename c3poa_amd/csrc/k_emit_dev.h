// k_emit_dev.h -- what the length passes of k_emit.hip and k_bamout.hip share: the wave sum, the consensus length of a read in
// either calling form, and the quality sum of a read.  Device code.
#pragma once
#include "c3_dev.h"
#include "c3_emit.h"

__device__ __forceinline__ long long em_wave_sum(long long v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

__device__ __forceinline__ int64_t em_clen(const EmitArgs& a, int i) {
  if (!a.cons) return 0;
  if (a.cons_off) return a.cons_off[i + 1] - a.cons_off[i];
  return a.info[i].status == C3_ST_OK ? (int64_t)a.info[i].cons_len : 0;
}

// sum of the bytes q[0..L) by one wave: the unaligned head and tail bytewise, the aligned dwords by v_sad_u8
__device__ __forceinline__ long long em_byte_sum(const uint8_t* q, int64_t L, int lane) {
  const int64_t head = min(L, (int64_t)((4u - ((uintptr_t)q & 3u)) & 3u));
  long long acc = 0;
  if (lane < head) acc += q[lane];
  const int64_t nd = (L - head) >> 2;
  const uint32_t* q4 = (const uint32_t*)(q + head);
  for (int64_t k = lane; k < nd; k += 64) acc += __builtin_amdgcn_sad_u8(q4[k], 0u, 0u);
  const int64_t done = head + 4 * nd;
  if (lane < L - done) acc += q[done + lane];
  return em_wave_sum(acc);
}

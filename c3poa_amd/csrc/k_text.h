// k_text.h -- what the text kernels share (k_fastq.hip, k_fastx.hip): the workgroup shape of their record passes, the exclusive
// scan over a workgroup and the wave copy between any two byte addresses.  Device code only.
#pragma once
#include "c3_dev.h"

#define FQ_WAVES 4
#define FQ_LONG 32768                 // sequence bytes above which the workgroup shares a record

// exclusive scan over the 256 lanes of a workgroup; every lane calls it
template <class T> __device__ __forceinline__ T fq_block_excl(T v, T* lds, T* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T inc = v;
  for (int d = 1; d < 64; d <<= 1) { const T t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
  __syncthreads();                                       // (lds is reused from one call to the next)
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (int k = 0; k < FQ_WAVES; ++k) { const T x = lds[k]; if (k < wv) base += x; tot += x; }
  *total = tot;
  return base + inc - v;
}

// dst[0..len) = src[0..len) by the 64 lanes of a wave, any alignment on either side
__device__ __forceinline__ void fq_wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
  const uint32_t head = min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) dst[lane] = src[lane];
  const uint32_t nd = (len - head) >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  const uint8_t* s = src + head;
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
  const uint32_t* sa = (const uint32_t*)(s - sh);
  if (sh == 0) { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = sa[k]; }
  else         { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = __builtin_amdgcn_alignbyte(sa[k + 1], sa[k], sh); }   // sa[k + 1] holds byte s + 4k + 3 at least
  const uint32_t done = head + 4u * nd, tail = len - done;
  if ((uint32_t)lane < tail) dst[done + lane] = src[done + lane];
}

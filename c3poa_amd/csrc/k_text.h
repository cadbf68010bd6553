// k_text.h -- the one home of what the text kernels share (k_fastq, k_bam, k_fastx, k_fasta, k_dsplit, k_post, k_emit, k_bamout): the workgroup
// shape of their record passes (TX_WAVES, TX_LONG), the wave and workgroup scans, the wave copy between any two byte addresses,
// the cutter that shares a long record among the waves of a workgroup, and the one-column exclusive scan over a functor (three
// kernels and their launcher).  Device code, but for that launcher.
#pragma once
#include "c3_dev.h"

#define TX_WAVES 4                    // waves per workgroup of every record pass
#define TX_LONG 32768                 // bytes above which the workgroup shares a record

// inclusive scan over the 64 lanes of a wave
template <class T> __device__ __forceinline__ T tx_wave_incl(T v) {
  const int lane = threadIdx.x & 63;
  for (int d = 1; d < 64; d <<= 1) { const T t = __shfl_up(v, d, 64); if (lane >= d) v += t; }
  return v;
}

// exclusive scan over the 256 lanes of a workgroup; every lane calls it
template <class T> __device__ __forceinline__ T tx_block_excl(T v, T* lds, T* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const T inc = tx_wave_incl(v);
  __syncthreads();                                       // (lds is reused from one call to the next)
  if (lane == 63) lds[wv] = inc;
  __syncthreads();
  T base = 0, tot = 0;
  for (int k = 0; k < TX_WAVES; ++k) { const T x = lds[k]; if (k < wv) base += x; tot += x; }
  *total = tot;
  return base + inc - v;
}

// dst[0..len) = src[0..len) by the 64 lanes of a wave, any alignment on either side: the destination is brought to a dword with
// byte stores, the interior is whole dwords from two aligned source dwords joined by v_alignbyte, the end is byte stores
__device__ __forceinline__ void tx_wave_copy(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
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

// this wave's piece [b, e) of len bytes shared by `parts` waves, in whole 256-byte rows
__device__ __forceinline__ void tx_piece(uint32_t len, int part, int parts, uint32_t* b, uint32_t* e) {
  const uint32_t piece = (((len + parts - 1) / parts) + 255u) & ~255u;
  *b = min(len, piece * (uint32_t)part); *e = min(len, *b + piece);
}

// ---- a one-column exclusive scan over items 0 .. F::n(): term(i), put(i, exclusive sum) for every item with a term, total(sum).
// Per-workgroup sums, one small workgroup over those, then every workgroup again with its base.
template <class F> __global__ __launch_bounds__(256) void k_tx_xsum(F f, long long* bsum) {
  __shared__ long long lds[TX_WAVES];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  long long t;
  (void)tx_block_excl(i < f.n() ? f.term(i) : 0ll, lds, &t);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}
template <class F> __global__ __launch_bounds__(256) void k_tx_xscan(F f, long long* bsum, int nb) {
  __shared__ long long lds[TX_WAVES];
  long long run = 0;
  for (int i0 = 0; i0 < nb; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const long long v = i < nb ? bsum[i] : 0;
    long long tot;
    const long long ex = tx_block_excl(v, lds, &tot);
    if (i < nb) bsum[i] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) f.total(run);
}
template <class F> __global__ __launch_bounds__(256) void k_tx_xfin(F f, const long long* bsum) {
  __shared__ long long lds[TX_WAVES];
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long v = i < f.n() ? f.term(i) : 0ll;
  long long t;
  const long long ex = bsum[blockIdx.x] + tx_block_excl(v, lds, &t);
  if (v) f.put(i, ex);
}
// n_bound: at least F::n(), known on the host; bsum holds (n_bound + 255) / 256 sums
template <class F> static void tx_xscan(const F& f, long long n_bound, long long* bsum, hipStream_t s) {
  const int nb = (int)((n_bound + 255) / 256);
  if (nb) hipLaunchKernelGGL(k_tx_xsum<F>, dim3(nb), dim3(256), 0, s, f, bsum);
  hipLaunchKernelGGL(k_tx_xscan<F>, dim3(1), dim3(256), 0, s, f, bsum, nb);
  if (nb) hipLaunchKernelGGL(k_tx_xfin<F>, dim3(nb), dim3(256), 0, s, f, (const long long*)bsum);
}

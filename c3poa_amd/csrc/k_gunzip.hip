// k_gunzip.hip -- a plain gzip stream inflated in parallel on the GPU (include/c3poa.h "gzip input").  The
// rule (which piece is accepted, when a piece is decoded again) is the host procedure of c3_gunzip_run.h; the header test,
// the piece decoder and the symbol rule are c3_gunzip.h, which the host statement (c3_gunzip.cpp) runs as well.  This file
// is their device policy and the four kernels around it.  The compressed file lies in a buffer that is zero for 512 bytes
// past its n bytes; no kernel reads beyond that, and none writes outside the slab, window or output range it is given.
//
// k_gunzip_find     one wave per piece.  64 consecutive bit offsets at a time, one per lane: four dwords around the offset,
//                   the cheap reject of c3_gz_quick in every lane, a ballot, then the survivors in ascending order through
//                   the full wave-uniform parse (c3_gz_header_at, tables in LDS).  The first that parses is the candidate.
// k_gunzip_decode   one wave per piece, GZ_WAVES pieces per workgroup: k_inflate's wave-uniform bit reader and literal run,
//                   with 16-bit symbols as the sink.  A match flushes the run, fences (workgroup scope) and copies 64 symbols
//                   per step from the slab; sources in front of the slab become markers.  As in k_inflate, a source at
//                   distance < length is at - dist + i mod dist, written before the match began: one fence per match.
// k_gunzip_window   one workgroup walks the accepted pieces: window s + 1 from window s (in LDS) and piece s's last symbols,
//                   barriers between steps; every window also goes to global memory for k_gunzip_resolve.
// k_gunzip_resolve  one workgroup per 16 KiB of a piece's symbols: markers to bytes (coalesced), then the CRC-32 of the chunk
//                   by slices (table CRC, shifted to the chunk's end with bgzf_crc_shift, XOR-reduced).
// No kernel waits for another workgroup; every loop ends by a bit count, a slab size, a piece count or a chunk length.
#include "c3_dev.h"
#include "c3_gunzip.h"
#include "c3_launch.h"

#define GZ_WAVES 4
#define GZ_CHUNK 16384
#define GZ_RES_THREADS 256

__device__ __forceinline__ void gz_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ int64_t gz_uni64(int64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
  return (int64_t)((uint64_t)hi << 32 | lo);
}

struct GzDev {
  const uint32_t* pa;             // the piece's base dword
  const uint8_t* pay;             // the same address, by bytes
  uint32_t nwords;                // dwords from there that hold bytes of the file
  uint16_t* sym;
  int ln;
  uint32_t cbase, cv;             // lane k holds dword cbase + k
  uint32_t pend, npend, pbase;    // literal run: lane k holds sym[pbase + k], k < npend

  __device__ __forceinline__ void init(const uint8_t* comp, int64_t n, int64_t base, uint16_t* slab, int lane) {
    pay = comp + base; pa = (const uint32_t*)pay;
    const int64_t w = ((n + 3) >> 2) - (base >> 2);
    nwords = (uint32_t)(w < 0 ? 0 : w > 0x7FFFFFFF ? 0x7FFFFFFF : w);
    sym = slab; ln = lane;
    cbase = 0x80000000u; cv = 0; pend = 0; npend = 0; pbase = 0;
  }
  __device__ __forceinline__ uint32_t word(uint32_t i) {
    if (i - cbase >= 64u) {
      cbase = i & ~63u;
      const uint32_t k = cbase + (uint32_t)ln;
      cv = k < nwords ? pa[k] : 0u;
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)cv, (int)(i - cbase));
  }
  __device__ __forceinline__ void flush() {
    if ((uint32_t)ln < npend) sym[pbase + (uint32_t)ln] = (uint16_t)pend;
    pbase += npend; npend = 0;
  }
  __device__ __forceinline__ void lit(uint32_t b, uint32_t at) {
    if (npend == 0) pbase = at;
    pend = (uint32_t)ln == npend ? b : pend;
    if (++npend == 64u) flush();
  }
  __device__ __forceinline__ void match(uint32_t len, uint32_t dist, uint32_t at) {
    flush();
    gz_fence();
    for (uint32_t i = (uint32_t)ln; i < len; i += 64u) {
      const uint32_t j = dist >= len ? i : i % dist;
      const int32_t from = (int32_t)(at + j) - (int32_t)dist;            // < at: written before this match (at < 2^24, dist <= 2^15)
      sym[at + i] = from >= 0 ? sym[from] : (uint16_t)(C3_GZ_MARK | (uint32_t)((int32_t)C3_GZ_WIN + from));
    }
  }
  __device__ __forceinline__ void stored(uint32_t pos, uint32_t len, uint32_t at) {
    flush();
    for (uint32_t i = (uint32_t)ln; i < len; i += 64u) sym[at + i] = pay[pos + i];
  }
  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ void sync() { gz_fence(); }
  static __device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
};

// cand[k], 1 <= k < np: the first bit of piece k of [s0, s1) at which a dynamic block header parses, or -1
__global__ __launch_bounds__(64 * GZ_WAVES) void k_gunzip_find(const uint8_t* comp, int64_t n, int64_t s0, int64_t s1, int64_t piece, int64_t np, int64_t* cand) {
  __shared__ C3InfTab tab[GZ_WAVES];
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t k = 1 + (int64_t)blockIdx.x * GZ_WAVES + wv;
  if (k >= np) return;
  const int64_t q0 = 8 * (s0 + k * piece);
  const int64_t e = s0 + (k + 1) * piece, q1 = 8 * (e < s1 ? e : s1);
  const uint32_t* words = (const uint32_t*)comp;                         // comp is 256-aligned
  int64_t found = -1;
  for (int64_t g = q0; g < q1 && found < 0; g += 64) {
    const int64_t q = g + lane;
    bool pass = false;
    if (q < q1) {                                                        // q < 8 n: dwords (q >> 5) + 0..3 lie inside the zero tail at most
      const int64_t w = q >> 5;
      const uint64_t lo = (uint64_t)words[w] | (uint64_t)words[w + 1] << 32, hi = (uint64_t)words[w + 2] | (uint64_t)words[w + 3] << 32;
      const int sh = (int)(q & 31);
      pass = c3_gz_quick(sh ? lo >> sh | hi << (64 - sh) : lo, hi >> sh);
    }
    unsigned long long mask = __ballot(pass);
    while (mask) {                                                       // at most 64 turns
      const int l = __builtin_ctzll(mask);
      mask &= mask - 1;
      const int64_t qq = g + l;
      const C3GzRel r = c3_gz_rel(qq, 0, n);
      GzDev io;
      io.init(comp, n, r.base, nullptr, lane);
      if (c3_gz_header_at(io, &tab[wv], r.sbit, r.total)) { found = qq; break; }
    }
  }
  if (lane == 0) cand[k] = found;
}

__global__ __launch_bounds__(64 * GZ_WAVES) void k_gunzip_decode(const uint8_t* comp, int64_t n, const C3GzJob* jobs, int nj, uint16_t* arena, C3GzRes* res) {
  __shared__ C3InfTab tab[GZ_WAVES];
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  const int m = blockIdx.x * GZ_WAVES + wv;
  if (m >= nj) return;
  const int64_t start = gz_uni64(jobs[m].start), limit = gz_uni64(jobs[m].limit), slab = gz_uni64(jobs[m].slab);
  const uint32_t cap = GzDev::uni(jobs[m].cap);
  C3GzRes r;
  if (start < 0 || start >= 8 * n) {                                     // (the host never asks for it)
    r.status = C3_GZ_BAD; r.reason = C3_INF_INPUT; r.nsym = 0; r.bb_nsym = 0; r.stop = start; r.bb = start;
  } else {
    const C3GzRel q = c3_gz_rel(start, limit, n);
    GzDev io;
    io.init(comp, n, q.base, arena + slab, lane);
    c3_gz_piece(io, &tab[wv], q.sbit, q.total, q.limit, cap, &r);
    io.flush();
    r.stop += 8 * q.base; r.bb += 8 * q.base;
  }
  if (lane == 0) res[m] = r;
}

// wins[0..32768) is the window in front of segment 0; window s + 1 is written behind it.  The current window lives in LDS;
// a thread owns bytes t + 1024 j: it loads its 32 symbols at once, looks the markers up in LDS, and after a barrier
// replaces its bytes (LDS for the next step, global memory for k_gunzip_resolve)
__global__ __launch_bounds__(1024) void k_gunzip_window(const uint16_t* __restrict__ arena, const C3GzSeg* __restrict__ segs, int ns, uint8_t* __restrict__ wins) {
  __shared__ uint8_t win[C3_GZ_WIN];
  const uint32_t t = threadIdx.x;
  for (uint32_t j = 0; j < C3_GZ_WIN / 1024u; ++j) win[t + 1024u * j] = wins[t + 1024u * j];
  __syncthreads();
  for (int s = 0; s + 1 < ns; ++s) {
    const C3GzSeg g = segs[s];
    const uint16_t* sym = arena + g.slab;
    uint16_t v[C3_GZ_WIN / 1024u];
#pragma unroll
    for (uint32_t j = 0; j < C3_GZ_WIN / 1024u; ++j) {                   // c3_gz_next_window, loads first
      const uint32_t i = t + 1024u * j;
      v[j] = i + g.nsym >= C3_GZ_WIN ? sym[i + g.nsym - C3_GZ_WIN] : (uint16_t)win[i + g.nsym];
    }
    uint8_t b[C3_GZ_WIN / 1024u];
#pragma unroll
    for (uint32_t j = 0; j < C3_GZ_WIN / 1024u; ++j) {
      const uint32_t i = t + 1024u * j;
      const int x = i + g.nsym >= C3_GZ_WIN ? c3_gz_byte(v[j], win, g.wlen) : (int)v[j];
      b[j] = (uint8_t)(x < 0 ? 0 : x);                                   // (k_gunzip_resolve reports the marker)
    }
    __syncthreads();                                                     // every look-up of this step before the window changes
    uint8_t* nxt = wins + (size_t)(s + 1) * C3_GZ_WIN;
#pragma unroll
    for (uint32_t j = 0; j < C3_GZ_WIN / 1024u; ++j) { win[t + 1024u * j] = b[j]; nxt[t + 1024u * j] = b[j]; }
    __syncthreads();
  }
}

// res[c] = (CRC-32 of chunk c's bytes, 1 if one of its markers points in front of the member)
__global__ __launch_bounds__(GZ_RES_THREADS) void k_gunzip_resolve(const uint16_t* arena, const C3GzSeg* segs, const C3GzChunk* chunks, int nchunks,
                                                                   const uint8_t* wins, uint8_t* out, uint2* res) {
  __shared__ uint32_t crc_tab[256], x2n[20], red[GZ_RES_THREADS / 64], any_bad;
  const int t = threadIdx.x, c = blockIdx.x;
  crc_tab[t] = bgzf_crc_entry((uint32_t)t);
  if (t == 0) { bgzf_x2n_init(x2n); any_bad = 0; }
  __syncthreads();
  if (c >= nchunks) return;
  const C3GzChunk ch = chunks[c];
  const C3GzSeg g = segs[ch.seg];
  const uint32_t from = ch.from < g.nsym ? ch.from : g.nsym;
  const uint32_t len = min(min(ch.len, (uint32_t)GZ_CHUNK), g.nsym - from);
  const uint16_t* sym = arena + g.slab + from;
  const uint8_t* win = wins + (size_t)ch.seg * C3_GZ_WIN;
  uint8_t* o = out + g.out + from;
  bool bad = false;
  for (uint32_t i = (uint32_t)t; i < len; i += GZ_RES_THREADS) {
    const int v = c3_gz_byte(sym[i], win, g.wlen);
    if (v < 0) bad = true;
    o[i] = (uint8_t)(v < 0 ? 0 : v);
  }
  if (bad) any_bad = 1;
  __syncthreads();
  const uint32_t per = (len + GZ_RES_THREADS - 1) / GZ_RES_THREADS;
  const uint32_t start = min(len, (uint32_t)t * per), clen = min(per, len - start);
  uint32_t x = 0xFFFFFFFFu;
  for (uint32_t i = 0; i < clen; ++i) x = crc_tab[(x ^ o[start + i]) & 0xFFu] ^ (x >> 8);
  x = clen ? ~x : 0u;
  const uint32_t after = len - start - clen;
  if (clen && after) x = bgzf_crc_shift(x2n, after, x);
  for (int d = 32; d > 0; d >>= 1) x ^= __shfl_xor(x, d, 64);
  if ((t & 63) == 0) red[t >> 6] = x;
  __syncthreads();
  if (t == 0) {
    uint32_t y = 0;
    for (int w = 0; w < GZ_RES_THREADS / 64; ++w) y ^= red[w];
    res[c] = make_uint2(y, any_bad);
  }
}

extern "C" void c3k_launch_gunzip_find(const uint8_t* comp, int64_t n, int64_t s0, int64_t s1, int64_t piece, int64_t np, int64_t* cand, hipStream_t s) {
  hipLaunchKernelGGL(k_gunzip_find, dim3((unsigned)((np - 1 + GZ_WAVES - 1) / GZ_WAVES)), dim3(64 * GZ_WAVES), 0, s, comp, n, s0, s1, piece, np, cand);
}
extern "C" void c3k_launch_gunzip_decode(const uint8_t* comp, int64_t n, const C3GzJob* jobs, int nj, uint16_t* arena, C3GzRes* res, hipStream_t s) {
  hipLaunchKernelGGL(k_gunzip_decode, dim3((nj + GZ_WAVES - 1) / GZ_WAVES), dim3(64 * GZ_WAVES), 0, s, comp, n, jobs, nj, arena, res);
}
extern "C" void c3k_launch_gunzip_window(const uint16_t* arena, const C3GzSeg* segs, int ns, uint8_t* wins, hipStream_t s) {
  hipLaunchKernelGGL(k_gunzip_window, dim3(1), dim3(1024), 0, s, arena, segs, ns, wins);
}
extern "C" void c3k_launch_gunzip_resolve(const uint16_t* arena, const C3GzSeg* segs, const C3GzChunk* chunks, int nchunks, const uint8_t* wins, uint8_t* out,
                                          uint2* res, hipStream_t s) {
  hipLaunchKernelGGL(k_gunzip_resolve, dim3(nchunks), dim3(GZ_RES_THREADS), 0, s, arena, segs, chunks, nchunks, wins, out, res);
}
extern "C" int c3k_gunzip_chunk(void) { return GZ_CHUNK; }

// k_inflate.hip -- BGZF members of --inflate gpu inflated on the GPU (include/c3poa.h "BGZF input").  The
// decoder is c3_inflate.h, the one the host statement c3_bgzf_decompress_host (c3_inflate.cpp) runs; this file is its
// device policy: where payload words come from and where bytes go.
//
// k_inflate: one wave per member, INF_WAVES members per workgroup.  The decode is wave-uniform: every lane runs the same
// bit reader on the same values (table look-ups are LDS reads at a uniform address + readfirstlane), so all 64 lanes are
// there for the data movement between symbols and no lane-0 region exists.
//   payload   64 dwords at a time in one VGPR (lane k holds dword base + k, two aligned loads joined by v_alignbyte: the
//             payload starts at any byte); the bit reader's refill is a v_readlane.  Reads stay inside the member: the
//             last dword pair ends within the 8-byte trailer that follows the payload.
//   tables    C3InfTab in LDS per wave (3.7 KB): built from the code lengths by c3_inf_build; its clear and fill loops
//             run over the lanes.
//   literals  gathered into a run of up to 64 (lane k keeps byte k), stored by the wave as one byte store per lane.
//   matches   the wave stores its pending run, makes its stores visible to its loads (workgroup-scope fence: the stores
//             have completed at the CU's L1/L2 before the loads issue), and copies 64 bytes per step from global memory;
//             distance < length reads out[at - dist + i mod dist], which is all written before the match began, so one
//             fence per match is enough.  No 32 KiB window in LDS: 8 of them do not fit a CU.
//   CRC-32    lane k takes slice k of the output (table CRC, table in LDS), shifts it to the end with bgzf_crc_shift of
//             c3_bgzf.h (the same code k_bgzf uses) and the wave XOR-reduces.
// res[m] = (status, CRC of the output); the host compares the CRC with the trailer.  A failed check ends the member with
// its status; nothing outside [out + ooff, out + ooff + isize) is written and nothing outside the member is read.
#include "c3_dev.h"
#include "c3_inflate.h"
#include "c3_launch.h"

#define INF_WAVES 4

struct InfLds {
  C3InfTab tab[INF_WAVES];
  uint32_t crc_tab[256];
  uint32_t x2n[20];
};

__device__ __forceinline__ void inf_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

struct InfDev {
  const uint8_t* pay;             // the payload (any alignment)
  const uint32_t* pa;             // pay rounded down to a dword
  uint32_t sh, nwords;            // pay - pa in bytes; dwords that hold payload bytes
  uint8_t* out;
  int ln;
  uint32_t cbase, cv;             // lane k holds payload dword cbase + k
  uint32_t pend, npend, pbase;    // literal run: lane k holds out[pbase + k], k < npend

  __device__ __forceinline__ uint32_t word(uint32_t i) {
    if (i - cbase >= 64u) {
      cbase = i & ~63u;
      const uint32_t k = cbase + (uint32_t)ln;
      uint32_t v = 0;
      if (k < nwords) v = __builtin_amdgcn_alignbyte(pa[k + 1], pa[k], sh);
      cv = v;
    }
    return (uint32_t)__builtin_amdgcn_readlane((int)cv, (int)(i - cbase));
  }
  __device__ __forceinline__ void flush() {
    if ((uint32_t)ln < npend) out[pbase + (uint32_t)ln] = (uint8_t)pend;
    pbase += npend; npend = 0;
  }
  __device__ __forceinline__ void lit(uint32_t b, uint32_t at) {
    if (npend == 0) pbase = at;
    pend = (uint32_t)ln == npend ? b : pend;
    if (++npend == 64u) flush();
  }
  __device__ __forceinline__ void match(uint32_t len, uint32_t dist, uint32_t at) {
    flush();
    inf_fence();
    const uint8_t* s = out + (at - dist);
    if (dist >= len) { for (uint32_t i = (uint32_t)ln; i < len; i += 64u) out[at + i] = s[i]; }
    else             { for (uint32_t i = (uint32_t)ln; i < len; i += 64u) out[at + i] = s[i % dist]; }
  }
  __device__ __forceinline__ void stored(uint32_t pos, uint32_t len, uint32_t at) {
    flush();
    for (uint32_t i = (uint32_t)ln; i < len; i += 64u) out[at + i] = pay[pos + i];
  }
  __device__ __forceinline__ int lane() const { return ln; }
  __device__ __forceinline__ int lanes() const { return 64; }
  __device__ __forceinline__ void sync() { inf_fence(); }
  static __device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
};

__global__ __launch_bounds__(64 * INF_WAVES) void k_inflate(const uint8_t* comp, const C3BgzfMember* mem, int nm, uint8_t* out, int2* res) {
  __shared__ InfLds L;
  const int t = threadIdx.x, lane = t & 63;
  const int wv = __builtin_amdgcn_readfirstlane(t >> 6);
  L.crc_tab[t] = bgzf_crc_entry((uint32_t)t);
  if (t == 0) bgzf_x2n_init(L.x2n);
  __syncthreads();
  const int m = blockIdx.x * INF_WAVES + wv;
  if (m >= nm) return;
  const uint32_t poff = InfDev::uni(mem[m].poff), plen = InfDev::uni(mem[m].plen);
  const uint32_t ooff = InfDev::uni(mem[m].ooff), isize = InfDev::uni(mem[m].isize);
  InfDev io;
  io.pay = comp + poff;
  io.sh = poff & 3u;                                  // comp is 256-aligned
  io.pa = (const uint32_t*)(comp + (poff - io.sh));
  io.nwords = (plen + 3u) >> 2;
  io.out = out + ooff;
  io.ln = lane;
  io.cbase = 0x80000000u; io.cv = 0;
  io.pend = 0; io.npend = 0; io.pbase = 0;
  const int st = c3_inflate_member(io, &L.tab[wv], plen, isize);
  uint32_t crc = 0;
  if (st == C3_INF_OK) {
    io.flush();
    inf_fence();
    const uint32_t per = (isize + 63u) >> 6;
    const uint32_t start = min(isize, (uint32_t)lane * per), clen = min(per, isize - start);
    uint32_t c = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < clen; ++i) c = L.crc_tab[(c ^ io.out[start + i]) & 0xFFu] ^ (c >> 8);
    c = clen ? ~c : 0u;
    const uint32_t after = isize - start - clen;
    if (clen && after) c = bgzf_crc_shift(L.x2n, after, c);
    for (int d = 32; d > 0; d >>= 1) c ^= __shfl_xor(c, d, 64);
    crc = c;
  }
  if (lane == 0) res[m] = make_int2(st, (int)crc);
}

extern "C" void c3k_launch_inflate(const uint8_t* comp, const C3BgzfMember* mem, int nm, uint8_t* out, int2* res, hipStream_t s) {
  hipLaunchKernelGGL(k_inflate, dim3((nm + INF_WAVES - 1) / INF_WAVES), dim3(64 * INF_WAVES), 0, s, comp, mem, nm, out, res);
}

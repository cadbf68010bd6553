// k_bgzf.hip -- BGZF members of --bgzf on the GPU (include/c3poa.h "BGZF output").  Same bytes as the host
// statement c3_bgzf_compress_host (c3_bgzf.cpp); code lengths and codes come from the procedures of c3_bgzf.h that the
// host calls too.
//
// k_bgzf: one workgroup of 256 lanes per block of BGZF_BLOCK = 256 x 255 input bytes; lane t owns bytes [255t, 255t + 255)
// of the block and reads them as realigned dwords (v_alignbyte of two aligned loads), three times (histogram, bit count,
// encode + CRC; the block stays in L2 between the passes).
//   1. histogram: LDS atomics into per-wave copies (FASTQ bytes hit a handful of bins), summed into cnt[257] (+ end-of-block).
//   2. code lengths: the symbols with a count are ranked by (count, symbol) by all lanes at once; lane 0 then runs the
//      package-merge of c3_bgzf.h for the literal code (limit 15) and for the code-length code (limit 7), the canonical
//      codes, and the exact bit count of the dynamic block, which decides against a stored block.
//   3. encode: each lane's bit count from the length table, a workgroup exclusive scan gives its bit offset; lanes pack
//      32-bit words of an LDS image of the whole member and join at word boundaries with LDS OR (the image starts zeroed).
//      Lane 0 writes the header and the code table first.  CRC-32: a table CRC per lane over its chunk, shifted to the end
//      of the block by multiplication with x^(8 * bytes after it) mod p (zlib's crc32_combine), XOR-reduced.
//   4. the image leaves with 16-byte stores to the block's 64 KiB slot; sizes[block] = member bytes.
// k_bgzf_pack: one workgroup per member copies it from its slot to packed[exclusive scan of sizes] (each workgroup sums
// the sizes before it), so the device-to-host copy is one copy of compressed bytes.
//
// Resources (hipcc -O3 gfx950, -Rpass-analysis=kernel-resource-usage): k_bgzf 50 VGPRs, 0 AGPRs, 97 SGPRs, ScratchSize 0,
// LDS 76 228 bytes per workgroup = 2 workgroups per CU (occupancy 2 waves/SIMD, bound by LDS: the 64 KiB member image);
// k_bgzf_pack 10 VGPRs, 20 SGPRs, ScratchSize 0, 32 bytes LDS.
#include "c3_dev.h"
#include "c3_bgzf.h"
#include "c3_launch.h"

struct BgzfLds {
  uint32_t img[BGZF_SLOT / 4];                      // the member (header, deflate bits, trailer)
  union {
    uint32_t hist[4][BGZF_NSYM];                    // per-wave histograms (phase 1)
    uint32_t pm[4 * BGZF_NSYM];                     // package-merge lists (phase 2)
  } u;
  uint32_t cnt[BGZF_NSYM];                          // counts (end-of-block = 1)
  uint32_t w[BGZF_NSYM];                            // sorted leaf weights
  uint32_t tab[BGZF_NSYM];                          // reversed code | length << 16
  uint32_t crc_tab[256];
  uint32_t pmbits[15 * BGZF_PM_WORDS];
  uint32_t x2n[20];                                 // x^(2^k) mod p
  uint16_t sym[BGZF_NSYM + 1];
  uint8_t len[BGZF_NSYM + 3], depth[BGZF_NSYM + 3];
  uint32_t cl[19], clc[19], clw[19];
  uint8_t cllen[19], clsym[20], cldep[20];
  uint32_t wsum[4], wcrc[4];
  int nsym, stored, hclen, hdr_bits;
};

__constant__ int k_cl_order[19] = BGZF_CL_ORDER;

__device__ __forceinline__ uint32_t ld_word(const uint8_t* src, int64_t byte) {
  return *(const uint32_t*)(src + byte);            // byte is a multiple of 4, the buffer 256-aligned
}

// lane t's chunk as 4-byte groups: fn(value, valid bytes) for each group
template <class F>
__device__ __forceinline__ void for_chunk(const uint8_t* blk, int start, int clen, F&& fn) {
  if (clen <= 0) return;
  const int r = start & 3;
  int64_t a = start - r;
  uint32_t lo = ld_word(blk, a);
  const int ng = (clen + 3) >> 2;
  for (int g = 0; g < ng; ++g) {
    const uint32_t hi = ld_word(blk, a + 4);
    const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)r);
    fn(v, min(4, clen - 4 * g));
    lo = hi; a += 4;
  }
}

__device__ __forceinline__ void or_byte(uint32_t* img, int pos, uint32_t b) { atomicOr(&img[pos >> 2], (b & 0xFFu) << (8 * (pos & 3))); }

__global__ __launch_bounds__(256) void k_bgzf(const uint8_t* src, long long n, uint8_t* slots, int* sizes) {
  __shared__ BgzfLds L;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int b = blockIdx.x;
  const uint8_t* blk = src + (long long)b * BGZF_BLOCK;
  const int nb = (int)min((long long)BGZF_BLOCK, n - (long long)b * BGZF_BLOCK);
  const int start = 255 * t;
  const int clen = max(0, min(255, nb - start));
  // ---- setup: zero image and histograms, CRC table, x^(2^k)
  {
    uint4* im = (uint4*)L.img;
    for (int i = t; i < BGZF_SLOT / 16; i += 256) im[i] = make_uint4(0, 0, 0, 0);
    for (int i = t; i < 4 * BGZF_NSYM; i += 256) (&L.u.hist[0][0])[i] = 0;
    L.crc_tab[t] = bgzf_crc_entry((uint32_t)t);
    if (t == 0) bgzf_x2n_init(L.x2n);
  }
  __syncthreads();
  // ---- 1. histogram
  for_chunk(blk, start, clen, [&](uint32_t v, int m) {
    for (int q = 0; q < m; ++q) atomicAdd(&L.u.hist[wv][(v >> (8 * q)) & 0xFFu], 1u);
  });
  __syncthreads();
  for (int s = t; s < BGZF_NSYM; s += 256)
    L.cnt[s] = s == 256 ? 1u : L.u.hist[0][s] + L.u.hist[1][s] + L.u.hist[2][s] + L.u.hist[3][s];
  if (t == 0) L.nsym = 0;
  __syncthreads();
  // ---- 2. code lengths: rank of every used symbol by (count, symbol)
  for (int s = t; s < BGZF_NSYM; s += 256) {
    const uint32_t c = L.cnt[s];
    L.len[s] = 0;
    if (c) {
      int rank = 0;
      for (int u = 0; u < BGZF_NSYM; ++u) { const uint32_t cu = L.cnt[u]; rank += (cu && (cu < c || (cu == c && u < s))) ? 1 : 0; }
      L.sym[rank] = (uint16_t)s; L.w[rank] = c;
      atomicAdd(&L.nsym, 1);
    }
  }
  __syncthreads();
  if (t == 0) {
    const int* ORD = k_cl_order;
    const int k = L.nsym;
    bgzf_pm_lengths(L.w, k, 15, L.u.pm, L.pmbits, L.depth);
    for (int i = 0; i < k; ++i) L.len[L.sym[i]] = L.depth[i];
    for (int v = 0; v < 19; ++v) L.clc[v] = 0;
    for (int s = 0; s < BGZF_NSYM; ++s) L.clc[L.len[s]]++;
    L.clc[1]++;
    // code-length code: leaves by (count, symbol), 19 symbols (insertion sort on one lane)
    int kc = 0;
    for (int v = 0; v < 19; ++v) {
      if (!L.clc[v]) continue;
      int j = kc++;
      while (j > 0 && L.clc[L.clsym[j - 1]] > L.clc[v]) { L.clsym[j] = L.clsym[j - 1]; --j; }
      L.clsym[j] = (uint8_t)v;
    }
    for (int i = 0; i < kc; ++i) L.clw[i] = L.clc[L.clsym[i]];
    bgzf_pm_lengths(L.clw, kc, 7, L.u.pm, L.pmbits, L.cldep);
    for (int v = 0; v < 19; ++v) L.cllen[v] = 0;
    for (int i = 0; i < kc; ++i) L.cllen[L.clsym[i]] = L.cldep[i];
    bgzf_canon_codes(L.cllen, 19, L.cl);
    int hclen = 19;
    while (hclen > 4 && L.cllen[ORD[hclen - 1]] == 0) --hclen;
    long long bits = 3 + 14 + 3 * hclen;
    for (int v = 0; v < 19; ++v) bits += (long long)L.clc[v] * L.cllen[v];
    const int hdr = (int)bits;
    for (int s = 0; s < BGZF_NSYM; ++s) bits += (long long)L.cnt[s] * L.len[s];
    L.stored = bits >= 3 + 5 + 32 + 8LL * nb;
    L.hclen = hclen; L.hdr_bits = hdr;
  }
  __syncthreads();
  if (t == 0 && !L.stored) {
    // canonical literal codes into tab[] (lane 0; tab doubles as the rcode array), then the header bits
    bgzf_canon_codes(L.len, BGZF_NSYM, L.tab);
    for (int s = 0; s < BGZF_NSYM; ++s) L.tab[s] |= (uint32_t)L.len[s] << 16;
    const int* ORD = k_cl_order;
    // the deflate bits start at bit 8 * BGZF_HDR = 144: 16 bits into word 4 (its low half is BSIZE, ORed in at the end)
    int wi = 4, na = 16;
    uint64_t acc = 0;
    auto put = [&](uint32_t v, int l) {
      acc |= (uint64_t)v << na; na += l;
      while (na >= 32) { atomicOr(&L.img[wi++], (uint32_t)acc); acc >>= 32; na -= 32; }
    };
    put(1 | (2 << 1), 3);
    put(0, 5); put(0, 5); put((uint32_t)(L.hclen - 4), 4);
    for (int x = 0; x < L.hclen; ++x) put(L.cllen[ORD[x]], 3);
    for (int s = 0; s < BGZF_NSYM; ++s) put(L.cl[L.len[s]], L.cllen[L.len[s]]);
    put(L.cl[1], L.cllen[1]);
    if (na > 0) atomicOr(&L.img[wi], (uint32_t)acc);
  }
  __syncthreads();
  const bool stored = L.stored != 0;
  // ---- 3. encode + CRC
  uint32_t nbits = 0;
  if (!stored)
    for_chunk(blk, start, clen, [&](uint32_t v, int m) {
      for (int q = 0; q < m; ++q) nbits += L.tab[(v >> (8 * q)) & 0xFFu] >> 16;
    });
  // exclusive scan of nbits over the workgroup
  uint32_t inc = nbits;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(inc, d, 64); if (lane >= d) inc += y; }
  if (lane == 63) L.wsum[wv] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (int x = 0; x < 4; ++x) { if (x < wv) before += L.wsum[x]; all += L.wsum[x]; }
  const uint32_t data0 = 8 * BGZF_HDR + (uint32_t)L.hdr_bits;
  uint32_t crc = 0xFFFFFFFFu;
  if (!stored) {
    uint32_t pos = data0 + before + inc - nbits;
    uint64_t acc = 0; int na = (int)(pos & 31); uint32_t wi = pos >> 5;
    for_chunk(blk, start, clen, [&](uint32_t v, int m) {
      for (int q = 0; q < m; ++q) {
        const uint32_t c = (v >> (8 * q)) & 0xFFu;
        crc = L.crc_tab[(crc ^ c) & 0xFFu] ^ (crc >> 8);
        const uint32_t e = L.tab[c];
        acc |= (uint64_t)(e & 0xFFFFu) << na; na += (int)(e >> 16);
        if (na >= 32) { atomicOr(&L.img[wi], (uint32_t)acc); ++wi; acc >>= 32; na -= 32; }
      }
    });
    if (nbits && na > 0) atomicOr(&L.img[wi], (uint32_t)acc);
    if (t == 255) {                                    // end-of-block after the last lane's bits
      const uint32_t e = L.tab[256], p = data0 + all;
      const uint64_t x = (uint64_t)(e & 0xFFFFu) << (p & 31);
      atomicOr(&L.img[p >> 5], (uint32_t)x);
      if ((p & 31) + (e >> 16) > 32) atomicOr(&L.img[(p >> 5) + 1], (uint32_t)(x >> 32));
    }
  } else {
    uint8_t* im8 = (uint8_t*)L.img;
    int p = BGZF_HDR + 5 + start;
    for_chunk(blk, start, clen, [&](uint32_t v, int m) {
      for (int q = 0; q < m; ++q) {
        const uint32_t c = (v >> (8 * q)) & 0xFFu;
        crc = L.crc_tab[(crc ^ c) & 0xFFu] ^ (crc >> 8);
        im8[p++] = (uint8_t)c;
      }
    });
  }
  crc = clen > 0 ? ~crc : 0u;
  // shift lane t's CRC to the end of the block: multiply by x^(8 * after)
  {
    const uint32_t after = (uint32_t)(nb - start - clen);
    if (clen > 0 && after) crc = bgzf_crc_shift(L.x2n, after, crc);
    for (int d = 32; d > 0; d >>= 1) crc ^= __shfl_xor(crc, d, 64);
    if (lane == 0) L.wcrc[wv] = crc;
  }
  __syncthreads();
  int size;
  if (stored) size = BGZF_HDR + 5 + nb + 8;
  else size = BGZF_HDR + (int)((data0 + all + (L.tab[256] >> 16) - 8 * BGZF_HDR + 7) >> 3) + 8;
  if (t == 0) {
    const uint32_t crc_all = L.wcrc[0] ^ L.wcrc[1] ^ L.wcrc[2] ^ L.wcrc[3];
    // 1f 8b 08 04 | MTIME 0 | XFL 0, OS ff, XLEN 6 | 'B' 'C' SLEN 2 | BSIZE
    L.img[0] = 0x04088b1fu; L.img[1] = 0; L.img[2] = 0x0006ff00u; L.img[3] = 0x00024342u;
    atomicOr(&L.img[4], (uint32_t)(size - 1) & 0xFFFFu);
    if (stored) {
      or_byte(L.img, BGZF_HDR, 1);
      or_byte(L.img, BGZF_HDR + 1, (uint32_t)nb); or_byte(L.img, BGZF_HDR + 2, (uint32_t)nb >> 8);
      or_byte(L.img, BGZF_HDR + 3, ~(uint32_t)nb); or_byte(L.img, BGZF_HDR + 4, ~(uint32_t)nb >> 8);
    }
    const int tr = size - 8;
    for (int k = 0; k < 4; ++k) { or_byte(L.img, tr + k, crc_all >> (8 * k)); or_byte(L.img, tr + 4 + k, (uint32_t)nb >> (8 * k)); }
  }
  __syncthreads();
  // ---- 4. out
  uint4* dst = (uint4*)(slots + (size_t)b * BGZF_SLOT);
  const uint4* im = (const uint4*)L.img;
  const int n16 = (size + 15) >> 4;
  for (int i = t; i < n16; i += 256) dst[i] = im[i];
  if (t == 0) sizes[b] = size;
}

__global__ __launch_bounds__(256) void k_bgzf_pack(const uint8_t* slots, const int* sizes, uint8_t* packed) {
  __shared__ long long part[4];
  const int t = threadIdx.x, b = blockIdx.x;
  long long s = 0;
  for (int i = t; i < b; i += 256) s += sizes[i];
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((t & 63) == 0) part[t >> 6] = s;
  __syncthreads();
  const long long off = part[0] + part[1] + part[2] + part[3];
  const int size = sizes[b];
  const uint8_t* in = slots + (size_t)b * BGZF_SLOT;
  uint8_t* out = packed + off;
  for (int i = t; i < size; i += 256) out[i] = in[i];
}

extern "C" void c3k_launch_bgzf(const uint8_t* src, long long n, int n_blocks, uint8_t* slots, int* sizes, uint8_t* packed, hipStream_t s) {
  hipLaunchKernelGGL(k_bgzf, dim3(n_blocks), dim3(256), 0, s, src, n, slots, sizes);
  hipLaunchKernelGGL(k_bgzf_pack, dim3(n_blocks), dim3(256), 0, s, (const uint8_t*)slots, (const int*)sizes, packed);
}

// k_bamout.hip -- the main CLI's records as unaligned BAM, made on the GPU (include/c3poa.h "Records written as unaligned BAM";
// DESIGN.md 5.15).  Which records a read writes is c3_emit.h, what a record is made of c3_bamout.h; the host statement
// c3_emit_group_bam_host (c3_bamout.cpp) applies both as well.  Two kinds per splint (consensus, subreads), so the three scan
// kernels of k_emit.hip place the records unchanged with K = 2; this file finds the lengths and writes the bytes.
//
//   k_bamout_len   k_emit_len with the BAM record lengths.  The quality sum of a read with a consensus record (the aq tag is
//       made from it in the write pass) is kept in the third length slot, which no scan reads at K = 2.
//   k_bamout_write   one wave per read, the four waves of a workgroup together on the body segments of a read above TX_LONG
//       bases, as k_emit_write.  The 36 fixed bytes, the decimals and the tags are byte stores of the first lanes (nothing in a
//       record is aligned), the name goes through tx_wave_copy.  The bases are PACKED, not copied: a lane takes eight source
//       bases from two or three aligned dwords joined by v_alignbyte and stores one dword of nibbles; the packed bytes in front
//       of the first aligned destination dword and behind the last whole one are byte stores, the half byte of an odd l_seq
//       among them.  Byte -> nibble is a 256-entry table in LDS, filled once per workgroup from c3_bamout_code: the rule wants
//       every byte value mapped (lower case, IUPAC letters, '=', anything else N), arithmetic for the letters would still need
//       the table behind it, and the pass waits for its loads and stores, not for eight ds_read_u8 per dword (A, C, G and T sit
//       in three different banks, equal addresses broadcast).  Qualities are copied dword-wise with a packed saturating
//       subtract of 33 and a minimum with 93 on the even and the odd bytes; a consensus without QVs gets 0xFF dwords.
//       A shared read is cut in whole 256-byte rows of the PACKED bases (tx_piece over (l_seq + 1) / 2), so every part starts at
//       an even base; its qualities in rows of the quality bytes.  A wave writes nothing outside its read's own ranges
//       [roff, roff + len) and loads no dword that does not hold a byte of the segment it works on.
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_bamout.h"
#include "c3_launch.h"
#include "k_text.h"
#include "k_emit_dev.h"

__global__ __launch_bounds__(64 * TX_WAVES) void k_bamout_len(EmitArgs a) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * TX_WAVES + (int)(threadIdx.x >> 6);
  if (i >= a.n) return;
  const c3_read_result& r = a.info[i];
  const int64_t so = a.off[i], L = a.off[i + 1] - so, nl = a.name_off[i + 1] - a.name_off[i], clen = em_clen(a, i);
  const int s = a.sid[i];
  const C3EmitDec d = c3_emit_of(r, s, a.n_splints, a.zero, clen);
  long long sub = 0;
  for (int j = lane; j < d.np; j += 64) {
    int32_t idx; int64_t b, e;
    c3_emit_piece(r, d, L, j, &idx, &b, &e);
    sub += c3_bamout_sub_len(nl, idx, e - b);
  }
  sub = em_wave_sum(sub);
  long long tot = 0;
  if (d.cons && L > 0) tot = em_byte_sum(a.quals + so, L, lane) - 33ll * L;
  if (lane != 0) return;
  EmitHead h;
  for (int k = 0; k < 8; ++k) h.aq[k] = 0;
  h.aql = d.cons ? c3_emit_avgq(tot, L > 0 ? L : 1, h.aq) : 0;
  h.s = d.any ? s : -1; h.cons = d.cons; h.np = d.np;
  a.head[i] = h;
  int64_t* len = a.len + (size_t)i * C3_EMIT_KINDS;
  len[C3_BAMOUT_SUB] = d.any ? sub : 0;
  len[C3_BAMOUT_CONS] = d.cons ? c3_bamout_cons_len(nl, c3_emit_head_tail_len(h.aql, L, d.ns, clen), clen) : 0;
  len[2] = tot;                                                          // (not a length: the quality sum, for the aq tag)
}

// eight bases (b0 the lowest byte of lo) -> four packed bytes, the first base of a pair in the high nibble
__device__ __forceinline__ uint32_t bo_pack8(uint32_t lo, uint32_t hi, const uint8_t* tab) {
  const uint32_t p0 = (uint32_t)tab[lo & 255u] << 4 | tab[(lo >> 8) & 255u], p1 = (uint32_t)tab[(lo >> 16) & 255u] << 4 | tab[lo >> 24];
  const uint32_t p2 = (uint32_t)tab[hi & 255u] << 4 | tab[(hi >> 8) & 255u], p3 = (uint32_t)tab[(hi >> 16) & 255u] << 4 | tab[hi >> 24];
  return p0 | p1 << 8 | p2 << 16 | p3 << 24;
}

// dst[0 .. (n + 1) / 2) = the n bases src[0 .. n) packed, by the 64 lanes of a wave, any alignment on either side
__device__ __forceinline__ void bo_wave_pack(uint8_t* dst, const uint8_t* src, uint32_t n, int lane, const uint8_t* tab) {
  const uint32_t nb = (n + 1u) >> 1, nfull = n >> 1;                      // packed bytes; those that hold two bases
  const uint32_t head = min(nfull, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) dst[lane] = (uint8_t)(tab[src[2 * lane]] << 4 | tab[src[2 * lane + 1]]);
  const uint32_t nd = (nfull - head) >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  const uint8_t* s = src + 2u * head;
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
  const uint32_t* sa = (const uint32_t*)(s - sh);
  if (sh == 0) { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = bo_pack8(sa[2u * k], sa[2u * k + 1u], tab); }
  else {
    for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) {                 // sa[2k + 2] holds base s + 8k + 7 at least
      const uint32_t x0 = sa[2u * k], x1 = sa[2u * k + 1u], x2 = sa[2u * k + 2u];
      d4[k] = bo_pack8(__builtin_amdgcn_alignbyte(x1, x0, sh), __builtin_amdgcn_alignbyte(x2, x1, sh), tab);
    }
  }
  const uint32_t k = head + 4u * nd + (uint32_t)lane;                     // at most three whole bytes and the half one
  if (k < nb) {
    uint32_t v = (uint32_t)tab[src[2u * k]] << 4;
    if (2u * k + 1u < n) v |= tab[src[2u * k + 1u]];
    dst[k] = (uint8_t)v;
  }
}

// four quality bytes: min(max(b - 33, 0), 93) on the even and on the odd bytes as two 16-bit lanes each
typedef unsigned short bo_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t bo_qual4(uint32_t x) {
  const bo_us2 c33 = {33, 33}, c93 = {93, 93};
  const bo_us2 e = __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_bit_cast(bo_us2, x & 0x00FF00FFu), c33), c93);
  const bo_us2 o = __builtin_elementwise_min(__builtin_elementwise_sub_sat(__builtin_bit_cast(bo_us2, (x >> 8) & 0x00FF00FFu), c33), c93);
  return __builtin_bit_cast(uint32_t, e) | __builtin_bit_cast(uint32_t, o) << 8;
}

// dst[0 .. len) = the quality bytes src[0 .. len) as BAM stores them: tx_wave_copy with bo_qual4 on the way
__device__ __forceinline__ void bo_wave_qual(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
  const uint32_t head = min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) dst[lane] = (uint8_t)c3_bamout_qual(src[lane]);
  const uint32_t nd = (len - head) >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  const uint8_t* s = src + head;
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
  const uint32_t* sa = (const uint32_t*)(s - sh);
  if (sh == 0) { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = bo_qual4(sa[k]); }
  else         { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = bo_qual4(__builtin_amdgcn_alignbyte(sa[k + 1], sa[k], sh)); }
  const uint32_t done = head + 4u * nd, tail = len - done;
  if ((uint32_t)lane < tail) dst[done + lane] = (uint8_t)c3_bamout_qual(src[done + lane]);
}

__device__ __forceinline__ void bo_wave_fill(uint8_t* dst, uint32_t len, int lane) {
  const uint32_t head = min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) dst[lane] = (uint8_t)C3_BAMOUT_NOQUAL;
  const uint32_t nd = (len - head) >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = 0x01010101u * C3_BAMOUT_NOQUAL;
  const uint32_t done = head + 4u * nd, tail = len - done;
  if ((uint32_t)lane < tail) dst[done + lane] = (uint8_t)C3_BAMOUT_NOQUAL;
}

// seq and qual of one record at body: the whole of them (parts == 1) or this wave's share.  The bases are shared in whole
// 256-byte rows of the packed bytes, so a part starts at an even base and only the last one can end in a half byte.
__device__ __forceinline__ void bo_body(uint8_t* body, const uint8_t* seq, const uint8_t* qual, uint32_t n, int lane, int part, int parts,
                                        const uint8_t* tab) {
  const uint32_t nb = (n + 1u) >> 1;
  uint32_t b = 0, e = nb, qb = 0, qe = n;
  if (parts > 1) { tx_piece(nb, part, parts, &b, &e); tx_piece(n, part, parts, &qb, &qe); }
  if (b < e) bo_wave_pack(body + b, seq + 2u * b, min(n, 2u * e) - 2u * b, lane, tab);
  if (qual) bo_wave_qual(body + nb + qb, qual + qb, qe - qb, lane);
  else bo_wave_fill(body + nb + qb, qe - qb, lane);
}

__device__ __forceinline__ void bo_fixed(uint8_t* out, int64_t total, uint32_t l_read_name, uint32_t l_seq, int lane) {
  if (lane < C3_BAMOUT_FIXED) out[lane] = (uint8_t)(c3_bamout_fixed(lane >> 2, (uint32_t)(total - 4), l_read_name, l_seq) >> (8 * (lane & 3)));
}

// the records of read i by one wave; part / parts: this wave's share of the body segments of a long read (part 0 also
// writes the fixed fields, names and tags), 0 / 1 for a read the wave has to itself
__device__ __forceinline__ void bo_write_read(const EmitArgs& a, int i, int lane, int part, int parts, const uint8_t* tab) {
  const EmitHead h = a.head[i];
  if (wave_first(h.s) < 0) return;
  const c3_read_result& r = a.info[i];
  const int64_t so = a.off[i], no = a.name_off[i], L = a.off[i + 1] - so;
  const uint32_t nl = (uint32_t)(a.name_off[i + 1] - no);
  const int64_t clen = em_clen(a, i);
  const C3EmitDec d = c3_emit_of(r, h.s, a.n_splints, a.zero, clen);
  const uint8_t* name = a.names + no;
  const int64_t* roff = a.roff + (size_t)i * C3_EMIT_KINDS;
  uint8_t* out = a.arena + roff[C3_BAMOUT_SUB];
  const int np = wave_first(h.np);
  for (int j = 0; j < np; ++j) {
    int32_t idx; int64_t b, e;
    c3_emit_piece(r, d, L, j, &idx, &b, &e);
    const uint32_t len = (uint32_t)wave_first((int)(e - b));
    const int dn = c3_emit_dec_len(idx);
    const uint32_t lrn = nl + (uint32_t)dn + 2u;
    const int64_t total = c3_bamout_sub_len(nl, idx, len);
    if (part == 0) {
      bo_fixed(out, total, lrn, len, lane);
      tx_wave_copy(out + C3_BAMOUT_FIXED, name, nl, lane);
      uint8_t* t = out + C3_BAMOUT_FIXED + nl;                           // _<idx> NUL
      if (lane == 0) t[0] = '_';
      else if (lane <= dn) t[lane] = (uint8_t)c3_emit_dec_char(idx, lane - 1);
      else if (lane == dn + 1) t[lane] = 0;
    }
    bo_body(out + C3_BAMOUT_FIXED + lrn, a.seqs + so + b, a.quals + so + b, len, lane, part, parts, tab);
    out += total;
  }
  if (!wave_first(h.cons)) return;
  const int ht = c3_emit_head_tail_len(h.aql, L, d.ns, clen);
  const uint32_t cl = (uint32_t)clen, lrn = nl + (uint32_t)ht;
  out = a.arena + roff[C3_BAMOUT_CONS];
  uint8_t* body = out + C3_BAMOUT_FIXED + lrn;
  if (part == 0) {
    bo_fixed(out, c3_bamout_cons_len(nl, ht, clen), lrn, cl, lane);
    tx_wave_copy(out + C3_BAMOUT_FIXED, name, nl, lane);
    if (lane < ht) out[C3_BAMOUT_FIXED + nl + lane] = lane == ht - 1 ? (uint8_t)0 : (uint8_t)c3_emit_head_tail_char(lane, a.head[i].aq, h.aql, L, d.ns, clen);
    if (lane < C3_BAMOUT_TAGS) body[((cl + 1u) >> 1) + cl + lane] = c3_bamout_tag_byte(lane, d.ns, L, a.len[(size_t)i * C3_EMIT_KINDS + 2]);
  }
  bo_body(body, a.cons + a.cons_at[i], a.qv ? a.qv + a.cons_at[i] : nullptr, cl, lane, part, parts, tab);
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_bamout_write(EmitArgs a) {
  __shared__ uint8_t tab[256];
  tab[threadIdx.x] = (uint8_t)c3_bamout_code(threadIdx.x);               // (64 * TX_WAVES = 256 lanes: one entry each)
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wv = wave_first((int)(threadIdx.x >> 6));
  const int i0 = blockIdx.x * TX_WAVES;
  {
    const int i = i0 + wv;
    if (i < a.n && a.off[i + 1] - a.off[i] <= TX_LONG) bo_write_read(a, i, lane, 0, 1, tab);
  }
  for (int k = 0; k < TX_WAVES; ++k) {                   // long reads of the workgroup: a quarter of every body segment each
    const int i = i0 + k;
    if (i >= a.n) break;
    if (a.off[i + 1] - a.off[i] <= TX_LONG) continue;
    bo_write_read(a, i, lane, wv, TX_WAVES, tab);
  }
}
static_assert(64 * TX_WAVES == 256, "k_bamout_write fills its 256-entry table with one lane per entry");

extern "C" void c3k_launch_bamout_len(const EmitArgs* a, hipStream_t s) {
  if (a->n > 0) hipLaunchKernelGGL(k_bamout_len, dim3((a->n + TX_WAVES - 1) / TX_WAVES), dim3(64 * TX_WAVES), 0, s, *a);
}
extern "C" void c3k_launch_bamout_write(const EmitArgs* a, hipStream_t s) {
  if (a->n > 0) hipLaunchKernelGGL(k_bamout_write, dim3((a->n + TX_WAVES - 1) / TX_WAVES), dim3(64 * TX_WAVES), 0, s, *a);
}

// k_post.hip -- post-processing records made on the GPU (include/c3poa.h "Post-processing on the GPU").
// The rule of one read is c3_post.h, which the host statement c3_post_emit_host (c3_post.cpp) applies as well; this file
// finds the lengths, scans them and moves the bytes.  S = 3 * n_dest + 3 output streams (c3poa.h) lie back to back in one
// arena; column S of the sums counts the kept reads.
//
//   k_post_classify   one lane per read: the adapter rule, the oligo-dT pieces cut and matched (c3_match_rule, the function
//       k_match_index runs), the decision (p, m, direction, destination, kept) and the byte length of the read's five
//       records and of its PSL rows (decimal digit counts included).
//   k_post_rsum / k_post_rscan / k_post_rfin   exclusive scans of the lengths per stream, as k_fastq_rsum / _rscan / _rfin:
//       per-workgroup sums (a read adds to at most six streams: a wave scan per stream, the four waves joined through LDS),
//       one small workgroup over those, then every workgroup again with its base, writing the arena offset of each record.
//       No atomics anywhere: the order of the records in a stream is the input order by construction.
//   k_post_emit   the pass that moves every byte once: one wave per read, the four waves of a workgroup together on the
//       body segments of a read above TX_LONG bytes.  Literals and decimals are written by the first few lanes; forward
//       segments go dword-wise from two aligned source dwords joined by v_alignbyte (tx_wave_copy of k_text.h); reverse
//       segments walk the source dwords from the end, swap the bytes of each and complement them through a 256-byte table in
//       LDS (qualities skip the table).  A wave writes nothing outside its record's own range [roff, roff + length) and reads
//       nothing outside the dwords that hold the batch's bytes (the host keeps 16 bytes of slack behind every buffer).
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_post.h"
#include "c3_launch.h"
#include "k_text.h"

#define PO_COLS (C3_POST_MAX_STREAMS + 1)

__global__ __launch_bounds__(256) void k_post_classify(PostArgs a) {
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  if (i >= a.n) return;
  const int64_t so = a.off[i], no = a.name_off[i];
  const int32_t L = (int32_t)(a.off[i + 1] - so), nlen = (int32_t)(a.name_off[i + 1] - no);
  const int32_t* tab = a.table + (size_t)i * a.o.n_ad * 24;
  C3PostDec d;
  c3_post_adapters(tab, a.ad_len, a.ad_class, a.o, &d);
  if (d.kept && a.o.has_index) c3_post_oligo((const char*)a.seqs + so, L, a.o, (const char*)a.idx_cat, a.idx_off, a.idx_dest, &d);
  a.dec[i] = d;
  C3PostSeg seg[C3_POST_MAX_SEG];
  for (int k = 0; k < 5; ++k) { int64_t t; (void)c3_post_plan(k, d, L, nlen, a.o, seg, &t); a.len[(size_t)i * C3_POST_REC + k] = t; }
  int64_t psl = 0;
  for (int e = 0; e < a.o.n_ad * 2; ++e) {
    const int32_t* r = tab + (size_t)e * 12;
    if (r[0] < C3_POST_MIN_SCORE) continue;
    const int ad = e >> 1;
    psl += c3_post_psl_row(nullptr, r, nullptr, nlen, L, nullptr, (int32_t)(a.ad_name_off[ad + 1] - a.ad_name_off[ad]), a.ad_len[ad], e & 1);
  }
  a.len[(size_t)i * C3_POST_REC + 5] = psl;
}

// what read i adds to column c of the sums, and which of its records (0..5, -1: none) that is
struct PoRead { long long len[C3_POST_REC]; int kept, dest; };
__device__ __forceinline__ PoRead po_load(const PostArgs& a, int i) {
  PoRead r;
  if (i < a.n) {
    for (int k = 0; k < C3_POST_REC; ++k) r.len[k] = a.len[(size_t)i * C3_POST_REC + k];
    r.kept = a.dec[i].kept; r.dest = a.dec[i].dest;
  } else {
    for (int k = 0; k < C3_POST_REC; ++k) r.len[k] = 0;
    r.kept = 0; r.dest = 0;
  }
  return r;
}
__device__ __forceinline__ long long po_contrib(const PoRead& r, int c, int S, int* rec) {
  int k = -1;
  if (c == S) { *rec = -1; return r.kept; }
  if (c >= S - 3) k = c - (S - 3) + 3;
  else if (r.kept && c / 3 == r.dest) k = c % 3;
  *rec = k;
  return k == 0 ? r.len[0] : k == 1 ? r.len[1] : k == 2 ? r.len[2] : k == 3 ? r.len[3] : k == 4 ? r.len[4] : k == 5 ? r.len[5] : 0;
}

__global__ __launch_bounds__(256) void k_post_rsum(PostArgs a) {
  __shared__ long long lds[TX_WAVES][PO_COLS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, SC = a.S + 1;
  const PoRead r = po_load(a, blockIdx.x * 256 + (int)threadIdx.x);
  for (int c = 0; c < SC; ++c) {
    int rec;
    const long long inc = tx_wave_incl(po_contrib(r, c, a.S, &rec));
    if (lane == 63) lds[wv][c] = inc;
  }
  __syncthreads();
  if ((int)threadIdx.x < SC) {
    long long t = 0;
    for (int k = 0; k < TX_WAVES; ++k) t += lds[k][threadIdx.x];
    a.bsum[(size_t)blockIdx.x * SC + threadIdx.x] = t;
  }
}

// bsum[nb][S + 1] -> exclusive prefix sums per column, in place; stream_off[S + 1] and the kept count
__global__ __launch_bounds__(256) void k_post_rscan(PostArgs a, int nb) {
  __shared__ long long lds[TX_WAVES];
  __shared__ long long tot[PO_COLS];
  const int SC = a.S + 1;
  for (int c = 0; c < SC; ++c) {
    long long run = 0;
    for (int i0 = 0; i0 < nb; i0 += 256) {
      const int i = i0 + (int)threadIdx.x;
      const long long v = i < nb ? a.bsum[(size_t)i * SC + c] : 0;
      long long t;
      const long long ex = tx_block_excl(v, lds, &t);
      if (i < nb) a.bsum[(size_t)i * SC + c] = run + ex;
      run += t;
    }
    if (threadIdx.x == 0) tot[c] = run;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long at = 0;
    for (int s = 0; s < a.S; ++s) { a.stream_off[s] = at; at += tot[s]; }
    a.stream_off[a.S] = at;
    a.stream_off[a.S + 1] = tot[a.S];                   // kept reads
  }
}

__global__ __launch_bounds__(256) void k_post_rfin(PostArgs a) {
  __shared__ long long lds[TX_WAVES][PO_COLS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, SC = a.S + 1;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const PoRead r = po_load(a, i);
  long long e0 = 0, e1 = 0, e2 = 0, e3 = 0, e4 = 0, e5 = 0;
  for (int c = 0; c < a.S; ++c) {
    int rec;
    const long long v = po_contrib(r, c, a.S, &rec);
    const long long inc = tx_wave_incl(v);
    if (lane == 63) lds[wv][c] = inc;
    const long long ex = inc - v;
    if (rec == 0) e0 = ex; else if (rec == 1) e1 = ex; else if (rec == 2) e2 = ex; else if (rec == 3) e3 = ex; else if (rec == 4) e4 = ex; else if (rec == 5) e5 = ex;
  }
  __syncthreads();
  if (i >= a.n) return;
  const long long ex[C3_POST_REC] = {e0, e1, e2, e3, e4, e5};
#pragma unroll
  for (int k = 0; k < C3_POST_REC; ++k) {
    const int c = k == 5 ? a.S - 1 : c3_post_stream(k, r.dest, a.o.n_dest);
    long long base = a.stream_off[c] + a.bsum[(size_t)blockIdx.x * SC + c];
    for (int w = 0; w < wv; ++w) base += lds[w][c];
    a.roff[(size_t)i * C3_POST_REC + k] = base + ex[k];
  }
}

// the reverse of tx_wave_copy: dst[j] = T(src[len - 1 - j]), T = the complement table (COMP) or the identity: destination dwords in ascending order, the
// source dword of each (any alignment: two aligned dwords joined by v_alignbyte) taken from the end and byte-swapped
template <bool COMP> __device__ __forceinline__ uint8_t po_tr(const uint8_t* tab, uint8_t c) { return COMP ? tab[c] : c; }
template <bool COMP> __device__ __forceinline__ void po_copy_rev(uint8_t* dst, const uint8_t* src, uint32_t len, int lane, const uint8_t* tab) {
  const uint32_t head = min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) dst[lane] = po_tr<COMP>(tab, src[len - 1u - (uint32_t)lane]);
  const uint32_t rest = len - head, nd = rest >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  if (nd) {
    const uint8_t* q0 = src + rest - 4u;                 // source bytes of destination dword 0; dword k: q0 - 4k >= src
    const uint32_t sh = (uint32_t)((uintptr_t)q0 & 3u);
    const uint32_t* sa = (const uint32_t*)(q0 - sh);
    for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) {
      const uint32_t* p = sa - k;
      uint32_t w = sh == 0 ? p[0] : __builtin_amdgcn_alignbyte(p[1], p[0], sh);      // p[1] holds byte q0 - 4k + 3, p[0] byte q0 - 4k
      w = __builtin_bswap32(w);
      if (COMP) w = (uint32_t)tab[w & 255u] | ((uint32_t)tab[(w >> 8) & 255u] << 8) | ((uint32_t)tab[(w >> 16) & 255u] << 16) | ((uint32_t)tab[w >> 24] << 24);
      d4[k] = w;
    }
  }
  const uint32_t done = head + 4u * nd, tail = len - done;             // the first `tail` source bytes are left
  if ((uint32_t)lane < tail) dst[done + lane] = po_tr<COMP>(tab, src[tail - 1u - (uint32_t)lane]);
}

// records 0..4 of read i by one wave; part / parts: this wave's share of the body segments of a long read (part 0 also
// writes the short segments), 0 / 1 for a read the wave has to itself
__device__ __forceinline__ void po_emit_records(const PostArgs& a, int i, int lane, int part, int parts, const uint8_t* comp) {
  const C3PostDec d = a.dec[i];
  if (!d.kept) return;
  const int64_t so = a.off[i], no = a.name_off[i];
  const int32_t L = (int32_t)(a.off[i + 1] - so), nlen = (int32_t)(a.name_off[i + 1] - no);
  const uint8_t* seq = a.seqs + so;
  const uint8_t* qual = a.quals ? a.quals + so : nullptr;
  C3PostSeg seg[C3_POST_MAX_SEG];
  for (int k = 0; k < 5; ++k) {
    int64_t t;
    const int ns = c3_post_plan(k, d, L, nlen, a.o, seg, &t);
    uint8_t* out = a.arena + a.roff[(size_t)i * C3_POST_REC + k];
    for (int j = 0; j < ns; ++j) {
      const int kind = wave_first(seg[j].kind), sa = wave_first(seg[j].a), sl = wave_first(seg[j].len);
      if (kind == C3_SEG_LIT) {
        if (part == 0 && lane < sl) out[lane] = (uint8_t)c3_post_lit(sa)[lane];
      } else if (kind == C3_SEG_DEC) {
        if (part == 0 && lane < sl) out[lane] = (uint8_t)c3_post_digit((uint32_t)sa, sl, lane);
      } else if (kind == C3_SEG_NAME) {
        if (part == 0) tx_wave_copy(out, a.names + no, (uint32_t)sl, lane);
      } else {
        uint32_t b = 0, e = (uint32_t)sl;                             // this wave's piece of the destination
        if (parts > 1) tx_piece((uint32_t)sl, part, parts, &b, &e);
        const uint8_t* src = (kind == C3_SEG_SEQ_F || kind == C3_SEG_SEQ_R) ? seq + sa : qual + sa;
        if (kind == C3_SEG_SEQ_F || kind == C3_SEG_QUAL_F) tx_wave_copy(out + b, src + b, e - b, lane);
        else if (kind == C3_SEG_SEQ_R) po_copy_rev<true>(out + b, src + ((uint32_t)sl - e), e - b, lane, comp);
        else po_copy_rev<false>(out + b, src + ((uint32_t)sl - e), e - b, lane, comp);
      }
      out += sl;
    }
  }
}

// the PSL rows of read i: one lane per table entry, placed by a wave scan of the row lengths
__device__ __forceinline__ void po_emit_psl(const PostArgs& a, int i, int lane) {
  const int64_t no = a.name_off[i];
  const int32_t L = (int32_t)(a.off[i + 1] - a.off[i]), nlen = (int32_t)(a.name_off[i + 1] - no);
  const int32_t* tab = a.table + (size_t)i * a.o.n_ad * 24;
  uint8_t* out = a.arena + a.roff[(size_t)i * C3_POST_REC + 5];
  const int ne = a.o.n_ad * 2;
  for (int e0 = 0; e0 < ne; e0 += 64) {
    const int e = e0 + lane;
    const bool on = e < ne && tab[(size_t)(e < ne ? e : 0) * 12] >= C3_POST_MIN_SCORE;
    const int ad = on ? e >> 1 : 0;
    const char* an = (const char*)a.ad_names + a.ad_name_off[ad];
    const int32_t anl = (int32_t)(a.ad_name_off[ad + 1] - a.ad_name_off[ad]);
    const int32_t* r = tab + (size_t)(on ? e : 0) * 12;
    const int len = on ? (int)c3_post_psl_row(nullptr, r, nullptr, nlen, L, nullptr, anl, a.ad_len[ad], e & 1) : 0;
    const int inc = wave_scan_add(len);
    if (on) (void)c3_post_psl_row((char*)out + (inc - len), r, (const char*)a.names + no, nlen, L, an, anl, a.ad_len[ad], e & 1);
    out += wave_bcast(inc, 63);
  }
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_post_emit(PostArgs a) {
  __shared__ uint8_t comp[256];
  comp[threadIdx.x] = c3_post_comp((uint8_t)threadIdx.x);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int wv = wave_first((int)(threadIdx.x >> 6));
  const int i0 = blockIdx.x * TX_WAVES;
  {
    const int i = i0 + wv;
    if (i < a.n) {
      if (a.o.n_ad > 0) po_emit_psl(a, i, lane);
      if (a.off[i + 1] - a.off[i] <= TX_LONG) po_emit_records(a, i, lane, 0, 1, comp);
    }
  }
  for (int k = 0; k < TX_WAVES; ++k) {                   // long reads of the workgroup: a quarter of every body segment each
    const int i = i0 + k;
    if (i >= a.n) break;
    if (a.off[i + 1] - a.off[i] <= TX_LONG) continue;
    po_emit_records(a, i, lane, wv, TX_WAVES, comp);
  }
}

extern "C" void c3k_launch_post_classify(const PostArgs* a, hipStream_t s) {
  if (a->n > 0) hipLaunchKernelGGL(k_post_classify, dim3((a->n + 255) / 256), dim3(256), 0, s, *a);
}
// bsum holds (S + 1) * ((n + 255) / 256) sums; stream_off S + 2 entries (the last = kept reads)
extern "C" void c3k_launch_post_scan(const PostArgs* a, hipStream_t s) {
  const int nb = (a->n + 255) / 256;
  if (nb) hipLaunchKernelGGL(k_post_rsum, dim3(nb), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_post_rscan, dim3(1), dim3(256), 0, s, *a, nb);
  if (nb) hipLaunchKernelGGL(k_post_rfin, dim3(nb), dim3(256), 0, s, *a);
}
extern "C" void c3k_launch_post_emit(const PostArgs* a, hipStream_t s) {
  if (a->n > 0) hipLaunchKernelGGL(k_post_emit, dim3((a->n + TX_WAVES - 1) / TX_WAVES), dim3(64 * TX_WAVES), 0, s, *a);
}

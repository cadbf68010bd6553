// k_emit.hip -- the main CLI's records made on the GPU (include/c3poa.h "Records formatted on the GPU").
// The rule of one read is c3_emit.h, which the host statement c3_emit_group_host (c3_emit.cpp) applies as well; this file
// finds the lengths, scans them and moves the bytes.  K kinds (consensus FASTA, subread FASTQ, consensus FASTQ) per splint:
// stream s * K + kind; column S * K of the sums counts the records.  All pointers are device pointers: the same kernels
// serve the resident batch (c3_batch_emit_snapshot) and an uploaded group (c3_emit_group).
//
//   k_emit_len   one wave per read: which records (c3_emit_of), the bytes they add to each kind (lanes over the subread
//       records, a wave sum), and for a consensus record the quality sum of the whole read (dword loads, v_sad_u8 per dword)
//       and from it the average-quality text of the header, kept per read with the decision.
//   k_emit_rsum / k_emit_rscan / k_emit_rfin   exclusive scans of the lengths per stream, as k_post_rsum / _rscan / _rfin:
//       per-workgroup sums (a wave scan per column, the four waves joined through LDS), one small workgroup over those, then
//       every workgroup again with its base, writing the arena offset of each read's bytes of each kind.  No atomics: the
//       order of the records in a stream is the read order by construction.
//   k_emit_write   the pass that moves every byte once: one wave per read, the four waves of a workgroup together on the
//       body segments of a read above TX_LONG bases.  Header literals and decimals are written by the first few lanes; names
//       and body segments (a subread's bases or qualities, a consensus, a QV run) go dword-wise from two aligned source
//       dwords joined by v_alignbyte (tx_wave_copy of k_text.h).  A wave writes nothing outside its read's own ranges
//       [roff, roff + len) and reads no dword that does not hold a byte of the segment it copies.
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_emit.h"
#include "c3_launch.h"
#include "k_text.h"
#include "k_emit_dev.h"

__global__ __launch_bounds__(64 * TX_WAVES) void k_emit_len(EmitArgs a) {
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
    sub += c3_emit_sub_len(nl, idx, e - b);
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
  len[C3_EMIT_SUB_FQ] = d.any ? sub : 0;
  len[C3_EMIT_CONS_FA] = d.cons ? c3_emit_cons_len(C3_EMIT_CONS_FA, nl, h.aql, L, d.ns, clen) : 0;
  len[C3_EMIT_CONS_FQ] = d.cons && a.K == 3 ? c3_emit_cons_len(C3_EMIT_CONS_FQ, nl, h.aql, L, d.ns, clen) : 0;
}

// what read i adds to column c of the sums
struct EmRead { long long len[C3_EMIT_KINDS]; int s, rec; };
__device__ __forceinline__ EmRead em_load(const EmitArgs& a, int i) {
  EmRead r;
  r.s = -1; r.rec = 0;
  for (int k = 0; k < C3_EMIT_KINDS; ++k) r.len[k] = 0;
  if (i < a.n) {
    const EmitHead h = a.head[i];
    r.s = h.s;
    if (h.s >= 0) {
      for (int k = 0; k < a.K; ++k) r.len[k] = a.len[(size_t)i * C3_EMIT_KINDS + k];
      r.rec = h.np + (h.cons ? a.K - 1 : 0);
    }
  }
  return r;
}
__device__ __forceinline__ long long em_contrib(const EmRead& r, int c, int K, int SK) {
  if (c == SK) return r.rec;
  if (r.s < 0 || c / K != r.s) return 0;
  const int k = c % K;
  return k == 0 ? r.len[0] : k == 1 ? r.len[1] : r.len[2];
}

// The two passes below visit ALL S * K + 1 columns in every workgroup (a wave sum or scan each), although a read adds to at
// most K + 1 of them: 0.07 ms per 100 000 reads at one splint, linear in the splint count (193 passes at 64 splints), and not
// measured at more than one splint.  A read-major pass over the splints a workgroup actually holds would remove the factor.
__global__ __launch_bounds__(256) void k_emit_rsum(EmitArgs a) {
  __shared__ long long lds[TX_WAVES][C3_EMIT_MAX_COLS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, SK = a.n_splints * a.K, SC = SK + 1;
  const EmRead r = em_load(a, blockIdx.x * 256 + (int)threadIdx.x);
  for (int c = 0; c < SC; ++c) {
    const long long t = em_wave_sum(em_contrib(r, c, a.K, SK));
    if (lane == 0) lds[wv][c] = t;
  }
  __syncthreads();
  for (int c = (int)threadIdx.x; c < SC; c += 256) {
    long long t = 0;
    for (int k = 0; k < TX_WAVES; ++k) t += lds[k][c];
    a.bsum[(size_t)blockIdx.x * SC + c] = t;
  }
}

// bsum[nb][S * K + 1] -> exclusive prefix sums per column, in place; stream_off[S * K + 1] and the record count
__global__ __launch_bounds__(256) void k_emit_rscan(EmitArgs a, int nb) {
  __shared__ long long lds[TX_WAVES];
  __shared__ long long tot[C3_EMIT_MAX_COLS];
  const int SK = a.n_splints * a.K, SC = SK + 1;
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
    for (int c = 0; c < SK; ++c) { a.stream_off[c] = at; at += tot[c]; }
    a.stream_off[SK] = at;
    a.stream_off[SK + 1] = tot[SK];                     // records
  }
}

__global__ __launch_bounds__(256) void k_emit_rfin(EmitArgs a) {
  __shared__ long long lds[TX_WAVES][C3_EMIT_MAX_COLS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, SK = a.n_splints * a.K, SC = SK + 1;
  const int i = blockIdx.x * 256 + (int)threadIdx.x;
  const EmRead r = em_load(a, i);
  long long e0 = 0, e1 = 0, e2 = 0;
  for (int c = 0; c < SK; ++c) {
    const long long v = em_contrib(r, c, a.K, SK);
    const long long inc = tx_wave_incl(v);
    if (lane == 63) lds[wv][c] = inc;
    if (r.s >= 0 && c / a.K == r.s) { const int k = c % a.K; const long long ex = inc - v; if (k == 0) e0 = ex; else if (k == 1) e1 = ex; else e2 = ex; }
  }
  __syncthreads();
  if (i >= a.n) return;
  const long long ex[C3_EMIT_KINDS] = {e0, e1, e2};
#pragma unroll
  for (int k = 0; k < C3_EMIT_KINDS; ++k) {
    long long at = 0;
    if (r.s >= 0 && k < a.K) {
      const int c = r.s * a.K + k;
      at = a.stream_off[c] + a.bsum[(size_t)blockIdx.x * SC + c] + ex[k];
      for (int w = 0; w < wv; ++w) at += lds[w][c];
    }
    a.roff[(size_t)i * C3_EMIT_KINDS + k] = at;
  }
}

// a body segment: the whole of it (parts == 1) or this wave's share in whole 256-byte rows
__device__ __forceinline__ void em_body(uint8_t* dst, const uint8_t* src, uint32_t len, int lane, int part, int parts) {
  uint32_t b = 0, e = len;
  if (parts > 1) tx_piece(len, part, parts, &b, &e);
  tx_wave_copy(dst + b, src + b, e - b, lane);
}

// the records of read i by one wave; part / parts: this wave's share of the body segments of a long read (part 0 also
// writes the headers and literals), 0 / 1 for a read the wave has to itself
__device__ __forceinline__ void em_write_read(const EmitArgs& a, int i, int lane, int part, int parts) {
  const EmitHead h = a.head[i];
  if (wave_first(h.s) < 0) return;
  const c3_read_result& r = a.info[i];
  const int64_t so = a.off[i], no = a.name_off[i], L = a.off[i + 1] - so;
  const uint32_t nl = (uint32_t)(a.name_off[i + 1] - no);
  const int64_t clen = em_clen(a, i);
  const C3EmitDec d = c3_emit_of(r, h.s, a.n_splints, a.zero, clen);
  const uint8_t* name = a.names + no;
  const int64_t* roff = a.roff + (size_t)i * C3_EMIT_KINDS;
  uint8_t* out = a.arena + roff[C3_EMIT_SUB_FQ];
  const int np = wave_first(h.np);
  for (int j = 0; j < np; ++j) {
    int32_t idx; int64_t b, e;
    c3_emit_piece(r, d, L, j, &idx, &b, &e);
    const uint32_t len = (uint32_t)wave_first((int)(e - b));
    const int dn = c3_emit_dec_len(idx);
    if (part == 0) {
      if (lane == 0) out[0] = '@';
      tx_wave_copy(out + 1, name, nl, lane);
      uint8_t* t = out + 1 + nl;                                       // _<idx>\n
      if (lane == 0) t[0] = '_';
      else if (lane <= dn) t[lane] = (uint8_t)c3_emit_dec_char(idx, lane - 1);
      else if (lane == dn + 1) t[lane] = '\n';
      uint8_t* m = t + dn + 2 + len;                                   // \n+\n between the bases and the qualities, \n at the end
      if (lane < 3) m[lane] = lane == 1 ? '+' : '\n';
      if (lane == 3) m[3 + len] = '\n';
    }
    uint8_t* body = out + 1 + nl + dn + 2;
    em_body(body, a.seqs + so + b, len, lane, part, parts);
    em_body(body + len + 3, a.quals + so + b, len, lane, part, parts);
    out += c3_emit_sub_len(nl, idx, len);
  }
  if (!wave_first(h.cons)) return;
  const int ht = c3_emit_head_tail_len(h.aql, L, d.ns, clen);
  const uint32_t cl = (uint32_t)clen;
  for (int kind = 0; kind < a.K; kind += 2) {                          // C3_EMIT_CONS_FA, and C3_EMIT_CONS_FQ with the QVs
    out = a.arena + roff[kind];
    if (part == 0) {
      if (lane == 0) out[0] = kind == C3_EMIT_CONS_FA ? '>' : '@';
      tx_wave_copy(out + 1, name, nl, lane);
      if (lane < ht) out[1 + nl + lane] = (uint8_t)c3_emit_head_tail_char(lane, a.head[i].aq, h.aql, L, d.ns, clen);
    }
    uint8_t* body = out + 1 + nl + ht;
    em_body(body, a.cons + a.cons_at[i], cl, lane, part, parts);
    if (kind == C3_EMIT_CONS_FQ) {
      if (part == 0 && lane < 3) body[cl + lane] = lane == 1 ? '+' : '\n';
      em_body(body + cl + 3, a.qv + a.cons_at[i], cl, lane, part, parts);
      if (part == 0 && lane == 0) body[2 * (size_t)cl + 3] = '\n';
    } else if (part == 0 && lane == 0) body[cl] = '\n';
  }
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_emit_write(EmitArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = wave_first((int)(threadIdx.x >> 6));
  const int i0 = blockIdx.x * TX_WAVES;
  {
    const int i = i0 + wv;
    if (i < a.n && a.off[i + 1] - a.off[i] <= TX_LONG) em_write_read(a, i, lane, 0, 1);
  }
  for (int k = 0; k < TX_WAVES; ++k) {                   // long reads of the workgroup: a quarter of every body segment each
    const int i = i0 + k;
    if (i >= a.n) break;
    if (a.off[i + 1] - a.off[i] <= TX_LONG) continue;
    em_write_read(a, i, lane, wv, TX_WAVES);
  }
}

extern "C" void c3k_launch_emit_len(const EmitArgs* a, hipStream_t s) {
  if (a->n > 0) hipLaunchKernelGGL(k_emit_len, dim3((a->n + TX_WAVES - 1) / TX_WAVES), dim3(64 * TX_WAVES), 0, s, *a);
}
// bsum holds (S * K + 1) * ((n + 255) / 256) sums; stream_off S * K + 2 entries (the last = records)
extern "C" void c3k_launch_emit_scan(const EmitArgs* a, hipStream_t s) {
  const int nb = (a->n + 255) / 256;
  if (nb) hipLaunchKernelGGL(k_emit_rsum, dim3(nb), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_emit_rscan, dim3(1), dim3(256), 0, s, *a, nb);
  if (nb) hipLaunchKernelGGL(k_emit_rfin, dim3(nb), dim3(256), 0, s, *a);
}
extern "C" void c3k_launch_emit_write(const EmitArgs* a, hipStream_t s) {
  if (a->n > 0) hipLaunchKernelGGL(k_emit_write, dim3((a->n + TX_WAVES - 1) / TX_WAVES), dim3(64 * TX_WAVES), 0, s, *a);
}

// k_fastx.hip -- strict records of either kind (two-line FASTA, four-line FASTQ) parsed on the GPU for the text path of the
// post-processing step (include/c3poa.h "Post-processing, text in / file bytes out").  The rule of one record is
// c3_fastx.h, which the host statement c3_fastx_strict_parse_host (c3_fastx.cpp) applies as well.  The text occupies bytes
// [0, hi) of a 256-aligned device buffer with at least 256 bytes of slack behind hi; the positions of its '\n' come from
// k_fastq_count / k_fastq_lines, which do not care what the lines mean.  Same tile, scan and gather structure as k_fastq.hip:
//
//   k_fastx_high      the first byte >= 0x80: one aligned 16-byte load per lane (grid-stride), a wave minimum, one atomicMin per
//       wave that saw one -- a minimum, not a place, so there is no scan to take it from.
//   k_fastx_records   one lane per candidate record r (lines kind * r .. kind * r + kind - 1): '\r' stripped, the strictness
//       test, the high byte, sequence and name length; a departure does atomicMin on the first bad record.
//   k_fastx_rsum / k_fastx_rscan / k_fastx_rfin   exclusive scans of (sequence bytes, name bytes, 2-bit words) and the longest
//       sequence over the records in front of the first bad one: per-workgroup sums, one small workgroup over those, then
//       every workgroup again with its base, writing off[], name_off[], woff[] and the source positions.  woff and the longest
//       sequence are what the 2-bit pack and k_adapter need, so no offset has to visit the host first.
//   k_fastx_gather    the pass that moves every byte once, as k_fastq_gather does (one wave per record, four on a record above
//       TX_LONG bytes), qualities only when asked for; lane 0 of the record's wave writes the name hash.
// No atomics where a scan gives the place, no scratch, no load outside the dwords that hold text bytes or their 16 bytes of slack.
#include "c3_dev.h"
#include "c3_fastx.h"
#include "c3_launch.h"
#include "k_text.h"

__global__ __launch_bounds__(256) void k_fastx_high(const uint8_t* buf, uint32_t hi, C3FxHdr* hdr) {
  const uint32_t n16 = (hi + 15u) >> 4;
  uint32_t first = UINT32_MAX;
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) {
    const uint4 v = *(const uint4*)(buf + 16u * i);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 3; k >= 0; --k) {
      const uint32_t m = w[k] & 0x80808080u;
      if (m) { const uint32_t pos = 16u * i + 4u * k + (((uint32_t)__ffs((int)m) - 1u) >> 3); if (pos < hi) first = min(first, pos); }
    }
  }
  for (int d = 32; d > 0; d >>= 1) first = min(first, (uint32_t)__shfl_xor((int)first, d, 64));
  if ((threadIdx.x & 63) == 0 && first != UINT32_MAX) atomicMin(&hdr->first_high, first);
}

__global__ __launch_bounds__(256) void k_fastx_records(FxArgs a) {
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  if (r > a.n_full) return;
  if (r == a.n_full) { if (a.partial) atomicMin(&a.hdr->first_bad, (uint32_t)r); return; }      // an incomplete record at the end of the file
  const char* t = (const char*)a.buf;
  int32_t b[4] = {0, 0, 0, 0}, e[4] = {0, 0, 0, 0}, raw_end = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k < a.kind) {
      const int32_t ln = a.kind * r + k;
      b[k] = ln == 0 ? 0 : a.nl[ln - 1] + 1;
      raw_end = ln < a.L ? a.nl[ln] : (int32_t)a.hi;
      e[k] = c3_fastq_line_end(t, b[k], raw_end);
    }
  const uint32_t fh = a.hdr->first_high;
  if (c3_fastx_strict(t, a.kind, b, e) && !(fh >= (uint32_t)b[0] && fh < (uint32_t)raw_end)) {
    a.slen[r] = e[1] - b[1];
    a.nlen[r] = c3_fastq_name_len(t, b[0], e[0]);
  } else {
    a.slen[r] = 0; a.nlen[r] = 0;
    atomicMin(&a.hdr->first_bad, (uint32_t)r);
  }
}

__device__ __forceinline__ int fx_n_rec(const FxArgs& a) { return (int)min(a.hdr->first_bad, (uint32_t)a.n_full); }
// (sequence bytes, name bytes, 2-bit words) of record r, zero at and behind the first bad record
__device__ __forceinline__ void fx_terms(const FxArgs& a, int r, int n_rec, long long* s, long long* n, long long* w) {
  *s = 0; *n = 0; *w = 0;
  if (r < n_rec) { *s = a.slen[r]; *n = a.nlen[r]; *w = (*s + 15) / 16 + 2; }                   // + 2 words: aligned-window overread (c3_batch_stage)
}

__global__ __launch_bounds__(256) void k_fastx_rsum(FxArgs a) {
  __shared__ long long lds[TX_WAVES];
  long long s, n, w, ts, tn, tw, tm;
  fx_terms(a, blockIdx.x * 256 + (int)threadIdx.x, fx_n_rec(a), &s, &n, &w);
  long long mx = s;
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, (long long)__shfl_xor(mx, d, 64));
  (void)tx_block_excl(s, lds, &ts); (void)tx_block_excl(n, lds, &tn); (void)tx_block_excl(w, lds, &tw);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
  __syncthreads();
  tm = max(max(lds[0], lds[1]), max(lds[2], lds[3]));
  if (threadIdx.x == 0) { long long* o = a.bsum + 4 * blockIdx.x; o[0] = ts; o[1] = tn; o[2] = tw; o[3] = tm; }
}

// bsum[0..4 * nb) -> exclusive prefix sums per column (column 3: the maximum), in place; the header and the closing entries
__global__ __launch_bounds__(256) void k_fastx_rscan(FxArgs a, int nb) {
  __shared__ long long lds[TX_WAVES];
  long long run[3] = {0, 0, 0}, mx = 0;
  for (int i0 = 0; i0 < nb; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const long long v = i < nb ? a.bsum[4 * i + c] : 0;
      long long tot;
      const long long ex = tx_block_excl(v, lds, &tot);
      if (i < nb) a.bsum[4 * i + c] = run[c] + ex;
      run[c] += tot;
    }
    if (i < nb) mx = max(mx, a.bsum[4 * i + 3]);
  }
  for (int d = 32; d > 0; d >>= 1) mx = max(mx, (long long)__shfl_xor(mx, d, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    C3FxHdr* h = a.hdr;
    const int n_rec = fx_n_rec(a);
    h->departed = h->first_bad != UINT32_MAX ? 1 : 0;
    h->n_records = n_rec; h->base_bytes = run[0]; h->name_bytes = run[1]; h->words = run[2];
    h->max_len = (int32_t)max(max(lds[0], lds[1]), max(lds[2], lds[3]));
    const int last = a.kind * n_rec - 1;                 // the record's last line: the next record starts behind its '\n'
    h->consumed = n_rec == 0 ? 0 : (last < a.L ? (int64_t)a.nl[last] + 1 : (int64_t)a.hi);
    a.off[n_rec] = run[0]; a.name_off[n_rec] = run[1]; a.woff[n_rec] = run[2];
  }
}

__global__ __launch_bounds__(256) void k_fastx_rfin(FxArgs a) {
  __shared__ long long lds[TX_WAVES];
  const int n_rec = fx_n_rec(a);
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  long long s, n, w, t;
  fx_terms(a, r, n_rec, &s, &n, &w);
  const long long es = tx_block_excl(s, lds, &t), en = tx_block_excl(n, lds, &t), ew = tx_block_excl(w, lds, &t);
  if (r >= n_rec) return;
  const long long* base = a.bsum + 4 * blockIdx.x;
  a.off[r] = base[0] + es; a.name_off[r] = base[1] + en; a.woff[r] = base[2] + ew;
  const int32_t l0 = a.kind * r;
  const int32_t b0 = l0 == 0 ? 0 : a.nl[l0 - 1] + 1;
  a.src[r] = make_int4(a.nl[l0] + 1, a.kind == 4 ? a.nl[l0 + 2] + 1 : 0, b0 + 1, 0);           // sequence, quality, name
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fastx_gather(FxArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long i0 = (long long)blockIdx.x * TX_WAVES;
  {
    const long long i = i0 + wv;
    if (i < a.n_records) {
      const int4 p = a.src[i];
      const int64_t no = a.name_off[i], so = a.off[i];
      const uint32_t nlen = (uint32_t)(a.name_off[i + 1] - no), sl = (uint32_t)(a.off[i + 1] - so);
      tx_wave_copy(a.names + no, a.buf + p.z, nlen, lane);
      if (lane == 0) a.hash[i] = c3_fasta_hash(a.buf + p.z, (int64_t)nlen);
      if (sl <= TX_LONG) {
        tx_wave_copy(a.seqs + so, a.buf + p.x, sl, lane);
        if (a.quals) tx_wave_copy(a.quals + so, a.buf + p.y, sl, lane);
      }
    }
  }
  for (int k = 0; k < TX_WAVES; ++k) {                  // long records of the workgroup: a quarter (in whole 256-byte rows) each
    const long long i = i0 + k;
    if (i >= a.n_records) break;
    const int64_t so = a.off[i];
    const uint32_t sl = (uint32_t)(a.off[i + 1] - so);
    if (sl <= TX_LONG) continue;
    const int4 p = a.src[i];
    uint32_t b, e;
    tx_piece(sl, wv, TX_WAVES, &b, &e);
    tx_wave_copy(a.seqs + so + b, a.buf + p.x + b, e - b, lane);
    if (a.quals) tx_wave_copy(a.quals + so + b, a.buf + p.y + b, e - b, lane);
  }
}

// hdr->first_high must hold UINT32_MAX before the launch
extern "C" void c3k_launch_fastx_high(const FxArgs* a, hipStream_t s) {
  const uint32_t n16 = (a->hi + 15u) >> 4;
  const unsigned grid = (unsigned)std::min<uint32_t>((n16 + 255u) / 256u, 2048u);
  if (grid) hipLaunchKernelGGL(k_fastx_high, dim3(grid), dim3(256), 0, s, a->buf, a->hi, a->hdr);
}
// n_full whole candidate records (partial: one more, incomplete, at the end of the file); hdr->first_bad must hold UINT32_MAX;
// bsum holds 4 * ((n_full + 255) / 256 + 1) entries
extern "C" void c3k_launch_fastx_records(const FxArgs* a, hipStream_t s) {
  const int nb1 = (a->n_full + 1 + 255) / 256, nb = (a->n_full + 255) / 256;
  hipLaunchKernelGGL(k_fastx_records, dim3(nb1), dim3(256), 0, s, *a);
  if (nb) hipLaunchKernelGGL(k_fastx_rsum, dim3(nb), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_fastx_rscan, dim3(1), dim3(256), 0, s, *a, nb);
  if (nb) hipLaunchKernelGGL(k_fastx_rfin, dim3(nb), dim3(256), 0, s, *a);
}
extern "C" void c3k_launch_fastx_gather(const FxArgs* a, hipStream_t s) {
  if (a->n_records <= 0) return;
  hipLaunchKernelGGL(k_fastx_gather, dim3((unsigned)((a->n_records + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, *a);
}

// k_fasta.hip -- FASTA text parsed, demultiplexed and formatted on the GPU (include/c3poa.h "Sample demultiplexer, text in /
// file bytes out").  The rule is c3_fasta.h, which the host statements (c3_fasta.cpp) apply as well; this file
// finds the lines, scans the lengths and moves the bytes.  The text occupies bytes [0, hi) of a 256-aligned device buffer with
// 256 bytes of slack behind hi; positions are 32-bit offsets into it (C3_FASTA_MAX_TEXT).
//
//   k_fasta_count / k_fasta_scan / k_fasta_lines   the positions of all '\n' and '\r' in order: nl[k], so line k is
//       (nl[k-1], nl[k]) and line T, the last, ends at hi.  Tile geometry of k_fastq_count / _scan / _lines: 64 KiB per
//       workgroup, 16 KiB per wave in 16 steps of one 16-byte load per lane, order inside a wave by a DPP scan, the 4 counts per
//       tile scanned by one small workgroup (no look-back: DESIGN.md 5.5).  The same pass finds the first byte >= 0x80 with one
//       atomicMin, which only a departure touches.
//   k_fasta_lsum / k_fasta_lscan / k_fasta_lfin   one lane per line: stripped end (a backward loop bounded by the line), kind,
//       then exclusive scans of (headers, name bytes, sequence bytes) in the k_fastq_rsum / rscan / rfin shape.  The scanned
//       sequence bytes of a sequence line are its place in the sequence arena; the values at a header line are the record's
//       number, name_off[] and off[].  The header lane also hashes the name.  k_fasta_settle (one lane) then states which records
//       the text delivers (c3_fasta_verdict), consumed and the byte totals.
//   k_tx_xsum / k_tx_xscan / k_tx_xfin <FaKept>, <FaLen>   the one-column exclusive scan of k_text.h, used twice by
//       c3_demux_emit: over the records (kept = more than 300 sequence bytes -> krec[]) and over the kept records (output
//       length -> roff[]).
//   k_fasta_gather   moves every name and sequence byte once: one wave per record, the four waves of a workgroup together on a
//       record above TX_LONG bytes (a line above TX_LONG in quarters, shorter lines dealt round).  Dword path of tx_wave_copy.
//       A wave writes only inside its record's range of names / seqs.
//   k_demux_heads   the first 300 bytes of every kept record into k_demux's slots, one wave per record.
//   k_demux_emit    one wave per kept record as k_post_emit: literals and index names by the first lanes, name and sequence
//       dword-wise; a wave writes only inside [roff[i], roff[i] + length).
#include "c3_dev.h"
#include "c3_fasta.h"
#include "c3_launch.h"
#include "k_text.h"

#define FA_TILE 65536u
#define FA_SUB (FA_TILE / TX_WAVES)
#define FA_STEP 1024u                 // 64 lanes x 16 bytes

// 0x80 in every byte of w that equals the byte repeated in c4 (exact: no borrow runs into the neighbouring byte)
__device__ __forceinline__ uint32_t fa_eqmask(uint32_t w, uint32_t c4) {
  const uint32_t x = w ^ c4;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
// the 0x80 bits of the four bytes of m as bits 0..3
__device__ __forceinline__ uint32_t fa_nibble(uint32_t m) { return ((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u); }

// bit j set: byte p + j of the text [0, hi) is '\n' or '\r'; *high likewise for bytes >= 0x80; p is 16-aligned
__device__ __forceinline__ uint32_t fa_lane_mask(const uint8_t* buf, uint32_t p, uint32_t hi, uint32_t* high) {
  *high = 0;
  if (p >= hi) return 0;
  const uint4 v = *(const uint4*)(buf + p);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t out = 0, hb = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t m = fa_eqmask(w[k], 0x0A0A0A0Au) | fa_eqmask(w[k], 0x0D0D0D0Du);
    uint32_t g = w[k] & 0x80808080u;
    const uint32_t q = p + 4u * k;
    if (q + 4u > hi) {                                   // the end of the text: byte by byte
      uint32_t keep = 0;
      for (uint32_t j = 0; j < 4; ++j) if (q + j < hi) keep |= 0x80u << (8 * j);
      m &= keep; g &= keep;
    }
    out |= fa_nibble(m) << (4 * k);
    hb |= fa_nibble(g) << (4 * k);
  }
  *high = hb;
  return out;
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fasta_count(const uint8_t* buf, uint32_t hi, int32_t* cnt, C3FaHdr* hdr) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * FA_TILE + (uint32_t)wv * FA_SUB;
  int c = 0;
  uint32_t first = UINT32_MAX;
  if (base < hi)
    for (uint32_t s = 0; s < FA_SUB; s += FA_STEP) {
      const uint32_t p = base + s + 16u * lane;
      uint32_t high;
      c += __popc(fa_lane_mask(buf, p, hi, &high));
      if (high && first == UINT32_MAX) first = p + (uint32_t)__ffs((int)high) - 1u;
    }
  c = wave_scan_add(c);
  if (lane == 63) cnt[blockIdx.x * TX_WAVES + wv] = c;
  if (first != UINT32_MAX) atomicMin(&hdr->first_high, first);
}

// cnt[0..m) -> exclusive prefix sums, in place; the header gets the terminator count
__global__ __launch_bounds__(256) void k_fasta_scan(int32_t* cnt, int m, C3FaHdr* hdr) {
  __shared__ int lds[TX_WAVES];
  int run = 0;
  for (int i0 = 0; i0 < m; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    const int v = i < m ? cnt[i] : 0;
    int tot;
    const int ex = tx_block_excl(v, lds, &tot);
    if (i < m) cnt[i] = run + ex;
    run += tot;
  }
  if (threadIdx.x == 0) hdr->n_term = run;
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fasta_lines(const uint8_t* buf, uint32_t hi, const int32_t* cnt, int32_t* nl) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * FA_TILE + (uint32_t)wv * FA_SUB;
  if (base >= hi) return;
  int at = cnt[blockIdx.x * TX_WAVES + wv];
  for (uint32_t s = 0; s < FA_SUB; s += FA_STEP) {
    const uint32_t p = base + s + 16u * lane;
    uint32_t high;
    uint32_t m = fa_lane_mask(buf, p, hi, &high);
    const int c = __popc(m);
    const int inc = wave_scan_add(c);
    int k = at + inc - c;
    while (m) { nl[k++] = (int32_t)(p + (uint32_t)__ffs((int)m) - 1u); m &= m - 1u; }
    at += wave_bcast(inc, 63);
  }
}

// line k of the text, k in 0 .. T: [begin, end) without its terminator
__device__ __forceinline__ int32_t fa_begin(const FaArgs& a, int32_t k) { return k == 0 ? 0 : a.nl[k - 1] + 1; }
__device__ __forceinline__ int32_t fa_end(const FaArgs& a, int32_t k) { return k < a.T ? a.nl[k] : (int32_t)a.hi; }

// kind of line k and its (header, name bytes, sequence bytes) from its stripped end; zero behind the last line
struct FaLine { int kind; long long h, nb, sb; };
__device__ __forceinline__ FaLine fa_line_terms(const FaArgs& a, int32_t k, int32_t b, int32_t se) {
  FaLine t = {C3_FA_BLANK, 0, 0, 0};
  if (k > a.T) return t;
  t.kind = c3_fasta_kind(a.buf, b, se);
  if (t.kind == C3_FA_HEADER) { t.h = 1; t.nb = se - b - 1; }
  else if (t.kind == C3_FA_SEQ) t.sb = se - b;
  return t;
}

__global__ __launch_bounds__(256) void k_fasta_lsum(FaArgs a) {
  __shared__ long long lds[TX_WAVES];
  const int32_t k = blockIdx.x * 256 + (int)threadIdx.x;
  int32_t b = 0, se = 0;
  if (k <= a.T) { b = fa_begin(a, k); se = c3_fasta_strip_end(a.buf, b, fa_end(a, k)); a.lse[k] = se; }
  const FaLine t = fa_line_terms(a, k, b, se);
  long long th, tn, ts;
  (void)tx_block_excl(t.h, lds, &th); (void)tx_block_excl(t.nb, lds, &tn); (void)tx_block_excl(t.sb, lds, &ts);
  if (threadIdx.x == 0) { a.bsum[3 * blockIdx.x] = th; a.bsum[3 * blockIdx.x + 1] = tn; a.bsum[3 * blockIdx.x + 2] = ts; }
}

// bsum[0 .. 3 * nb) -> exclusive prefix sums per stream, in place; the header count and the closing entries of the record arrays
__global__ __launch_bounds__(256) void k_fasta_lscan(FaArgs a, int nb) {
  __shared__ long long lds[TX_WAVES];
  long long run[3] = {0, 0, 0};
  for (int i0 = 0; i0 < nb; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    for (int c = 0; c < 3; ++c) {
      const long long v = i < nb ? a.bsum[3 * i + c] : 0;
      long long tot;
      const long long ex = tx_block_excl(v, lds, &tot);
      if (i < nb) a.bsum[3 * i + c] = run[c] + ex;
      run[c] += tot;
    }
  }
  if (threadIdx.x == 0) {
    a.hdr->n_headers = run[0];
    a.name_off[run[0]] = run[1]; a.off[run[0]] = run[2]; a.rec_line[run[0]] = a.T + 1;
  }
}

__global__ __launch_bounds__(256) void k_fasta_lfin(FaArgs a) {
  __shared__ long long lds[TX_WAVES];
  const int32_t k = blockIdx.x * 256 + (int)threadIdx.x;
  int32_t b = 0, se = 0;
  if (k <= a.T) { b = fa_begin(a, k); se = a.lse[k]; }
  const FaLine ln = fa_line_terms(a, k, b, se);
  long long t;
  const long long eh = a.bsum[3 * blockIdx.x] + tx_block_excl(ln.h, lds, &t);
  const long long en = a.bsum[3 * blockIdx.x + 1] + tx_block_excl(ln.nb, lds, &t);
  const long long es = a.bsum[3 * blockIdx.x + 2] + tx_block_excl(ln.sb, lds, &t);
  if (k > a.T) return;
  if (ln.kind == C3_FA_HEADER) {
    a.rec_line[eh] = k; a.name_off[eh] = en; a.off[eh] = es;
    a.hash[eh] = c3_fasta_hash(a.buf + b + 1, se - b - 1);
  } else if (ln.kind == C3_FA_SEQ) {
    a.ldst[k] = (uint32_t)es;
    if (eh == 0) atomicMin(&a.hdr->first_headless, (uint32_t)b);
  }
  const uint32_t fh = a.hdr->first_high;                // settled by k_fasta_count
  if (fh != UINT32_MAX && (uint32_t)b <= fh && fh <= (uint32_t)fa_end(a, k)) a.hdr->rec_of_high = (int32_t)(eh + ln.h) - 1;
}

__global__ void k_fasta_settle(FaArgs a) {
  C3FaHdr* hd = a.hdr;
  const int64_t H = hd->n_headers;
  const C3FaVerdict v = c3_fasta_verdict(H, a.at_eof, hd->first_high == UINT32_MAX ? -1 : (int64_t)hd->first_high,
                                         hd->first_headless == UINT32_MAX ? -1 : (int64_t)hd->first_headless, hd->rec_of_high);
  const int64_t hb_next = v.n_records < H ? fa_begin(a, a.rec_line[v.n_records]) : 0;
  hd->n_records = v.n_records; hd->departed = v.departed;
  hd->consumed = c3_fasta_consumed(v, H, a.at_eof, a.hi, hb_next);
  hd->name_bytes = v.n_records ? a.name_off[v.n_records] : 0;
  hd->base_bytes = v.n_records ? a.off[v.n_records] : 0;
  hd->n_kept = 0; hd->out_bytes = 0;
}

// ---- the functors of the one-column scan (tx_xscan of k_text.h)
struct FaKept {                                          // over the delivered records: which are kept, krec[] in order
  FaArgs a;
  __device__ long long n() const { return a.hdr->n_records; }
  __device__ long long term(long long r) const { return a.off[r + 1] - a.off[r] > C3_DEMUX_HEAD ? 1 : 0; }
  __device__ void put(long long r, long long ex) const { a.krec[ex] = (int32_t)r; }
  __device__ void total(long long t) const { a.hdr->n_kept = t; }
};
struct FaLen {                                           // over the kept records: the output length, roff[]
  FaArgs a;
  __device__ long long n() const { return a.n_kept; }
  __device__ long long term(long long i) const {
    const int32_t r = a.krec[i], wa = a.win[2 * i], wb = a.win[2 * i + 1];
    return c3_demux_rec_len(a.name_off[r + 1] - a.name_off[r], a.off[r + 1] - a.off[r], wa < 0 ? 0 : a.a_no[wa + 1] - a.a_no[wa],
                            wb < 0 ? 0 : a.b_no[wb + 1] - a.b_no[wb]);
  }
  __device__ void put(long long i, long long ex) const { a.roff[i] = ex; }
  __device__ void total(long long t) const { a.hdr->out_bytes = t; }
};

// the sequence lines of record r; part / parts: this wave's share (0 / 1: the wave has the record to itself)
__device__ __forceinline__ void fa_gather_seq(const FaArgs& a, long long r, int lane, int part, int parts) {
  const int32_t k0 = wave_first(a.rec_line[r]) + 1, k1 = wave_first(a.rec_line[r + 1]);
  int turn = 0;
  for (int32_t k = k0; k < k1; ++k) {
    const int32_t b = wave_first(a.nl[k - 1]) + 1, se = wave_first(a.lse[k]);
    if (se <= b) continue;
    const uint32_t len = (uint32_t)(se - b);
    uint8_t* dst = a.seqs + wave_first((int)a.ldst[k]);
    if (parts > 1 && len > TX_LONG) {
      uint32_t pb, pe;
      tx_piece(len, part, parts, &pb, &pe);
      tx_wave_copy(dst + pb, a.buf + b + pb, pe - pb, lane);
    } else if (parts == 1 || (turn++ % parts) == part) {
      tx_wave_copy(dst, a.buf + b, len, lane);
    }
  }
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fasta_gather(FaArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = wave_first((int)(threadIdx.x >> 6));
  const long long i0 = (long long)blockIdx.x * TX_WAVES;
  {
    const long long r = i0 + wv;
    if (r < a.n_records) {
      const int64_t no = a.name_off[r];
      tx_wave_copy(a.names + no, a.buf + fa_begin(a, a.rec_line[r]) + 1, (uint32_t)(a.name_off[r + 1] - no), lane);
      if (a.off[r + 1] - a.off[r] <= TX_LONG) fa_gather_seq(a, r, lane, 0, 1);
    }
  }
  for (int k = 0; k < TX_WAVES; ++k) {                  // long records of the workgroup
    const long long r = i0 + k;
    if (r >= a.n_records) break;
    if (a.off[r + 1] - a.off[r] > TX_LONG) fa_gather_seq(a, r, lane, wv, TX_WAVES);
  }
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_demux_heads(FaArgs a) {
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * TX_WAVES + (threadIdx.x >> 6);
  if (i >= a.n_kept) return;
  tx_wave_copy(a.heads + (size_t)i * C3_DEMUX_HEAD, a.seqs + a.off[a.krec[i]], C3_DEMUX_HEAD, lane);     // kept: more than 300 bytes
}

// output record of kept record i; part / parts as in fa_gather_seq (part 0 also writes everything but the sequence)
__device__ __forceinline__ void fa_emit_record(const FaArgs& a, long long i, int lane, int part, int parts) {
  const int32_t r = wave_first(a.krec[i]), wa = wave_first(a.win[2 * i]), wb = wave_first(a.win[2 * i + 1]);
  const int64_t no = a.name_off[r], so = a.off[r];
  const uint32_t nlen = (uint32_t)(a.name_off[r + 1] - no), sl = (uint32_t)(a.off[r + 1] - so);
  const uint32_t al = wa < 0 ? 0u : (uint32_t)(a.a_no[wa + 1] - a.a_no[wa]), bl = wb < 0 ? 0u : (uint32_t)(a.b_no[wb + 1] - a.b_no[wb]);
  uint8_t* o = a.out + a.roff[i];
  uint8_t* body = o + 4u + nlen + al + bl;
  if (part == 0) {
    tx_wave_copy(o + 1, a.names + no, nlen, lane);
    for (uint32_t j = (uint32_t)lane; j < al; j += 64u) o[2u + nlen + j] = a.a_names[a.a_no[wa] + j];
    for (uint32_t j = (uint32_t)lane; j < bl; j += 64u) o[3u + nlen + al + j] = a.b_names[a.b_no[wb] + j];
    if (lane == 0) { o[0] = '>'; o[1u + nlen] = '|'; o[2u + nlen + al] = '_'; o[3u + nlen + al + bl] = '\n'; body[sl] = '\n'; }
  }
  uint32_t pb = 0, pe = sl;
  if (parts > 1) tx_piece(sl, part, parts, &pb, &pe);
  tx_wave_copy(body + pb, a.seqs + so + pb, pe - pb, lane);
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_demux_emit(FaArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = wave_first((int)(threadIdx.x >> 6));
  const long long i0 = (long long)blockIdx.x * TX_WAVES;
  {
    const long long i = i0 + wv;
    if (i < a.n_kept) { const int32_t r = a.krec[i]; if (a.off[r + 1] - a.off[r] <= TX_LONG) fa_emit_record(a, i, lane, 0, 1); }
  }
  for (int k = 0; k < TX_WAVES; ++k) {                  // long records of the workgroup: a quarter of the sequence each
    const long long i = i0 + k;
    if (i >= a.n_kept) break;
    const int32_t r = a.krec[i];
    if (a.off[r + 1] - a.off[r] > TX_LONG) fa_emit_record(a, i, lane, wv, TX_WAVES);
  }
}

static inline int fa_tiles(uint32_t hi) { return (int)(((uint64_t)hi + FA_TILE - 1) / FA_TILE); }

// hdr's first three words are preset to all ones by the caller; hi > 0
extern "C" void c3k_launch_fasta_count(const FaArgs* a, hipStream_t s) {
  const int tiles = fa_tiles(a->hi);
  hipLaunchKernelGGL(k_fasta_count, dim3(tiles), dim3(64 * TX_WAVES), 0, s, a->buf, a->hi, a->cnt, a->hdr);
  hipLaunchKernelGGL(k_fasta_scan, dim3(1), dim3(256), 0, s, a->cnt, tiles * TX_WAVES, a->hdr);
}
// a->T terminators: lines 0 .. T; bsum holds 3 * ((T + 1 + 255) / 256) sums; with `kept`, krec[] and hdr->n_kept as well
extern "C" void c3k_launch_fasta_records(const FaArgs* a, int kept, hipStream_t s) {
  const int nb = (a->T + 1 + 255) / 256;
  hipLaunchKernelGGL(k_fasta_lines, dim3(fa_tiles(a->hi)), dim3(64 * TX_WAVES), 0, s, a->buf, a->hi, (const int32_t*)a->cnt, a->nl);
  hipLaunchKernelGGL(k_fasta_lsum, dim3(nb), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_fasta_lscan, dim3(1), dim3(256), 0, s, *a, nb);
  hipLaunchKernelGGL(k_fasta_lfin, dim3(nb), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_fasta_settle, dim3(1), dim3(1), 0, s, *a);
  if (kept) tx_xscan(FaKept{*a}, (long long)a->T + 1, a->bsum, s);      // at most one record per line
}
extern "C" void c3k_launch_fasta_gather(const FaArgs* a, hipStream_t s) {
  if (a->n_records <= 0) return;
  hipLaunchKernelGGL(k_fasta_gather, dim3((unsigned)((a->n_records + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, *a);
}
extern "C" void c3k_launch_demux_heads(const FaArgs* a, hipStream_t s) {
  if (a->n_kept <= 0) return;
  hipLaunchKernelGGL(k_demux_heads, dim3((unsigned)((a->n_kept + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, *a);
}
// bsum holds (n_kept + 255) / 256 sums
extern "C" void c3k_launch_demux_len(const FaArgs* a, hipStream_t s) { tx_xscan(FaLen{*a}, a->n_kept, a->bsum, s); }
extern "C" void c3k_launch_demux_emit(const FaArgs* a, hipStream_t s) {
  if (a->n_kept <= 0) return;
  hipLaunchKernelGGL(k_demux_emit, dim3((unsigned)((a->n_kept + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, *a);
}

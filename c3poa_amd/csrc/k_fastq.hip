// k_fastq.hip -- strict four-line FASTQ text parsed on the GPU (include/c3poa.h "FASTQ records on the GPU").
// The rule of one record is c3_fastq.h, which the host statement c3_fastq_parse_host (c3_fastq.cpp) applies as well; this
// file finds the lines, scans the lengths and moves the bytes.  The text occupies bytes [lo, hi) of a 256-aligned device
// buffer with at least 256 bytes of slack behind hi (lo <= 3: the stand-alone call keeps the caller's misalignment);
// positions are 32-bit offsets into that buffer (C3_FASTQ_MAX_TEXT).
//
//   k_fastq_count / k_fastq_scan / k_fastq_lines   the positions of all '\n' in order: nl[k], so line k is (nl[k-1], nl[k]).
//       One workgroup of 256 lanes per 64 KiB tile; each of its 4 waves owns 16 KiB of the tile and walks it in 16 steps of
//       1 KiB, a lane taking one aligned 16-byte load per step (coalesced: a wave reads 1 KiB in one instruction).  '\n' are
//       found by a byte compare on the four dwords (exact zero-byte mask) and counted with popcount.  Because a wave owns a
//       contiguous piece, order inside a wave is a 64-lane DPP scan and no LDS or barrier is needed; the counts of all waves
//       of all tiles (4 per tile, at most 16 384 + 4 for a full stretch) are scanned by ONE small workgroup (k_fastq_scan,
//       scan through LDS) rather than by a decoupled look-back: the list is tiny, the host needs the total anyway to size
//       nl[], and a look-back would add a spin between workgroups for no time that shows.
//   k_fastq_records   one lane per candidate record r (lines 4r .. 4r+3): '\r' stripped, the strictness test, sequence and
//       name length; a departure does atomicMin on the first bad record.
//   k_fastq_rsum / k_fastq_rscan / k_fastq_rfin   exclusive scans of (kept, sequence bytes, name bytes) over the records in
//       front of the first bad one: per-workgroup sums, one small workgroup over those, then every workgroup again with its
//       base, writing off[], name_off[] and the source positions of the kept records.
//   k_fastq_gather   the pass that moves every byte once: one wave per kept record, the four waves of a workgroup together
//       on a record above TX_LONG bytes.  Source and destination sit at any byte (tx_wave_copy of k_text.h): the destination
//       is brought to a dword with byte stores, the interior is whole dwords from two aligned source dwords joined by
//       v_alignbyte (as k_bgzf and k_inflate read their input), the end is byte stores.  Nothing outside a record's own
//       destination range is written (other waves write its neighbours), nothing outside the dwords that hold text bytes is read.
#include "c3_dev.h"
#include "c3_fastq.h"
#include "c3_launch.h"
#include "k_text.h"

#define FQ_TILE 65536u
#define FQ_SUB (FQ_TILE / TX_WAVES)
#define FQ_STEP 1024u                 // 64 lanes x 16 bytes

// 0x80 in every byte of w that is '\n' (exact: no borrow runs into the neighbouring byte)
__device__ __forceinline__ uint32_t fq_nlmask(uint32_t w) {
  const uint32_t x = w ^ 0x0A0A0A0Au;
  return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}

// bit j set: byte p + j of the buffer is a '\n' of the text [lo, hi); p is 16-aligned
__device__ __forceinline__ uint32_t fq_lane_mask(const uint8_t* buf, uint32_t p, uint32_t lo, uint32_t hi) {
  if (p >= hi) return 0;
  const uint4 v = *(const uint4*)(buf + p);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t out = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t m = fq_nlmask(w[k]);
    const uint32_t q = p + 4u * k;
    if (q < lo || q + 4u > hi) {                       // the two ends of the text: byte by byte
      uint32_t keep = 0;
      for (uint32_t j = 0; j < 4; ++j) if (q + j >= lo && q + j < hi) keep |= 0x80u << (8 * j);
      m &= keep;
    }
    out |= (((m >> 7) & 1u) | ((m >> 14) & 2u) | ((m >> 21) & 4u) | ((m >> 28) & 8u)) << (4 * k);
  }
  return out;
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fastq_count(const uint8_t* buf, uint32_t lo, uint32_t hi, int32_t* cnt) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * FQ_TILE + (uint32_t)wv * FQ_SUB;
  int c = 0;
  if (base < hi)
    for (uint32_t s = 0; s < FQ_SUB; s += FQ_STEP) c += __popc(fq_lane_mask(buf, base + s + 16u * lane, lo, hi));
  c = wave_scan_add(c);
  if (lane == 63) cnt[blockIdx.x * TX_WAVES + wv] = c;
}

// cnt[0..m) -> exclusive prefix sums, in place; the header gets the line counts and is made ready for k_fastq_records
__global__ __launch_bounds__(256) void k_fastq_scan(int32_t* cnt, int m, const uint8_t* buf, uint32_t lo, uint32_t hi, int at_eof, C3FqHdr* hdr) {
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
  if (threadIdx.x == 0) {
    const int virt = (at_eof && hi > lo && buf[hi - 1] != '\n') ? 1 : 0;
    hdr->n_lines = run; hdr->n_lines_v = run + virt; hdr->first_bad = INT32_MAX; hdr->departed = 0;
    hdr->n_records = hdr->n_kept = hdr->n_short = hdr->consumed = hdr->name_bytes = hdr->base_bytes = 0;
  }
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fastq_lines(const uint8_t* buf, uint32_t lo, uint32_t hi, const int32_t* cnt, int32_t* nl) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t base = blockIdx.x * FQ_TILE + (uint32_t)wv * FQ_SUB;
  if (base >= hi) return;
  int at = cnt[blockIdx.x * TX_WAVES + wv];
  for (uint32_t s = 0; s < FQ_SUB; s += FQ_STEP) {
    const uint32_t p = base + s + 16u * lane;
    uint32_t m = fq_lane_mask(buf, p, lo, hi);
    const int c = __popc(m);
    const int inc = wave_scan_add(c);
    int k = at + inc - c;
    while (m) { nl[k++] = (int32_t)(p + (uint32_t)__ffs((int)m) - 1u); m &= m - 1u; }
    at += wave_bcast(inc, 63);
  }
}

// line k of the text: [begin, end) with the '\r' rule applied; L real '\n', line L (if any) ends at hi
struct FqLines {
  const char* t; const int32_t* nl; int32_t lo, hi, L;
  __device__ __forceinline__ int32_t begin(int32_t k) const { return k == 0 ? lo : nl[k - 1] + 1; }
  __device__ __forceinline__ int32_t end_raw(int32_t k) const { return k < L ? nl[k] : hi; }
};

__global__ __launch_bounds__(256) void k_fastq_records(const uint8_t* buf, uint32_t lo, uint32_t hi, const int32_t* nl, int L, int n_full,
                                                       int partial, int32_t* slen, int32_t* nlen, C3FqHdr* hdr) {
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  if (r > n_full) return;
  if (r == n_full) { if (partial) atomicMin(&hdr->first_bad, r); return; }        // an incomplete record at the end of the file
  const FqLines ln{(const char*)buf, nl, (int32_t)lo, (int32_t)hi, L};
  int32_t b[4], e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { b[k] = ln.begin(4 * r + k); e[k] = c3_fastq_line_end(ln.t, b[k], ln.end_raw(4 * r + k)); }
  if (c3_fastq_strict(ln.t, b, e)) {
    slen[r] = e[1] - b[1];
    nlen[r] = c3_fastq_name_len(ln.t, b[0], e[0]);
  } else {
    slen[r] = 0; nlen[r] = 0;
    atomicMin(&hdr->first_bad, r);
  }
}

// (kept, sequence bytes, name bytes) of record r, zero at and behind the first bad record
__device__ __forceinline__ void fq_rec_terms(int r, int n_rec, const int32_t* slen, const int32_t* nlen, int min_len, long long* k, long long* s, long long* n) {
  *k = 0; *s = 0; *n = 0;
  if (r < n_rec) { const int32_t sl = slen[r]; if (sl >= min_len) { *k = 1; *s = sl; *n = nlen[r]; } }
}

__global__ __launch_bounds__(256) void k_fastq_rsum(const int32_t* slen, const int32_t* nlen, int n_full, int min_len, const C3FqHdr* hdr, long long* bsum) {
  __shared__ long long lds[TX_WAVES];
  const int n_rec = min(hdr->first_bad, n_full);
  long long k, s, n, tk, ts, tn;
  fq_rec_terms(blockIdx.x * 256 + (int)threadIdx.x, n_rec, slen, nlen, min_len, &k, &s, &n);
  (void)tx_block_excl(k, lds, &tk); (void)tx_block_excl(s, lds, &ts); (void)tx_block_excl(n, lds, &tn);
  if (threadIdx.x == 0) { bsum[3 * blockIdx.x] = tk; bsum[3 * blockIdx.x + 1] = ts; bsum[3 * blockIdx.x + 2] = tn; }
}

// bsum[0..3 * nb) -> exclusive prefix sums per stream, in place; the header and the closing entries of off / name_off
__global__ __launch_bounds__(256) void k_fastq_rscan(long long* bsum, int nb, const int32_t* nl, uint32_t lo, uint32_t hi, int L, int n_full,
                                                     C3FqHdr* hdr, int64_t* off, int64_t* name_off) {
  __shared__ long long lds[TX_WAVES];
  long long run[3] = {0, 0, 0};
  for (int i0 = 0; i0 < nb; i0 += 256) {
    const int i = i0 + (int)threadIdx.x;
    for (int c = 0; c < 3; ++c) {
      const long long v = i < nb ? bsum[3 * i + c] : 0;
      long long tot;
      const long long ex = tx_block_excl(v, lds, &tot);
      if (i < nb) bsum[3 * i + c] = run[c] + ex;
      run[c] += tot;
    }
  }
  if (threadIdx.x == 0) {
    const int fb = hdr->first_bad;
    const int n_rec = min(fb, n_full);
    hdr->departed = fb != INT32_MAX ? 1 : 0;
    hdr->n_records = n_rec; hdr->n_kept = run[0]; hdr->n_short = n_rec - run[0];
    hdr->base_bytes = run[1]; hdr->name_bytes = run[2];
    const int last = 4 * n_rec - 1;                      // the record's last line: the next record starts behind its '\n'
    hdr->consumed = n_rec == 0 ? 0 : (last < L ? (int64_t)nl[last] + 1 : (int64_t)hi) - (int64_t)lo;
    off[run[0]] = run[1]; name_off[run[0]] = run[2];
  }
}

__global__ __launch_bounds__(256) void k_fastq_rfin(const int32_t* slen, const int32_t* nlen, const int32_t* nl, uint32_t lo, int n_full, int min_len,
                                                    const C3FqHdr* hdr, const long long* bsum, int64_t* off, int64_t* name_off, int4* src) {
  __shared__ long long lds[TX_WAVES];
  const int n_rec = min(hdr->first_bad, n_full);
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  long long k, s, n, t;
  fq_rec_terms(r, n_rec, slen, nlen, min_len, &k, &s, &n);
  const long long ek = tx_block_excl(k, lds, &t), es = tx_block_excl(s, lds, &t), en = tx_block_excl(n, lds, &t);
  if (!k) return;
  const long long i = bsum[3 * blockIdx.x] + ek;
  off[i] = bsum[3 * blockIdx.x + 1] + es;
  name_off[i] = bsum[3 * blockIdx.x + 2] + en;
  const int32_t b0 = r == 0 ? (int32_t)lo : nl[4 * r - 1] + 1;
  src[i] = make_int4(nl[4 * r] + 1, nl[4 * r + 2] + 1, b0 + 1, 0);        // sequence, quality, name
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_fastq_gather(const uint8_t* buf, const int4* src, const int64_t* off, const int64_t* name_off,
                                                                long long n_kept, uint8_t* names, uint8_t* seqs, uint8_t* quals) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long i0 = (long long)blockIdx.x * TX_WAVES;
  {
    const long long i = i0 + wv;
    if (i < n_kept) {
      const int4 p = src[i];
      const int64_t no = name_off[i], so = off[i];
      const uint32_t nlen = (uint32_t)(name_off[i + 1] - no), sl = (uint32_t)(off[i + 1] - so);
      tx_wave_copy(names + no, buf + p.z, nlen, lane);
      if (seqs && sl <= TX_LONG) {
        tx_wave_copy(seqs + so, buf + p.x, sl, lane);
        tx_wave_copy(quals + so, buf + p.y, sl, lane);
      }
    }
  }
  if (!seqs) return;
  for (int k = 0; k < TX_WAVES; ++k) {                  // long records of the workgroup: a quarter (in whole 256-byte rows) each
    const long long i = i0 + k;
    if (i >= n_kept) break;
    const int64_t so = off[i];
    const uint32_t sl = (uint32_t)(off[i + 1] - so);
    if (sl <= TX_LONG) continue;
    const int4 p = src[i];
    uint32_t b, e;
    tx_piece(sl, wv, TX_WAVES, &b, &e);
    tx_wave_copy(seqs + so + b, buf + p.x + b, e - b, lane);
    tx_wave_copy(quals + so + b, buf + p.y + b, e - b, lane);
  }
}

extern "C" void c3k_launch_fastq_count(const uint8_t* buf, uint32_t lo, uint32_t hi, int32_t* cnt, int at_eof, C3FqHdr* hdr, hipStream_t s) {
  const int tiles = (int)(((uint64_t)hi + FQ_TILE - 1) / FQ_TILE);
  hipLaunchKernelGGL(k_fastq_count, dim3(tiles), dim3(64 * TX_WAVES), 0, s, buf, lo, hi, cnt);
  hipLaunchKernelGGL(k_fastq_scan, dim3(1), dim3(256), 0, s, cnt, tiles * TX_WAVES, buf, lo, hi, at_eof, hdr);
}
extern "C" void c3k_launch_fastq_lines(const uint8_t* buf, uint32_t lo, uint32_t hi, const int32_t* cnt, int32_t* nl, hipStream_t s) {
  const int tiles = (int)(((uint64_t)hi + FQ_TILE - 1) / FQ_TILE);
  hipLaunchKernelGGL(k_fastq_lines, dim3(tiles), dim3(64 * TX_WAVES), 0, s, buf, lo, hi, cnt, nl);
}
// n_full whole candidate records (partial: one more, incomplete, at the end of the file); bsum holds 3 * ((n_full + 256) / 256) sums
extern "C" void c3k_launch_fastq_records(const uint8_t* buf, uint32_t lo, uint32_t hi, const int32_t* nl, int L, int n_full, int partial, int min_len,
                                         int32_t* slen, int32_t* nlen, long long* bsum, C3FqHdr* hdr, int64_t* off, int64_t* name_off, int4* src,
                                         hipStream_t s) {
  const int nb1 = (n_full + 1 + 255) / 256, nb = (n_full + 255) / 256;
  hipLaunchKernelGGL(k_fastq_records, dim3(nb1), dim3(256), 0, s, buf, lo, hi, nl, L, n_full, partial, slen, nlen, hdr);
  if (nb) hipLaunchKernelGGL(k_fastq_rsum, dim3(nb), dim3(256), 0, s, slen, nlen, n_full, min_len, hdr, bsum);
  hipLaunchKernelGGL(k_fastq_rscan, dim3(1), dim3(256), 0, s, bsum, nb, nl, lo, hi, L, n_full, hdr, off, name_off);
  if (nb) hipLaunchKernelGGL(k_fastq_rfin, dim3(nb), dim3(256), 0, s, slen, nlen, nl, lo, n_full, min_len, hdr, bsum, off, name_off, src);
}
extern "C" void c3k_launch_fastq_gather(const uint8_t* buf, const int4* src, const int64_t* off, const int64_t* name_off, long long n_kept,
                                        uint8_t* names, uint8_t* seqs, uint8_t* quals, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k_fastq_gather, dim3((unsigned)((n_kept + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, buf, src, off, name_off, n_kept, names, seqs, quals);
}

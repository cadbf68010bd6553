// k_bam.hip -- the inflated bytes of an unaligned BAM file parsed on the GPU (include/c3poa.h "Unaligned BAM records on the GPU";
// DESIGN.md 5.12).  The rule of one record is c3_bam.h, which the host statement c3_bam_parse_host (c3_bam.cpp) applies as
// well; this file finds the record starts, scans the lengths and moves the bytes.  The data occupies bytes [lo, hi) of a
// 256-aligned device buffer with at least 256 bytes of slack behind hi (lo <= 3: the stand-alone call keeps the caller's
// misalignment); positions are 32-bit offsets into that buffer (C3_FASTQ_MAX_TEXT; one record more stays below 2^32).
//
// BAM records are a linked list: record k + 1 begins at p_k + 4 + block_size_k.  No workgroup hands anything to another inside
// a launch; the phases are launches on one stream, and every loop runs to a count known at launch.
//   k_bam_header    one lane: the file header's extent (at_start), the first record's byte.
//   k_bam_guess     one wave per tile of C3_BAM_TILE bytes: the first byte of the tile that looks like a record header (the
//       fixed fields are consistent and the name ends in NUL; in the tile that holds the first record, that record), found
//       64 candidate bytes at a time with a ballot, then the walk from it to the tile's end: where it left and how many starts
//       it passed.  The guess is a heuristic and can never change the result: k_bam_resolve uses a tile's walk only when the
//       true chain enters the tile exactly at the guess, and then the walk IS the chain (the same function of the same bytes).
//   k_bam_resolve   one wave goes through the tiles in order, 64 at a time in registers: the entry of a tile is the exit of
//       the last tile that held a start; entry == guess accepts the tile's walk, anything else is walked again here from the
//       true entry; a tile the chain jumps over holds no start; a start without a whole, valid block_size ends the chain.
//       The counts are summed on the way (their exclusive scan), so the host learns the number of starts with the header.
//   k_bam_fill      one lane per tile walks it once more from its true first start and writes rec_pos[].
//   k_bam_records   one lane per record start: the rule (c3_bam_record), l_seq, the name length and the three source
//       positions; a record that is not strict or not whole does atomicMin on the first bad record.
//   k_bam_rsum / k_bam_rscan / k_bam_rfin   the (kept, bases, names) scans of k_fastq over the records in front of it.
//   k_bam_gather    one wave per kept record, the four waves of a workgroup together on a record above TX_LONG bases.  Names
//       by tx_wave_copy.  Bases: the destination is brought to a dword with byte stores, then each lane takes 8 bases at a
//       time: three aligned source dwords joined by v_alignbyte give the packed dword at any byte, a nibble swap and (at an
//       odd base) a 4-bit shift put the codes in order, a 16-entry table held in two 64-bit registers maps them, two dword
//       stores.  Qualities: the wave copy with min(q, 93) + 33 applied to the four bytes of each dword.  Nothing outside a
//       record's own destination range is written; nothing outside the dwords that hold data (plus the slack) is read.
#include "c3_dev.h"
#include "c3_bam.h"
#include "c3_launch.h"
#include "k_text.h"

#define BAM_TILE ((uint32_t)C3_BAM_TILE)
#define BAM_WALK_MAX (C3_BAM_TILE / (4 + C3_BAM_MIN_BLOCK) + 2)        // a step advances 38 bytes at least

// the dword at any byte p of the buffer: two aligned dwords joined (the second lies in the data or the slack)
__device__ __forceinline__ uint32_t bam_ld32(const uint8_t* buf, int64_t p) {
  const uint32_t* a = (const uint32_t*)(buf + (p & ~(int64_t)3));
  const uint32_t sh = (uint32_t)(p & 3);
  return sh ? __builtin_amdgcn_alignbyte(a[1], a[0], sh) : a[0];
}

struct BamWalk { int64_t exit; int32_t cnt, stop; };

// the chain from record start p while it stays below lim (the tile's end, or hi): the starts it passes (written to out when
// given), where it leaves, and whether it ended at a start whose block_size is cut by hi or out of range
__device__ __forceinline__ BamWalk bam_walk(const uint8_t* buf, int64_t p, int64_t lim, int64_t hi, uint32_t* out) {
  BamWalk w{p, 0, 0};
  for (int it = 0; it < BAM_WALK_MAX && p < lim; ++it) {
    if (out) out[w.cnt] = (uint32_t)p;
    ++w.cnt;
    if (p + 4 > hi) { w.stop = 1; break; }
    const uint32_t bs = bam_ld32(buf, p);                // checked before it is added
    if (!c3_bam_block_ok(bs)) { w.stop = 1; break; }
    p += 4 + (int64_t)bs;
  }
  w.exit = p;
  return w;
}

__global__ void k_bam_header(const uint8_t* buf, uint32_t lo, uint32_t hi, int at_start, C3BamHdr* hdr) {
  if (threadIdx.x != 0) return;
  int64_t nx = lo;
  const int st = at_start ? c3_bam_header(buf, (int64_t)lo, (int64_t)hi, &nx) : C3_BAM_OK;
  hdr->hstat = st; hdr->first_bad = INT32_MAX; hdr->departed = 0; hdr->reason = 0;
  hdr->start = st == C3_BAM_OK ? nx : (int64_t)lo; hdr->chain_end = hdr->start; hdr->n_starts = 0;
  hdr->n_records = hdr->n_kept = hdr->n_short = hdr->consumed = hdr->name_bytes = hdr->base_bytes = hdr->bad_at = 0;
}

// does byte p look like a record header?  (a heuristic over the fixed fields; whole inside [lo, hi))
__device__ __forceinline__ bool bam_plausible(const uint8_t* buf, int64_t p, int64_t hi) {
  if (p + 36 > hi) return false;
  const uint32_t bs = bam_ld32(buf, p);
  if (!c3_bam_block_ok(bs)) return false;
  const uint32_t w12 = bam_ld32(buf, p + 12), w16 = bam_ld32(buf, p + 16), ls = bam_ld32(buf, p + 20);
  const uint32_t lrn = w12 & 0xFFu, nc = w16 & 0xFFFFu, flag = w16 >> 16;
  if (lrn == 0 || ls == 0 || (flag & (0x10u | 0x100u | 0x800u))) return false;
  if (32ull + lrn + 4ull * nc + ((uint64_t)ls + 1) / 2 + (uint64_t)ls > (uint64_t)bs) return false;
  const int64_t z = p + 36 + lrn - 1;
  if (z >= hi || buf[z] != 0) return false;
  // ... and a name of printable bytes: low quality values look like the fixed fields often enough, and the NUL is then found
  // in the next record's header (measured on cfg2 reads: one tile in six guessed wrong without this, none with it)
  for (int64_t k = p + 36; k < z; ++k) { const uint32_t c = buf[k]; if ((c < 0x20u && c != 9u) || c > 0x7Eu) return false; }
  return true;
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_bam_guess(const uint8_t* buf, uint32_t lo, uint32_t hi, int n_tiles, C3BamTile* tiles, const C3BamHdr* hdr) {
  const int lane = threadIdx.x & 63;
  const int t = (int)blockIdx.x * TX_WAVES + (int)(threadIdx.x >> 6);
  if (t >= n_tiles) return;
  const int64_t tb = (int64_t)t * BAM_TILE, lim = min(tb + (int64_t)BAM_TILE, (int64_t)hi);
  const int64_t start = hdr->start;
  int64_t g = -1;
  if (hdr->hstat == C3_BAM_OK) {
    if (start >= tb && start < lim) g = start;
    else if (start < tb) {
      for (uint32_t s = 0; s < BAM_TILE; s += 64u) {
        const int64_t p = tb + s + lane;
        const bool ok = p < lim && bam_plausible(buf, p, (int64_t)hi);
        const unsigned long long m = __ballot(ok);
        if (m) { g = tb + s + (int64_t)__ffsll((long long)m) - 1; break; }
      }
    }
  }
  BamWalk w{0, 0, 0};
  if (g >= 0) w = bam_walk(buf, g, lim, (int64_t)hi, nullptr);        // (every lane walks the same bytes: wave-uniform)
  if (lane == 0) {
    C3BamTile& o = tiles[t];
    o.guess = g >= 0 ? (uint32_t)g : C3_BAM_NONE; o.gexit = (uint32_t)w.exit; o.gcnt = w.cnt; o.gstop = w.stop;
  }
}

// One wave.  64 tiles at a time are loaded, a lane each (one coalesced load per 64 tiles instead of a dependent load per tile);
// the chain then runs through them in registers: entry, ended and total are wave-uniform and made so by readfirstlane /
// readlane, which keeps them and the branches on them on the scalar unit; tile l's walk comes from lane l, and a tile whose
// guess was not the entry is walked again by the whole wave (uniformly: the same bytes).  Positions fit 32 bits (c3_bam.h).
__global__ __launch_bounds__(64) void k_bam_resolve(const uint8_t* buf, uint32_t lo, uint32_t hi, int n_tiles, C3BamTile* tiles, C3BamHdr* hdr) {
  const int lane = (int)threadIdx.x;
  bool ended = __builtin_amdgcn_readfirstlane(hdr->hstat) != C3_BAM_OK;
  uint32_t entry = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hdr->start);
  int32_t total = 0;
  for (int t0 = 0; t0 < n_tiles; t0 += 64) {
    const int t = t0 + lane;
    C3BamTile g;
    g.guess = C3_BAM_NONE; g.gexit = 0; g.gcnt = 0; g.gstop = 0;
    if (t < n_tiles) g = tiles[t];
    uint32_t my_first = C3_BAM_NONE;
    int32_t my_cnt = 0, my_base = 0;
    const int nl = min(64, n_tiles - t0);
    for (int l = 0; l < nl; ++l) {
      const uint32_t lim = min((uint32_t)(t0 + l + 1) * BAM_TILE, hi);
      uint32_t first = C3_BAM_NONE;
      int32_t cnt = 0;
      if (!ended && entry < lim) {
        first = entry;
        int32_t stop;
        if ((uint32_t)__builtin_amdgcn_readlane((int)g.guess, l) == first) {
          entry = (uint32_t)__builtin_amdgcn_readlane((int)g.gexit, l);
          cnt = __builtin_amdgcn_readlane(g.gcnt, l); stop = __builtin_amdgcn_readlane(g.gstop, l);
        } else {
          const BamWalk w = bam_walk(buf, (int64_t)first, (int64_t)lim, (int64_t)hi, nullptr);
          entry = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w.exit);
          cnt = __builtin_amdgcn_readfirstlane(w.cnt); stop = __builtin_amdgcn_readfirstlane(w.stop);
        }
        if (stop) ended = true;
      }
      if (lane == l) { my_first = first; my_cnt = cnt; my_base = total; }
      total += cnt;
    }
    if (t < n_tiles) { tiles[t].first = my_first; tiles[t].cnt = my_cnt; tiles[t].base = my_base; }
  }
  if (lane == 0) { hdr->n_starts = total; hdr->chain_end = (int64_t)entry; }
}

__global__ __launch_bounds__(64) void k_bam_fill(const uint8_t* buf, uint32_t hi, int n_tiles, const C3BamTile* tiles, uint32_t* rec_pos) {
  const int t = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (t >= n_tiles) return;
  const C3BamTile g = tiles[t];
  if (g.cnt <= 0) return;
  const int64_t lim = min(((int64_t)t + 1) * BAM_TILE, (int64_t)hi);
  (void)bam_walk(buf, (int64_t)g.first, lim, (int64_t)hi, rec_pos + g.base);
}

__global__ __launch_bounds__(256) void k_bam_records(const uint8_t* buf, uint32_t hi, const uint32_t* rec_pos, int n_starts,
                                                     int32_t* slen, int32_t* nlen, int32_t* reason, int4* rsrc, C3BamHdr* hdr) {
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  if (r >= n_starts) return;
  C3BamRec rec;
  const int st = c3_bam_record(buf, (int64_t)rec_pos[r], (int64_t)hi, &rec);
  reason[r] = st;
  if (st == C3_BAM_OK) {
    slen[r] = (int32_t)rec.l_seq; nlen[r] = (int32_t)rec.name_len;
    rsrc[r] = make_int4((int)rec.seq, (int)rec.qual, (int)rec.name, 0);
  } else {
    slen[r] = 0; nlen[r] = 0;
    atomicMin(&hdr->first_bad, r);
  }
}

// (kept, bases, name bytes) of record r, zero at and behind the first bad record
__device__ __forceinline__ void bam_rec_terms(int r, int n_rec, const int32_t* slen, const int32_t* nlen, int min_len, long long* k, long long* s, long long* n) {
  *k = 0; *s = 0; *n = 0;
  if (r < n_rec) { const int32_t sl = slen[r]; if (sl >= min_len) { *k = 1; *s = sl; *n = nlen[r]; } }
}

__global__ __launch_bounds__(256) void k_bam_rsum(const int32_t* slen, const int32_t* nlen, int n_starts, int min_len, const C3BamHdr* hdr, long long* bsum) {
  __shared__ long long lds[TX_WAVES];
  const int n_rec = min(hdr->first_bad, n_starts);
  long long k, s, n, tk, ts, tn;
  bam_rec_terms(blockIdx.x * 256 + (int)threadIdx.x, n_rec, slen, nlen, min_len, &k, &s, &n);
  (void)tx_block_excl(k, lds, &tk); (void)tx_block_excl(s, lds, &ts); (void)tx_block_excl(n, lds, &tn);
  if (threadIdx.x == 0) { bsum[3 * blockIdx.x] = tk; bsum[3 * blockIdx.x + 1] = ts; bsum[3 * blockIdx.x + 2] = tn; }
}

// bsum[0..3 * nb) -> exclusive prefix sums per stream, in place; the header and the closing entries of off / name_off
__global__ __launch_bounds__(256) void k_bam_rscan(long long* bsum, int nb, const uint32_t* rec_pos, const int32_t* reason, uint32_t lo, int n_starts,
                                                   int at_eof, C3BamHdr* hdr, int64_t* off, int64_t* name_off) {
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
    const int n_rec = min(fb, n_starts);
    int departed = 0, why = 0;
    int64_t end = hdr->chain_end;
    if (fb < n_starts) {
      const int st = reason[fb];
      end = (int64_t)rec_pos[fb];
      if (st != C3_BAM_INCOMPLETE) { departed = 1; why = st; }
      else if (at_eof) { departed = 1; why = C3_BAM_TRUNCATED; }
    }
    hdr->departed = departed; hdr->reason = why; hdr->bad_at = departed ? end - (int64_t)lo : 0;
    hdr->n_records = n_rec; hdr->n_kept = run[0]; hdr->n_short = n_rec - run[0];
    hdr->base_bytes = run[1]; hdr->name_bytes = run[2];
    hdr->consumed = end - (int64_t)lo;
    off[run[0]] = run[1]; name_off[run[0]] = run[2];
  }
}

__global__ __launch_bounds__(256) void k_bam_rfin(const int32_t* slen, const int32_t* nlen, const int4* rsrc, int n_starts, int min_len,
                                                  const C3BamHdr* hdr, const long long* bsum, int64_t* off, int64_t* name_off, int4* src) {
  __shared__ long long lds[TX_WAVES];
  const int n_rec = min(hdr->first_bad, n_starts);
  const int r = blockIdx.x * 256 + (int)threadIdx.x;
  long long k, s, n, t;
  bam_rec_terms(r, n_rec, slen, nlen, min_len, &k, &s, &n);
  const long long ek = tx_block_excl(k, lds, &t), es = tx_block_excl(s, lds, &t), en = tx_block_excl(n, lds, &t);
  if (!k) return;
  const long long i = bsum[3 * blockIdx.x] + ek;
  off[i] = bsum[3 * blockIdx.x + 1] + es;
  name_off[i] = bsum[3 * blockIdx.x + 2] + en;
  src[i] = rsrc[r];                                        // packed bases, qualities, name
}

// ---- the byte maps of the gather ----
constexpr uint64_t bam_tab(int h) {                        // codes 8h .. 8h + 7 of "=ACMGRSVTWYHKDBN", code k in byte k
  const char* s = "=ACMGRSVTWYHKDBN";
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v |= (uint64_t)(uint8_t)s[8 * h + k] << (8 * k);
  return v;
}
__device__ __forceinline__ uint32_t bam_lut(uint32_t code, uint64_t t0, uint64_t t1) {
  return (uint32_t)(((code & 8u) ? t1 : t0) >> ((code & 7u) * 8u)) & 0xFFu;
}
// four codes (the first in bits 0..3) -> four characters (the first in byte 0)
__device__ __forceinline__ uint32_t bam_dec4(uint32_t x, uint64_t t0, uint64_t t1) {
  return bam_lut(x & 15u, t0, t1) | (bam_lut((x >> 4) & 15u, t0, t1) << 8) | (bam_lut((x >> 8) & 15u, t0, t1) << 16) | (bam_lut((x >> 12) & 15u, t0, t1) << 24);
}
__device__ __forceinline__ uint32_t bam_qual4(uint32_t w) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) r |= (min((w >> (8 * k)) & 0xFFu, 93u) + 33u) << (8 * k);
  return r;
}

// dst[0..len) = the characters of bases b0 .. b0 + len of the packed bases at S, by the 64 lanes of a wave
__device__ __forceinline__ void bam_wave_bases(uint8_t* dst, const uint8_t* S, uint32_t b0, uint32_t len, int lane) {
  const uint64_t t0 = bam_tab(0), t1 = bam_tab(1);
  const uint32_t head = min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) { const uint32_t b = b0 + lane, x = S[b >> 1]; dst[lane] = (uint8_t)bam_lut((b & 1u) ? x : x >> 4, t0, t1); }
  const uint32_t nd = (len - head) >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  for (uint32_t u = (uint32_t)lane; 2u * u < nd; u += 64u) {
    const uint32_t b = b0 + head + 8u * u;                   // 8 bases from base b: bytes B .. B + 4 of the packed bases
    const uint8_t* B = S + (b >> 1);
    const uint32_t sh = (uint32_t)((uintptr_t)B & 3u);
    const uint32_t* a = (const uint32_t*)(B - sh);
    const uint32_t a0 = a[0], a1 = a[1], a2 = a[2];
    const uint32_t w0 = sh ? __builtin_amdgcn_alignbyte(a1, a0, sh) : a0, w1 = sh ? __builtin_amdgcn_alignbyte(a2, a1, sh) : a1;
    uint64_t v = ((uint64_t)w1 << 32) | w0;
    v = ((v & 0xF0F0F0F0F0F0F0F0ull) >> 4) | ((v & 0x0F0F0F0F0F0F0F0Full) << 4);      // high nibble first -> code i in bits 4i
    if (b & 1u) v >>= 4;
    const uint32_t x = (uint32_t)v;
    d4[2u * u] = bam_dec4(x & 0xFFFFu, t0, t1);
    if (2u * u + 1u < nd) d4[2u * u + 1u] = bam_dec4(x >> 16, t0, t1);
  }
  const uint32_t done = head + 4u * nd, tail = len - done;
  if ((uint32_t)lane < tail) { const uint32_t b = b0 + done + lane, x = S[b >> 1]; dst[done + lane] = (uint8_t)bam_lut((b & 1u) ? x : x >> 4, t0, t1); }
}

// dst[0..len) = min(src[k], 93) + 33: tx_wave_copy with the map applied
__device__ __forceinline__ void bam_wave_quals(uint8_t* dst, const uint8_t* src, uint32_t len, int lane) {
  const uint32_t head = min(len, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if ((uint32_t)lane < head) dst[lane] = c3_bam_qual(src[lane]);
  const uint32_t nd = (len - head) >> 2;
  uint32_t* d4 = (uint32_t*)(dst + head);
  const uint8_t* s = src + head;
  const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
  const uint32_t* sa = (const uint32_t*)(s - sh);
  if (sh == 0) { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = bam_qual4(sa[k]); }
  else         { for (uint32_t k = (uint32_t)lane; k < nd; k += 64u) d4[k] = bam_qual4(__builtin_amdgcn_alignbyte(sa[k + 1], sa[k], sh)); }
  const uint32_t done = head + 4u * nd, tail = len - done;
  if ((uint32_t)lane < tail) dst[done + lane] = c3_bam_qual(src[done + lane]);
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_bam_gather(const uint8_t* buf, const int4* src, const int64_t* off, const int64_t* name_off,
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
      tx_wave_copy(names + no, buf + (uint32_t)p.z, nlen, lane);
      if (sl <= TX_LONG) {
        bam_wave_bases(seqs + so, buf + (uint32_t)p.x, 0u, sl, lane);
        bam_wave_quals(quals + so, buf + (uint32_t)p.y, sl, lane);
      }
    }
  }
  for (int k = 0; k < TX_WAVES; ++k) {                  // long records of the workgroup: a quarter (in whole 256-base rows) each
    const long long i = i0 + k;
    if (i >= n_kept) break;
    const int64_t so = off[i];
    const uint32_t sl = (uint32_t)(off[i + 1] - so);
    if (sl <= TX_LONG) continue;
    const int4 p = src[i];
    uint32_t b, e;
    tx_piece(sl, wv, TX_WAVES, &b, &e);
    bam_wave_bases(seqs + so + b, buf + (uint32_t)p.x, b, e - b, lane);
    bam_wave_quals(quals + so + b, buf + (uint32_t)p.y + b, e - b, lane);
  }
}

// header -> guesses -> chain: afterwards hdr holds hstat, start, n_starts and chain_end, tiles[] each tile's first start, count and base
extern "C" void c3k_launch_bam_chain(const uint8_t* buf, uint32_t lo, uint32_t hi, int at_start, C3BamTile* tiles, C3BamHdr* hdr, hipStream_t s) {
  const int n_tiles = (int)(((uint64_t)hi + BAM_TILE - 1) / BAM_TILE);
  hipLaunchKernelGGL(k_bam_header, dim3(1), dim3(64), 0, s, buf, lo, hi, at_start, hdr);
  hipLaunchKernelGGL(k_bam_guess, dim3((n_tiles + TX_WAVES - 1) / TX_WAVES), dim3(64 * TX_WAVES), 0, s, buf, lo, hi, n_tiles, tiles, (const C3BamHdr*)hdr);
  hipLaunchKernelGGL(k_bam_resolve, dim3(1), dim3(64), 0, s, buf, lo, hi, n_tiles, tiles, hdr);
}
// n_starts record starts (> 0): rec_pos[], the rule per record, the scans; bsum holds 3 * ((n_starts + 255) / 256) sums
extern "C" void c3k_launch_bam_records(const uint8_t* buf, uint32_t lo, uint32_t hi, const C3BamTile* tiles, int n_starts, int at_eof, int min_len,
                                       uint32_t* rec_pos, int32_t* slen, int32_t* nlen, int32_t* reason, int4* rsrc, long long* bsum, C3BamHdr* hdr,
                                       int64_t* off, int64_t* name_off, int4* src, hipStream_t s) {
  const int n_tiles = (int)(((uint64_t)hi + BAM_TILE - 1) / BAM_TILE);
  const int nb = (n_starts + 255) / 256;
  hipLaunchKernelGGL(k_bam_fill, dim3((n_tiles + 63) / 64), dim3(64), 0, s, buf, hi, n_tiles, tiles, rec_pos);
  hipLaunchKernelGGL(k_bam_records, dim3(nb), dim3(256), 0, s, buf, hi, (const uint32_t*)rec_pos, n_starts, slen, nlen, reason, rsrc, hdr);
  hipLaunchKernelGGL(k_bam_rsum, dim3(nb), dim3(256), 0, s, (const int32_t*)slen, (const int32_t*)nlen, n_starts, min_len, (const C3BamHdr*)hdr, bsum);
  hipLaunchKernelGGL(k_bam_rscan, dim3(1), dim3(256), 0, s, bsum, nb, (const uint32_t*)rec_pos, (const int32_t*)reason, lo, n_starts, at_eof, hdr, off, name_off);
  hipLaunchKernelGGL(k_bam_rfin, dim3(nb), dim3(256), 0, s, (const int32_t*)slen, (const int32_t*)nlen, (const int4*)rsrc, n_starts, min_len,
                     (const C3BamHdr*)hdr, (const long long*)bsum, off, name_off, src);
}
extern "C" void c3k_launch_bam_gather(const uint8_t* buf, const int4* src, const int64_t* off, const int64_t* name_off, long long n_kept,
                                      uint8_t* names, uint8_t* seqs, uint8_t* quals, hipStream_t s) {
  if (n_kept <= 0) return;
  hipLaunchKernelGGL(k_bam_gather, dim3((unsigned)((n_kept + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, buf, src, off, name_off, n_kept, names, seqs, quals);
}

// k_dsplit.hip -- the stable multi-way partition of the demultiplexer's text path (include/c3poa.h "Sample demultiplexer, pieces
// of text in / per-sample streams out").  The rule is c3_dsplit.h, which the host statement (c3_dsplit.cpp)
// applies as well; this file sums the lengths and moves the bytes.  The records lie parsed on the device (names / name_off,
// seqs / quals / off), krec[] lists the kept ones in input order and win[] holds k_demux's winners for them.
//
//   k_tx_xsum / k_tx_xscan / k_tx_xfin <DsKept>   krec[] and the kept count for a FASTQ text (k_fasta makes them itself): the
//       one-column exclusive scan of k_text.h over the records.
//   k_dsplit_key    one lane per kept record: its stream (c3_dsplit_stream) and its output length (c3_demux_rec_len).
//   k_dsplit_tile   one workgroup per tile of 256 kept records: keys and lengths of the tile in LDS, every lane walks the lanes in
//       front of it and adds the lengths of those with its own key (LDS broadcast reads) -> rank[]; the last record of each
//       stream in the tile writes that stream's tile sum into base[tile][s] (the table is zeroed beforehand).  No atomics.
//   k_dsplit_cols   one lane per stream walks its column of base[][] down the tiles: exclusive sums in place, the total into
//       stream_off[s + 1]; neighbouring lanes read neighbouring words.  k_dsplit_offs (one workgroup) then turns the totals into
//       stream_off[0 .. S].  A record's place is stream_off[s] + base[tile][s] + rank, which depends on nothing but the input.
//   k_dsplit_emit   one wave per kept record in the shape of k_demux_emit: literals and index names by the first lanes, name,
//       sequence and quality dword-wise (tx_wave_copy), the four waves of a workgroup together on a record above TX_LONG bytes.
//       A wave writes only inside [place, place + length).
// Resources (hipcc -O3 gfx950, -Rpass-analysis=kernel-resource-usage): DESIGN.md 5.10.
#include "k_text.h"
#include "c3_dsplit.h"
#include "c3_launch.h"

static_assert(C3_DS_TILE == 64 * TX_WAVES, "a placement tile is one workgroup of lanes");

// ---- krec[] of a FASTQ text: the functor of the one-column scan (tx_xscan of k_text.h) ----
struct DsKept {                                          // over the parsed records: which are kept, krec[] in order
  DsArgs a;
  __device__ long long n() const { return a.n_records; }
  __device__ long long term(long long r) const { return c3_dsplit_kept(a.off[r + 1] - a.off[r]) ? 1 : 0; }
  __device__ void put(long long r, long long ex) const { a.krec[ex] = (int32_t)r; }
  __device__ void total(long long t) const { *a.n_kept_out = t; }
};

// ---- placement ----
__global__ __launch_bounds__(256) void k_dsplit_key(DsArgs a) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_kept) return;
  const int32_t r = a.krec[i], wa = a.win[2 * i], wb = a.win[2 * i + 1];
  a.key[i] = c3_dsplit_stream(wa, wb, a.n_a, a.n_b, a.split);
  a.rank[i] = c3_demux_rec_len(a.name_off[r + 1] - a.name_off[r], a.off[r + 1] - a.off[r], c3_dsplit_index_len(a.a_no, wa),
                               c3_dsplit_index_len(a.b_no, wb), a.quals != nullptr);      // the length; k_dsplit_tile makes it the rank
}

__global__ __launch_bounds__(C3_DS_TILE) void k_dsplit_tile(DsArgs a) {
  __shared__ int32_t key_s[C3_DS_TILE];
  __shared__ int64_t len_s[C3_DS_TILE];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * C3_DS_TILE + t;
  const int cnt = (int)min((long long)C3_DS_TILE, a.n_kept - (long long)blockIdx.x * C3_DS_TILE);      // >= 1: one workgroup per started tile
  int32_t k = -1; int64_t len = 0;
  if (t < cnt) { k = a.key[i]; len = a.rank[i]; }
  key_s[t] = k; len_s[t] = len;
  __syncthreads();
  if (t >= cnt) return;
  int64_t before = 0;
  for (int j = 0; j < t; ++j) if (key_s[j] == k) before += len_s[j];
  bool last = true;
  for (int j = t + 1; j < cnt; ++j) if (key_s[j] == k) { last = false; break; }
  a.rank[i] = before;
  if (last) a.base[(size_t)blockIdx.x * a.S + k] = before + len;
}

__global__ __launch_bounds__(256) void k_dsplit_cols(DsArgs a) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s >= a.S) return;
  int64_t run = 0;
  for (int tl = 0; tl < a.tiles; ++tl) {
    int64_t* p = a.base + (size_t)tl * a.S + s;
    const int64_t v = *p;
    *p = run;
    run += v;
  }
  a.stream_off[s + 1] = run;
}

// stream_off[1 .. S] hold the stream totals: -> stream_off[0 .. S], the exclusive sums and the grand total
__global__ __launch_bounds__(256) void k_dsplit_offs(DsArgs a) {
  __shared__ long long lds[TX_WAVES];
  long long run = 0;
  for (int s0 = 0; s0 < a.S; s0 += 256) {
    const int s = s0 + (int)threadIdx.x;
    const long long v = s < a.S ? (long long)a.stream_off[s + 1] : 0;
    long long tot;
    const long long ex = tx_block_excl(v, lds, &tot);
    if (s < a.S) a.stream_off[s + 1] = run + ex + v;      // (a lane rewrites only the word it read)
    run += tot;
  }
  if (threadIdx.x == 0) a.stream_off[0] = 0;
}

// ---- the records ----
// output record of kept record i; part / parts: this wave's share of sequence and quality (part 0 also writes everything else)
__device__ __forceinline__ void ds_emit_record(const DsArgs& a, long long i, int lane, int part, int parts) {
  const int32_t r = wave_first(a.krec[i]), wa = wave_first(a.win[2 * i]), wb = wave_first(a.win[2 * i + 1]), s = wave_first(a.key[i]);
  const int64_t no = a.name_off[r], so = a.off[r];
  const uint32_t nlen = (uint32_t)(a.name_off[r + 1] - no), sl = (uint32_t)(a.off[r + 1] - so);
  const uint32_t al = (uint32_t)c3_dsplit_index_len(a.a_no, wa), bl = (uint32_t)c3_dsplit_index_len(a.b_no, wb);
  uint8_t* o = a.out + a.stream_off[s] + a.base[(size_t)(i / C3_DS_TILE) * a.S + s] + a.rank[i];
  uint8_t* body = o + 4u + nlen + al + bl;
  uint8_t* qbody = body + sl + 3u;
  if (part == 0) {
    tx_wave_copy(o + 1, a.names + no, nlen, lane);
    for (uint32_t j = (uint32_t)lane; j < al; j += 64u) o[2u + nlen + j] = a.a_names[a.a_no[wa] + j];
    for (uint32_t j = (uint32_t)lane; j < bl; j += 64u) o[3u + nlen + al + j] = a.b_names[a.b_no[wb] + j];
    if (lane == 0) {
      o[0] = a.quals ? '@' : '>'; o[1u + nlen] = '|'; o[2u + nlen + al] = '_'; o[3u + nlen + al + bl] = '\n'; body[sl] = '\n';
      if (a.quals) { body[sl + 1u] = '+'; body[sl + 2u] = '\n'; qbody[sl] = '\n'; }
    }
  }
  uint32_t pb = 0, pe = sl;
  if (parts > 1) tx_piece(sl, part, parts, &pb, &pe);
  tx_wave_copy(body + pb, a.seqs + so + pb, pe - pb, lane);
  if (a.quals) tx_wave_copy(qbody + pb, a.quals + so + pb, pe - pb, lane);
}

__global__ __launch_bounds__(64 * TX_WAVES) void k_dsplit_emit(DsArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = wave_first((int)(threadIdx.x >> 6));
  const long long i0 = (long long)blockIdx.x * TX_WAVES;
  {
    const long long i = i0 + wv;
    if (i < a.n_kept) { const int32_t r = a.krec[i]; if (a.off[r + 1] - a.off[r] <= TX_LONG) ds_emit_record(a, i, lane, 0, 1); }
  }
  for (int k = 0; k < TX_WAVES; ++k) {                  // long records of the workgroup: a quarter of sequence and quality each
    const long long i = i0 + k;
    if (i >= a.n_kept) break;
    const int32_t r = a.krec[i];
    if (a.off[r + 1] - a.off[r] > TX_LONG) ds_emit_record(a, i, lane, wv, TX_WAVES);
  }
}

// bsum holds (n_records + 255) / 256 sums; *n_kept_out the count afterwards
extern "C" void c3k_launch_dsplit_krec(const DsArgs* a, hipStream_t s) { tx_xscan(DsKept{*a}, a->n_records, a->bsum, s); }
// n_kept > 0, tiles = (n_kept + C3_DS_TILE - 1) / C3_DS_TILE, base[tiles][S] zeroed by the caller; stream_off[S + 1] afterwards
extern "C" void c3k_launch_dsplit_place(const DsArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(k_dsplit_key, dim3((unsigned)((a->n_kept + 255) / 256)), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_dsplit_tile, dim3((unsigned)a->tiles), dim3(C3_DS_TILE), 0, s, *a);
  hipLaunchKernelGGL(k_dsplit_cols, dim3((unsigned)((a->S + 255) / 256)), dim3(256), 0, s, *a);
  hipLaunchKernelGGL(k_dsplit_offs, dim3(1), dim3(256), 0, s, *a);
}
extern "C" void c3k_launch_dsplit_emit(const DsArgs* a, hipStream_t s) {
  if (a->n_kept <= 0) return;
  hipLaunchKernelGGL(k_dsplit_emit, dim3((unsigned)((a->n_kept + TX_WAVES - 1) / TX_WAVES)), dim3(64 * TX_WAVES), 0, s, *a);
}

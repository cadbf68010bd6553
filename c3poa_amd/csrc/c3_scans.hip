// c3_scans.hip -- side stages that borrow the batch handle's stream: splint / adapter finders over the resident batch,
// match_index, the post-processing records (k_post), the sample demultiplexer (k_demux) and its text-in / file-bytes-out path
// (k_fasta), the main CLI's records (k_emit).
#include "c3_host.h"
#include "c3_post.h"
#include "c3_fasta.h"

// splint / strand finder (replaces the blat step of bin/preprocess.py:12-45,61-77): every read of the resident
// batch is scored against every splint on both strands with the conk kernel; out[i*n_spl*2 + s*2 + rc] =
// {max of the track, its offset, mean of the track, read length}.  assign_* picks the best candidate and
// accepts it when max >= 6 * mean (the same contrast test call_peaks applies later, bin/call_peaks.py:13) and
// max >= match*51*52/2 (a perfect 51-base match: the `matches > 50` filter of bin/preprocess.py:32).
extern "C" int c3_scan_splints(c3_handle* h, int32_t* out /* [n][n_spl][2][4] */, int16_t* assign_splint, char* assign_strand) {
  if (!h || h->n <= 0 || h->n_spl <= 0) return C3_E_STATE;
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t items = (size_t)h->n * h->n_spl * 2;
  DBuf scan;
  HIPCHK(scan.ensure(sizeof(int32_t) * 4 * items));
  HIPCHK(zero_cnt(h, &dev_cnt(h)->queue));
  ConkArgs a; memset(&a, 0, sizeof(a));
  a.b = dev_batch(h); a.sp_codes = h->d_sp_codes.as<uint8_t>(); a.sp_len = h->d_sp_len.as<int>();
  a.track = nullptr; a.info = h->d_info.as<C3Info>(); a.cnt = dev_cnt(h);
  a.match = h->cfg.conk_match; a.mismatch = h->cfg.conk_mismatch; a.penalty = h->cfg.conk_penalty;
  a.n_spl = h->n_spl; a.scan = scan.as<int32_t>();
  const int waves = (int)std::min<size_t>(items, (size_t)h->n_cus * 32);
  c3k_launch_conk(&a, h->max_spl, (waves + 3) / 4, 1, h->stream);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> tmp(4 * items);
  HIPCHK(hipMemcpyAsync(tmp.data(), scan.p, sizeof(int32_t) * 4 * items, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (out) memcpy(out, tmp.data(), sizeof(int32_t) * 4 * items);
  for (int i = 0; i < h->n; ++i) {
    int best = -1, bs = -1;
    for (int c = 0; c < h->n_spl * 2; ++c) { const int32_t* e = &tmp[((size_t)i * h->n_spl * 2 + c) * 4]; if (e[0] > bs) { bs = e[0]; best = c; } }
    // matches > 50 of bin/preprocess.py:32, as the diagonal sum of a perfect 51-base match
    const long long floor51 = (long long)h->cfg.conk_match * 51 * 52 / 2;
    bool ok = best >= 0 && bs >= floor51 && (long long)bs >= 6LL * tmp[((size_t)i * h->n_spl * 2 + best) * 4 + 2];
    if (assign_splint) assign_splint[i] = ok ? (int16_t)(best >> 1) : (int16_t)-1;
    if (assign_strand) assign_strand[i] = ok ? ((best & 1) ? '-' : '+') : '?';
  }
  return C3_E_OK;
}

// adapter finder of the post-processing step (replaces the blat call of C3POa_postprocessing.py:229-236): best local
// affine alignment of every read of the resident batch against every entry of the splint table (= the adapters,
// c3_set_splints) on both strands, traced back.  out[(i*n_ad + a)*2 + rc][12] = score, qStart, qEnd, tStart, tEnd
// (PSL conventions: query = read, forward coordinates; target = adapter, forward coordinates), matches, mismatches,
// qBaseInsert, tBaseInsert, qNumInsert, tNumInsert, read length.  score 0 = no alignment.
extern "C" int c3_scan_adapters(c3_handle* h, int32_t* out) {
  if (!h || h->n <= 0 || h->n_spl <= 0 || !out) return C3_E_STATE;
  HIPCHK(hipSetDevice(h->cfg.device));
  const size_t items = (size_t)h->n * h->n_spl * 2;
  DBuf res;
  HIPCHK(res.ensure(sizeof(int32_t) * 12 * items));
  const int rc = c3h::adapters_device(h, dev_batch(h), h->maxL, res.as<int32_t>());
  if (rc != C3_E_OK) return rc;
  HIPCHK(hipMemcpyAsync(out, res.p, sizeof(int32_t) * 12 * items, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return C3_E_OK;
}
// k_adapter over the batch b (on the device, longest read max_len) against the splint table, queued on the handle's stream:
// d_out[b.n * n_spl * 2][12] stays on the device.  The direction bytes live until the stream has run the kernel.
int c3h::adapters_device(c3_handle* h, const C3Batch& b, int64_t max_len, int32_t* d_out) {
  const size_t items = (size_t)b.n * h->n_spl * 2;
  const long long dcap = (long long)(max_len + 1) * (h->max_spl + 1) + 64;
  const int grid = (int)std::min<size_t>(items, (size_t)h->n_cus * 16);
  DBuf dd;
  HIPCHK(dd.ensure((size_t)dcap * grid));
  HIPCHK(h->d_counter.ensure(sizeof(C3Counters)));
  HIPCHK(zero_cnt(h, &dev_cnt(h)->queue));
  AdapterArgs a; memset(&a, 0, sizeof(a));
  a.b = b; a.p = dev_params(h->cfg); a.cnt = dev_cnt(h);
  a.ad_codes = h->d_sp_codes.as<uint8_t>(); a.ad_len = h->d_sp_len.as<int>(); a.n_ad = h->n_spl;
  a.D = dd.as<uint8_t>(); a.dcap = dcap; a.out = d_out;
  c3k_launch_adapter(&a, grid, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));        // (dd is freed on return)
  return C3_E_OK;
}

// match_index for a batch of pieces (C3POa_postprocessing.py:266-285): pieces = n slots of 64 bytes, lens[n] (<= 64);
// at most 16 indexes of at most 32 bases (idx_off[n_idx+1] into idx_cat); out[i] = winning index number or -1.
extern "C" int c3_match_index_batch(c3_handle* h, int n, const char* pieces, const int32_t* lens, int n_idx,
                                    const char* idx_cat, const int64_t* idx_off, int32_t* out) {
  if (!h || n <= 0 || !pieces || !lens || !idx_cat || !idx_off || !out) return C3_E_ARG;
  if (n_idx < 2) { for (int i = 0; i < n; ++i) out[i] = -1; return C3_E_OK; }      // the reference needs a runner-up
  if (n_idx > 16) return c3_fail(h, C3_E_LIMIT, "more than 16 indexes");
  for (int k = 0; k < n_idx; ++k) if (idx_off[k + 1] - idx_off[k] > 32 || idx_off[k + 1] < idx_off[k]) return c3_fail(h, C3_E_LIMIT, "index longer than 32 bases");
  for (int i = 0; i < n; ++i) if (lens[i] < 0 || lens[i] > 64) return c3_fail(h, C3_E_ARG, "piece longer than 64 bases");
  HIPCHK(hipSetDevice(h->cfg.device));
  DBuf dp, dl, di, doff, dout;
  const size_t ib = (size_t)idx_off[n_idx];
  HIPCHK(dout.ensure(sizeof(int) * (size_t)n));
  HIPCHK(dp.put(pieces, (size_t)n * 64, h->stream)); HIPCHK(dl.put(lens, sizeof(int) * (size_t)n, h->stream));
  HIPCHK(di.put(idx_cat, ib, h->stream, 16)); HIPCHK(doff.put(idx_off, sizeof(int64_t) * (size_t)(n_idx + 1), h->stream));
  c3k_launch_match_index(dp.as<char>(), dl.as<int>(), n, n_idx, di.as<char>(), doff.as<long long>(), dout.as<int>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return C3_E_OK;
}

// post-processing records (C3POa_postprocessing.py:238-398 and the PSL text): k_post over one batch.  The host statement is
// c3_post_emit_host (c3_post.cpp), which also holds the checks both share (c3_post_check_args).  Three steps on the
// handle's stream: upload + classify + scans, the stream sizes read back (the arena is sized from them), emit + download.
extern "C" int c3_post_emit(c3_handle* h, const c3_post_args* a, char* arena, int64_t cap, int64_t* stream_off, int64_t* n_kept) {
  if (!h) return C3_E_ARG;
  const double t_call = dbg_now_ms();
  int rc = c3_post_check_args("c3_post_emit", a, arena, cap, stream_off, n_kept);
  if (rc != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  HIPCHK(hipSetDevice(h->cfg.device));
  PostArgs p; memset(&p, 0, sizeof(p));
  const int S = 3 * a->n_dest + 3, n = a->n;
  const size_t sb = n ? (size_t)a->off[n] : 0, nmb = n ? (size_t)a->name_off[n] : 0, tb = sizeof(int32_t) * 24 * (size_t)n * a->n_ad;
  // every input buffer keeps 16 bytes of slack: the dword copies of k_post_emit read whole aligned dwords
  struct Up { const void* src; size_t bytes; } up[6] = {
    {a->names, nmb}, {a->name_off, sizeof(int64_t) * (n + 1)}, {a->seqs, sb}, {a->quals, a->quals ? sb : 0}, {a->off, sizeof(int64_t) * (n + 1)},
    {a->table, tb}};
  DBuf* d = h->d_post;
  for (int k = 0; k < 6; ++k) {
    HIPCHK(d[k].ensure(up[k].bytes + 16));
    if (n > 0 && up[k].bytes) HIPCHK(hipMemcpyAsync(d[k].p, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream));
  }
  p.n = n;
  p.names = d[0].as<uint8_t>(); p.name_off = d[1].as<int64_t>(); p.seqs = d[2].as<uint8_t>(); p.quals = a->quals ? d[3].as<uint8_t>() : nullptr;
  p.off = d[4].as<int64_t>(); p.table = d[5].as<int32_t>();
  std::vector<int64_t> so;
  if ((rc = c3h::post_sizes(h, a, p, so)) != C3_E_OK) return rc;
  const int64_t need = so[S];
  memcpy(stream_off, so.data(), sizeof(int64_t) * (S + 1));
  *n_kept = so[S + 1];
  h->ptm = c3_post_timing{};
  if (need > cap) return c3_fail(h, C3_E_LIMIT, "c3_post_emit: arena too small (bytes needed in stream_off[S])");
  if ((rc = c3h::post_write(h, p, need)) != C3_E_OK) return rc;
  if (need) HIPCHK(hipMemcpyAsync(arena, h->d_post[15].p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventElapsedTime(&h->ptm.ms_classify, h->ev_post[0], h->ev_post[1]));
  HIPCHK(hipEventElapsedTime(&h->ptm.ms_scan, h->ev_post[1], h->ev_post[2]));
  HIPCHK(hipEventElapsedTime(&h->ptm.ms_emit, h->ev_post[3], h->ev_post[4]));
  h->ptm.n_reads = n; h->ptm.n_kept = so[S + 1]; h->ptm.in_bytes = (int64_t)(nmb + sb * (a->quals ? 2 : 1) + tb); h->ptm.out_bytes = need;
  h->ptm.ms_call = (float)(dbg_now_ms() - t_call);
  return C3_E_OK;
}
// The first half of k_post on a batch whose arrays lie on the device (p.n, p.names, p.name_off, p.seqs, p.quals, p.off and
// p.table set by the caller): the descriptors of `a` uploaded, classify + scans, and so[S + 2] (stream starts, total, kept
// reads) read back and checked.  c3_post_emit and the text path (c3_text.hip) share it.
int c3h::post_sizes(c3_handle* h, const c3_post_args* a, PostArgs& p, std::vector<int64_t>& so) {
  for (hipEvent_t& ev : h->ev_post) if (!ev) HIPCHK(hipEventCreate(&ev));
  p.S = 3 * a->n_dest + 3;
  p.o.n_ad = a->n_ad; p.o.class5 = a->class5; p.o.undirectional = a->undirectional != 0; p.o.trim = a->trim != 0; p.o.barcoded = a->barcoded != 0;
  p.o.quals = p.quals != nullptr; p.o.has_index = a->has_index != 0; p.o.n_idx = a->has_index ? a->n_idx : 0; p.o.n_dest = a->n_dest;
  const int S = p.S, n = p.n, nb = (n + 255) / 256;
  const size_t anb = a->n_ad ? (size_t)a->ad_name_off[a->n_ad] : 0, ib = p.o.n_idx ? (size_t)a->idx_off[p.o.n_idx] : 0;
  struct Up { const void* src; size_t bytes; } up[7] = {
    {a->ad_len, sizeof(int32_t) * a->n_ad}, {a->ad_class, sizeof(int32_t) * a->n_ad}, {a->ad_names, anb},
    {a->ad_name_off, a->n_ad ? sizeof(int64_t) * (a->n_ad + 1) : 0}, {a->idx_cat, ib}, {a->idx_off, p.o.n_idx ? sizeof(int64_t) * (p.o.n_idx + 1) : 0},
    {a->idx_dest, sizeof(int32_t) * p.o.n_idx}};
  DBuf* d = h->d_post;
  for (int k = 0; k < 7; ++k) {
    HIPCHK(d[6 + k].ensure(up[k].bytes + 16));
    if (n > 0 && up[k].bytes) HIPCHK(hipMemcpyAsync(d[6 + k].p, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream));
  }
  DBuf& work = d[13]; DBuf& offs = d[14];
  // work = dec [n] | len [n][6] | roff [n][6] | bsum [nb][S + 1]
  const size_t w_dec = 0, w_len = w_dec + sizeof(C3PostDec) * n, w_roff = w_len + sizeof(int64_t) * C3_POST_REC * n, w_bsum = w_roff + sizeof(int64_t) * C3_POST_REC * n;
  HIPCHK(work.ensure(w_bsum + sizeof(long long) * (size_t)(nb + 1) * (S + 1)));
  HIPCHK(offs.ensure(sizeof(int64_t) * (S + 2)));
  p.ad_len = d[6].as<int32_t>(); p.ad_class = d[7].as<int32_t>();
  p.ad_names = d[8].as<uint8_t>(); p.ad_name_off = d[9].as<int64_t>(); p.idx_cat = d[10].as<uint8_t>(); p.idx_off = d[11].as<int64_t>();
  p.idx_dest = d[12].as<int32_t>();
  p.dec = (C3PostDec*)(work.as<uint8_t>() + w_dec); p.len = (int64_t*)(work.as<uint8_t>() + w_len); p.roff = (int64_t*)(work.as<uint8_t>() + w_roff);
  p.bsum = (long long*)(work.as<uint8_t>() + w_bsum); p.stream_off = offs.as<int64_t>();
  HIPCHK(hipEventRecord(h->ev_post[0], h->stream));
  c3k_launch_post_classify(&p, h->stream);
  HIPCHK(hipEventRecord(h->ev_post[1], h->stream));
  c3k_launch_post_scan(&p, h->stream);
  HIPCHK(hipEventRecord(h->ev_post[2], h->stream));
  HIPCHK(hipGetLastError());
  so.assign((size_t)S + 2, 0);
  HIPCHK(hipMemcpyAsync(so.data(), offs.p, sizeof(int64_t) * (S + 2), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int64_t need = 0;                                              // the sums come from lengths the rule bounds: anything else is a kernel fault
  for (int s = 0; s <= S; ++s) { if (so[s] < need) return c3_fail(h, C3_E_HIP, "k_post: stream offsets out of order"); need = so[s]; }
  if (so[0] != 0 || so[S + 1] < 0 || so[S + 1] > n) return c3_fail(h, C3_E_HIP, "k_post: header out of range");
  return C3_E_OK;
}
// The second half: the records of the batch written into d_post[15] (`need` = so[S] bytes), queued on the handle's stream.
int c3h::post_write(c3_handle* h, PostArgs& p, int64_t need) {
  DBuf& out = h->d_post[15];
  HIPCHK(out.ensure((size_t)need + 256));                         // (256: what k_bgzf may read behind a stream, c3_text.hip)
  p.arena = out.as<uint8_t>();
  HIPCHK(hipEventRecord(h->ev_post[3], h->stream));
  c3k_launch_post_emit(&p, h->stream);
  HIPCHK(hipEventRecord(h->ev_post[4], h->stream));
  HIPCHK(hipGetLastError());
  return C3_E_OK;
}
extern "C" int c3_post_emit_timing(c3_handle* h, c3_post_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->ptm;
  return C3_E_OK;
}

// meta of k_demux = Peq [I][K+1] words (bit j of Peq[k][c]: byte j of index k has code c), lengths [I] words, byte codes [256]
static std::vector<uint32_t> dmx_meta(int n_a, const char* a_cat, const int64_t* a_off, int n_b, const char* b_cat, const int64_t* b_off,
                                      const uint8_t* tab, int K1) {
  const int I = n_a + n_b;
  std::vector<uint32_t> meta((size_t)I * K1 + I + 64, 0u);
  for (int k = 0; k < I; ++k) {
    const char* cat = k < n_a ? a_cat : b_cat;
    const int64_t* off = k < n_a ? a_off + k : b_off + (k - n_a);
    const int m = (int)(off[1] - off[0]);
    for (int j = 0; j < m; ++j) meta[(size_t)k * K1 + tab[(uint8_t)cat[off[0] + j]]] |= 1u << j;
    meta[(size_t)I * K1 + k] = (uint32_t)m;
  }
  memcpy(&meta[(size_t)I * K1 + I], tab, 256);
  return meta;
}

// sample demultiplexer (paper/Demultiplex_R2C2_reads.py, demultiplex): k_demux over n heads of 300 bytes; the host
// statement is c3_demux_host (c3_index.cpp), which also holds the checks both share (c3_demux_prepare).
extern "C" int c3_demux_indexes(c3_handle* h, int n, const char* heads, int n_a, const char* a_cat, const int64_t* a_off,
                                int n_b, const char* b_cat, const int64_t* b_off, int32_t* win, uint8_t* dist) {
  if (!h) return C3_E_ARG;
  if (n < 0 || (n > 0 && (!heads || !win))) return c3_fail(h, C3_E_ARG, "heads / win missing");
  uint8_t tab[256]; int K = 0; const char* msg = "";
  const int rc = c3_demux_prepare(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, &K, &msg);
  if (rc != C3_E_OK) return c3_fail(h, rc, msg);
  if (n == 0) return C3_E_OK;
  const int I = n_a + n_b, K1 = K + 1;
  const std::vector<uint32_t> meta = dmx_meta(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, K1);
  const size_t hb = (size_t)n * C3_DEMUX_HEAD, wb = sizeof(int32_t) * 2 * (size_t)n, db = dist ? (size_t)n * I : 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(h->d_dmx_out.ensure(wb + db));
  HIPCHK(h->d_dmx_heads.put(heads, hb, h->stream)); HIPCHK(h->d_dmx_meta.put(meta.data(), sizeof(uint32_t) * meta.size(), h->stream));
  uint8_t* d_out = h->d_dmx_out.as<uint8_t>();
  c3k_launch_demux(h->d_dmx_heads.as<uint8_t>(), n, h->d_dmx_meta.as<uint8_t>(), n_a, n_b, K1, (int32_t*)d_out,
                   dist ? d_out + wb : nullptr, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(win, d_out, wb, hipMemcpyDeviceToHost, h->stream));
  if (dist) HIPCHK(hipMemcpyAsync(dist, d_out + wb, db, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));      // meta is a host vector of this frame
  return C3_E_OK;
}

// ---- FASTA text parsed, demultiplexed and formatted on the device (k_fasta.hip; host statements c3_fasta.cpp) ----
// One parse = two waits: the terminator count (sizes nl[] and the line and record tables), the header (sizes the arenas and
// answers the capacity question before any byte is gathered).  c3_demux_emit waits once more for the output size.
using namespace c3h::fa;                         // FA_TEXT .. FA_N: the slots of c3_handle::d_fa (c3_host.h)
static_assert(FA_N <= sizeof(c3_handle::d_fa) / sizeof(DBuf), "c3_handle::d_fa is too short");

static int fa_read_hdr(c3_handle* h) {
  HIPCHK(hipMemcpyAsync(h->h_fa_hdr, h->d_fa[FA_HDR].p, sizeof(C3FaHdr), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return C3_E_OK;
}

// the text (n > 0) uploaded and parsed (c3h::fasta_parse_resident)
static int fa_parse_device(c3_handle* h, const char* text, int64_t n, int at_eof, int kept, FaArgs* a) {
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(h->d_fa[FA_TEXT].ensure((size_t)n + 256));
  HIPCHK(hipMemcpyAsync(h->d_fa[FA_TEXT].p, text, (size_t)n, hipMemcpyHostToDevice, h->stream));
  return c3h::fasta_parse_resident(h, h->d_fa[FA_TEXT].as<uint8_t>(), n, at_eof, kept, a);
}

// The text d_text[0, n) (n > 0; on the device, queued on h->stream, 256-aligned with 256 bytes of slack behind it) parsed: line and
// record tables and the header on the device and in h->h_fa_hdr; no byte gathered yet.  kept: krec[] and n_kept as well.
int c3h::fasta_parse_resident(c3_handle* h, const uint8_t* d_text, int64_t n, int at_eof, int kept, FaArgs* a) {
  memset(a, 0, sizeof *a);
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->h_fa_hdr) HIPCHK(hipHostMalloc((void**)&h->h_fa_hdr, sizeof(C3FaHdr), hipHostMallocDefault));
  for (hipEvent_t& ev : h->ev_fa) if (!ev) HIPCHK(hipEventCreate(&ev));
  DBuf* d = h->d_fa;
  const size_t tiles = ((size_t)n + 65535) / 65536;
  HIPCHK(d[FA_HDR].ensure(sizeof(C3FaHdr))); HIPCHK(d[FA_CNT].ensure(tiles * 4 * sizeof(int32_t)));
  HIPCHK(hipMemsetAsync(d[FA_HDR].p, 0xFF, 12, h->stream));           // first_high, first_headless: none; rec_of_high: -1
  a->buf = d_text; a->hi = (uint32_t)n; a->at_eof = at_eof ? 1 : 0;
  a->cnt = d[FA_CNT].as<int32_t>(); a->hdr = d[FA_HDR].as<C3FaHdr>();
  HIPCHK(hipEventRecord(h->ev_fa[0], h->stream));
  c3k_launch_fasta_count(a, h->stream);
  HIPCHK(hipEventRecord(h->ev_fa[1], h->stream));
  HIPCHK(hipGetLastError());
  int rc = fa_read_hdr(h);
  if (rc) return rc;
  const int64_t T = h->h_fa_hdr->n_term;
  if (T < 0 || T > n) return c3_fail(h, C3_E_HIP, "k_fasta: terminator count out of range");
  const size_t nl = (size_t)T + 1, nb = (nl + 255) / 256;
  HIPCHK(d[FA_NL].ensure((nl + 4) * sizeof(int32_t))); HIPCHK(d[FA_LSE].ensure((nl + 1) * sizeof(int32_t))); HIPCHK(d[FA_LDST].ensure((nl + 1) * sizeof(uint32_t)));
  HIPCHK(d[FA_BSUM].ensure((nb + 1) * 3 * sizeof(long long)));
  HIPCHK(d[FA_OFF].ensure((nl + 2) * sizeof(int64_t))); HIPCHK(d[FA_NOFF].ensure((nl + 2) * sizeof(int64_t)));
  HIPCHK(d[FA_RECL].ensure((nl + 2) * sizeof(int32_t))); HIPCHK(d[FA_HASH].ensure((nl + 2) * sizeof(uint64_t)));
  if (kept) HIPCHK(d[FA_KREC].ensure((nl + 2) * sizeof(int32_t)));
  a->nl = d[FA_NL].as<int32_t>(); a->T = (int32_t)T; a->lse = d[FA_LSE].as<int32_t>(); a->ldst = d[FA_LDST].as<uint32_t>();
  a->bsum = d[FA_BSUM].as<long long>(); a->off = d[FA_OFF].as<int64_t>(); a->name_off = d[FA_NOFF].as<int64_t>();
  a->rec_line = d[FA_RECL].as<int32_t>(); a->hash = d[FA_HASH].as<uint64_t>(); a->krec = d[FA_KREC].as<int32_t>();
  HIPCHK(hipEventRecord(h->ev_fa[2], h->stream));
  c3k_launch_fasta_records(a, kept, h->stream);
  HIPCHK(hipEventRecord(h->ev_fa[3], h->stream));
  HIPCHK(hipGetLastError());
  if ((rc = fa_read_hdr(h)) != C3_E_OK) return rc;
  const C3FaHdr& f = *h->h_fa_hdr;
  if (f.n_headers < 0 || f.n_headers > (int64_t)nl || f.n_records < 0 || f.n_records > f.n_headers || f.consumed < 0 || f.consumed > n ||
      f.name_bytes < 0 || f.name_bytes > n || f.base_bytes < 0 || f.base_bytes > n || f.departed < 0 || f.departed > 2 ||
      f.n_kept < 0 || f.n_kept > f.n_records)
    return c3_fail(h, C3_E_HIP, "k_fasta: header out of range");
  a->n_records = f.n_records; a->n_kept = f.n_kept;
  return C3_E_OK;
}

// names and sequences of the delivered records gathered into the arenas (queued, not waited for)
int c3h::fasta_gather_resident(c3_handle* h, FaArgs* a) {
  const C3FaHdr& f = *h->h_fa_hdr;
  HIPCHK(h->d_fa[FA_NAMES].ensure((size_t)f.name_bytes + 256)); HIPCHK(h->d_fa[FA_SEQS].ensure((size_t)f.base_bytes + 256));
  a->names = h->d_fa[FA_NAMES].as<uint8_t>(); a->seqs = h->d_fa[FA_SEQS].as<uint8_t>();
  c3k_launch_fasta_gather(a, h->stream);
  HIPCHK(hipGetLastError());
  return C3_E_OK;
}

extern "C" int c3_fasta_parse(c3_handle* h, const char* text, int64_t n, int at_eof, char* names, int64_t names_cap, int64_t* name_off,
                              char* seqs, int64_t bases_cap, int64_t* off, uint64_t* name_hash, int64_t max_records, c3_fasta_info* info) {
  int rc = c3_fasta_check_args("c3_fasta_parse", text, n, names, names_cap, name_off, seqs, bases_cap, off, name_hash, max_records, info);
  if (!h) return rc ? rc : host_fail(C3_E_ARG, "c3_fasta_parse: null handle");
  if (rc) return c3_fail(h, rc, c3_last_error(nullptr));
  if (n == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  FaArgs a;
  if ((rc = fa_parse_device(h, text, n, at_eof, 0, &a)) != C3_E_OK) return rc;
  const C3FaHdr& f = *h->h_fa_hdr;
  info->n_records = f.n_records; info->consumed = f.consumed; info->name_bytes = f.name_bytes; info->base_bytes = f.base_bytes; info->departed = f.departed;
  if (f.n_records > max_records || f.name_bytes > names_cap || f.base_bytes > bases_cap)
    return c3_fail(h, C3_E_LIMIT, "c3_fasta_parse: capacity too small (needed sizes in info)");
  if (f.n_records == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  if ((rc = c3h::fasta_gather_resident(h, &a)) != C3_E_OK) return rc;
  const size_t R = (size_t)f.n_records;
  HIPCHK(hipMemcpyAsync(off, a.off, (R + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(name_off, a.name_off, (R + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(name_hash, a.hash, R * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  if (f.name_bytes) HIPCHK(hipMemcpyAsync(names, a.names, (size_t)f.name_bytes, hipMemcpyDeviceToHost, h->stream));
  if (f.base_bytes) HIPCHK(hipMemcpyAsync(seqs, a.seqs, (size_t)f.base_bytes, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  return C3_E_OK;
}

// the index sets of a search over nk kept records on the device: k_demux's meta (kept in the handle until the next call, so the
// upload needs no wait), the index names and their offsets, room for the heads and the winners; a's pointers to them filled
int c3h::demux_sets_device(c3_handle* h, const c3_demux_sets* st, const uint8_t* tab, int K, int64_t nk, FaArgs* a) {
  DBuf* d = h->d_fa;
  h->dmx_meta_host = dmx_meta(st->n_a, st->a_cat, st->a_off, st->n_b, st->b_cat, st->b_off, tab, K + 1);
  const size_t anb = (size_t)st->a_name_off[st->n_a], bnb = (size_t)st->b_name_off[st->n_b];
  HIPCHK(h->d_dmx_heads.ensure((size_t)nk * C3_DEMUX_HEAD + 16)); HIPCHK(h->d_dmx_out.ensure(sizeof(int32_t) * 2 * (size_t)nk));
  HIPCHK(h->d_dmx_meta.put(h->dmx_meta_host.data(), sizeof(uint32_t) * h->dmx_meta_host.size(), h->stream));
  HIPCHK(d[FA_ANAMES].ensure(anb + 16)); HIPCHK(d[FA_BNAMES].ensure(bnb + 16));
  if (anb) HIPCHK(hipMemcpyAsync(d[FA_ANAMES].p, st->a_names, anb, hipMemcpyHostToDevice, h->stream));
  if (bnb) HIPCHK(hipMemcpyAsync(d[FA_BNAMES].p, st->b_names, bnb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(d[FA_ANO].put(st->a_name_off, sizeof(int64_t) * (size_t)(st->n_a + 1), h->stream)); HIPCHK(d[FA_BNO].put(st->b_name_off, sizeof(int64_t) * (size_t)(st->n_b + 1), h->stream));
  a->heads = h->d_dmx_heads.as<uint8_t>(); a->win = h->d_dmx_out.as<int32_t>();
  a->a_names = d[FA_ANAMES].as<uint8_t>(); a->a_no = d[FA_ANO].as<int64_t>(); a->b_names = d[FA_BNAMES].as<uint8_t>(); a->b_no = d[FA_BNO].as<int64_t>();
  return C3_E_OK;
}

extern "C" int c3_demux_emit(c3_handle* h, const char* text, int64_t n, int at_eof,
                             int n_a, const char* a_cat, const int64_t* a_off, const char* a_names, const int64_t* a_name_off,
                             int n_b, const char* b_cat, const int64_t* b_off, const char* b_names, const int64_t* b_name_off,
                             char* out, int64_t cap, uint64_t* name_hash, int64_t max_records, c3_demux_info* info) {
  const double t_call = dbg_now_ms();
  int rc = c3_demux_emit_check_args("c3_demux_emit", text, n, n_a, a_names, a_name_off, n_b, b_names, b_name_off, out, cap, name_hash, max_records, info);
  if (!h) return rc ? rc : host_fail(C3_E_ARG, "c3_demux_emit: null handle");
  if (rc) return c3_fail(h, rc, c3_last_error(nullptr));
  uint8_t tab[256]; int K = 0; const char* msg = "";
  if ((rc = c3_demux_prepare(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, &K, &msg)) != C3_E_OK) return c3_fail(h, rc, msg);
  h->dtm = c3_demux_timing{};
  if (n == 0) return C3_E_OK;
  FaArgs a;
  if ((rc = fa_parse_device(h, text, n, at_eof, 1, &a)) != C3_E_OK) return rc;
  const C3FaHdr& f = *h->h_fa_hdr;
  const int64_t R = f.n_records, nk = f.n_kept;
  info->n_records = R; info->n_kept = nk; info->consumed = f.consumed; info->departed = f.departed;
  if (R > max_records) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit: more records than max_records (needed sizes in info)");
  if (nk > INT32_MAX) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit: too many records in one text");
  float ms[5] = {0, 0, 0, 0, 0};
  if (nk > 0) {
    DBuf* d = h->d_fa;
    const int K1 = K + 1;
    const c3_demux_sets st = {n_a, a_cat, a_off, a_names, a_name_off, n_b, b_cat, b_off, b_names, b_name_off};
    if ((rc = c3h::demux_sets_device(h, &st, tab, K, nk, &a)) != C3_E_OK) return rc;
    const size_t anb = (size_t)a_name_off[n_a], bnb = (size_t)b_name_off[n_b];
    HIPCHK(d[FA_ROFF].ensure(sizeof(int64_t) * ((size_t)nk + 1)));
    a.roff = d[FA_ROFF].as<int64_t>();
    HIPCHK(hipEventRecord(h->ev_fa[4], h->stream));
    if ((rc = c3h::fasta_gather_resident(h, &a)) != C3_E_OK) return rc;
    c3k_launch_demux_heads(&a, h->stream);
    HIPCHK(hipEventRecord(h->ev_fa[5], h->stream));
    c3k_launch_demux(a.heads, (int)nk, h->d_dmx_meta.as<uint8_t>(), n_a, n_b, K1, h->d_dmx_out.as<int32_t>(), nullptr, h->stream);
    HIPCHK(hipEventRecord(h->ev_fa[6], h->stream));
    c3k_launch_demux_len(&a, h->stream);
    HIPCHK(hipEventRecord(h->ev_fa[7], h->stream));
    HIPCHK(hipGetLastError());
    if ((rc = fa_read_hdr(h)) != C3_E_OK) return rc;
    const int64_t need = f.out_bytes;
    // a record is at least its five literals and 301 sequence bytes, at most everything the text holds plus two index names
    if (need < nk * (C3_DEMUX_HEAD + 6) || need > n + nk * (int64_t)(5 + anb + bnb)) return c3_fail(h, C3_E_HIP, "k_fasta: output size out of range");
    info->out_bytes = need;
    if (need > cap) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit: out too small (bytes needed in info)");
    HIPCHK(d[FA_OUT].ensure((size_t)need + 16));
    a.out = d[FA_OUT].as<uint8_t>();
    HIPCHK(hipEventRecord(h->ev_fa[8], h->stream));
    c3k_launch_demux_emit(&a, h->stream);
    HIPCHK(hipEventRecord(h->ev_fa[9], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, a.out, (size_t)need, hipMemcpyDeviceToHost, h->stream));
  }
  if (R > 0) HIPCHK(hipMemcpyAsync(name_hash, a.hash, (size_t)R * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  float t01, t23;
  HIPCHK(hipEventElapsedTime(&t01, h->ev_fa[0], h->ev_fa[1])); HIPCHK(hipEventElapsedTime(&t23, h->ev_fa[2], h->ev_fa[3]));
  if (nk > 0) {
    HIPCHK(hipEventElapsedTime(&ms[0], h->ev_fa[4], h->ev_fa[5])); HIPCHK(hipEventElapsedTime(&ms[1], h->ev_fa[5], h->ev_fa[6]));
    HIPCHK(hipEventElapsedTime(&ms[2], h->ev_fa[6], h->ev_fa[7])); HIPCHK(hipEventElapsedTime(&ms[3], h->ev_fa[8], h->ev_fa[9]));
  }
  h->dtm.ms_parse = t01 + t23 + ms[0]; h->dtm.ms_demux = ms[1]; h->dtm.ms_emit = ms[2] + ms[3];
  h->dtm.n_records = R; h->dtm.n_kept = nk; h->dtm.in_bytes = n; h->dtm.out_bytes = info->out_bytes;
  h->dtm.ms_call = (float)(dbg_now_ms() - t_call);
  return C3_E_OK;
}
extern "C" int c3_demux_emit_timing(c3_handle* h, c3_demux_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->dtm;
  return C3_E_OK;
}

// ---- the main CLI's records (k_emit.hip; host statement and shared checks: c3_emit.cpp; the rule: c3_emit.h) ------------------
// The three steps of one formatting on stream s, all pointers of p on the device: lengths + scans, the stream sizes read back
// (so[S * K + 2]: starts, total, records; the arena is sized from them), the write pass.  cap >= 0: C3_E_LIMIT without the
// write pass when the streams need more.  Serves c3_emit_group (below) and c3_batch_emit_snapshot (c3_handle.hip).
int c3h::emit_run(c3_handle* h, EmitArgs& p, EmitBufs& eb, hipStream_t s, std::vector<int64_t>& so, int64_t cap) {
  for (hipEvent_t& ev : eb.ev) if (!ev) HIPCHK(hipEventCreate(&ev));
  const int n = p.n, SK = p.n_splints * p.K, nb = (n + 255) / 256;
  // work = head [n] | len [n][3] | roff [n][3] | bsum [nb][SK + 1]
  const size_t w_len = sizeof(EmitHead) * (size_t)n, w_roff = w_len + sizeof(int64_t) * C3_EMIT_KINDS * (size_t)n;
  const size_t w_bsum = w_roff + sizeof(int64_t) * C3_EMIT_KINDS * (size_t)n;
  static_assert(sizeof(EmitHead) % 8 == 0, "the arrays behind head[] hold 64-bit entries");
  HIPCHK(eb.work.ensure(w_bsum + sizeof(long long) * (size_t)(nb + 1) * (SK + 1)));
  HIPCHK(eb.offs.ensure(sizeof(int64_t) * (SK + 2)));
  uint8_t* w = eb.work.as<uint8_t>();
  p.head = (EmitHead*)w; p.len = (int64_t*)(w + w_len); p.roff = (int64_t*)(w + w_roff); p.bsum = (long long*)(w + w_bsum);
  p.stream_off = eb.offs.as<int64_t>(); p.arena = nullptr;
  HIPCHK(hipEventRecord(eb.ev[0], s));
  if (p.bam) c3k_launch_bamout_len(&p, s); else c3k_launch_emit_len(&p, s);
  HIPCHK(hipEventRecord(eb.ev[1], s));
  c3k_launch_emit_scan(&p, s);
  HIPCHK(hipEventRecord(eb.ev[2], s));
  HIPCHK(hipGetLastError());
  so.assign((size_t)SK + 2, 0);
  HIPCHK(hipMemcpyAsync(so.data(), eb.offs.p, sizeof(int64_t) * (SK + 2), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int64_t need = 0;                                              // the sums come from lengths the rule bounds: anything else is a kernel fault
  for (int x = 0; x <= SK; ++x) { if (so[x] < need) return c3_fail(h, C3_E_HIP, "k_emit: stream offsets out of order"); need = so[x]; }
  if (so[0] != 0 || so[SK + 1] < 0 || so[SK + 1] > (int64_t)n * (C3_EMIT_MAX_SUB + 4)) return c3_fail(h, C3_E_HIP, "k_emit: header out of range");
  if (cap >= 0 && need > cap) return C3_E_LIMIT;
  HIPCHK(eb.arena.ensure((size_t)need + 256));                  // (256: what k_bgzf may read behind a chunk, c3_batch_emit_fetch)
  p.arena = eb.arena.as<uint8_t>();
  HIPCHK(hipEventRecord(eb.ev[3], s));
  if (p.bam) c3k_launch_bamout_write(&p, s); else c3k_launch_emit_write(&p, s);
  HIPCHK(hipEventRecord(eb.ev[4], s));
  HIPCHK(hipGetLastError());
  return C3_E_OK;
}

// the stand-alone call: three steps on the handle's stream: upload + lengths + scans, the stream sizes read back, write + download
// (bam: the records of c3_emit_group_bam, K = 2 whatever qv is; who: the call's name in its error texts)
static int emit_group(c3_handle* h, const char* who, int bam, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                      const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                      int64_t* stream_off, int64_t* n_records) {
  if (!h) return C3_E_ARG;
  const double t_call = dbg_now_ms();
  int rc = c3_emit_check_args(who, b, res, cons, cons_off, qv, splint_id, n_splints, zero, arena, cap, stream_off, n_records);
  if (rc == C3_E_OK && bam) rc = c3_bamout_check_names(who, b->names, b->name_off, b->n);
  if (rc != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  HIPCHK(hipSetDevice(h->cfg.device));
  const int n = b->n, K = qv && !bam ? 3 : 2, SK = n_splints * K;
  h->etm = c3_emit_timing{};
  if (n == 0) { for (int x = 0; x <= SK; ++x) stream_off[x] = 0; *n_records = 0; return C3_E_OK; }
  const size_t sb = (size_t)b->off[n], nmb = (size_t)b->name_off[n], cb = cons ? (size_t)cons_off[n] : 0, ob = sizeof(int64_t) * (size_t)(n + 1);
  // every input buffer keeps 16 bytes of slack, as k_post's
  struct Up { const void* src; size_t bytes; } up[10] = {
    {b->names, nmb}, {b->name_off, ob}, {b->seqs, sb}, {b->quals, sb}, {b->off, ob}, {res, sizeof(c3_read_result) * (size_t)n},
    {splint_id, sizeof(int16_t) * (size_t)n}, {cons, cb}, {qv, qv ? cb : 0}, {cons_off, cons ? ob : 0}};
  DBuf* d = h->d_emit;
  for (int k = 0; k < 10; ++k) {
    HIPCHK(d[k].ensure(up[k].bytes + 16));
    if (up[k].bytes) HIPCHK(hipMemcpyAsync(d[k].p, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream));
  }
  EmitArgs p; memset(&p, 0, sizeof(p));
  p.n = n; p.n_splints = n_splints; p.K = K; p.zero = zero; p.bam = bam;
  p.names = d[0].as<uint8_t>(); p.name_off = d[1].as<int64_t>(); p.seqs = d[2].as<uint8_t>(); p.quals = d[3].as<uint8_t>(); p.off = d[4].as<int64_t>();
  p.info = d[5].as<c3_read_result>(); p.sid = d[6].as<int16_t>();
  p.cons = cons ? d[7].as<uint8_t>() : nullptr; p.qv = qv ? d[8].as<uint8_t>() : nullptr;
  p.cons_at = d[9].as<int64_t>(); p.cons_off = cons ? d[9].as<int64_t>() : nullptr;
  std::vector<int64_t> so;
  c3h::EmitBufs& eb = h->emit_sa;
  const int rr = c3h::emit_run(h, p, eb, h->stream, so, cap);
  if (rr != C3_E_OK && rr != C3_E_LIMIT) return rr;
  memcpy(stream_off, so.data(), sizeof(int64_t) * (SK + 1));
  *n_records = so[SK + 1];
  if (rr == C3_E_LIMIT) return c3_fail(h, C3_E_LIMIT, (std::string(who) + ": arena too small (bytes needed in stream_off[S])").c_str());
  const int64_t need = so[SK];
  if (need) HIPCHK(hipMemcpyAsync(arena, eb.arena.p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventElapsedTime(&h->etm.ms_len, eb.ev[0], eb.ev[1]));
  HIPCHK(hipEventElapsedTime(&h->etm.ms_scan, eb.ev[1], eb.ev[2]));
  HIPCHK(hipEventElapsedTime(&h->etm.ms_write, eb.ev[3], eb.ev[4]));
  h->etm.n_reads = n; h->etm.n_records = so[SK + 1]; h->etm.in_bytes = (int64_t)(nmb + 2 * sb + cb * (qv ? 2 : 1)); h->etm.out_bytes = need;
  h->etm.ms_call = (float)(dbg_now_ms() - t_call);
  return C3_E_OK;
}
extern "C" int c3_emit_group(c3_handle* h, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                             const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                             int64_t* stream_off, int64_t* n_records) {
  return emit_group(h, "c3_emit_group", 0, b, res, cons, cons_off, qv, splint_id, n_splints, zero, arena, cap, stream_off, n_records);
}
// the same group as unaligned BAM records (k_bamout.hip; host statement: c3_bamout.cpp)
extern "C" int c3_emit_group_bam(c3_handle* h, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                                 const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                                 int64_t* stream_off, int64_t* n_records) {
  return emit_group(h, "c3_emit_group_bam", 1, b, res, cons, cons_off, qv, splint_id, n_splints, zero, arena, cap, stream_off, n_records);
}
extern "C" int c3_emit_timing_get(c3_handle* h, c3_emit_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->etm;
  return C3_E_OK;
}

// c3_dtext.hip -- the text path of the sample demultiplexer (include/c3poa.h "Sample demultiplexer, pieces of text in /
// per-sample streams out"): pieces of a read file in, the renamed records out as one stream or one per sample,
// everything in between on the device.
//   text   = the shared text front's load (c3_tfront.hip)
//   parse  = kind 4: the front's tables and gather, then k_dsplit_krec for the kept records;
//            kind 2: k_fasta on the resident text (c3h::fasta_parse_resident / fasta_gather_resident, shared with c3_demux_emit)
//   search = k_demux_heads, k_demux (index sets by c3h::demux_sets_device)
//   place  = k_dsplit_key / _tile / _cols / _offs: stream_off[] and every record's place; format = k_dsplit_emit;
//            k_bgzf per non-empty stream when asked (c3h::bgzf_stream_device)
// Waits of a call: line count and parse header (kind 4) or terminator count and header (kind 2), the kept count (kind 4), the
// stream sizes, the delivery; two more per compressed chunk.  Every refusal leaves the handle's text as it was: the front's
// commit is the last thing a call does.
#include "c3_host.h"

void c3h::demux_text_free(c3_handle* h) {
  DemuxText& t = h->dx;
  if (t.h_soff) (void)hipHostFree(t.h_soff);
  t.h_soff = nullptr;
  for (hipEvent_t ev : t.ev) if (ev) (void)hipEventDestroy(ev);
  text_free(t);
}

extern "C" int c3_demux_text_reset(c3_handle* h) {
  if (!h) return C3_E_ARG;
  c3h::text_reset(h->dx);
  return C3_E_OK;
}

extern "C" int c3_demux_text_timing_get(c3_handle* h, c3_demux_text_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->dx.tm;
  return C3_E_OK;
}

extern "C" int c3_demux_emit_text(c3_handle* h, const char* src, int64_t n, int at_eof, int flags, const c3_demux_sets* sets,
                                  char* arena, int64_t cap, int64_t* stream_off, uint64_t* name_hash, int64_t max_records,
                                  c3_demux_text_info* info) {
  const double t_call = dbg_now_ms();
  uint8_t tab[256]; int K = 0, S = 0;
  int rc = c3_demux_text_check_args("c3_demux_emit_text", src, n, flags, sets, arena, cap, stream_off, name_hash, max_records, info, &S, tab, &K);
  if (!h) return rc ? rc : host_fail(C3_E_ARG, "c3_demux_emit_text: null handle");
  if (rc) return c3_fail(h, rc, c3_last_error(nullptr));
  const bool in_z = (flags & C3_DEMUX_IN_BGZF) != 0, out_z = (flags & C3_DEMUX_OUT_BGZF) != 0, keep_q = (flags & C3_DEMUX_KEEP_QUALS) != 0;
  const int split = (flags & C3_DEMUX_SPLIT) ? 1 : 0;
  DemuxText& t = h->dx;
  c3h::TextLoad ld;
  if ((rc = c3h::text_load(h, t, src, n, in_z, keep_q, "c3_demux_emit_text", "C3_DEMUX_KEEP_QUALS", t.ev, 6, &ld)) != C3_E_OK) return rc;
  if (!t.h_soff) HIPCHK(hipHostMalloc((void**)&t.h_soff, (C3_DEMUX_MAX_STREAMS + 2) * sizeof(int64_t), hipHostMallocDefault));
  const int64_t total = ld.total;
  const int kind = ld.kind;
  DBuf& text = t.text[ld.nxt];
  t.tm = c3_demux_text_timing{};
  t.tm.n_streams = S; t.tm.in_bytes = n; t.tm.text_bytes = total; t.tm.ms_inflate = ld.ms_inflate;
  for (int s = 0; s <= S; ++s) stream_off[s] = 0;
  info->text_bytes = total; info->kind = kind;
  int waits = ld.waits;
  auto wait = [&]() { ++waits; return hipStreamSynchronize(h->stream); };
  auto commit = [&](int64_t consumed) {
    c3h::text_commit(t, ld, consumed, at_eof);
    t.tm.n_waits = waits; t.tm.ms_call = (float)(dbg_now_ms() - t_call);
  };
  if (total == 0) { HIPCHK(wait()); commit(0); return C3_E_OK; }
  if (!kind) { HIPCHK(wait()); info->departed = 1; commit(0); return C3_E_OK; }      // neither '>' nor '@'

  // ---- parse: the records' tables, then (R known to fit) the gather and the kept records ----
  DsArgs p; memset(&p, 0, sizeof p);
  FaArgs fa; memset(&fa, 0, sizeof fa);
  FxArgs f; memset(&f, 0, sizeof f);
  int64_t R = 0, nk = 0, consumed = 0;
  const uint64_t* d_hash = nullptr;
  HIPCHK(hipEventRecord(t.ev[0], h->stream));
  if (kind == 2) {
    if ((rc = c3h::fasta_parse_resident(h, text.as<uint8_t>(), total, at_eof, 1, &fa)) != C3_E_OK) return rc;
    waits += 2;
    const C3FaHdr& x = *h->h_fa_hdr;
    R = x.n_records; nk = x.n_kept; consumed = x.consumed; info->departed = x.departed;
    d_hash = fa.hash;
  } else {
    if ((rc = c3h::text_tables(h, t, ld, at_eof, f, &waits)) != C3_E_OK) return rc;
    const C3FxHdr& x = *t.h_hdr;
    R = x.n_records; consumed = x.consumed; info->departed = x.departed;
    d_hash = f.hash;
  }
  info->n_records = R; info->consumed = consumed;
  t.tm.n_records = R;
  if (R > max_records) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit_text: more records than max_records (the need in info)");
  if (R == 0) { HIPCHK(wait()); commit(consumed); return C3_E_OK; }
  if (kind == 2) {
    if (nk > 0) {
      if ((rc = c3h::fasta_gather_resident(h, &fa)) != C3_E_OK) return rc;
      p.off = fa.off; p.name_off = fa.name_off; p.names = fa.names; p.seqs = fa.seqs; p.quals = nullptr; p.krec = fa.krec;
    }
  } else {
    if ((rc = c3h::text_gather(h, t, f, keep_q)) != C3_E_OK) return rc;
    HIPCHK(t.krec.ensure(((size_t)R + 1) * sizeof(int32_t))); HIPCHK(t.kb.ensure((((size_t)R + 255) / 256 + 1) * sizeof(long long)));
    HIPCHK(t.nkept.ensure(sizeof(long long)));
    p.n_records = R; p.off = f.off; p.name_off = f.name_off; p.names = f.names; p.seqs = f.seqs; p.quals = f.quals;
    p.krec = t.krec.as<int32_t>(); p.bsum = t.kb.as<long long>(); p.n_kept_out = t.nkept.as<long long>();
    c3k_launch_dsplit_krec(&p, h->stream);
    HIPCHK(hipGetLastError());
    long long nk_dev = -1;
    HIPCHK(hipMemcpyAsync(&nk_dev, t.nkept.p, sizeof nk_dev, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(wait());
    if (nk_dev < 0 || nk_dev > R) return c3_fail(h, C3_E_HIP, "k_dsplit: kept count out of range");
    nk = nk_dev;
    fa.seqs = t.seqs.as<uint8_t>(); fa.off = f.off; fa.krec = p.krec;      // what k_demux_heads reads
  }
  HIPCHK(hipEventRecord(t.ev[1], h->stream));
  if (nk > INT32_MAX) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit_text: too many records in one text");
  t.tm.n_kept = nk;

  // ---- search and place ----
  int64_t* so = t.h_soff;                                          // plain stream offsets [S + 1]
  for (int s = 0; s <= S; ++s) so[s] = 0;
  const int64_t anb = sets->a_name_off[sets->n_a], bnb = sets->b_name_off[sets->n_b];
  if (nk > 0) {
    fa.n_kept = nk;
    if ((rc = c3h::demux_sets_device(h, sets, tab, K, nk, &fa)) != C3_E_OK) return rc;
    c3k_launch_demux_heads(&fa, h->stream);
    c3k_launch_demux(fa.heads, (int)nk, h->d_dmx_meta.as<uint8_t>(), sets->n_a, sets->n_b, K + 1, h->d_dmx_out.as<int32_t>(), nullptr, h->stream);
    HIPCHK(hipEventRecord(t.ev[2], h->stream));
    const int64_t tiles = (nk + C3_DS_TILE - 1) / C3_DS_TILE;
    HIPCHK(t.key.ensure((size_t)nk * sizeof(int32_t))); HIPCHK(t.rank.ensure((size_t)nk * sizeof(int64_t)));
    HIPCHK(t.base.ensure((size_t)tiles * S * sizeof(int64_t))); HIPCHK(t.soff.ensure(((size_t)S + 1) * sizeof(int64_t)));
    HIPCHK(hipMemsetAsync(t.base.p, 0, (size_t)tiles * S * sizeof(int64_t), h->stream));
    p.n_kept = nk; p.win = fa.win; p.n_a = sets->n_a; p.n_b = sets->n_b; p.split = split; p.S = S;
    p.a_names = fa.a_names; p.a_no = fa.a_no; p.b_names = fa.b_names; p.b_no = fa.b_no;
    p.key = t.key.as<int32_t>(); p.rank = t.rank.as<int64_t>(); p.base = t.base.as<int64_t>(); p.tiles = (int32_t)tiles;
    p.stream_off = t.soff.as<int64_t>();
    c3k_launch_dsplit_place(&p, h->stream);
    HIPCHK(hipEventRecord(t.ev[3], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(so, t.soff.p, ((size_t)S + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(wait());
    // a record is at least its five literals and 301 sequence bytes, at most twice what the text holds plus three literals and two index names
    bool ok = so[0] == 0 && so[S] >= nk * (C3_DEMUX_HEAD + 6) && so[S] <= 2 * total + nk * (8 + anb + bnb);
    for (int s = 0; s < S && ok; ++s) ok = so[s + 1] >= so[s];
    if (!ok) return c3_fail(h, C3_E_HIP, "k_dsplit: stream sizes out of range");
  }
  int64_t need = 0;
  for (int s = 0; s < S; ++s) { stream_off[s] = need; const int64_t len = so[s + 1] - so[s]; need += (out_z && len) ? c3_bgzf_bound(len) : len; }
  stream_off[S] = need;
  info->n_kept = nk; info->out_bytes = need;
  if (need > cap) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit_text: arena too small (bytes needed in stream_off[S])");

  // ---- format and deliver ----
  int64_t out = 0;
  if (nk > 0) {
    HIPCHK(t.out.ensure((size_t)so[S] + 16));
    p.out = t.out.as<uint8_t>();
    HIPCHK(hipEventRecord(t.ev[4], h->stream));
    c3k_launch_dsplit_emit(&p, h->stream);
    HIPCHK(hipEventRecord(t.ev[5], h->stream));
    HIPCHK(hipGetLastError());
    if (!out_z) {
      HIPCHK(hipMemcpyAsync(arena, t.out.p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
      out = need;
    } else {
      const double t_z = dbg_now_ms();
      for (int s = 0; s < S; ++s) {
        stream_off[s] = out;
        const int64_t len = so[s + 1] - so[s];
        if (!len) continue;
        if ((rc = c3h::bgzf_stream_device(h, t.zs, t.out.as<char>() + so[s], len, arena, cap, &out, &waits)) != C3_E_OK) return rc;
      }
      stream_off[S] = out;
      t.tm.ms_bgzf = (float)(dbg_now_ms() - t_z);
    }
  }
  HIPCHK(hipMemcpyAsync(name_hash, d_hash, (size_t)R * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(wait());
  info->out_bytes = out;
  HIPCHK(hipEventElapsedTime(&t.tm.ms_parse, t.ev[0], t.ev[1]));
  if (nk > 0) {
    HIPCHK(hipEventElapsedTime(&t.tm.ms_demux, t.ev[1], t.ev[2])); HIPCHK(hipEventElapsedTime(&t.tm.ms_split, t.ev[2], t.ev[3]));
    HIPCHK(hipEventElapsedTime(&t.tm.ms_emit, t.ev[4], t.ev[5]));
  }
  t.tm.out_bytes = out;
  commit(consumed);
  return C3_E_OK;
}

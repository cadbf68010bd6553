// c3_dtext.hip -- the text path of the sample demultiplexer (include/c3poa.h "Sample demultiplexer, pieces of text in /
// per-sample streams out"): pieces of a read file in, the renamed records out as one stream or one per sample,
// everything in between on the device.
//   text   = the kept tail (device to device) + the piece (copied up, or its BGZF members inflated by k_inflate in place)
//   parse  = kind 4: k_fastq_count / _lines, k_fastx (as c3_text.hip drives them), then k_dsplit_krec for the kept records;
//            kind 2: k_fasta on the resident text (c3h::fasta_parse_resident / fasta_gather_resident, shared with c3_demux_emit)
//   search = k_demux_heads, k_demux (index sets by c3h::demux_sets_device)
//   place  = k_dsplit_key / _tile / _cols / _offs: stream_off[] and every record's place; format = k_dsplit_emit;
//            k_bgzf per non-empty stream when asked (c3h::bgzf_stream_device)
// Waits of a call: line count and parse header (kind 4) or terminator count and header (kind 2), the kept count (kind 4), the
// stream sizes, the delivery; two more per compressed chunk.  Every refusal leaves the handle's text as it was: the buffers are
// double and the switch is the last thing a call does.
#include "c3_host.h"
#include "c3_bgzf.h"
#include "c3_fastq.h"

void c3h::demux_text_free(c3_handle* h) {
  DemuxText& t = h->dx;
  if (t.h_hdr) (void)hipHostFree(t.h_hdr);
  if (t.h_lhdr) (void)hipHostFree(t.h_lhdr);
  if (t.h_soff) (void)hipHostFree(t.h_soff);
  if (t.zs.h_sizes) (void)hipHostFree(t.zs.h_sizes);
  for (hipEvent_t ev : t.ev) if (ev) (void)hipEventDestroy(ev);
  if (t.z) c3_bgzf_destroy(t.z);
  t.h_hdr = nullptr; t.h_lhdr = nullptr; t.h_soff = nullptr; t.zs.h_sizes = nullptr; t.z = nullptr;
}

extern "C" int c3_demux_text_reset(c3_handle* h) {
  if (!h) return C3_E_ARG;
  h->dx.kind = 0; h->dx.text_n = 0; h->dx.tail_from = 0;
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
  if (keep_q && t.kind == 2) return c3_fail(h, C3_E_ARG, "c3_demux_emit_text: C3_DEMUX_KEEP_QUALS on a FASTA text");
  int64_t nm = 0, piece = n;
  if (in_z && (rc = c3_bgzf_scan(src, n, &nm, &piece)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  const int64_t tail_n = t.kind ? t.text_n - t.tail_from : 0, total = tail_n + piece;
  if (total > C3_FASTX_MAX_TEXT) return c3_fail(h, C3_E_LIMIT, "c3_demux_emit_text: tail and piece longer than C3_FASTX_MAX_TEXT");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!t.h_hdr) HIPCHK(hipHostMalloc((void**)&t.h_hdr, sizeof(C3FxHdr), hipHostMallocDefault));
  if (!t.h_lhdr) HIPCHK(hipHostMalloc((void**)&t.h_lhdr, sizeof(C3FqHdr), hipHostMallocDefault));
  if (!t.h_soff) HIPCHK(hipHostMalloc((void**)&t.h_soff, (C3_DEMUX_MAX_STREAMS + 2) * sizeof(int64_t), hipHostMallocDefault));
  if (!t.zs.h_sizes) HIPCHK(hipHostMalloc((void**)&t.zs.h_sizes, BGZF_CHUNK_BLOCKS * sizeof(int), hipHostMallocDefault));
  for (hipEvent_t& ev : t.ev) if (!ev) HIPCHK(hipEventCreate(&ev));
  t.tm = c3_demux_text_timing{};
  t.tm.n_streams = S; t.tm.in_bytes = n; t.tm.text_bytes = total;
  for (int s = 0; s <= S; ++s) stream_off[s] = 0;
  info->text_bytes = total; info->kind = t.kind;
  int waits = 0;
  auto wait = [&]() { ++waits; return hipStreamSynchronize(h->stream); };

  // ---- the text: tail + piece in the other buffer ----
  const int nxt = t.cur ^ 1;
  DBuf& text = t.text[nxt];
  HIPCHK(text.ensure((size_t)total + 256));
  if (tail_n) HIPCHK(hipMemcpyAsync(text.p, t.text[t.cur].as<char>() + t.tail_from, (size_t)tail_n, hipMemcpyDeviceToDevice, h->stream));
  if (!in_z) {
    if (piece) HIPCHK(hipMemcpyAsync(text.as<char>() + tail_n, src, (size_t)piece, hipMemcpyHostToDevice, h->stream));
  } else if (nm > 0) {
    const double t_z = dbg_now_ms();
    if (!t.z && (rc = c3_bgzf_create(h->cfg.device, &t.z)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
    int64_t got = 0;
    if ((rc = c3h::bgzf_inflate_to_device(t.z, src, n, nm, text.as<uint8_t>() + tail_n, &got)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
    if (got != piece) return c3_fail(h, C3_E_DATA, "c3_demux_emit_text: inflated size differs from the headers");
    t.tm.ms_inflate = (float)(dbg_now_ms() - t_z);
  }
  // the file's kind: its first byte
  int kind = t.kind;
  if (!kind && total > 0) {
    char first = 0;
    if (!in_z) first = src[0];
    else { HIPCHK(hipMemcpyAsync(&first, text.p, 1, hipMemcpyDeviceToHost, h->stream)); HIPCHK(wait()); }
    kind = c3_fastx_kind_of(first);
    if (keep_q && kind == 2) return c3_fail(h, C3_E_ARG, "c3_demux_emit_text: C3_DEMUX_KEEP_QUALS on a FASTA text");
  }
  info->kind = kind;
  auto commit = [&](int64_t consumed) {                           // the switch: this call's text becomes the kept one
    t.cur = nxt; t.text_n = total; t.tail_from = consumed; t.kind = kind;
    if (at_eof) (void)c3_demux_text_reset(h);
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
    f.buf = text.as<uint8_t>(); f.hi = (uint32_t)total; f.kind = 4;
    const size_t tiles = ((size_t)total + 65535) / 65536;
    HIPCHK(t.cnt.ensure(tiles * 4 * sizeof(int32_t))); HIPCHK(t.lhdr.ensure(sizeof(C3FqHdr))); HIPCHK(t.hdr.ensure(sizeof(C3FxHdr)));
    f.hdr = t.hdr.as<C3FxHdr>();
    c3k_launch_fastq_count(f.buf, 0, f.hi, t.cnt.as<int32_t>(), at_eof, t.lhdr.as<C3FqHdr>(), h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t.h_lhdr, t.lhdr.p, sizeof(C3FqHdr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(wait());
    const int L = t.h_lhdr->n_lines, Lv = t.h_lhdr->n_lines_v;
    if (L < 0 || (int64_t)L > total || Lv < L || Lv > L + 1) return c3_fail(h, C3_E_HIP, "k_fastq: line count out of range");
    f.L = L; f.n_full = Lv / 4; f.partial = (at_eof && (Lv % 4)) ? 1 : 0;
    if (f.n_full > 0 || f.partial) {
      const size_t nr = (size_t)f.n_full + 1, nb = ((size_t)f.n_full + 255) / 256;
      HIPCHK(t.nl.ensure(((size_t)L + 4) * sizeof(int32_t))); HIPCHK(t.slen.ensure(nr * sizeof(int32_t))); HIPCHK(t.nlen.ensure(nr * sizeof(int32_t)));
      HIPCHK(t.bsum.ensure((nb + 1) * 4 * sizeof(long long)));
      HIPCHK(t.off.ensure(nr * sizeof(int64_t))); HIPCHK(t.name_off.ensure(nr * sizeof(int64_t))); HIPCHK(t.woff.ensure(nr * sizeof(int64_t)));
      HIPCHK(t.src.ensure(nr * sizeof(int4))); HIPCHK(t.hash.ensure(nr * sizeof(uint64_t)));
      f.nl = t.nl.as<int32_t>(); f.slen = t.slen.as<int32_t>(); f.nlen = t.nlen.as<int32_t>(); f.bsum = t.bsum.as<long long>();
      f.off = t.off.as<int64_t>(); f.name_off = t.name_off.as<int64_t>(); f.woff = t.woff.as<int64_t>(); f.src = t.src.as<int4>(); f.hash = t.hash.as<uint64_t>();
      HIPCHK(hipMemsetAsync(t.hdr.p, 0xFF, 8, h->stream));          // first_bad, first_high: none
      c3k_launch_fastq_lines(f.buf, 0, f.hi, t.cnt.as<int32_t>(), t.nl.as<int32_t>(), h->stream);
      c3k_launch_fastx_high(&f, h->stream);
      c3k_launch_fastx_records(&f, h->stream);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(t.h_hdr, t.hdr.p, sizeof(C3FxHdr), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(wait());
      const C3FxHdr& x = *t.h_hdr;
      if (x.n_records < 0 || x.n_records > f.n_full || x.consumed < 0 || x.consumed > total || x.base_bytes < 0 || x.base_bytes > total ||
          x.name_bytes < 0 || x.name_bytes > total)
        return c3_fail(h, C3_E_HIP, "k_fastx: header out of range");
      R = x.n_records; consumed = x.consumed; info->departed = x.departed;
    }
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
    const C3FxHdr x = *t.h_hdr;
    HIPCHK(t.names.ensure((size_t)x.name_bytes + 256)); HIPCHK(t.seqs.ensure((size_t)x.base_bytes + 256));
    if (keep_q) HIPCHK(t.quals.ensure((size_t)x.base_bytes + 256));
    f.n_records = R; f.names = t.names.as<uint8_t>(); f.seqs = t.seqs.as<uint8_t>(); f.quals = keep_q ? t.quals.as<uint8_t>() : nullptr;
    c3k_launch_fastx_gather(&f, h->stream);
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
        if ((rc = c3h::bgzf_stream_device(h, t.zs, t.out.as<char>() + so[s], len, arena, cap, &out)) != C3_E_OK) return rc;
        waits += 2 * (int)((len + (int64_t)BGZF_CHUNK_BLOCKS * BGZF_BLOCK - 1) / ((int64_t)BGZF_CHUNK_BLOCKS * BGZF_BLOCK));
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

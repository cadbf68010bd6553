// c3_text.hip -- the text path of the post-processing step (include/c3poa.h "Post-processing, text in / file bytes out";
// DESIGN.md 5.9): pieces of a consensus file in, the streams of c3_post_emit out, everything in between on the device.
//   text   = the kept tail (device to device) + the piece (copied up, or its BGZF members inflated by k_inflate in place)
//   parse  = k_fastq_count / _lines (the '\n'), k_fastx (records of the file's kind, offsets, word offsets, hashes, gather)
//   batch  = the 2-bit pack of c3_batch_stage made from the gathered bases where they lie, k_adapter over it (c3h::adapters_device)
//   format = k_post on the gathered arrays and the table (c3h::post_sizes / post_write), k_bgzf over the read streams when asked
// Three waits size the buffers (line count, parse header, stream sizes); a fourth per compressed chunk (member sizes).  Every
// refusal leaves the handle's text as it was: the buffers are double and the switch is the last thing a call does.
#include "c3_host.h"
#include "c3_bgzf.h"
#include "c3_fastq.h"

void c3h::post_text_free(c3_handle* h) {
  PostText& t = h->pt;
  if (t.h_hdr) (void)hipHostFree(t.h_hdr);
  if (t.h_lhdr) (void)hipHostFree(t.h_lhdr);
  if (t.zs.h_sizes) (void)hipHostFree(t.zs.h_sizes);
  for (hipEvent_t ev : t.ev) if (ev) (void)hipEventDestroy(ev);
  if (t.z) c3_bgzf_destroy(t.z);
  t.h_hdr = nullptr; t.h_lhdr = nullptr; t.zs.h_sizes = nullptr; t.z = nullptr;
}

extern "C" int c3_post_text_reset(c3_handle* h) {
  if (!h) return C3_E_ARG;
  h->pt.kind = 0; h->pt.text_n = 0; h->pt.tail_from = 0;
  return C3_E_OK;
}

extern "C" int c3_post_text_timing_get(c3_handle* h, c3_post_text_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->pt.tm;
  return C3_E_OK;
}

// stream [src, src + len) of the device arena compressed as one text into arena + *out (k_bgzf in chunks of BGZF_CHUNK_BLOCKS
// blocks, staged 4-byte aligned with 256 bytes of slack, as c3_batch_emit_fetch does)
int c3h::bgzf_stream_device(c3_handle* h, ZStage& t, const char* src, int64_t len, char* arena, int64_t cap, int64_t* out) {
  const int64_t CH = (int64_t)BGZF_CHUNK_BLOCKS * BGZF_BLOCK;
  for (int64_t c0 = 0; c0 < len; c0 += CH) {
    const int64_t cn = std::min(CH, len - c0);
    const int nb = (int)((cn + BGZF_BLOCK - 1) / BGZF_BLOCK);
    HIPCHK(t.zin.ensure((size_t)cn + 256)); HIPCHK(t.zslots.ensure((size_t)nb * BGZF_SLOT));
    HIPCHK(t.zsizes.ensure((size_t)nb * sizeof(int))); HIPCHK(t.zpacked.ensure((size_t)nb * BGZF_MAX_MEMBER));
    HIPCHK(hipMemcpyAsync(t.zin.p, src + c0, (size_t)cn, hipMemcpyDeviceToDevice, h->stream));
    c3k_launch_bgzf(t.zin.as<uint8_t>(), (long long)cn, nb, t.zslots.as<uint8_t>(), t.zsizes.as<int>(), t.zpacked.as<uint8_t>(), h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t.h_sizes, t.zsizes.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int64_t tot = 0;
    for (int b = 0; b < nb; ++b) {
      const int sz = t.h_sizes[b];
      if (sz < BGZF_HDR + 13 || sz > BGZF_MAX_MEMBER) return c3_fail(h, C3_E_HIP, "k_bgzf: member size out of range");
      tot += sz;
    }
    if (*out + tot > cap) return c3_fail(h, C3_E_HIP, "k_bgzf: members beyond their bound");      // (cannot be: cap >= the sum of the bounds)
    HIPCHK(hipMemcpyAsync(arena + *out, t.zpacked.p, (size_t)tot, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));                      // (zpacked is written again by the next chunk)
    *out += tot;
  }
  return C3_E_OK;
}

extern "C" int c3_post_emit_text(c3_handle* h, const char* src, int64_t n, int at_eof, int flags, const c3_post_args* plan,
                                 char* arena, int64_t cap, int64_t* stream_off, uint64_t* name_hash, int64_t max_records,
                                 c3_post_text_info* info) {
  if (!h) return C3_E_ARG;
  const double t_call = dbg_now_ms();
  if (info) memset(info, 0, sizeof *info);
  if (!info || n < 0 || (n > 0 && !src) || !plan || !name_hash || max_records < 0 ||
      (flags & ~(C3_POST_IN_BGZF | C3_POST_OUT_BGZF | C3_POST_KEEP_QUALS)))
    return c3_fail(h, C3_E_ARG, "c3_post_emit_text: bad arguments");
  // the plan, as c3_post_emit checks it for a batch of no reads
  c3_post_args a = *plan;
  a.n = 0; a.names = a.seqs = a.quals = nullptr; a.name_off = a.off = nullptr; a.table = nullptr;
  int64_t nk0 = 0;
  int rc = c3_post_check_args("c3_post_emit_text", &a, arena, cap, stream_off, &nk0);
  if (rc != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  if (h->n_spl <= 0) return c3_fail(h, C3_E_STATE, "c3_set_splints must be called first");
  if (a.n_ad != h->n_spl) return c3_fail(h, C3_E_ARG, "c3_post_emit_text: plan->n_ad differs from the rows of c3_set_splints");
  const int S = 3 * a.n_dest + 3;
  const bool in_z = (flags & C3_POST_IN_BGZF) != 0, out_z = (flags & C3_POST_OUT_BGZF) != 0, keep_q = (flags & C3_POST_KEEP_QUALS) != 0;
  PostText& t = h->pt;
  if (keep_q && t.kind == 2) return c3_fail(h, C3_E_ARG, "c3_post_emit_text: C3_POST_KEEP_QUALS on a FASTA text");
  int64_t nm = 0, piece = n;
  if (in_z && (rc = c3_bgzf_scan(src, n, &nm, &piece)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  const int64_t tail_n = t.kind ? t.text_n - t.tail_from : 0, total = tail_n + piece;
  if (total > C3_FASTX_MAX_TEXT) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: tail and piece longer than C3_FASTX_MAX_TEXT");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!t.h_hdr) HIPCHK(hipHostMalloc((void**)&t.h_hdr, sizeof(C3FxHdr), hipHostMallocDefault));
  if (!t.h_lhdr) HIPCHK(hipHostMalloc((void**)&t.h_lhdr, sizeof(C3FqHdr), hipHostMallocDefault));
  if (!t.zs.h_sizes) HIPCHK(hipHostMalloc((void**)&t.zs.h_sizes, BGZF_CHUNK_BLOCKS * sizeof(int), hipHostMallocDefault));
  for (hipEvent_t& ev : t.ev) if (!ev) HIPCHK(hipEventCreate(&ev));
  t.tm = c3_post_text_timing{};
  for (int s = 0; s <= S; ++s) stream_off[s] = 0;
  info->text_bytes = total;

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
    if (got != piece) return c3_fail(h, C3_E_DATA, "c3_post_emit_text: inflated size differs from the headers");
    t.tm.ms_inflate = (float)(dbg_now_ms() - t_z);
  }
  // the file's kind: its first byte
  int kind = t.kind;
  if (!kind && total > 0) {
    char first = 0;
    if (!in_z) first = src[0];
    else { HIPCHK(hipMemcpyAsync(&first, text.p, 1, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); }
    kind = c3_fastx_kind_of(first);
    if (keep_q && kind == 2) return c3_fail(h, C3_E_ARG, "c3_post_emit_text: C3_POST_KEEP_QUALS on a FASTA text");
  }
  auto commit = [&](int64_t consumed) {                           // the switch: this call's text becomes the kept one
    t.cur = nxt; t.text_n = total; t.tail_from = consumed; t.kind = kind;
    if (at_eof) (void)c3_post_text_reset(h);
  };
  if (total == 0) { HIPCHK(hipStreamSynchronize(h->stream)); commit(0); return C3_E_OK; }
  if (!kind) { HIPCHK(hipStreamSynchronize(h->stream)); info->departed = 1; commit(0); return C3_E_OK; }      // neither '>' nor '@'

  // ---- parse ----
  FxArgs f; memset(&f, 0, sizeof f);
  f.buf = text.as<uint8_t>(); f.hi = (uint32_t)total; f.kind = kind;
  const size_t tiles = ((size_t)total + 65535) / 65536;
  HIPCHK(t.cnt.ensure(tiles * 4 * sizeof(int32_t))); HIPCHK(t.lhdr.ensure(sizeof(C3FqHdr))); HIPCHK(t.hdr.ensure(sizeof(C3FxHdr)));
  f.hdr = t.hdr.as<C3FxHdr>();
  HIPCHK(hipEventRecord(t.ev[0], h->stream));
  c3k_launch_fastq_count(f.buf, 0, f.hi, t.cnt.as<int32_t>(), at_eof, t.lhdr.as<C3FqHdr>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t.h_lhdr, t.lhdr.p, sizeof(C3FqHdr), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const int L = t.h_lhdr->n_lines, Lv = t.h_lhdr->n_lines_v;
  if (L < 0 || (int64_t)L > total || Lv < L || Lv > L + 1) return c3_fail(h, C3_E_HIP, "k_fastq: line count out of range");
  f.L = L; f.n_full = Lv / kind; f.partial = (at_eof && (Lv % kind)) ? 1 : 0;
  int64_t R = 0, consumed = 0;
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
    HIPCHK(hipEventRecord(t.ev[1], h->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(t.h_hdr, t.hdr.p, sizeof(C3FxHdr), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const C3FxHdr& x = *t.h_hdr;
    if (x.n_records < 0 || x.n_records > f.n_full || x.consumed < 0 || x.consumed > total || x.base_bytes < 0 || x.base_bytes > total ||
        x.name_bytes < 0 || x.name_bytes > total || x.words < 0 || x.words > total / 16 + 3 * x.n_records || x.max_len < 0 || x.max_len > total)
      return c3_fail(h, C3_E_HIP, "k_fastx: header out of range");
    R = x.n_records; consumed = x.consumed; info->departed = x.departed;
    HIPCHK(hipEventElapsedTime(&t.tm.ms_parse, t.ev[0], t.ev[1]));
  } else {
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  info->n_records = R; info->consumed = consumed;
  t.tm.n_records = R; t.tm.in_bytes = n; t.tm.text_bytes = total;
  if (R > max_records) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: more records than max_records (the need in info)");
  if (R * a.n_ad * 2 > INT32_MAX) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: too many records in one piece");
  if (R == 0) { commit(consumed); t.tm.ms_call = (float)(dbg_now_ms() - t_call); return C3_E_OK; }
  const C3FxHdr x = *t.h_hdr;
  if (x.base_bytes >= (1ll << 31) || x.name_bytes >= (1ll << 31)) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: batch of 2^31 bytes or more");

  // ---- gather, pack, k_adapter ----
  HIPCHK(t.names.ensure((size_t)x.name_bytes + 256)); HIPCHK(t.seqs.ensure((size_t)x.base_bytes + 256));
  if (keep_q) HIPCHK(t.quals.ensure((size_t)x.base_bytes + 256));
  HIPCHK(t.pk.ensure(sizeof(uint32_t) * (size_t)x.words + 64));
  HIPCHK(t.table.ensure(sizeof(int32_t) * 24 * (size_t)R * a.n_ad + 16));
  f.n_records = R; f.names = t.names.as<uint8_t>(); f.seqs = t.seqs.as<uint8_t>(); f.quals = keep_q ? t.quals.as<uint8_t>() : nullptr;
  HIPCHK(hipEventRecord(t.ev[2], h->stream));
  c3k_launch_fastx_gather(&f, h->stream);
  c3k_launch_pack(f.seqs, f.off, f.woff, (int)R, t.pk.as<uint32_t>(), (int)std::min<int64_t>((R + 3) / 4, (int64_t)h->n_cus * 32), h->stream);
  HIPCHK(hipEventRecord(t.ev[3], h->stream));
  HIPCHK(hipGetLastError());
  C3Batch b; memset(&b, 0, sizeof b);
  b.n = (int)R; b.pk = t.pk.as<uint32_t>(); b.woff = f.woff; b.off = f.off;
  if ((rc = c3h::adapters_device(h, b, x.max_len, t.table.as<int32_t>())) != C3_E_OK) return rc;
  HIPCHK(hipEventRecord(t.ev[4], h->stream));

  // ---- k_post ----
  PostArgs p; memset(&p, 0, sizeof p);
  p.n = (int)R; p.names = f.names; p.name_off = f.name_off; p.seqs = f.seqs; p.quals = f.quals; p.off = f.off; p.table = t.table.as<int32_t>();
  std::vector<int64_t> so;
  if ((rc = c3h::post_sizes(h, &a, p, so)) != C3_E_OK) return rc;
  const int n_z = out_z ? 3 * a.n_dest + 1 : 0;                  // the read streams and the 10x stream
  int64_t need = 0;
  for (int s = 0; s < S; ++s) { stream_off[s] = need; const int64_t len = so[s + 1] - so[s]; need += (s < n_z && len) ? c3_bgzf_bound(len) : len; }
  stream_off[S] = need;
  info->n_kept = so[S + 1]; info->out_bytes = need;
  if (need > cap) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: arena too small (bytes needed in stream_off[S])");
  if ((rc = c3h::post_write(h, p, so[S])) != C3_E_OK) return rc;
  const char* d_arena = h->d_post[15].as<char>();
  int64_t out = 0;
  if (!out_z) {
    if (need) HIPCHK(hipMemcpyAsync(arena, d_arena, (size_t)need, hipMemcpyDeviceToHost, h->stream));
    out = need;
  } else {
    const double t_z = dbg_now_ms();
    for (int s = 0; s < S; ++s) {
      stream_off[s] = out;
      const int64_t len = so[s + 1] - so[s];
      if (s < n_z) { if ((rc = c3h::bgzf_stream_device(h, t.zs, d_arena + so[s], len, arena, cap, &out)) != C3_E_OK) return rc; }
      else if (len) { HIPCHK(hipMemcpyAsync(arena + out, d_arena + so[s], (size_t)len, hipMemcpyDeviceToHost, h->stream)); out += len; }
    }
    stream_off[S] = out;
    t.tm.ms_bgzf = (float)(dbg_now_ms() - t_z);
  }
  HIPCHK(hipMemcpyAsync(name_hash, f.hash, (size_t)R * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  info->out_bytes = out;
  float ms_a = 0, ms_b = 0, ms_c = 0;
  HIPCHK(hipEventElapsedTime(&t.tm.ms_gather, t.ev[2], t.ev[3]));
  HIPCHK(hipEventElapsedTime(&t.tm.ms_adapter, t.ev[3], t.ev[4]));
  HIPCHK(hipEventElapsedTime(&ms_a, h->ev_post[0], h->ev_post[1])); HIPCHK(hipEventElapsedTime(&ms_b, h->ev_post[1], h->ev_post[2]));
  HIPCHK(hipEventElapsedTime(&ms_c, h->ev_post[3], h->ev_post[4]));
  t.tm.ms_post = ms_a + ms_b + ms_c;
  t.tm.n_kept = so[S + 1]; t.tm.out_bytes = out;
  commit(consumed);
  t.tm.ms_call = (float)(dbg_now_ms() - t_call);
  return C3_E_OK;
}

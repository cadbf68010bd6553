// c3_tfront.hip -- the text front that c3_post_emit_text (c3_text.hip) and c3_demux_emit_text (c3_dtext.hip) share:
//   load   = the kept tail (device to device) + the piece (copied up, or its BGZF members inflated by k_inflate in place) in the
//            other text buffer; the file's kind from its first byte
//   tables = k_fastq_count / _lines (the '\n'), k_fastx_high / _records (records of the file's kind, offsets, word offsets, hashes)
//   gather = k_fastx_gather into names / seqs / quals
//   commit = the switch of the double buffer, the last thing a successful call does: every refusal leaves the kept text untouched
// and the compression of one device-resident stream for their BGZF output.  Messages carry the entry point's name.
#include "c3_host.h"
#include "c3_fastq.h"

static int fail_as(c3_handle* h, int code, const char* who, const char* what) { return c3_fail(h, code, (std::string(who) + ": " + what).c_str()); }

void c3h::text_free(TextFront& t) {
  if (t.h_hdr) (void)hipHostFree(t.h_hdr);
  if (t.h_lhdr) (void)hipHostFree(t.h_lhdr);
  if (t.z) c3_bgzf_destroy(t.z);
  t.h_hdr = nullptr; t.h_lhdr = nullptr; t.z = nullptr;
}

void c3h::text_reset(TextFront& t) { t.kind = 0; t.text_n = 0; t.tail_from = 0; }

int c3h::text_load(c3_handle* h, TextFront& t, const char* src, int64_t n, bool in_z, bool keep_q, const char* who, const char* keep_flag,
                   hipEvent_t* ev, int n_ev, TextLoad* ld) {
  const std::string keep_on_fasta = std::string(keep_flag) + " on a FASTA text";
  if (keep_q && t.kind == 2) return fail_as(h, C3_E_ARG, who, keep_on_fasta.c_str());
  int rc;
  int64_t nm = 0, piece = n;
  if (in_z && (rc = c3_bgzf_scan(src, n, &nm, &piece)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  const int64_t tail_n = t.kind ? t.text_n - t.tail_from : 0, total = tail_n + piece;
  if (total > C3_FASTX_MAX_TEXT) return fail_as(h, C3_E_LIMIT, who, "tail and piece longer than C3_FASTX_MAX_TEXT");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!t.h_hdr) HIPCHK(hipHostMalloc((void**)&t.h_hdr, sizeof(C3FxHdr), hipHostMallocDefault));
  if (!t.h_lhdr) HIPCHK(hipHostMalloc((void**)&t.h_lhdr, sizeof(C3FqHdr), hipHostMallocDefault));
  HIPCHK(t.zs.pin());
  for (int i = 0; i < n_ev; ++i) if (!ev[i]) HIPCHK(hipEventCreate(&ev[i]));
  *ld = TextLoad{};
  ld->nxt = t.cur ^ 1; ld->total = total;

  DBuf& text = t.text[ld->nxt];
  HIPCHK(text.ensure((size_t)total + 256));
  if (tail_n) HIPCHK(hipMemcpyAsync(text.p, t.text[t.cur].as<char>() + t.tail_from, (size_t)tail_n, hipMemcpyDeviceToDevice, h->stream));
  if (!in_z) {
    if (piece) HIPCHK(hipMemcpyAsync(text.as<char>() + tail_n, src, (size_t)piece, hipMemcpyHostToDevice, h->stream));
  } else if (nm > 0) {
    const double t_z = dbg_now_ms();
    if (!t.z && (rc = c3_bgzf_create(h->cfg.device, &t.z)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
    int64_t got = 0;
    if ((rc = c3h::bgzf_inflate_to_device(t.z, src, n, nm, text.as<uint8_t>() + tail_n, &got)) != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
    if (got != piece) return fail_as(h, C3_E_DATA, who, "inflated size differs from the headers");
    ld->ms_inflate = (float)(dbg_now_ms() - t_z);
  }
  // the file's kind: its first byte
  ld->kind = t.kind;
  if (!ld->kind && total > 0) {
    char first = 0;
    if (!in_z) first = src[0];
    else { HIPCHK(hipMemcpyAsync(&first, text.p, 1, hipMemcpyDeviceToHost, h->stream)); HIPCHK(hipStreamSynchronize(h->stream)); ++ld->waits; }
    ld->kind = c3_fastx_kind_of(first);
    if (keep_q && ld->kind == 2) return fail_as(h, C3_E_ARG, who, keep_on_fasta.c_str());
  }
  return C3_E_OK;
}

int c3h::text_tables(c3_handle* h, TextFront& t, const TextLoad& ld, int at_eof, FxArgs& f, int* waits, hipEvent_t ev_begin, hipEvent_t ev_records) {
  const int64_t total = ld.total;
  memset(&f, 0, sizeof f);
  memset(t.h_hdr, 0, sizeof *t.h_hdr);
  f.buf = t.text[ld.nxt].as<uint8_t>(); f.hi = (uint32_t)total; f.kind = ld.kind;
  const size_t tiles = ((size_t)total + 65535) / 65536;
  HIPCHK(t.cnt.ensure(tiles * 4 * sizeof(int32_t))); HIPCHK(t.lhdr.ensure(sizeof(C3FqHdr))); HIPCHK(t.hdr.ensure(sizeof(C3FxHdr)));
  f.hdr = t.hdr.as<C3FxHdr>();
  if (ev_begin) HIPCHK(hipEventRecord(ev_begin, h->stream));
  c3k_launch_fastq_count(f.buf, 0, f.hi, t.cnt.as<int32_t>(), at_eof, t.lhdr.as<C3FqHdr>(), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t.h_lhdr, t.lhdr.p, sizeof(C3FqHdr), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream)); if (waits) ++*waits;
  const int L = t.h_lhdr->n_lines, Lv = t.h_lhdr->n_lines_v;
  if (L < 0 || (int64_t)L > total || Lv < L || Lv > L + 1) return c3_fail(h, C3_E_HIP, "k_fastq: line count out of range");
  f.L = L; f.n_full = Lv / f.kind; f.partial = (at_eof && (Lv % f.kind)) ? 1 : 0;
  if (f.n_full == 0 && !f.partial) return C3_E_OK;                     // no whole record yet: everything stays unconsumed
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
  if (ev_records) HIPCHK(hipEventRecord(ev_records, h->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(t.h_hdr, t.hdr.p, sizeof(C3FxHdr), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream)); if (waits) ++*waits;
  const C3FxHdr& x = *t.h_hdr;
  if (x.n_records < 0 || x.n_records > f.n_full || x.consumed < 0 || x.consumed > total || x.base_bytes < 0 || x.base_bytes > total ||
      x.name_bytes < 0 || x.name_bytes > total || x.words < 0 || x.words > total / 16 + 3 * x.n_records || x.max_len < 0 || x.max_len > total)
    return c3_fail(h, C3_E_HIP, "k_fastx: header out of range");
  f.n_records = x.n_records;
  return C3_E_OK;
}

int c3h::text_gather(c3_handle* h, TextFront& t, FxArgs& f, bool keep_q, hipEvent_t ev_begin) {
  const C3FxHdr& x = *t.h_hdr;
  HIPCHK(t.names.ensure((size_t)x.name_bytes + 256)); HIPCHK(t.seqs.ensure((size_t)x.base_bytes + 256));
  if (keep_q) HIPCHK(t.quals.ensure((size_t)x.base_bytes + 256));
  f.names = t.names.as<uint8_t>(); f.seqs = t.seqs.as<uint8_t>(); f.quals = keep_q ? t.quals.as<uint8_t>() : nullptr;
  if (ev_begin) HIPCHK(hipEventRecord(ev_begin, h->stream));
  c3k_launch_fastx_gather(&f, h->stream);
  return C3_E_OK;
}

void c3h::text_commit(TextFront& t, const TextLoad& ld, int64_t consumed, int at_eof) {
  t.cur = ld.nxt; t.text_n = ld.total; t.tail_from = consumed; t.kind = ld.kind;
  if (at_eof) text_reset(t);
}

// stream [src, src + len) of a device arena compressed as one text into arena + *out on the handle's stream
int c3h::bgzf_stream_device(c3_handle* h, ZStage& z, const char* src, int64_t len, char* arena, int64_t cap, int64_t* out, int* waits) {
  const ZStatus st = bgzf_chunks(z, h->stream, len, [&](char* d_zin, int64_t c0, int64_t cn) {
    return hipMemcpyAsync(d_zin, src + c0, (size_t)cn, hipMemcpyDeviceToDevice, h->stream); }, arena, cap, out, true);
  if (waits) *waits += st.waits;
  if (st.e != hipSuccess) return c3_hip_fail(h, st.e, st.what, __FILE__, __LINE__);
  if (st.bad) return c3_fail(h, C3_E_HIP, st.bad == ZStatus::MEMBER_SIZE ? "k_bgzf: member size out of range" : "k_bgzf: members beyond their bound");
  return C3_E_OK;
}

// c3_text.hip -- the text path of the post-processing step (include/c3poa.h "Post-processing, text in / file bytes out";
// DESIGN.md 5.9): pieces of a consensus file in, the streams of c3_post_emit out, everything in between on the device.
//   text, parse = the shared text front (c3_tfront.hip): load, tables, gather
//   batch  = the 2-bit pack of c3_batch_stage made from the gathered bases where they lie, k_adapter over it (c3h::adapters_device)
//   format = k_post on the gathered arrays and the table (c3h::post_sizes / post_write), k_bgzf over the read streams when asked
// Three waits size the buffers (line count, parse header, stream sizes); two more per compressed chunk (member sizes, members).
// Every refusal leaves the handle's text as it was: the front's commit is the last thing a call does.
#include "c3_host.h"

void c3h::post_text_free(c3_handle* h) {
  for (hipEvent_t ev : h->pt.ev) if (ev) (void)hipEventDestroy(ev);
  text_free(h->pt);
}

extern "C" int c3_post_text_reset(c3_handle* h) {
  if (!h) return C3_E_ARG;
  c3h::text_reset(h->pt);
  return C3_E_OK;
}

extern "C" int c3_post_text_timing_get(c3_handle* h, c3_post_text_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->pt.tm;
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
  c3h::TextLoad ld;
  if ((rc = c3h::text_load(h, t, src, n, in_z, keep_q, "c3_post_emit_text", "C3_POST_KEEP_QUALS", t.ev, 8, &ld)) != C3_E_OK) return rc;
  const int64_t total = ld.total;
  t.tm = c3_post_text_timing{};
  t.tm.ms_inflate = ld.ms_inflate;
  for (int s = 0; s <= S; ++s) stream_off[s] = 0;
  info->text_bytes = total;
  if (total == 0) { HIPCHK(hipStreamSynchronize(h->stream)); c3h::text_commit(t, ld, 0, at_eof); return C3_E_OK; }
  if (!ld.kind) { HIPCHK(hipStreamSynchronize(h->stream)); info->departed = 1; c3h::text_commit(t, ld, 0, at_eof); return C3_E_OK; }      // neither '>' nor '@'

  // ---- parse (ms_parse: k_fastq_count through k_fastx_records) ----
  FxArgs f;
  if ((rc = c3h::text_tables(h, t, ld, at_eof, f, nullptr, t.ev[0], t.ev[1])) != C3_E_OK) return rc;
  if (f.n_full > 0 || f.partial) HIPCHK(hipEventElapsedTime(&t.tm.ms_parse, t.ev[0], t.ev[1]));
  else HIPCHK(hipStreamSynchronize(h->stream));                   // no record pass ran
  const C3FxHdr x = *t.h_hdr;
  const int64_t R = x.n_records, consumed = x.consumed;
  info->departed = x.departed;
  info->n_records = R; info->consumed = consumed;
  t.tm.n_records = R; t.tm.in_bytes = n; t.tm.text_bytes = total;
  if (R > max_records) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: more records than max_records (the need in info)");
  if (R * a.n_ad * 2 > INT32_MAX) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: too many records in one piece");
  if (R == 0) { c3h::text_commit(t, ld, consumed, at_eof); t.tm.ms_call = (float)(dbg_now_ms() - t_call); return C3_E_OK; }
  if (x.base_bytes >= (1ll << 31) || x.name_bytes >= (1ll << 31)) return c3_fail(h, C3_E_LIMIT, "c3_post_emit_text: batch of 2^31 bytes or more");

  // ---- gather, pack, k_adapter ----
  HIPCHK(t.pk.ensure(sizeof(uint32_t) * (size_t)x.words + 64));
  HIPCHK(t.table.ensure(sizeof(int32_t) * 24 * (size_t)R * a.n_ad + 16));
  if ((rc = c3h::text_gather(h, t, f, keep_q, t.ev[2])) != C3_E_OK) return rc;
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
  c3h::text_commit(t, ld, consumed, at_eof);
  t.tm.ms_call = (float)(dbg_now_ms() - t_call);
  return C3_E_OK;
}

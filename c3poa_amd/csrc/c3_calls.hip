// c3_calls.hip -- the reference-shaped calls on ONE read or one consensus, built on the batch pipeline of the same handle:
// c3_poa_msa, c3_determine_consensus, c3_zero_repeats, c3_call_peaks, c3_pairwise_consensus, c3_consensus_qv.
#include "c3_host.h"

// make the handle hold exactly one read: a dummy splint when none is set, the upload, and -- rec != null -- its record
static int load_one_read(c3_handle* h, const std::string& seq, const std::string& ql, const c3_read_result* rec) {
  if (h->n_spl <= 0) { const char sp[] = "ACGT"; int64_t o[2] = {0, 4}; int rc = c3_set_splints(h, 1, sp, o); if (rc) return rc; }
  int64_t off[2] = {0, (int64_t)seq.size()};
  int16_t sid = 0; char st = '+';
  int rc = c3_batch_upload(h, 1, seq.data(), ql.data(), off, &sid, &st);
  if (rc) return rc;
  if (rec) HIPCHK(hipMemcpy(h->d_info.p, rec, sizeof(*rec), hipMemcpyHostToDevice));
  return 0;
}

// the consensus of the one resident read into out (none: *out_len = 0)
static int one_consensus(c3_handle* h, char* out, int cap, int* out_len) {
  c3_read_result res;
  int64_t co[2];
  const int rc = c3_batch_results(h, &res, out, cap, co);
  if (rc) return rc;
  *out_len = (res.status == C3_ST_OK) ? res.cons_len : 0;
  return C3_E_OK;
}

// inject a pre-split "read": [front][sub0]...[subn-1][tail]; skips conk/peaks
static int inject(c3_handle* h, int n, const char* const* subs, const char* const* quals, const int* lens,
                  const char* front, const char* front_q, int front_len, const char* tail, const char* tail_q, int tail_len) {
  if (n < 1 || n > C3_MAX_SUB) return c3_fail(h, C3_E_LIMIT, "1..250 subreads");
  std::string seq, ql;
  c3_read_result r; memset(&r, 0, sizeof(r));
  if (front && front_len > 0) { seq.append(front, front_len); if (front_q) ql.append(front_q, front_len); else ql.append(front_len, 'I'); r.has_front = 1; r.front_end = front_len; }
  for (int i = 0; i < n; ++i) {
    r.sub_beg[i] = (int)seq.size(); seq.append(subs[i], lens[i]);
    if (quals && quals[i]) ql.append(quals[i], lens[i]); else ql.append(lens[i], 'I');
    r.sub_end[i] = (int)seq.size();
  }
  r.n_sub = n; r.n_peaks = n + 1; r.status = C3_ST_OK;
  if (tail && tail_len > 0) { r.has_tail = 1; r.tail_beg = (int)seq.size(); seq.append(tail, tail_len); if (tail_q) ql.append(tail_q, tail_len); else ql.append(tail_len, 'I'); }
  int rc = load_one_read(h, seq, ql, &r);
  if (rc) return rc;
  h->injected = true;
  return 0;
}

// stand-alone QVs of one consensus (k_qv on one workgroup); the host statement and the shared refusals are in c3_qv.cpp.
// The pieces are 2-bit packed here the way c3_batch_stage packs reads (every piece starts on a word).
extern "C" int c3_consensus_qv(c3_handle* h, const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat,
                               const int64_t* piece_off, const int32_t* modes, char* qv_out) {
  if (!h) return C3_E_ARG;
  const char* msg = "";
  const int rc0 = c3_qv_check(cons, n, n_pieces, seq_cat, qual_cat, piece_off, modes, qv_out, &msg);
  if (rc0 != C3_E_OK) return c3_fail(h, rc0, msg);
  HIPCHK(hipSetDevice(h->cfg.device));
  const int np = n_pieces;
  std::vector<int64_t> woff((size_t)np + 1, 0);
  long long max_m = 1;
  for (int k = 0; k < np; ++k) {
    const int64_t m = piece_off[k + 1] - piece_off[k];
    max_m = std::max<long long>(max_m, m);
    woff[(size_t)k + 1] = woff[(size_t)k] + (m + 15) / 16 + 2;
  }
  std::vector<uint32_t> pk((size_t)woff[(size_t)np] + 1, 0u);
  for (int k = 0; k < np; ++k)
    for (int64_t x = 0; x < piece_off[k + 1] - piece_off[k]; ++x)
      pk[(size_t)(woff[(size_t)k] + x / 16)] |= (uint32_t)code_of(seq_cat[piece_off[k] + x]) << ((x & 15) * 2);
  const size_t qb = np ? (size_t)piece_off[np] : 0;
  // one device buffer: consensus | QVs | qualities | packed pieces | word offsets | base offsets | modes
  const size_t o_qv = (size_t)n + 64, o_q = o_qv + (size_t)n + 64, o_pk = (o_q + qb + 64 + 255) / 256 * 256;
  const size_t o_wo = o_pk + 4 * pk.size() + 64, o_off = o_wo + 8 * woff.size() + 64, o_md = o_off + 8 * ((size_t)np + 1) + 64;
  DBuf d; HIPCHK(d.ensure(o_md + 4 * (size_t)np + 64));
  char* b = d.as<char>();
  HIPCHK(hipMemcpyAsync(b, cons, (size_t)n, hipMemcpyHostToDevice, h->stream));
  if (np) {
    HIPCHK(hipMemcpyAsync(b + o_q, qual_cat, qb, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(b + o_pk, pk.data(), 4 * pk.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(b + o_wo, woff.data(), 8 * woff.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(b + o_off, piece_off, 8 * ((size_t)np + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(b + o_md, modes, 4 * (size_t)np, hipMemcpyHostToDevice, h->stream));
  }
  QvArgs a; memset(&a, 0, sizeof(a));
  int grid = 0;
  const int rc = c3h::qv_scratch(h, max_m, n, 1, a, &grid);
  if (rc) return rc;
  a.cons = b; a.qv = b + o_qv; a.qual = (const uint8_t*)(b + o_q); a.pk = (const uint32_t*)(b + o_pk);
  a.sa_np = np; a.sa_n = n; a.sa_woff = (const int64_t*)(b + o_wo); a.sa_off = (const int64_t*)(b + o_off); a.sa_mode = (const int32_t*)(b + o_md);
  c3k_launch_qv(&a, 1, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(qv_out, b + o_qv, (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));           // pk / woff are host vectors of this frame
  return C3_E_OK;
}

// pairwise_consensus(msa_rows, subreads, quals) (bin/consensus.py:76-81; call site determine_consensus.py:36-40): rows are
// the two MSA rows ('-' = gap, msa_len columns), subA/subB the ungapped subreads with their qualities.  Identical
// subreads share the later quality (the seqDict collision of consensus.py:77-79).
extern "C" int c3_pairwise_consensus(c3_handle* h, const char* rowA, const char* rowB, int msa_len,
                                     const char* subA, int lenA, const char* qualA, const char* subB, int lenB, const char* qualB,
                                     char* out, int cap, int* out_len) {
  if (!h || !rowA || !rowB || msa_len < 0 || !subA || !subB || !qualA || !qualB || !out || !out_len) return C3_E_ARG;
  *out_len = 0;
  if (msa_len == 0) return C3_E_OK;
  if (cap < msa_len) return C3_E_LIMIT;
  HIPCHK(hipSetDevice(h->cfg.device));
  auto code = [](char ch) -> uint8_t { switch (ch) { case 'A': case 'a': return 0; case 'C': case 'c': return 1; case 'G': case 'g': return 2;
                                                       case 'T': case 't': case 'U': case 'u': return 3; case '-': return 4; default: return 0; } };
  std::vector<uint8_t> rows((size_t)2 * msa_len);
  int na = 0, nb = 0;
  for (int i = 0; i < msa_len; ++i) { rows[i] = code(rowA[i]); rows[(size_t)msa_len + i] = code(rowB[i]); na += rows[i] != 4; nb += rows[(size_t)msa_len + i] != 4; }
  if (na != lenA || nb != lenB) return c3_fail(h, C3_E_ARG, "MSA rows do not spell the subreads");
  const bool same = lenA == lenB && memcmp(subA, subB, (size_t)lenA) == 0;
  DBuf d_rows, d_qa, d_qb, d_scr, d_out, d_len;
  HIPCHK(d_scr.ensure((size_t)2 * msa_len + 16)); HIPCHK(d_out.ensure((size_t)msa_len + 16)); HIPCHK(d_len.ensure(16));
  HIPCHK(d_rows.put(rows.data(), rows.size(), h->stream));
  HIPCHK(d_qa.put(same ? qualB : qualA, (size_t)lenA, h->stream, 16));
  HIPCHK(d_qb.put(qualB, (size_t)lenB, h->stream, 16));
  c3k_launch_pairwise(d_rows.as<uint8_t>(), msa_len, d_qa.as<uint8_t>(), lenA, d_qb.as<uint8_t>(), lenB, d_scr.as<uint8_t>(), d_out.as<uint8_t>(), d_len.as<int>(), h->stream);
  HIPCHK(hipGetLastError());
  std::vector<uint8_t> codes((size_t)msa_len);
  int n = 0;
  HIPCHK(hipMemcpyAsync(&n, d_len.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(codes.data(), d_out.p, (size_t)msa_len, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) out[i] = "ACGT"[codes[(size_t)i] & 3];
  *out_len = n;
  return C3_E_OK;
}

extern "C" int c3_call_peaks(c3_handle* h, const int32_t* scores, int n, int min_dist, int32_t* peaks, int cap, double* smoothed) {
  if (!h || !scores || n <= 0 || !peaks) return C3_E_ARG;
  int rc = load_one_read(h, std::string((size_t)n, 'A'), std::string((size_t)n, 'I'), nullptr);
  if (rc) return rc;
  HIPCHK(h->d_track.ensure(sizeof(int32_t) * (size_t)n + 64));
  HIPCHK(hipMemcpy(h->d_track.p, scores, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  h->stages_done |= C3_STAGE_CONK;
  { Override<int> md(h->cfg.mdistcutoff, min_dist); rc = c3_batch_run(h, C3_STAGE_PEAKS); }
  if (rc) return rc;
  int np = c3_fetch_raw_peaks(h, 0, peaks, cap);
  if (np < 0) return np;
  if (np == 0) {
    // k_peaks keeps at most C3_MAX_PEAKS - 1 peaks: beyond that it drops them all and marks the read, and 0 here would read as
    // "gated" (a read over the subread limit carries the same status, but its peaks are all there)
    int32_t status = C3_ST_OK;
    HIPCHK(hipMemcpy(&status, (const char*)h->d_info.p + offsetof(C3Info, status), sizeof(status), hipMemcpyDeviceToHost));
    if (status == C3_ST_LIMIT) return c3_fail(h, C3_E_LIMIT, "c3_call_peaks: more than 255 peaks (C3_MAX_PEAKS - 1)");
  }
  if (smoothed) { int r2 = c3_fetch_smoothed(h, 0, smoothed, n); if (r2 < 0) return r2; }
  return np;
}

extern "C" int c3_poa_msa(c3_handle* h, int n, const char* const* seqs, const int* lens,
                          char* cons, int cons_cap, int* cons_len, char* msa, int64_t msa_cap, int* msa_len) {
  if (!h) return C3_E_ARG;
  if (cons_len) *cons_len = 0;
  if (msa_len) *msa_len = 0;
  if (n == 0) return C3_E_OK;                       // msa([]) -> empty result (determine_consensus.py:43-47 with repeats==0)
  if (!seqs || !lens) return C3_E_ARG;
  int rc = inject(h, n, seqs, nullptr, lens, nullptr, nullptr, 0, nullptr, nullptr, 0);
  if (rc) return rc;
  Override<bool> keep_rows(h->debug_msa, msa != nullptr);
  rc = c3_batch_run(h, C3_STAGE_POA);
  if (rc == 0 && cons) {
    // pyabpoa semantics: the consensus is the heaviest bundle also for n == 2; the batch path gives the
    // pairwise-merged draft there, so only n != 2 is served from the draft
    if (n == 2) return c3_fail(h, C3_E_ARG, "out_cons with exactly 2 sequences is not a reference call shape");
    int C = c3_fetch_draft(h, 0, cons, cons_cap);
    if (C < 0) rc = C; else if (cons_len) *cons_len = C;
  }
  if (rc == 0 && msa) { int ml = 0; rc = c3h::fetch_msa_rows(h, 0, n, msa, msa_cap, &ml); if (rc == 0 && msa_len) *msa_len = ml; }
  return rc;
}

extern "C" int c3_zero_repeats(c3_handle* h, const char* d0, const char* q0, int n0, const char* d1, const char* q1, int n1,
                               int min_len, char* out, int cap, int* out_len) {
  if (!h || !d0 || !d1 || n0 <= 0 || n1 <= 0 || !out || !out_len) return C3_E_ARG;
  *out_len = 0;
  std::string seq(d0, n0), ql;
  seq.append(d1, n1);
  if (q0) ql.append(q0, n0); else ql.append(n0, 'I');
  if (q1) ql.append(q1, n1); else ql.append(n1, 'I');
  c3_read_result r; memset(&r, 0, sizeof(r));
  r.status = C3_ST_NO_CONSENSUS; r.n_peaks = 1; r.has_front = 1; r.has_tail = 1; r.front_end = n0; r.tail_beg = n0;
  int rc = load_one_read(h, seq, ql, &r);
  if (rc) return rc;
  { Override<int> md(h->cfg.mdistcutoff, min_len), zero(h->cfg.zero, 1); rc = c3_batch_run(h, C3_STAGE_POA | C3_STAGE_POLISH); }
  if (rc) return rc;
  return one_consensus(h, out, cap, out_len);
}

extern "C" int c3_determine_consensus(c3_handle* h, int n, const char* const* subs, const char* const* quals,
                                      const int* lens, const char* front, const char* front_q, int front_len,
                                      const char* tail, const char* tail_q, int tail_len,
                                      char* out, int cap, int* out_len, char* draft, int draft_cap, int* draft_len) {
  if (!h || !subs || !lens || !out || !out_len) return C3_E_ARG;
  *out_len = 0; if (draft_len) *draft_len = 0;
  int rc = inject(h, n, subs, quals, lens, front, front_q, front_len, tail, tail_q, tail_len);
  if (rc) return rc;
  rc = c3_batch_run(h, C3_STAGE_POA | C3_STAGE_POLISH);
  if (rc) return rc;
  if (draft) { int C = c3_fetch_draft(h, 0, draft, draft_cap); if (C < 0) return C; if (draft_len) *draft_len = C; }
  return one_consensus(h, out, cap, out_len);
}

// c3_gunzip_dev.hip -- c3_gunzip (include/c3poa.h "gzip input"): the procedure of c3_gunzip_run.h over the
// kernels of k_gunzip.hip on the device of a c3_bgzf.  The file goes up once; between launches the host sees only small
// copies: the candidates of a stretch, the (status, stop, length) of the pieces decoded, the (CRC, flag) of the chunks
// resolved.  Errors go to the text of c3_last_error(NULL).
#include "c3_host.h"
#include "c3_gunzip_run.h"

namespace {

struct DevBackend {
  c3_bgzf* z; const uint8_t* src; int64_t n;                 // file bytes [boff, n) lie at src + boff .. (src may point in front of them)
  int64_t boff = 0;                                          // a multiple of 256
  // where a stretch's bytes go: null = gz_out and the whole batch to the host; else begin_output asks for the device address
  // of the stretch's text (the reader's device parse) and only the last 32 KiB of a batch come to the host
  std::function<int(int64_t bytes, uint8_t** d_text)> place;
  uint8_t* d_text = nullptr;
  std::vector<C3GzChunk> chunks; std::vector<uint2> cres;

  const uint8_t* comp() const { return z->gz_comp.as<uint8_t>() - boff; }         // never dereferenced below boff
  int upload() {                                             // the bytes, zero for 512 bytes behind them
    const int64_t len = n - boff;
    ZCHK(hipStreamSynchronize(z->stream), "k_gunzip");
    ZCHK(z->gz_comp.ensure((size_t)len + 512), "input buffer");
    ZCHK(hipMemcpyAsync(z->gz_comp.p, src + boff, (size_t)len, hipMemcpyHostToDevice, z->stream), "copy in");
    ZCHK(hipMemsetAsync((char*)z->gz_comp.p + len, 0, 512, z->stream), "copy in");
    return 0;
  }
  int reserve(int64_t symbols, int64_t head, int n_heads) {
    ZCHK(hipStreamSynchronize(z->stream), "k_gunzip");      // (nothing queued may still use the arena that ensure replaces)
    ZCHK(z->gz_arena.ensure((size_t)(symbols + head * n_heads) * sizeof(uint16_t) + 256), "symbol arena");
    return 0;
  }
  int find(int64_t s0, int64_t s1, int64_t piece, int64_t* cand) {
    const int64_t np = (s1 - s0 + piece - 1) / piece;
    ZCHK(z->gz_cand.ensure((size_t)np * sizeof(int64_t)), "candidates");
    c3k_launch_gunzip_find(comp(), n, s0, s1, piece, np, z->gz_cand.as<int64_t>(), z->stream);
    ZCHK(hipGetLastError(), "k_gunzip_find launch");
    ZCHK(hipMemcpyAsync(cand + 1, z->gz_cand.as<int64_t>() + 1, (size_t)(np - 1) * sizeof(int64_t), hipMemcpyDeviceToHost, z->stream), "k_gunzip_find");
    ZCHK(hipStreamSynchronize(z->stream), "k_gunzip_find");
    for (int64_t k = 1; k < np; ++k)                         // nothing the device says is trusted: a candidate lies in its piece
      if (cand[k] < 8 * (s0 + k * piece) || cand[k] >= 8 * std::min(s1, s0 + (k + 1) * piece)) cand[k] = -1;
    return 0;
  }
  int decode(const C3GzJob* jobs, int nj, C3GzRes* res) {
    for (int j = 0; j < nj; ++j) if (jobs[j].start < 8 * boff) return host_fail(C3_E_HIP, "k_gunzip_decode: a piece in front of the loaded bytes");
    ZCHK(z->gz_jobs.ensure((size_t)nj * sizeof(C3GzJob)), "jobs");
    ZCHK(z->gz_res.ensure((size_t)nj * sizeof(C3GzRes)), "statuses");
    ZCHK(hipMemcpyAsync(z->gz_jobs.p, jobs, (size_t)nj * sizeof(C3GzJob), hipMemcpyHostToDevice, z->stream), "copy in");
    c3k_launch_gunzip_decode(comp(), n, z->gz_jobs.as<C3GzJob>(), nj, z->gz_arena.as<uint16_t>(), z->gz_res.as<C3GzRes>(), z->stream);
    ZCHK(hipGetLastError(), "k_gunzip_decode launch");
    ZCHK(hipMemcpyAsync(res, z->gz_res.p, (size_t)nj * sizeof(C3GzRes), hipMemcpyDeviceToHost, z->stream), "k_gunzip_decode");
    ZCHK(hipStreamSynchronize(z->stream), "k_gunzip_decode");
    for (int j = 0; j < nj; ++j) {                           // lengths and positions that cannot be are a failed piece
      C3GzRes& r = res[j];
      if (r.status < C3_GZ_LIMIT || r.status > C3_GZ_BAD || r.nsym > jobs[j].cap || r.bb_nsym > r.nsym || r.bb < jobs[j].start || r.stop < r.bb || r.stop > 8 * n + 64) {
        r.status = C3_GZ_BAD; r.reason = C3_INF_HEADER; r.nsym = r.bb_nsym = 0;
      }
    }
    return 0;
  }
  int begin_output(int64_t bytes) {
    d_text = nullptr;
    return place ? place(bytes, &d_text) : 0;
  }
  int put(const char* from, int64_t at, int64_t len) {
    if (d_text && len > 0) ZCHK(hipMemcpyAsync(d_text + at, from, (size_t)len, hipMemcpyHostToDevice, z->stream), "copy in");
    if (d_text) ZCHK(hipStreamSynchronize(z->stream), "copy in");
    return 0;
  }
  int finish(const C3GzSeg* segs, int ns, const uint8_t* win0, char* dst, int64_t base, int64_t bytes, uint32_t* crc, int* bad) {
    const uint32_t CH = (uint32_t)c3k_gunzip_chunk();
    chunks.clear();
    for (int s = 0; s < ns; ++s)
      for (uint32_t f = 0; f < segs[s].nsym; f += CH) chunks.push_back(C3GzChunk{(uint32_t)s, f, std::min(CH, segs[s].nsym - f), 0});
    const int nch = (int)chunks.size();
    for (int s = 0; s < ns; ++s) { crc[s] = 0; bad[s] = 0; }
    if (!nch) return 0;
    ZCHK(z->gz_segs.ensure((size_t)ns * sizeof(C3GzSeg)), "segments");
    ZCHK(z->gz_chunks.ensure((size_t)nch * sizeof(C3GzChunk)), "chunks");
    ZCHK(z->gz_cres.ensure((size_t)nch * sizeof(uint2)), "chunk results");
    ZCHK(z->gz_wins.ensure((size_t)ns * C3_GZ_WIN), "windows");
    if (!d_text) ZCHK(z->gz_out.ensure((size_t)bytes + 256), "output buffer");
    uint8_t* d_out = d_text ? d_text + base : z->gz_out.as<uint8_t>();
    ZCHK(hipMemcpyAsync(z->gz_segs.p, segs, (size_t)ns * sizeof(C3GzSeg), hipMemcpyHostToDevice, z->stream), "copy in");
    ZCHK(hipMemcpyAsync(z->gz_chunks.p, chunks.data(), (size_t)nch * sizeof(C3GzChunk), hipMemcpyHostToDevice, z->stream), "copy in");
    ZCHK(hipMemcpyAsync(z->gz_wins.p, win0, C3_GZ_WIN, hipMemcpyHostToDevice, z->stream), "copy in");
    c3k_launch_gunzip_window(z->gz_arena.as<uint16_t>(), z->gz_segs.as<C3GzSeg>(), ns, z->gz_wins.as<uint8_t>(), z->stream);
    ZCHK(hipGetLastError(), "k_gunzip_window launch");
    c3k_launch_gunzip_resolve(z->gz_arena.as<uint16_t>(), z->gz_segs.as<C3GzSeg>(), z->gz_chunks.as<C3GzChunk>(), nch, z->gz_wins.as<uint8_t>(),
                              d_out, z->gz_cres.as<uint2>(), z->stream);
    ZCHK(hipGetLastError(), "k_gunzip_resolve launch");
    cres.resize((size_t)nch);
    ZCHK(hipMemcpyAsync(cres.data(), z->gz_cres.p, (size_t)nch * sizeof(uint2), hipMemcpyDeviceToHost, z->stream), "k_gunzip_resolve");
    const int64_t keep = d_text ? std::min<int64_t>(bytes, C3_GZ_WIN) : bytes;       // the text stays on the device: only the next window comes back
    ZCHK(hipMemcpyAsync(dst + bytes - keep, d_out + bytes - keep, (size_t)keep, hipMemcpyDeviceToHost, z->stream), "copy out");
    ZCHK(hipStreamSynchronize(z->stream), "k_gunzip_resolve");
    uint32_t x2n[36];
    c3_gz_x2n_init(x2n);
    for (int c = 0; c < nch; ++c) {
      const int s = (int)chunks[(size_t)c].seg;
      crc[s] = c3_gz_crc_shift(x2n, chunks[(size_t)c].len, crc[s]) ^ cres[(size_t)c].x;
      if (cres[(size_t)c].y) bad[s] = 1;
    }
    return 0;
  }
};

}  // namespace

extern "C" int c3_gunzip(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!z) return host_fail(C3_E_ARG, "c3_gunzip: bad arguments");
  int rc = 0;
  if (!c3gz::check_args("c3_gunzip", src, n, dst, cap, out_len, &rc)) return rc;
  int64_t* st = c3_gunzip_stats_slot();
  memset(st, 0, C3_GZS_N * sizeof(int64_t));
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  DevBackend be{z, (const uint8_t*)src, n};
  if ((rc = be.upload()) != 0) return rc;
  c3gz::Run<DevBackend> run{"c3_gunzip", be, (const uint8_t*)src, n, dst, cap, c3gz::options(0), st};
  rc = run.run(out_len);
  (void)hipStreamSynchronize(z->stream);
  return rc;
}

// ---- the reader's stream (c3_reader_gunzip_on_device) -------------------------------------------------------------------------
// The file is read as it is needed: the loaded bytes reach from the dword row of the true position to a stretch and a
// look-ahead behind it (a piece runs on to the first block boundary behind the stretch, a member may end and the next header
// begin there).  A stretch that runs out of loaded bytes changes nothing and is run again with the look-ahead doubled, so
// what a stretch boundary cuts -- a block, a trailer, a member header -- is carried as the position in front of it.  `out`
// keeps the last 32 KiB delivered in front of the stretch's bytes: the window the next stretch starts from.
struct c3_gunzip_stream {
  c3_bgzf* z = nullptr;
  FILE* fp = nullptr; int64_t file_size = 0, look = 4 << 20;
  std::vector<uint8_t> buf; int64_t boff = 0;                // file bytes [boff, boff + buf.size())
  std::vector<char> out;
  DevBackend be{nullptr, nullptr, 0};
  c3gz::Run<DevBackend>* run = nullptr;
  int64_t pos = 0, stats[C3_GZS_N] = {0};
  bool started = false, failed = false;

  // bytes [from rounded down to 256, upto) of the file (or to its end) loaded and on the device
  int load(int64_t from, int64_t upto) {
    const int64_t nb = from & ~(int64_t)255, end = boff + (int64_t)buf.size();
    upto = std::min(upto, file_size);
    if (nb >= end) { buf.clear(); boff = nb; if (fseek(fp, (long)nb, SEEK_SET) != 0) return host_fail(C3_E_ARG, "gzip input: cannot seek"); }
    else if (nb > boff) { buf.erase(buf.begin(), buf.begin() + (nb - boff)); boff = nb; }
    const int64_t have = boff + (int64_t)buf.size();
    if (upto > have) {
      const size_t old = buf.size();
      buf.resize(old + (size_t)(upto - have));
      if (fread(buf.data() + old, 1, (size_t)(upto - have), fp) != (size_t)(upto - have)) return host_fail(C3_E_ARG, "gzip input: the file is shorter than it was");
    }
    const uint8_t* base = (const uint8_t*)((uintptr_t)buf.data() - (uintptr_t)boff);      // byte k of the file at base + k
    run->src = be.src = base;
    run->n = be.n = boff + (int64_t)buf.size();
    be.boff = boff;
    run->more = run->n < file_size;
    return be.upload();
  }
  // the next stretch into `out` (and, with be.place set, onto the device).  *bytes of it lie at out[*at ..)
  int next(int64_t* at, int64_t* bytes) {
    *at = *bytes = 0;
    if (failed) return C3_E_DATA;
    if (started && pos < 0) return C3_E_OK;
    ZCHK(hipSetDevice(z->device), "hipSetDevice");
    for (;;) {
      int rc = load(started ? pos >> 3 : 0, (started ? pos >> 3 : 0) + run->opt.stretch + look);
      if (rc == C3_E_OK && !started) {
        int64_t data = 0;
        const int why = c3gz::member_header(run->src, run->n, 0, &data);
        if (why == C3_INF_INPUT && run->more) rc = C3_GZ_AGAIN;
        else if (why) rc = c3gz::data_error(run->who, 0, 0, why);
        else { pos = 8 * data; started = true; }
      }
      if (rc == C3_E_OK) {
        const int64_t keep = std::min<int64_t>(C3_GZ_WIN, run->o);           // the window of this stretch moves to the front
        memmove(out.data(), out.data() + run->o - keep, (size_t)keep);
        run->o = keep;
        rc = run->stretch(&pos);
        if (rc == C3_E_OK) { *at = keep; *bytes = run->o - keep; return C3_E_OK; }
      }
      if (rc != C3_GZ_AGAIN) { failed = true; return rc; }
      look *= 2;
    }
  }
};

extern "C" int c3_gunzip_stream_open(c3_bgzf* z, const char* path, c3_gunzip_stream** out) {
  if (!z || !path || !out) return host_fail(C3_E_ARG, "c3_gunzip_stream_open: bad arguments");
  *out = nullptr;
  FILE* f = fopen(path, "rb");
  if (!f) return host_fail(C3_E_ARG, "c3_gunzip_stream_open: cannot open the file");
  c3_gunzip_stream* s = new c3_gunzip_stream();
  s->z = z; s->fp = f;
  s->look = c3gz::env_num("C3_GUNZIP_LOOK", 64, 1 << 30, 4 << 20);         // test hook: stretches that run out of loaded bytes
  fseek(f, 0, SEEK_END); s->file_size = (int64_t)ftell(f); rewind(f);
  s->be = DevBackend{z, nullptr, 0};
  s->out.resize((size_t)1 << 20);
  s->run = new c3gz::Run<DevBackend>{"gzip input", s->be, nullptr, 0, s->out.data(), (int64_t)s->out.size(), c3gz::options(0), s->stats};
  s->run->grow = &s->out;
  c3_gz_x2n_init(s->run->x2n);
  *out = s;
  return C3_E_OK;
}

// the next stretch inflated and brought to the host: *bytes of it at *text (valid until the next call); *eof: the file ends behind it
extern "C" int c3_gunzip_stream_next(c3_gunzip_stream* s, const char** text, int64_t* bytes, int* eof) {
  if (!s || !text || !bytes || !eof) return host_fail(C3_E_ARG, "c3_gunzip_stream_next: bad arguments");
  s->be.place = nullptr;
  int64_t at = 0;
  const int rc = s->file_size == 0 ? (int)C3_E_OK : s->next(&at, bytes);
  *text = s->out.data() + at;
  *eof = s->file_size == 0 || (s->started && s->pos < 0);
  return rc;
}

// the next stretch inflated behind the carry into the slot's text, left there and parsed by k_fastq (c3_bgzf_stretch_parse's rule)
extern "C" int c3_gunzip_stream_next_parse(c3_gunzip_stream* s, int slot, int64_t carry_from, int64_t carry_len, int* eof, int64_t* bytes, c3_fq_stretch* fq) {
  if (!s || !eof || !bytes || !fq) return host_fail(C3_E_ARG, "c3_gunzip_stream_next_parse: bad arguments");
  memset(fq, 0, sizeof *fq);
  c3_bgzf* z = s->z;
  bool placed = false;
  s->be.place = [&](int64_t n_bytes, uint8_t** d_text) { placed = true; return c3h::stretch_text_begin(z, slot, carry_from, carry_len, n_bytes, false, d_text); };
  int64_t at = 0;
  int rc = s->file_size == 0 ? (int)C3_E_OK : s->next(&at, bytes);
  s->be.place = nullptr;
  *eof = s->file_size == 0 || (s->started && s->pos < 0);
  if (rc != C3_E_OK) return rc;
  if (!placed) {                                             // (nothing left to inflate: the carry alone)
    uint8_t* d = nullptr;
    if ((rc = c3h::stretch_text_begin(z, slot, carry_from, carry_len, 0, false, &d)) != C3_E_OK) return rc;
  }
  return c3h::stretch_text_parse(z, slot, carry_len + *bytes, false, 0, *eof, fq);
}

extern "C" void c3_gunzip_stream_stats(const c3_gunzip_stream* s, int64_t* v, int n) { for (int i = 0; i < n; ++i) v[i] = s && i < C3_GZS_N ? s->stats[i] : 0; }
extern "C" void c3_gunzip_stream_close(c3_gunzip_stream* s) {
  if (!s) return;
  (void)hipSetDevice(s->z->device);
  (void)hipStreamSynchronize(s->z->stream);
  if (s->fp) fclose(s->fp);
  delete s->run;
  delete s;
}

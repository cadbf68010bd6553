// c3_stream.hip -- the stream handle c3_bgzf (include/c3poa.h): BGZF output and input, FASTQ records parsed on the GPU, and the
// reader's device stretches.  It shares no state with c3_handle; errors go to the text of c3_last_error(NULL) (ZCHK, host_fail).
#include "c3_host.h"
#include "c3_bgzf.h"
#include "c3_fastq.h"
#include "c3_bam.h"
#include "c3_inflate.h"

// ---- BGZF output (k_bgzf.hip; host statement c3_bgzf.cpp) ---------------------------------
// Input goes to the device in chunks of BGZF_CHUNK_BLOCKS blocks: staged in (host pieces land back to back; a device stream is
// copied device to device), k_bgzf + k_bgzf_pack, the member sizes back, then one copy of the packed members straight into the
// caller's buffer.  One loop serves c3_bgzf_compress_pieces, the two text paths and c3_batch_emit_fetch.
c3h::ZStatus c3h::bgzf_chunks(ZStage& z, hipStream_t s, int64_t len, const ZStageIn& stage_in, char* arena, int64_t cap, int64_t* out, bool wait_after_copy_out) {
  ZStatus st;
#define ZSTEP(x, w) do { if ((st.e = (x)) != hipSuccess) { st.what = w; return st; } } while (0)
  const char* env = getenv("C3_BGZF_CHUNK");                          // test hook: the loop's later rounds at a small size
  const int blocks = env ? atoi(env) : 0;
  const int64_t CH = (int64_t)(blocks >= 1 && blocks <= BGZF_CHUNK_BLOCKS ? blocks : BGZF_CHUNK_BLOCKS) * BGZF_BLOCK;
  for (int64_t c0 = 0; c0 < len; c0 += CH) {
    const int64_t cn = std::min(CH, len - c0);
    const int nb = (int)((cn + BGZF_BLOCK - 1) / BGZF_BLOCK);
    ZSTEP(z.reserve(cn), "staging buffers");
    ZSTEP(stage_in(z.zin.as<char>(), c0, cn), "copy in");
    c3k_launch_bgzf(z.zin.as<uint8_t>(), (long long)cn, nb, z.zslots.as<uint8_t>(), z.zsizes.as<int>(), z.zpacked.as<uint8_t>(), s);
    ZSTEP(hipGetLastError(), "k_bgzf launch");
    ZSTEP(hipMemcpyAsync(z.h_sizes, z.zsizes.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, s), "k_bgzf");
    ZSTEP(hipStreamSynchronize(s), "k_bgzf");
    ++st.waits;
    int64_t tot = 0;
    for (int b = 0; b < nb; ++b) {
      const int sz = z.h_sizes[b];
      if (sz < BGZF_HDR + 13 || sz > BGZF_MAX_MEMBER) { st.bad = ZStatus::MEMBER_SIZE; return st; }
      tot += sz;
    }
    if (*out + tot > cap) { st.bad = ZStatus::BEYOND_BOUND; return st; }      // (cannot be: cap >= the sum of the bounds)
    ZSTEP(hipMemcpyAsync(arena + *out, z.zpacked.p, (size_t)tot, hipMemcpyDeviceToHost, s), "copy out");
    if (wait_after_copy_out) { ZSTEP(hipStreamSynchronize(s), "copy out"); ++st.waits; }      // (zpacked is written again by the next chunk)
    *out += tot;
  }
#undef ZSTEP
  return st;
}

extern "C" int c3_bgzf_create(int device, c3_bgzf** out) {
  if (!out) return C3_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return host_fail(C3_E_NO_DEVICE, "no HIP device: the c3poa HIP backend has no CPU fallback"); }
  if (device < 0 || device >= ndev) return host_fail(C3_E_ARG, "bad device ordinal");
  c3_bgzf* z = new c3_bgzf();
  z->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = z->zs.pin();
  if (e != hipSuccess) { c3_bgzf_destroy(z); return host_fail(C3_E_HIP, hipGetErrorString(e)); }
  *out = z;
  return C3_E_OK;
}

extern "C" void c3_bgzf_destroy(c3_bgzf* z) {
  if (!z) return;
  (void)hipSetDevice(z->device);
  if (z->stream) { (void)hipStreamSynchronize(z->stream); (void)hipStreamDestroy(z->stream); }
  if (z->h_mem) (void)hipHostFree(z->h_mem);
  if (z->h_res) (void)hipHostFree(z->h_res);
  if (z->copy_stream) { (void)hipStreamSynchronize(z->copy_stream); (void)hipStreamDestroy(z->copy_stream); }
  if (z->h_hdr) (void)hipHostFree(z->h_hdr);
  if (z->h_bhdr) (void)hipHostFree(z->h_bhdr);
  for (auto& f : z->fq) { if (f.h_off) (void)hipHostFree(f.h_off); if (f.h_name_off) (void)hipHostFree(f.h_name_off); }
  delete z;
}

// the concatenation of pieces p[0..np) compressed as one text (the writers' formatter slices, c3_writer.cpp)
extern "C" int c3_bgzf_compress_pieces(c3_bgzf* z, const char* const* p, const int64_t* len, int np, char* dst, int64_t cap, int64_t* out_len) {
  if (!z || !out_len || np < 0 || (np > 0 && (!p || !len))) return host_fail(C3_E_ARG, "c3_bgzf_compress: bad arguments");
  int64_t n = 0;
  for (int i = 0; i < np; ++i) { if (len[i] < 0 || (len[i] > 0 && !p[i])) return host_fail(C3_E_ARG, "c3_bgzf_compress: bad piece"); n += len[i]; }
  if (cap < c3_bgzf_bound(n) || (n > 0 && !dst)) return host_fail(C3_E_ARG, "c3_bgzf_compress: cap < c3_bgzf_bound(n)");
  *out_len = 0;
  if (n == 0) return C3_E_OK;
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  ZCHK(z->zs.reserve(n), "staging buffers");
  int pi = 0; int64_t pin = 0;                                  // piece index / bytes of it already sent
  auto pieces_in = [&](char* d_zin, int64_t, int64_t cn) {
    for (int64_t at = 0; at < cn;) {
      while (pi < np && pin == len[pi]) { ++pi; pin = 0; }
      const int64_t k = std::min(len[pi] - pin, cn - at);
      const hipError_t e = hipMemcpyAsync(d_zin + at, p[pi] + pin, (size_t)k, hipMemcpyHostToDevice, z->stream);
      if (e != hipSuccess) return e;
      at += k; pin += k;
    }
    return hipSuccess;
  };
  int64_t o = 0;
  const c3h::ZStatus st = c3h::bgzf_chunks(z->zs, z->stream, n, pieces_in, dst, cap, &o, true);
  if (st.e != hipSuccess) return bgzf_fail(st.e, st.what);
  if (st.bad) return host_fail(C3_E_HIP, st.bad == c3h::ZStatus::MEMBER_SIZE ? "k_bgzf: member size out of range" : "k_bgzf: members beyond their bound");
  *out_len = o;
  return C3_E_OK;
}

extern "C" int c3_bgzf_compress(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!z || !out_len || n < 0 || (n > 0 && !src)) return host_fail(C3_E_ARG, "c3_bgzf_compress: bad arguments");
  return c3_bgzf_compress_pieces(z, &src, &n, 1, dst, cap, out_len);
}

// ---- BGZF input (k_inflate.hip; host statement c3_inflate.cpp) ----------------------------
// The host walks the member headers (c3_bgzf_member_at); INFLATE_CHUNK_MEMBERS members at a time go to the device: their
// bytes as they stand in src, the descriptors, k_inflate, (status, CRC) back, and -- only when every member of the chunk
// was accepted -- the inflated bytes straight into the caller's buffer.
#define INFLATE_CHUNK_MEMBERS 4096             // measured 1 024 .. 16 384 per launch: 2 048 leaves 2 waves per SIMD
static int inflate_chunk() {                                          // C3_INFLATE_CHUNK: measurement hook (tools/inflate_throughput.py)
  static const int v = [] { const char* e = getenv("C3_INFLATE_CHUNK"); const int x = e ? atoi(e) : 0; return x >= 64 && x <= 16384 ? x : INFLATE_CHUNK_MEMBERS; }();
  return v;
}

// nm members of src (all accepted by c3_bgzf_scan) inflated into the caller's dst, or -- d_dst != null -- left on the device
// at d_dst (the reader's device parse); either way every member's CRC is compared here before the call returns
static int bgzf_inflate_members(c3_bgzf* z, const char* src, int64_t n, int64_t nm, uint8_t* d_dst, char* dst, int64_t* out_len) {
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  const int CH = inflate_chunk();
  if (!z->h_mem) ZCHK(hipHostMalloc((void**)&z->h_mem, CH * sizeof(C3BgzfMember), hipHostMallocDefault), "descriptor buffers");
  if (!z->h_res) ZCHK(hipHostMalloc((void**)&z->h_res, CH * sizeof(int2), hipHostMallocDefault), "descriptor buffers");
  ZCHK(z->d_mem.ensure(CH * sizeof(C3BgzfMember)), "descriptors");
  ZCHK(z->d_res.ensure(CH * sizeof(int2)), "statuses");
  int64_t at = 0, o = 0, done = 0;
  while (done < nm) {
    const int k = (int)std::min<int64_t>(CH, nm - done);
    const int64_t c0 = at;
    uint32_t oo = 0;
    for (int i = 0; i < k; ++i) {
      C3BgzfMember& m = z->h_mem[i];
      const uint32_t size = c3_bgzf_member_at((const unsigned char*)src, n, at, &m);      // (c3_bgzf_scan accepted them all)
      m.poff += (uint32_t)(at - c0); m.ooff = oo;
      oo += m.isize; at += size;
    }
    const int64_t cn = at - c0;
    ZCHK(z->zs.zin.ensure((size_t)cn + 256), "input buffer");
    if (!d_dst) ZCHK(z->d_out.ensure((size_t)oo + 256), "output buffer");
    ZCHK(hipMemcpyAsync(z->zs.zin.p, src + c0, (size_t)cn, hipMemcpyHostToDevice, z->stream), "copy in");
    ZCHK(hipMemcpyAsync(z->d_mem.p, z->h_mem, (size_t)k * sizeof(C3BgzfMember), hipMemcpyHostToDevice, z->stream), "copy in");
    c3k_launch_inflate(z->zs.zin.as<uint8_t>(), z->d_mem.as<C3BgzfMember>(), k, d_dst ? d_dst + o : z->d_out.as<uint8_t>(), z->d_res.as<int2>(), z->stream);
    ZCHK(hipGetLastError(), "k_inflate launch");
    ZCHK(hipMemcpyAsync(z->h_res, z->d_res.p, (size_t)k * sizeof(int2), hipMemcpyDeviceToHost, z->stream), "k_inflate");
    ZCHK(hipStreamSynchronize(z->stream), "k_inflate");
    for (int i = 0; i < k; ++i) {
      int st = z->h_res[i].x;
      if (st == C3_INF_OK && (uint32_t)z->h_res[i].y != z->h_mem[i].crc) st = C3_INF_CRC;
      if (st != C3_INF_OK) return c3_bgzf_data_error("c3_bgzf_decompress", done + i, st);
    }
    if (oo && !d_dst) {
      ZCHK(hipMemcpyAsync(dst + o, z->d_out.p, (size_t)oo, hipMemcpyDeviceToHost, z->stream), "copy out");
      ZCHK(hipStreamSynchronize(z->stream), "copy out");
    }
    o += oo; done += k;
  }
  *out_len = o;
  return C3_E_OK;
}

int c3h::bgzf_inflate_to_device(c3_bgzf* z, const char* src, int64_t n, int64_t nm, uint8_t* d_dst, int64_t* out_len) {
  return bgzf_inflate_members(z, src, n, nm, d_dst, nullptr, out_len);
}

extern "C" int c3_bgzf_decompress(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!z || !out_len || n < 0 || (n > 0 && !src)) return host_fail(C3_E_ARG, "c3_bgzf_decompress: bad arguments");
  *out_len = 0;
  int64_t nm = 0, ob = 0;
  const int rc = c3_bgzf_scan(src, n, &nm, &ob);
  if (rc) return rc;
  if (cap < ob || (ob > 0 && !dst)) return host_fail(C3_E_ARG, "c3_bgzf_decompress: cap < inflated size (c3_bgzf_scan)");
  if (nm == 0) return C3_E_OK;
  return bgzf_inflate_members(z, src, n, nm, nullptr, dst, out_len);
}

// ---- FASTQ records on the GPU (k_fastq.hip; host statement c3_fastq.cpp) -------------------
// One parse = three waits: the line count (sizes nl[] and the record tables), the header (sizes the outputs, answers the
// capacity question before any byte is gathered), the finished arrays.
static int fq_prepare(c3_bgzf* z) {
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  if (!z->h_hdr) ZCHK(hipHostMalloc((void**)&z->h_hdr, sizeof(C3FqHdr), hipHostMallocDefault), "k_fastq buffers");
  if (!z->copy_stream) ZCHK(hipStreamCreateWithFlags(&z->copy_stream, hipStreamNonBlocking), "k_fastq buffers");
  ZCHK(z->d_hdr.ensure(sizeof(C3FqHdr)), "k_fastq buffers");
  return C3_E_OK;
}

// the text [lo, lo + n) of sl.text parsed: tables and header on the device, *info filled; no byte gathered yet
static int fq_parse_device(c3_bgzf* z, c3_bgzf::FqSlot& sl, uint32_t lo, int64_t n, int at_eof, int min_len, c3_fastq_info* info) {
  memset(info, 0, sizeof *info);
  sl.n_rec = 0;
  if (n == 0) return C3_E_OK;
  const uint32_t hi = lo + (uint32_t)n;
  const size_t tiles = ((size_t)hi + 65535) / 65536;
  const uint8_t* buf = sl.text.as<uint8_t>();
  C3FqHdr* hdr = z->d_hdr.as<C3FqHdr>();
  ZCHK(z->d_cnt.ensure(tiles * 4 * sizeof(int32_t)), "k_fastq counts");
  c3k_launch_fastq_count(buf, lo, hi, z->d_cnt.as<int32_t>(), at_eof, hdr, z->stream);
  ZCHK(hipGetLastError(), "k_fastq_count launch");
  ZCHK(hipMemcpyAsync(z->h_hdr, hdr, sizeof(C3FqHdr), hipMemcpyDeviceToHost, z->stream), "k_fastq_count");
  ZCHK(hipStreamSynchronize(z->stream), "k_fastq_count");
  const int L = z->h_hdr->n_lines, Lv = z->h_hdr->n_lines_v;
  if (L < 0 || (int64_t)L > n || Lv < L || Lv > L + 1) return host_fail(C3_E_HIP, "k_fastq: line count out of range");
  const int n_full = Lv / 4, partial = (at_eof && (Lv & 3)) ? 1 : 0;
  if (n_full == 0 && !partial) return C3_E_OK;                        // no whole record yet: everything stays unconsumed
  const size_t nr = (size_t)n_full + 1, nb = ((size_t)n_full + 255) / 256;
  ZCHK(z->d_nl.ensure(((size_t)L + 4) * sizeof(int32_t)), "k_fastq lines");
  ZCHK(z->d_slen.ensure(nr * sizeof(int32_t)), "k_fastq records");
  ZCHK(z->d_nlen.ensure(nr * sizeof(int32_t)), "k_fastq records");
  ZCHK(z->d_bsum.ensure((nb + 1) * 3 * sizeof(long long)), "k_fastq sums");
  ZCHK(sl.off.ensure(nr * sizeof(int64_t)), "k_fastq offsets");
  ZCHK(sl.name_off.ensure(nr * sizeof(int64_t)), "k_fastq offsets");
  ZCHK(sl.src.ensure(nr * sizeof(int4)), "k_fastq sources");
  c3k_launch_fastq_lines(buf, lo, hi, z->d_cnt.as<int32_t>(), z->d_nl.as<int32_t>(), z->stream);
  c3k_launch_fastq_records(buf, lo, hi, z->d_nl.as<int32_t>(), L, n_full, partial, min_len, z->d_slen.as<int32_t>(), z->d_nlen.as<int32_t>(),
                           z->d_bsum.as<long long>(), hdr, sl.off.as<int64_t>(), sl.name_off.as<int64_t>(), sl.src.as<int4>(), z->stream);
  ZCHK(hipGetLastError(), "k_fastq_records launch");
  ZCHK(hipMemcpyAsync(z->h_hdr, hdr, sizeof(C3FqHdr), hipMemcpyDeviceToHost, z->stream), "k_fastq_records");
  ZCHK(hipStreamSynchronize(z->stream), "k_fastq_records");
  const C3FqHdr& h = *z->h_hdr;
  if (h.n_records < 0 || h.n_records > n_full || h.n_kept < 0 || h.n_kept > h.n_records || h.consumed < 0 || h.consumed > n ||
      h.base_bytes < 0 || h.base_bytes > n || h.name_bytes < 0 || h.name_bytes > n) return host_fail(C3_E_HIP, "k_fastq: header out of range");
  info->n_records = h.n_records; info->n_kept = h.n_kept; info->n_short = h.n_short; info->consumed = h.consumed;
  info->name_bytes = h.name_bytes; info->base_bytes = h.base_bytes; info->departed = h.departed;
  sl.n_rec = h.n_kept;
  return C3_E_OK;
}

// the kept records of the parse that fq_parse_device just made, gathered into sl.names / sl.seqs / sl.quals (queued, not waited for)
static int fq_gather_device(c3_bgzf* z, c3_bgzf::FqSlot& sl, const c3_fastq_info& info, bool bam = false) {
  if (info.n_kept == 0) return C3_E_OK;
  ZCHK(sl.names.ensure((size_t)info.name_bytes + 256), "k_fastq names");
  ZCHK(sl.seqs.ensure((size_t)info.base_bytes + 256), "k_fastq bases");
  ZCHK(sl.quals.ensure((size_t)info.base_bytes + 256), "k_fastq qualities");
  (bam ? c3k_launch_bam_gather : c3k_launch_fastq_gather)(sl.text.as<uint8_t>(), sl.src.as<int4>(), sl.off.as<int64_t>(), sl.name_off.as<int64_t>(), (long long)info.n_kept,
                                                          sl.names.as<uint8_t>(), sl.seqs.as<uint8_t>(), sl.quals.as<uint8_t>(), z->stream);
  ZCHK(hipGetLastError(), bam ? "k_bam_gather launch" : "k_fastq_gather launch");
  return C3_E_OK;
}

extern "C" int c3_fastq_parse(c3_bgzf* z, const char* text, int64_t n, int at_eof, int min_len, char* names, int64_t names_cap,
                              int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off, int64_t max_records,
                              c3_fastq_info* info) {
  int rc = c3_fastq_check_args("c3_fastq_parse", text, n, names, names_cap, name_off, seqs, quals, bases_cap, off, max_records, info);
  if (rc) return rc;
  if (!z) return host_fail(C3_E_ARG, "c3_fastq_parse: null handle");
  if (n == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  if ((rc = fq_prepare(z)) != C3_E_OK) return rc;
  c3_bgzf::FqSlot& sl = z->fq[0];
  const uint32_t lo = (uint32_t)((uintptr_t)text & 3u);               // the text keeps its place inside a dword: the kernels see the caller's misalignment
  ZCHK(sl.text.ensure((size_t)lo + (size_t)n + 256), "k_fastq text");
  ZCHK(hipMemcpyAsync(sl.text.as<char>() + lo, text, (size_t)n, hipMemcpyHostToDevice, z->stream), "copy in");
  if ((rc = fq_parse_device(z, sl, lo, n, at_eof, min_len, info)) != C3_E_OK) return rc;
  if (info->n_kept > max_records || info->name_bytes > names_cap || info->base_bytes > bases_cap) {
    return host_fail(C3_E_LIMIT, "c3_fastq_parse: capacity too small (needed sizes in info)");
  }
  if (info->n_kept == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  if ((rc = fq_gather_device(z, sl, *info)) != C3_E_OK) return rc;
  const size_t nt = ((size_t)info->n_kept + 1) * sizeof(int64_t);
  ZCHK(hipMemcpyAsync(off, sl.off.p, nt, hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
  ZCHK(hipMemcpyAsync(name_off, sl.name_off.p, nt, hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
  if (info->name_bytes) ZCHK(hipMemcpyAsync(names, sl.names.p, (size_t)info->name_bytes, hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
  if (info->base_bytes) ZCHK(hipMemcpyAsync(seqs, sl.seqs.p, (size_t)info->base_bytes, hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
  if (info->base_bytes) ZCHK(hipMemcpyAsync(quals, sl.quals.p, (size_t)info->base_bytes, hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
  ZCHK(hipStreamSynchronize(z->stream), "k_fastq_gather");
  return C3_E_OK;
}

// ---- Unaligned BAM records on the GPU (k_bam.hip; host statement c3_bam.cpp) ---------------
// One parse = three waits, as for FASTQ: the chain (header status, number of record starts: sizes rec_pos[] and the record
// tables), the header after the scans (sizes the outputs, answers the capacity question), the finished arrays.
static int bam_prepare(c3_bgzf* z) {
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  if (!z->h_bhdr) ZCHK(hipHostMalloc((void**)&z->h_bhdr, sizeof(C3BamHdr), hipHostMallocDefault), "k_bam buffers");
  if (!z->copy_stream) ZCHK(hipStreamCreateWithFlags(&z->copy_stream, hipStreamNonBlocking), "k_bam buffers");
  ZCHK(z->d_bhdr.ensure(sizeof(C3BamHdr)), "k_bam buffers");
  return C3_E_OK;
}

// the data [lo, lo + n) of sl.text parsed: tables and header on the device, *info filled; no byte gathered yet
static int bam_parse_device(c3_bgzf* z, c3_bgzf::FqSlot& sl, uint32_t lo, int64_t n, int at_start, int at_eof, int min_len, c3_bam_info* info) {
  memset(info, 0, sizeof *info);
  sl.n_rec = 0;
  if (n == 0) return C3_E_OK;
  const uint32_t hi = lo + (uint32_t)n;
  const size_t tiles = ((size_t)hi + C3_BAM_TILE - 1) / C3_BAM_TILE;
  const uint8_t* buf = sl.text.as<uint8_t>();
  C3BamHdr* hdr = z->d_bhdr.as<C3BamHdr>();
  ZCHK(z->d_tiles.ensure(tiles * sizeof(C3BamTile)), "k_bam tiles");
  c3k_launch_bam_chain(buf, lo, hi, at_start, z->d_tiles.as<C3BamTile>(), hdr, z->stream);
  ZCHK(hipGetLastError(), "k_bam chain launch");
  ZCHK(hipMemcpyAsync(z->h_bhdr, hdr, sizeof(C3BamHdr), hipMemcpyDeviceToHost, z->stream), "k_bam chain");
  ZCHK(hipStreamSynchronize(z->stream), "k_bam chain");
  {
    const C3BamHdr& h = *z->h_bhdr;
    if (h.hstat == C3_BAM_HEADER) { info->departed = 1; info->reason = C3_BAM_HEADER; return C3_E_OK; }
    if (h.hstat == C3_BAM_INCOMPLETE) { if (at_eof) { info->departed = 1; info->reason = C3_BAM_TRUNCATED; } return C3_E_OK; }      // consumed = 0
    if (h.hstat != C3_BAM_OK || h.start < (int64_t)lo || h.start > (int64_t)hi || h.n_starts < 0 || h.n_starts > n / (4 + C3_BAM_MIN_BLOCK) + 1 ||
        (h.n_starts == 0 && h.start != (int64_t)hi)) return host_fail(C3_E_HIP, "k_bam: chain out of range");
    info->header_bytes = at_start ? h.start - (int64_t)lo : 0;
    if (h.n_starts == 0) { info->consumed = h.start - (int64_t)lo; return C3_E_OK; }        // the header alone
  }
  const int ns = (int)z->h_bhdr->n_starts;
  const size_t nr = (size_t)ns + 1, nb = ((size_t)ns + 255) / 256;
  ZCHK(z->d_rpos.ensure(nr * sizeof(uint32_t)), "k_bam records");
  ZCHK(z->d_slen.ensure(nr * sizeof(int32_t)), "k_bam records");
  ZCHK(z->d_nlen.ensure(nr * sizeof(int32_t)), "k_bam records");
  ZCHK(z->d_reason.ensure(nr * sizeof(int32_t)), "k_bam records");
  ZCHK(z->d_rsrc.ensure(nr * sizeof(int4)), "k_bam records");
  ZCHK(z->d_bsum.ensure((nb + 1) * 3 * sizeof(long long)), "k_bam sums");
  ZCHK(sl.off.ensure(nr * sizeof(int64_t)), "k_bam offsets");
  ZCHK(sl.name_off.ensure(nr * sizeof(int64_t)), "k_bam offsets");
  ZCHK(sl.src.ensure(nr * sizeof(int4)), "k_bam sources");
  c3k_launch_bam_records(buf, lo, hi, z->d_tiles.as<C3BamTile>(), ns, at_eof, min_len, z->d_rpos.as<uint32_t>(), z->d_slen.as<int32_t>(),
                         z->d_nlen.as<int32_t>(), z->d_reason.as<int32_t>(), z->d_rsrc.as<int4>(), z->d_bsum.as<long long>(), hdr,
                         sl.off.as<int64_t>(), sl.name_off.as<int64_t>(), sl.src.as<int4>(), z->stream);
  ZCHK(hipGetLastError(), "k_bam_records launch");
  ZCHK(hipMemcpyAsync(z->h_bhdr, hdr, sizeof(C3BamHdr), hipMemcpyDeviceToHost, z->stream), "k_bam_records");
  ZCHK(hipStreamSynchronize(z->stream), "k_bam_records");
  const C3BamHdr& h = *z->h_bhdr;
  if (h.n_records < 0 || h.n_records > ns || h.n_kept < 0 || h.n_kept > h.n_records || h.consumed < 0 || h.consumed > n ||
      h.base_bytes < 0 || h.base_bytes > n || h.name_bytes < 0 || h.name_bytes > n || h.bad_at < 0 || h.bad_at > n ||
      h.reason < 0 || h.reason > C3_BAM_TRUNCATED) return host_fail(C3_E_HIP, "k_bam: header out of range");
  info->n_records = h.n_records; info->n_kept = h.n_kept; info->n_short = h.n_short; info->consumed = h.consumed;
  info->name_bytes = h.name_bytes; info->base_bytes = h.base_bytes; info->departed = h.departed; info->reason = h.reason; info->bad_at = h.bad_at;
  sl.n_rec = h.n_kept;
  return C3_E_OK;
}

extern "C" int c3_bam_parse(c3_bgzf* z, const char* data, int64_t n, int at_start, int at_eof, int min_len, char* names, int64_t names_cap,
                            int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off, int64_t max_records,
                            c3_bam_info* info) {
  int rc = c3_bam_check_args("c3_bam_parse", data, n, names, names_cap, name_off, seqs, quals, bases_cap, off, max_records, info);
  if (rc) return rc;
  if (!z) return host_fail(C3_E_ARG, "c3_bam_parse: null handle");
  if (n == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  if ((rc = bam_prepare(z)) != C3_E_OK) return rc;
  c3_bgzf::FqSlot& sl = z->fq[0];
  const uint32_t lo = (uint32_t)((uintptr_t)data & 3u);               // the data keeps its place inside a dword: the kernels see the caller's misalignment
  ZCHK(sl.text.ensure((size_t)lo + (size_t)n + 256), "k_bam data");
  ZCHK(hipMemcpyAsync(sl.text.as<char>() + lo, data, (size_t)n, hipMemcpyHostToDevice, z->stream), "copy in");
  if ((rc = bam_parse_device(z, sl, lo, n, at_start, at_eof, min_len, info)) != C3_E_OK) return rc;
  if (info->n_kept > max_records || info->name_bytes > names_cap || info->base_bytes > bases_cap) {
    return host_fail(C3_E_LIMIT, "c3_bam_parse: capacity too small (needed sizes in info)");
  }
  if (info->n_kept == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  c3_fastq_info fi; memset(&fi, 0, sizeof fi);
  fi.n_kept = info->n_kept; fi.name_bytes = info->name_bytes; fi.base_bytes = info->base_bytes;
  if ((rc = fq_gather_device(z, sl, fi, true)) != C3_E_OK) return rc;
  const size_t nt = ((size_t)info->n_kept + 1) * sizeof(int64_t);
  ZCHK(hipMemcpyAsync(off, sl.off.p, nt, hipMemcpyDeviceToHost, z->stream), "k_bam_gather");
  ZCHK(hipMemcpyAsync(name_off, sl.name_off.p, nt, hipMemcpyDeviceToHost, z->stream), "k_bam_gather");
  if (info->name_bytes) ZCHK(hipMemcpyAsync(names, sl.names.p, (size_t)info->name_bytes, hipMemcpyDeviceToHost, z->stream), "k_bam_gather");
  ZCHK(hipMemcpyAsync(seqs, sl.seqs.p, (size_t)info->base_bytes, hipMemcpyDeviceToHost, z->stream), "k_bam_gather");
  ZCHK(hipMemcpyAsync(quals, sl.quals.p, (size_t)info->base_bytes, hipMemcpyDeviceToHost, z->stream), "k_bam_gather");
  ZCHK(hipStreamSynchronize(z->stream), "k_bam_gather");
  return C3_E_OK;
}

// ---- the reader's device stretches (c3_reader.cpp; not part of the public interface) ----------
// Stretch = `carry_len` bytes of the other slot's text from `carry_from` on (the record its end cut), then the inflated
// members of comp; it stays on the device, is parsed there with min_len 0 (the group rule, min_len included, is the
// reader's), and the record tables come back (c3_fq_stretch, c3_checks.h).  On return the slot holds the finished records
// until it is loaded again.
// the two halves around the inflater (k_inflate here, the k_gunzip kernels in c3_gunzip_dev.hip): _begin sizes the slot's text for
// the carry plus `bytes`, copies the carry and says where the inflated bytes go; _parse takes the finished text of `total` bytes
int c3h::stretch_text_begin(c3_bgzf* z, int slot, int64_t carry_from, int64_t carry_len, int64_t bytes, bool bam, uint8_t** d_at) {
  if (!z || slot < 0 || slot > 1 || carry_len < 0 || bytes < 0) return host_fail(C3_E_ARG, "c3_bgzf_stretch_parse: bad arguments");
  const int64_t total = carry_len + bytes;
  if (total > C3_FASTQ_MAX_TEXT) return host_fail(C3_E_LIMIT, "c3_bgzf_stretch_parse: stretch longer than C3_FASTQ_MAX_TEXT");
  int rc;
  if ((rc = bam ? bam_prepare(z) : fq_prepare(z)) != C3_E_OK) return rc;
  c3_bgzf::FqSlot& sl = z->fq[slot];
  const c3_bgzf::FqSlot& other = z->fq[slot ^ 1];
  if (carry_len > 0 && (carry_from < 0 || carry_from + carry_len > other.text_n)) return host_fail(C3_E_ARG, "c3_bgzf_stretch_parse: carry outside the other stretch");
  ZCHK(sl.text.ensure((size_t)total + 256), "stretch text");
  sl.text_n = 0;
  if (carry_len > 0) ZCHK(hipMemcpyAsync(sl.text.p, other.text.as<char>() + carry_from, (size_t)carry_len, hipMemcpyDeviceToDevice, z->stream), "carry");
  *d_at = sl.text.as<uint8_t>() + carry_len;
  return C3_E_OK;
}

int c3h::stretch_text_parse(c3_bgzf* z, int slot, int64_t total, bool bam, int at_start, int at_eof, c3_fq_stretch* out) {
  int rc;
  c3_bgzf::FqSlot& sl = z->fq[slot];
  sl.text_n = total;
  out->text_bytes = total;
  if (bam) {
    c3_bam_info bi;
    if ((rc = bam_parse_device(z, sl, 0, total, at_start, at_eof, 0, &bi)) != C3_E_OK) return rc;
    out->info.n_records = bi.n_records; out->info.n_kept = bi.n_kept; out->info.n_short = bi.n_short; out->info.consumed = bi.consumed;
    out->info.name_bytes = bi.name_bytes; out->info.base_bytes = bi.base_bytes; out->info.departed = bi.departed;
    out->reason = bi.reason; out->bad_at = bi.bad_at; out->header_bytes = bi.header_bytes;
  } else if ((rc = fq_parse_device(z, sl, 0, total, at_eof, 0, &out->info)) != C3_E_OK) return rc;
  const int64_t nk = out->info.n_kept;
  if (nk > 0) {
    if ((rc = fq_gather_device(z, sl, out->info, bam)) != C3_E_OK) return rc;
    if (sl.h_cap < (size_t)nk + 1) {
      if (sl.h_off) (void)hipHostFree(sl.h_off);
      if (sl.h_name_off) (void)hipHostFree(sl.h_name_off);
      sl.h_off = sl.h_name_off = nullptr; sl.h_cap = 0;
      const size_t want = (size_t)nk + 1 + (size_t)nk / 8 + 1024;
      ZCHK(hipHostMalloc((void**)&sl.h_off, want * sizeof(int64_t), hipHostMallocDefault), "stretch tables");
      ZCHK(hipHostMalloc((void**)&sl.h_name_off, want * sizeof(int64_t), hipHostMallocDefault), "stretch tables");
      sl.h_cap = want;
    }
    ZCHK(hipMemcpyAsync(sl.h_off, sl.off.p, ((size_t)nk + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
    ZCHK(hipMemcpyAsync(sl.h_name_off, sl.name_off.p, ((size_t)nk + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, z->stream), "k_fastq_gather");
    ZCHK(hipStreamSynchronize(z->stream), "k_fastq_gather");
    if (sl.h_off[0] != 0 || sl.h_name_off[0] != 0 || sl.h_off[nk] != out->info.base_bytes || sl.h_name_off[nk] != out->info.name_bytes)
      return host_fail(C3_E_HIP, "k_fastq: offsets do not match the header");
    out->off = sl.h_off; out->name_off = sl.h_name_off;
  }
  return C3_E_OK;
}

static int stretch_parse(c3_bgzf* z, int slot, const char* comp, int64_t ncomp, int64_t carry_from, int64_t carry_len,
                         bool bam, int at_start, int at_eof, c3_fq_stretch* out) {
  if (!z || !out || slot < 0 || slot > 1 || ncomp < 0 || (ncomp > 0 && !comp) || carry_len < 0) return host_fail(C3_E_ARG, "c3_bgzf_stretch_parse: bad arguments");
  memset(out, 0, sizeof *out);
  int64_t nm = 0, ob = 0;
  int rc = c3_bgzf_scan(comp, ncomp, &nm, &ob);
  if (rc) return rc;
  uint8_t* d_at = nullptr;
  if ((rc = c3h::stretch_text_begin(z, slot, carry_from, carry_len, ob, bam, &d_at)) != C3_E_OK) return rc;
  if (nm > 0) {
    int64_t got = 0;
    rc = bgzf_inflate_members(z, comp, ncomp, nm, d_at, nullptr, &got);
    if (rc) return rc;
    if (got != ob) return host_fail(C3_E_DATA, "c3_bgzf_stretch_parse: inflated size differs from the headers");
  }
  return c3h::stretch_text_parse(z, slot, carry_len + ob, bam, at_start, at_eof, out);
}

extern "C" int c3_bgzf_stretch_parse(c3_bgzf* z, int slot, const char* comp, int64_t ncomp, int64_t carry_from, int64_t carry_len,
                                     int at_eof, c3_fq_stretch* out) {
  return stretch_parse(z, slot, comp, ncomp, carry_from, carry_len, false, 0, at_eof, out);
}
// the inflated bytes of a BAM file: the same carry rule (a file header that is not whole yet is carried like a cut record:
// consumed = 0), the same slot arrays and tables, k_bam in place of k_fastq
extern "C" int c3_bgzf_stretch_parse_bam(c3_bgzf* z, int slot, const char* comp, int64_t ncomp, int64_t carry_from, int64_t carry_len,
                                         int at_start, int at_eof, c3_fq_stretch* out) {
  return stretch_parse(z, slot, comp, ncomp, carry_from, carry_len, true, at_start, at_eof, out);
}

// records [r0, r1) of the slot's stretch copied to the host (names / seqs / quals point at the place of record r0; seqs and
// quals may be null: names only).  Runs on copy_stream: the other slot may be being loaded on another thread meanwhile.
extern "C" int c3_bgzf_stretch_fetch(c3_bgzf* z, int slot, int64_t r0, int64_t r1, char* names, char* seqs, char* quals) {
  if (!z || slot < 0 || slot > 1 || !names) return host_fail(C3_E_ARG, "c3_bgzf_stretch_fetch: bad arguments");
  const c3_bgzf::FqSlot& sl = z->fq[slot];
  if (r0 < 0 || r1 < r0 || r1 > sl.n_rec) return host_fail(C3_E_ARG, "c3_bgzf_stretch_fetch: records outside the stretch");
  if (r0 == r1) return C3_E_OK;
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  const int64_t nb = sl.h_name_off[r0], ne = sl.h_name_off[r1], sb = sl.h_off[r0], se = sl.h_off[r1];
  if (ne > nb) ZCHK(hipMemcpyAsync(names, sl.names.as<char>() + nb, (size_t)(ne - nb), hipMemcpyDeviceToHost, z->copy_stream), "stretch fetch");
  if (seqs && se > sb) ZCHK(hipMemcpyAsync(seqs, sl.seqs.as<char>() + sb, (size_t)(se - sb), hipMemcpyDeviceToHost, z->copy_stream), "stretch fetch");
  if (quals && se > sb) ZCHK(hipMemcpyAsync(quals, sl.quals.as<char>() + sb, (size_t)(se - sb), hipMemcpyDeviceToHost, z->copy_stream), "stretch fetch");
  ZCHK(hipStreamSynchronize(z->copy_stream), "stretch fetch");
  return C3_E_OK;
}

// ---- the reader's device buffer sets (c3_reader_stage_on_device) ----------
extern "C" int c3_bgzf_sets_create(c3_bgzf* z, int n_sets) {
  if (!z || n_sets < 1) return host_fail(C3_E_ARG, "c3_bgzf_sets_create: bad arguments");
  if (z->dsets.size() < (size_t)n_sets) z->dsets.resize((size_t)n_sets);
  return C3_E_OK;
}

// grow-only; the first `keep` bytes of both arrays survive a growth (a group that outgrows its set while it is being filled)
extern "C" int c3_bgzf_set_reserve(c3_bgzf* z, int set, int64_t bytes, int64_t keep) {
  if (!z || set < 0 || (size_t)set >= z->dsets.size() || bytes < 0 || keep < 0) return host_fail(C3_E_ARG, "c3_bgzf_set_reserve: bad arguments");
  c3_bgzf::DevSet& d = z->dsets[(size_t)set];
  if ((size_t)bytes <= d.seqs.cap && (size_t)bytes <= d.quals.cap) return C3_E_OK;
  if ((size_t)keep > std::min(d.seqs.cap, d.quals.cap)) return host_fail(C3_E_ARG, "c3_bgzf_set_reserve: keep beyond the set");
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  if (!z->copy_stream) ZCHK(hipStreamCreateWithFlags(&z->copy_stream, hipStreamNonBlocking), "device set");
  const size_t want = keep ? std::max((size_t)bytes, d.seqs.cap + d.seqs.cap / 2) : (size_t)bytes;
  for (DBuf* b : {&d.seqs, &d.quals}) {
    DBuf nb;
    ZCHK(nb.ensure(want), "device set");
    if (keep) {
      ZCHK(hipMemcpyAsync(nb.p, b->p, (size_t)keep, hipMemcpyDeviceToDevice, z->copy_stream), "device set");
      ZCHK(hipStreamSynchronize(z->copy_stream), "device set");
    }
    *b = std::move(nb);                                              // (the old allocation goes with nb)
  }
  return C3_E_OK;
}

// records [r0, r1) of the slot's stretch into a device group: names to the host (at the place of record r0), bases and
// qualities device to device into set `set` from byte `at` on.  Runs on copy_stream and has landed on return, so the slot may
// be loaded again and another stream may read the set without an event.
extern "C" int c3_bgzf_stretch_stage(c3_bgzf* z, int slot, int64_t r0, int64_t r1, char* names, int set, int64_t at) {
  if (!z || slot < 0 || slot > 1 || !names || set < 0 || (size_t)set >= z->dsets.size() || at < 0) return host_fail(C3_E_ARG, "c3_bgzf_stretch_stage: bad arguments");
  const c3_bgzf::FqSlot& sl = z->fq[slot];
  if (r0 < 0 || r1 < r0 || r1 > sl.n_rec) return host_fail(C3_E_ARG, "c3_bgzf_stretch_stage: records outside the stretch");
  if (r0 == r1) return C3_E_OK;
  c3_bgzf::DevSet& d = z->dsets[(size_t)set];
  const int64_t nb = sl.h_name_off[r0], ne = sl.h_name_off[r1], sb = sl.h_off[r0], se = sl.h_off[r1];
  if ((size_t)(at + (se - sb)) > std::min(d.seqs.cap, d.quals.cap)) return host_fail(C3_E_ARG, "c3_bgzf_stretch_stage: run beyond the set");
  ZCHK(hipSetDevice(z->device), "hipSetDevice");
  if (ne > nb) ZCHK(hipMemcpyAsync(names, sl.names.as<char>() + nb, (size_t)(ne - nb), hipMemcpyDeviceToHost, z->copy_stream), "stretch stage");
  if (se > sb) {
    ZCHK(hipMemcpyAsync(d.seqs.as<char>() + at, sl.seqs.as<char>() + sb, (size_t)(se - sb), hipMemcpyDeviceToDevice, z->copy_stream), "stretch stage");
    ZCHK(hipMemcpyAsync(d.quals.as<char>() + at, sl.quals.as<char>() + sb, (size_t)(se - sb), hipMemcpyDeviceToDevice, z->copy_stream), "stretch stage");
  }
  ZCHK(hipStreamSynchronize(z->copy_stream), "stretch stage");
  return C3_E_OK;
}

extern "C" int c3_bgzf_set_get(const c3_bgzf* z, int set, const char** d_seqs, const char** d_quals, int* device) {
  if (!z || set < 0 || (size_t)set >= z->dsets.size() || !d_seqs || !d_quals || !device) return host_fail(C3_E_ARG, "c3_bgzf_set_get: bad arguments");
  *d_seqs = z->dsets[(size_t)set].seqs.as<char>(); *d_quals = z->dsets[(size_t)set].quals.as<char>(); *device = z->device;
  return C3_E_OK;
}

// text [from, from + len) of the slot's stretch copied to the host (a departure: the host parser takes over from there)
extern "C" int c3_bgzf_stretch_text(c3_bgzf* z, int slot, int64_t from, int64_t len, char* dst) {
  if (!z || slot < 0 || slot > 1 || from < 0 || len < 0 || (len > 0 && !dst)) return host_fail(C3_E_ARG, "c3_bgzf_stretch_text: bad arguments");
  const c3_bgzf::FqSlot& sl = z->fq[slot];
  if (from + len > sl.text_n) return host_fail(C3_E_ARG, "c3_bgzf_stretch_text: bytes outside the stretch");
  if (len == 0) return C3_E_OK;
  ZCHK(hipSetDevice(z->device), "stretch text");
  ZCHK(hipMemcpyAsync(dst, sl.text.as<char>() + from, (size_t)len, hipMemcpyDeviceToHost, z->copy_stream), "stretch text");
  ZCHK(hipStreamSynchronize(z->copy_stream), "stretch text");
  return C3_E_OK;
}

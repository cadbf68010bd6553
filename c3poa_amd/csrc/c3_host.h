// c3_host.h -- what the HIP host units share (c3_handle.hip, c3_stages.hip, c3_calls.hip, c3_scans.hip, c3_stream.hip, and the text
// paths: c3_tfront.hip -- the front that c3_text.hip and c3_dtext.hip share): the two handles, the owned device buffer, the
// error idioms and the few helpers that cross units.  Host only; no kernel includes it.
#pragma once
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_launch.h"
#include "c3_checks.h"
#include "c3_emit.h"
#include "c3_bamout.h"
#include "c3_post.h"
#include "c3_fastx.h"
#include "c3_dsplit.h"
#include "c3_bgzf.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

struct c3_handle;
namespace c3h {                                  // defined once, used by several units (mangled: not part of the C ABI)
extern thread_local double g_alloc_ms;           // host time spent growing device buffers (hipFree synchronises the device); c3_handle.hip
int qv_scratch(c3_handle* h, long long max_m, long long max_n, int n_items, QvArgs& a, int* grid);      // c3_stages.hip
int fetch_msa_rows(c3_handle* h, int read, int nrows, char* out, int64_t cap, int* msa_len);           // c3_handle.hip
struct EmitBufs;
int emit_run(c3_handle* h, EmitArgs& p, EmitBufs& eb, hipStream_t s, std::vector<int64_t>& so, int64_t cap);          // c3_scans.hip
// k_post in two halves on a batch whose arrays (p.n, p.names .. p.table) lie on the device; k_adapter on such a batch (c3_scans.hip)
int post_sizes(c3_handle* h, const c3_post_args* a, PostArgs& p, std::vector<int64_t>& so);
int post_write(c3_handle* h, PostArgs& p, int64_t need);
int adapters_device(c3_handle* h, const C3Batch& b, int64_t max_len, int32_t* d_out);
int bgzf_inflate_to_device(c3_bgzf* z, const char* src, int64_t n, int64_t nm, uint8_t* d_dst, int64_t* out_len);    // c3_stream.hip
// a reader's device stretch in two halves around its inflater (c3_stream.hip; the gzip stream of c3_gunzip_dev.hip uses them)
int stretch_text_begin(c3_bgzf* z, int slot, int64_t carry_from, int64_t carry_len, int64_t bytes, bool bam, uint8_t** d_at);
int stretch_text_parse(c3_bgzf* z, int slot, int64_t total, bool bam, int at_start, int at_eof, c3_fq_stretch* out);
// k_fasta on a text that lies on the device, the gather of its records, the index sets of a search (c3_scans.hip)
namespace fa { enum { FA_TEXT, FA_CNT, FA_NL, FA_LSE, FA_LDST, FA_BSUM, FA_HDR, FA_OFF, FA_NOFF, FA_RECL, FA_HASH, FA_NAMES, FA_SEQS, FA_KREC, FA_ROFF,
                      FA_OUT, FA_ANAMES, FA_ANO, FA_BNAMES, FA_BNO, FA_N }; }      // the slots of c3_handle::d_fa
int fasta_parse_resident(c3_handle* h, const uint8_t* d_text, int64_t n, int at_eof, int kept, FaArgs* a);
int fasta_gather_resident(c3_handle* h, FaArgs* a);
int demux_sets_device(c3_handle* h, const c3_demux_sets* st, const uint8_t* tab, int K, int64_t nk, FaArgs* a);
// ---- one BGZF chunk loop (c3_stream.hip) ----
struct ZStage;
// how a compression by chunks ended: a HIP error at step `what`, or a member size out of range / members beyond the arena's
// cap; waits = the stream waits it made.  Each caller maps it to its own error channel.
struct ZStatus { hipError_t e = hipSuccess; enum { OK, MEMBER_SIZE, BEYOND_BOUND } bad = OK; const char* what = ""; int waits = 0; };
// queues bytes [c0, c0 + cn) of a compression's source into the staging input d_zin on the loop's stream
typedef std::function<hipError_t(char* d_zin, int64_t c0, int64_t cn)> ZStageIn;
// len source bytes compressed by k_bgzf as one text into the host arena at *out, a chunk of blocks at a time (BGZF_CHUNK_BLOCKS, or
// the test hook C3_BGZF_CHUNK = 1 .. 2048: members are cut every BGZF_BLOCK bytes whatever the chunk).  wait_after_copy_out:
// wait for every chunk's packed members to land; otherwise the last copies are still queued on s at return.
ZStatus bgzf_chunks(ZStage& z, hipStream_t s, int64_t len, const ZStageIn& stage_in, char* arena, int64_t cap, int64_t* out, bool wait_after_copy_out);
// ---- the text front that c3_post_emit_text and c3_demux_emit_text share (c3_tfront.hip) ----
struct TextFront;
struct TextLoad { int nxt = 0, kind = 0, waits = 0; int64_t total = 0; float ms_inflate = 0; };       // what text_load made
void text_free(TextFront& t);
void text_reset(TextFront& t);
// the kept tail + the piece in text[cur ^ 1] (copied up, or inflated in place), the file's kind; who / keep_flag: the entry point
// and its keep-quals flag, for the messages; ev[n_ev]: the caller's events, created with the page-locked buffers on first use
int text_load(c3_handle* h, TextFront& t, const char* src, int64_t n, bool in_z, bool keep_q, const char* who, const char* keep_flag,
              hipEvent_t* ev, int n_ev, TextLoad* ld);
// k_fastq_count .. k_fastx_records over the loaded text: f filled, the checked header in t.h_hdr (zero when no record pass ran);
// *waits (optional) grows by the stream waits made; ev_begin / ev_records (optional) are recorded in front of k_fastq_count / directly after k_fastx_records
int text_tables(c3_handle* h, TextFront& t, const TextLoad& ld, int at_eof, FxArgs& f, int* waits, hipEvent_t ev_begin = nullptr, hipEvent_t ev_records = nullptr);
// names / seqs / quals sized by the header, k_fastx_gather queued (ev_begin, optional, recorded in front of it)
int text_gather(c3_handle* h, TextFront& t, FxArgs& f, bool keep_q, hipEvent_t ev_begin = nullptr);
// the switch: this call's text becomes the kept one (the last thing a successful call does)
void text_commit(TextFront& t, const TextLoad& ld, int64_t consumed, int at_eof);
// one device-resident stream compressed as one text into the host arena at *out (bgzf_chunks on h->stream, errors into h->err);
// *waits grows by the stream waits made
int bgzf_stream_device(c3_handle* h, ZStage& z, const char* d_src, int64_t len, char* arena, int64_t cap, int64_t* out, int* waits = nullptr);
void post_text_free(c3_handle* h);                                                                                     // c3_text.hip
void demux_text_free(c3_handle* h);                                                                                    // c3_dtext.hip
}

#define BGZF_CHUNK_BLOCKS 2048                   // BGZF blocks per device chunk of a compression (c3h::bgzf_chunks)

static inline double dbg_now_ms() { using namespace std::chrono; return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count(); }
// C3_DEBUG=1: progress lines on stderr, each stamped with the host clock (ms) -- shows the host gaps between the stages
#define DBG(...) do { if (getenv("C3_DEBUG")) { fprintf(stderr, "[c3 %.3f] ", dbg_now_ms()); fprintf(stderr, __VA_ARGS__); fflush(stderr); } } while (0)

// ---- handle -----------------------------------------------------------------------------
struct DBuf {                                   // owns one device allocation (move-only)
  void* p = nullptr; size_t cap = 0;
  DBuf() = default;
  DBuf(DBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DBuf& operator=(DBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  DBuf(const DBuf&) = delete;
  DBuf& operator=(const DBuf&) = delete;
  ~DBuf() { if (p) (void)hipFree(p); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    const double t0 = dbg_now_ms();
    if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    // test hook: fresh device memory usually reads as zero, which hides reads of cells nobody wrote; C3_DEBUG_POISON fills every
    // new buffer with a pattern instead (tests/test_gpu_band.py runs the pipeline that way)
    if (e == hipSuccess && getenv("C3_DEBUG_POISON")) e = hipMemset(p, 0xA5, want);
    c3h::g_alloc_ms += dbg_now_ms() - t0;
    return e;
  }
  // ensure(bytes + slack), then queue the upload of `bytes` from src on s
  hipError_t put(const void* src, size_t bytes, hipStream_t s, size_t slack = 0) {
    const hipError_t e = ensure(bytes + slack);
    return e != hipSuccess ? e : hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, s);
  }
  template <class T> T* as() const { return (T*)p; }
};

// k_emit: pass buffers and arena of one formatting (c3_emit_group has one set, the emit snapshot another), event pairs around
// k_emit_len / the scans / k_emit_write
struct c3h::EmitBufs { DBuf work, offs, arena; hipEvent_t ev[5] = {}; };

// staging of a compression by chunks (c3h::bgzf_chunks): the chunk, k_bgzf's slots, member sizes and packed members; the
// page-locked copy of the sizes.  Owned by c3_bgzf, c3_handle (the emit snapshot's fetch) and TextFront.
struct c3h::ZStage {
  DBuf zin, zslots, zsizes, zpacked; int* h_sizes = nullptr;
  ~ZStage() { if (h_sizes) (void)hipHostFree(h_sizes); }
  hipError_t pin() { return h_sizes ? hipSuccess : hipHostMalloc((void**)&h_sizes, BGZF_CHUNK_BLOCKS * sizeof(int), hipHostMallocDefault); }
  // room for one chunk of cn bytes, 4-byte aligned with 256 bytes of slack (k_bgzf reads up to 8 bytes past a chunk's end:
  // realigned dword loads); callers with several streams size it once for min(longest, a full chunk)
  hipError_t reserve(int64_t cn) {
    cn = std::min(cn, (int64_t)BGZF_CHUNK_BLOCKS * BGZF_BLOCK);
    const size_t nb = (size_t)((cn + BGZF_BLOCK - 1) / BGZF_BLOCK);
    hipError_t e = pin();
    if (e == hipSuccess) e = zin.ensure((size_t)cn + 256);
    if (e == hipSuccess) e = zslots.ensure(nb * BGZF_SLOT);
    if (e == hipSuccess) e = zsizes.ensure(nb * sizeof(int));
    if (e == hipSuccess) e = zpacked.ensure(nb * BGZF_MAX_MEMBER);
    return e;
  }
};
// what the two text paths share (c3_tfront.hip): text[cur] holds the text of the last call, its bytes [tail_from, text_n) being
// the unconsumed tail that goes in front of the next piece; the FASTQ/FASTX parse tables and arenas; staging, inflater, read-backs
struct c3h::TextFront {
  DBuf text[2]; int cur = 0, kind = 0; int64_t text_n = 0, tail_from = 0;
  DBuf cnt, nl, slen, nlen, bsum, hdr, lhdr, off, name_off, woff, src, hash, names, seqs, quals;
  ZStage zs;
  C3FxHdr* h_hdr = nullptr; C3FqHdr* h_lhdr = nullptr; c3_bgzf* z = nullptr;
};
// the text path of the post-processing step (c3_text.hip): the front, the 2-bit pack and k_adapter's table
struct PostText : c3h::TextFront {
  DBuf pk, table;
  hipEvent_t ev[8] = {};
  c3_post_text_timing tm = {};
};
// the text path of the demultiplexer (c3_dtext.hip): the front (a FASTA text is parsed into c3_handle::d_fa instead of its
// tables); the placement tables of k_dsplit and the output arena; the page-locked stream offsets
struct DemuxText : c3h::TextFront {
  DBuf krec, kb, nkept, key, rank, base, soff, out;
  int64_t* h_soff = nullptr;
  hipEvent_t ev[6] = {};
  c3_demux_text_timing tm = {};
};

struct Summary { int status, n_sub, max_sub, sum_sub, max_dang, front, tail, n_peaks; };
enum { EV_N = 10 };
struct c3_handle {
  c3_config cfg; std::string err; hipStream_t stream = nullptr; int n_cus = 256; size_t mem_total = 0;
  // staged (next) batch: copied on its own stream while the resident batch is being processed
  hipStream_t stream_up = nullptr; hipEvent_t ev_up[2] = {nullptr, nullptr};
  // results in flight (c3_batch_results_snapshot .. _fetch): snapshot of the records + compact consensus bytes, copied on a third stream
  hipStream_t stream_dn = nullptr; hipEvent_t ev_dn = nullptr; long long* h_tot = nullptr;
  std::atomic<bool> snap_pending{false}; int snap_n = 0, snap_kp = 0; long long snap_tot = 0; bool snap_cons = false;
  DBuf d_info_snap, d_coff_part;
  struct Staged { DBuf d_ascii, d_pk, d_woff, d_qual, d_off, d_strand, d_sid; std::vector<int64_t> off, woff; std::vector<int16_t> sid; std::string strand;
                  int n = 0; int64_t total = 0, words = 0, maxL = 0; bool pending = false; } st;
  hipEvent_t ev[EV_N] = {};
  // splints
  int n_spl = 0, max_spl = 0; std::vector<int> sp_len; DBuf d_sp_codes, d_sp_len;
  // batch
  int n = 0; int64_t total = 0, words = 0, maxL = 0; std::vector<int64_t> off, woff;
  DBuf d_ascii, d_pk, d_woff, d_qual, d_off, d_strand, d_sid, d_info, d_track, d_draft, d_tpos, d_cons, d_counter, d_gather, d_gather_off;
  DBuf d_raw, d_nraw, d_sum, d_work, d_bufA, d_bufB, d_cand, d_cst, d_msa, d_msa_off, d_msa_len;
  DBuf s_poa_i, s_poa_nk, s_poa_cells, s_poa_b, s_poa_sc, s_poa_desc, s_poa_jump, s_poa_path, d_overflow;      // POA scratch
  int n_poa_redo = 0;        // reads of the last run that needed the full-size second POA pass
  int n_poa_redo16 = 0;      // ... of them: because a score left the 16-bit cells
  // k_poa_pair: vq of subread 1 (16 bits per base of the batch), counted cells and done flag per read; its event pair and counters.
  // vq has a buffer of its own: d_tpos is the only per-base array of that size, and its -1 of failed reads is read later
  DBuf d_pair_vq, d_pair_cells, d_pair_done; hipEvent_t ev_pair[2] = {nullptr, nullptr}; bool pair_ran = false; int n_pair = 0, n_pair_declined = 0;
  DBuf s_eD, s_lw, d_wrec, d_wlay, d_wbase, d_wout;       // prep / windows
  DBuf s_win_i, s_win_nk, s_win_h, s_win_d, s_win_b, s_win_sc, s_win_desc, s_win_h2, s_win_d2, d_wovf;
  DBuf s_zero_d, d_zinfo, d_zflag, d_zwork; std::vector<int> zwork;  // zero-repeat rescue: k_zero direction bytes, per-read records, work list
  DBuf s_zero_l;                                                      // k_zero_long slots
  DBuf d_dmx_heads, d_dmx_meta, d_dmx_out;                            // demultiplexer: heads, Peq / lengths / byte codes, winners + distances
  DBuf d_qv, s_qv_dirs, s_qv_g, d_qv_cnt, d_gather_qv;                // QV stage: QV arena (like d_cons), direction slots, long-consensus slots, counters, snapshot
  hipEvent_t ev_qv[2] = {nullptr, nullptr}; c3_qv_timing qtm = {}; bool snap_qv = false;
  DBuf d_post[16]; hipEvent_t ev_post[5] = {}; c3_post_timing ptm = {};       // k_post: inputs, descriptors, pass buffers, arena; event times of the last call
  PostText pt;
  DemuxText dx; std::vector<uint32_t> dmx_meta_host;      // ... of the demultiplexer; k_demux's meta while its upload is queued
  // k_fasta: text, tables, arenas, output; event times of the last c3_demux_emit; page-locked copy of the device header
  DBuf d_fa[20]; hipEvent_t ev_fa[10] = {}; c3_demux_timing dtm = {}; struct C3FaHdr* h_fa_hdr = nullptr;
  // k_emit: inputs of c3_emit_group and its pass buffers; times of the last c3_emit_group / delivered emit snapshot
  DBuf d_emit[10]; c3h::EmitBufs emit_sa; c3_emit_timing etm = {};
  // emit snapshot in flight (c3_batch_emit_snapshot .. _fetch): names, pass buffers + arena, BGZF staging of the fetch
  c3h::EmitBufs emit_snap; DBuf d_emit_names, d_emit_noff; c3h::ZStage emit_zs;
  hipEvent_t ev_emit_dn = nullptr;
  std::atomic<bool> emit_pending{false}; int emit_S = 0, emit_flags = 0; std::vector<int64_t> emit_so; c3_emit_timing emit_tm = {};
  std::vector<Summary> sum; std::vector<int> work;
  int res_prefix = 0;            // entries of peaks[] / sub_beg[] / sub_end[] that any read of the resident batch uses (0: unknown)
  int peaks_grid = 0; bool debug_msa = false; bool injected = false;
  int n_windows = 0;
  c3_timing tm;
  unsigned long long phase_poa[16] = {0}, phase_win[16] = {0};
  int stages_done = 0;
};

// ---- errors: a c3_handle call fails into h->err (HIPCHK, c3_fail); a handle-free or c3_bgzf call into the text of
// c3_last_error(NULL) (ZCHK, host_fail) ------------------------------------------------------------------------------------
static inline int c3_hip_fail(c3_handle* h, hipError_t e, const char* what, const char* file, int line) {
  char buf[512];
  const char* base = strrchr(file, '/');
  snprintf(buf, sizeof buf, "HIP error %d (%s) at %s:%d: %s", (int)e, hipGetErrorString(e), base ? base + 1 : file, line, what);
  if (h) h->err = buf;
  return C3_E_HIP;
}
static inline int c3_fail(c3_handle* h, int code, const char* msg) { if (h) h->err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return c3_hip_fail(h, e_, #x, __FILE__, __LINE__); } while (0)
static inline int host_fail(int code, const char* msg) { c3_set_host_error(msg); return code; }
static inline int bgzf_fail(hipError_t e, const char* what) {
  char buf[256];
  snprintf(buf, sizeof buf, "HIP error %d (%s): %s", (int)e, hipGetErrorString(e), what);
  return host_fail(C3_E_HIP, buf);
}
#define ZCHK(x, what) do { hipError_t e_ = (x); if (e_ != hipSuccess) return bgzf_fail(e_, what); } while (0)

// a value overridden for the length of a scope: the saved one comes back on every way out
template <class T> struct Override {
  T& ref; const T saved;
  Override(T& r, T v) : ref(r), saved(r) { r = v; }
  ~Override() { ref = saved; }
  Override(const Override&) = delete;
};

// the device counter block (C3Counters, c3_args.h): zeroed and read by field
static inline C3Counters* dev_cnt(c3_handle* h) { return h->d_counter.as<C3Counters>(); }
template <class T> static inline hipError_t zero_cnt(c3_handle* h, T* field) { return hipMemsetAsync(field, 0, sizeof(T), h->stream); }
static inline hipError_t read_counters(c3_handle* h, C3Counters* c) {
  hipError_t e = hipMemcpyAsync(c, h->d_counter.p, sizeof(*c), hipMemcpyDeviceToHost, h->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

static inline int code_of(char c) {
  switch (c) { case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 0; }
}

static inline C3Batch dev_batch(c3_handle* h) {
  C3Batch b; b.n = h->n; b.pk = h->d_pk.as<uint32_t>(); b.woff = h->d_woff.as<int64_t>(); b.qual = h->d_qual.as<uint8_t>();
  b.off = h->d_off.as<int64_t>(); b.strand = h->d_strand.as<uint8_t>(); b.splint_id = h->d_sid.as<int16_t>();
  return b;
}
static inline C3Params dev_params(const c3_config& c) {
  C3Params p;
  p.conk_match = c.conk_match; p.conk_mismatch = c.conk_mismatch; p.conk_penalty = c.conk_penalty;
  p.sg_iters = c.sg_iters; p.sg_window = c.sg_window; p.sg_order = c.sg_order; p.mdist = c.mdistcutoff;
  p.poa_match = c.poa_match; p.poa_mismatch = c.poa_mismatch; p.o1 = c.poa_o1; p.e1 = c.poa_e1; p.o2 = c.poa_o2; p.e2 = c.poa_e2;
  p.band_b = c.poa_band_b; p.band_f = c.poa_band_f;
  p.pol_match = c.pol_match; p.pol_mismatch = c.pol_mismatch; p.pol_gap = c.pol_gap; p.pol_window = c.pol_window; p.pol_q = c.pol_q;
  p.dang_band = c.dang_band;
  p.zero = c.zero; p.zr_match = 2; p.zr_mismatch = 4; p.zr_gapo = 4; p.zr_gape = 2; p.zr_min_score = 80; p.zr_max_cells = (int)c.zero_max_cells;
  return p;
}

// the stream handle (c3_stream.hip): BGZF compress / inflate, FASTQ parse, the reader's stretches
struct c3_bgzf {
  int device = 0; hipStream_t stream = nullptr;
  c3h::ZStage zs;                                                // BGZF output; zs.zin also stages k_inflate's input
  C3BgzfMember* h_mem = nullptr; int2* h_res = nullptr;         // k_inflate: descriptors in, (status, CRC) out; first use
  DBuf d_mem, d_res, d_out;
  // k_fastq (first use): scratch of one parse, and two slots of text + finished records (the reader parses one stretch while
  // the groups of the other are copied out on copy_stream; the stand-alone call uses slot 0)
  struct FqSlot {
    DBuf text, names, seqs, quals, off, name_off, src;
    int64_t text_n = 0, n_rec = 0;
    int64_t* h_off = nullptr; int64_t* h_name_off = nullptr; size_t h_cap = 0;       // page-locked copies of off / name_off
  } fq[2];
  DBuf d_cnt, d_nl, d_slen, d_nlen, d_bsum, d_hdr;
  C3FqHdr* h_hdr = nullptr;
  // k_bam (first use): the chain tiles, the record starts and what the rule says of each; the slots and sums are k_fastq's
  DBuf d_tiles, d_rpos, d_reason, d_rsrc, d_bhdr;
  C3BamHdr* h_bhdr = nullptr;
  hipStream_t copy_stream = nullptr;
  // the reader's device buffer sets (c3_reader_stage_on_device): the home of a device group, filled from the slots on copy_stream
  struct DevSet { DBuf seqs, quals; };
  std::vector<DevSet> dsets;
  // k_gunzip (first use): the file, the symbol arena, candidates, jobs / results, segments / chunks / chunk results, windows, bytes
  DBuf gz_comp, gz_arena, gz_cand, gz_jobs, gz_res, gz_segs, gz_chunks, gz_cres, gz_wins, gz_out;
};

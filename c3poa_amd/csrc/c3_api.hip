// c3_api.hip -- C ABI (include/c3poa.h) and host orchestration of the HIP hot path.
// No CPU fallback exists in this library: without a gfx950 device c3_create fails.
#include "c3_dev.h"
#include "c3_args.h"
#include "c3_bgzf.h"
#include "c3_fastq.h"
#include "c3_inflate.h"
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// ---- kernel launchers (one translation unit per kernel family) --------------------------
extern "C" void c3k_launch_conk(const ConkArgs*, int, int, int, hipStream_t);
extern "C" void c3k_launch_adapter(const AdapterArgs*, int, hipStream_t);
extern "C" void c3k_launch_pairwise(const uint8_t*, int, const uint8_t*, int, const uint8_t*, int, uint8_t*, uint8_t*, int*, hipStream_t);
extern "C" void c3k_launch_post_classify(const PostArgs*, hipStream_t);
extern "C" void c3k_launch_post_scan(const PostArgs*, hipStream_t);
extern "C" void c3k_launch_post_emit(const PostArgs*, hipStream_t);
extern "C" void c3k_launch_match_index(const char*, const int*, int, int, const char*, const long long*, int*, hipStream_t);
extern "C" void c3k_launch_demux(const uint8_t*, int, const uint8_t*, int, int, int, int32_t*, uint8_t*, hipStream_t);
extern "C" void c3k_launch_peaks(const PeaksArgs*, int, hipStream_t);
extern "C" int c3k_peaks_blocks_per_cu(void);
extern "C" void c3k_launch_poa(const PoaArgs*, int, int, int, hipStream_t);
extern "C" void c3k_launch_prep(const PrepArgs*, int, hipStream_t);
extern "C" void c3k_launch_window(const WinArgs*, int, hipStream_t);
extern "C" void c3k_launch_stitch(const StitchArgs*, int, hipStream_t);
extern "C" void c3k_launch_zero(const ZeroArgs*, int, hipStream_t);
extern "C" void c3k_launch_zero_long(const ZeroArgs*, int, hipStream_t);
extern "C" void c3k_launch_zero_finish(const ZeroArgs*, int, hipStream_t);
extern "C" void c3k_launch_qv(const QvArgs*, int, hipStream_t);
extern "C" int c3k_qv_lds_max(void);
extern "C" void c3k_launch_bgzf(const uint8_t*, long long, int, uint8_t*, int*, uint8_t*, hipStream_t);
extern "C" void c3k_launch_inflate(const uint8_t*, const C3BgzfMember*, int, uint8_t*, int2*, hipStream_t);
extern "C" void c3k_launch_fastq_count(const uint8_t*, uint32_t, uint32_t, int32_t*, int, C3FqHdr*, hipStream_t);
extern "C" void c3k_launch_fastq_lines(const uint8_t*, uint32_t, uint32_t, const int32_t*, int32_t*, hipStream_t);
extern "C" void c3k_launch_fastq_records(const uint8_t*, uint32_t, uint32_t, const int32_t*, int, int, int, int, int32_t*, int32_t*, long long*,
                                         C3FqHdr*, int64_t*, int64_t*, int4*, hipStream_t);
extern "C" void c3k_launch_fastq_gather(const uint8_t*, const int4*, const int64_t*, const int64_t*, long long, uint8_t*, uint8_t*, uint8_t*, hipStream_t);

// ---- small kernels ----------------------------------------------------------------------
__device__ __forceinline__ uint32_t pack_code(uint32_t b) {
  // A/a=0 C/c=1 G/g=2 T/t/U/u=3, every other byte 0 (c3poa.h conventions)
  const uint32_t u = b & 0xDFu;                                // upper case
  const uint32_t c = (u >> 1) & 3u;                            // A0 C1 G3 T2 U2
  const bool ok = (u == 'A') | (u == 'C') | (u == 'G') | (u == 'T') | (u == 'U');
  return ok ? (c ^ (c >> 1)) : 0u;
}
__global__ __launch_bounds__(256) void k_pack(const uint8_t* ascii, const int64_t* off, const int64_t* woff, int n, uint32_t* pk) {
  // one wave per read (grid-stride); lane l packs word w = 64*it + l from 16 consecutive bytes (one 16-byte load per
  // lane -> a wave reads 1 KiB contiguous).  The tail word is assembled byte by byte.
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (int r = wave; r < n; r += n_waves) {
    const int64_t L = off[r + 1] - off[r];
    const int64_t nw = woff[r + 1] - woff[r];
    const uint8_t* s = ascii + off[r];
    uint32_t* dst = pk + woff[r];
    for (int64_t w = lane; w < nw; w += 64) {
      uint32_t x = 0;
      if (w * 16 + 16 <= L) {
        uint32_t v[4];
        __builtin_memcpy(v, s + w * 16, 16);
#pragma unroll
        for (int k = 0; k < 16; ++k) x |= pack_code((v[k >> 2] >> (8 * (k & 3))) & 0xFFu) << (2 * k);
      } else {
        for (int k = 0; k < 16; ++k) { int64_t i = w * 16 + k; if (i < L) x |= pack_code(s[i]) << (2 * k); }
      }
      dst[w] = x;
    }
  }
}
// consensus of read r lives at arena[off[r] ..]; compact copies go to out[coff[r] .. coff[r+1]) (one wave per read)
__global__ __launch_bounds__(256) void k_gather_cons(const char* arena, const int64_t* off, const int64_t* coff, int n, char* out) {
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_waves = (gridDim.x * blockDim.x) >> 6;
  for (int r = wave; r < n; r += n_waves) {
    const int64_t len = coff[r + 1] - coff[r];
    const char* src = arena + off[r]; char* dst = out + coff[r];
    for (int64_t k = lane; k < len; k += 64) dst[k] = src[k];
  }
}
// cons_off[i + 1] = sum over reads <= i of (status OK ? cons_len : 0), on the device (three tiny launches: block sums, scan of the
// block sums by one block, block-local scan + block offset): the host no longer needs the records before it can size the copy
__device__ __forceinline__ long long cons_len_of(const C3Info* p) { return p->status == C3_ST_OK ? (long long)p->cons_len : 0; }
__global__ __launch_bounds__(256) void k_coff_sums(const C3Info* info, int n, long long* part) {
  __shared__ long long sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  sh[threadIdx.x] = i < n ? cons_len_of(info + i) : 0;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) { if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d]; __syncthreads(); }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}
__global__ __launch_bounds__(1024) void k_coff_scan(long long* part, int nb, int64_t* coff, int n) {
  __shared__ long long sh[1024];
  long long carry = 0;
  for (int b0 = 0; b0 < nb; b0 += 1024) {
    const int b = b0 + threadIdx.x;
    const long long v = b < nb ? part[b] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) { long long t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0; __syncthreads(); sh[threadIdx.x] += t; __syncthreads(); }
    if (b < nb) part[b] = carry + sh[threadIdx.x] - v;               // exclusive
    carry += sh[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) { coff[0] = 0; coff[n] = carry; }
}
__global__ __launch_bounds__(256) void k_coff_final(const C3Info* info, int n, const long long* part, int64_t* coff) {
  __shared__ long long sh[256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  sh[threadIdx.x] = i < n ? cons_len_of(info + i) : 0;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) { long long t = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0; __syncthreads(); sh[threadIdx.x] += t; __syncthreads(); }
  if (i < n) coff[i + 1] = part[blockIdx.x] + sh[threadIdx.x];
}
__global__ void k_init_info(C3Info* info, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { C3Info* p = &info[i]; p->status = C3_ST_OK; p->n_peaks = 0; p->n_sub = 0; p->has_front = p->has_tail = 0;
               p->front_end = p->tail_beg = 0; p->cons_len = 0; p->draft_len = 0; p->n_win = 0; }
}
struct Summary { int status, n_sub, max_sub, sum_sub, max_dang, front, tail, n_peaks; };
__global__ void k_summary(const C3Info* info, const int64_t* off, int n, Summary* out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const C3Info* p = &info[i];
  Summary s; s.status = p->status; s.n_sub = p->n_sub; s.max_sub = 0; s.sum_sub = 0; s.max_dang = 0; s.n_peaks = p->n_peaks;
  for (int k = 0; k < p->n_sub; ++k) { int l = p->sub_end[k] - p->sub_beg[k]; s.sum_sub += l; if (l > s.max_sub) s.max_sub = l; }
  int L = (int)(off[i + 1] - off[i]);
  s.front = p->has_front ? p->front_end : 0; s.tail = p->has_tail ? L - p->tail_beg : 0;
  if (p->has_front) s.max_dang = p->front_end;
  if (p->has_tail && L - p->tail_beg > s.max_dang) s.max_dang = L - p->tail_beg;
  out[i] = s;
}

#include <atomic>
#include <chrono>
static inline double dbg_now_ms() { using namespace std::chrono; return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count(); }
// C3_DEBUG=1: progress lines on stderr, each stamped with the host clock (ms) -- shows the host gaps between the stages
#define DBG(...) do { if (getenv("C3_DEBUG")) { fprintf(stderr, "[c3 %.3f] ", dbg_now_ms()); fprintf(stderr, __VA_ARGS__); fflush(stderr); } } while (0)

// ---- handle -----------------------------------------------------------------------------
static thread_local double g_alloc_ms = 0.0;   // host time spent growing device buffers (hipFree synchronises the device)
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
    g_alloc_ms += dbg_now_ms() - t0;
    return e;
  }
  template <class T> T* as() const { return (T*)p; }
};

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
  DBuf s_eD, s_lw, d_wrec, d_wlay, d_wbase, d_wout;       // prep / windows
  DBuf s_win_i, s_win_nk, s_win_h, s_win_d, s_win_b, s_win_sc, s_win_desc, s_win_h2, s_win_d2, d_wovf;
  DBuf s_zero_d, d_zinfo, d_zflag, d_zwork; std::vector<int> zwork;  // zero-repeat rescue: k_zero direction bytes, per-read records, work list
  DBuf s_zero_l;                                                      // k_zero_long slots
  DBuf d_dmx_heads, d_dmx_meta, d_dmx_out;                            // demultiplexer: heads, Peq / lengths / byte codes, winners + distances
  DBuf d_qv, s_qv_dirs, s_qv_g, d_qv_cnt, d_gather_qv;                // QV stage: QV arena (like d_cons), direction slots, long-consensus slots, counters, snapshot
  hipEvent_t ev_qv[2] = {nullptr, nullptr}; c3_qv_timing qtm = {}; bool snap_qv = false;
  DBuf d_post[16]; hipEvent_t ev_post[5] = {}; c3_post_timing ptm = {};       // k_post: inputs, descriptors, pass buffers, arena; event times of the last call
  std::vector<Summary> sum; std::vector<int> work;
  int res_prefix = 0;            // entries of peaks[] / sub_beg[] / sub_end[] that any read of the resident batch uses (0: unknown)
  int peaks_grid = 0; bool debug_msa = false; bool injected = false;
  int n_windows = 0;
  c3_timing tm;
  unsigned long long phase_poa[16] = {0}, phase_win[16] = {0};
  int stages_done = 0;
};

static int c3_hip_fail(c3_handle* h, hipError_t e, const char* what, int line) {
  char buf[512];
  snprintf(buf, sizeof buf, "HIP error %d (%s) at c3_api.hip:%d: %s", (int)e, hipGetErrorString(e), line, what);
  if (h) h->err = buf;
  return C3_E_HIP;
}
static int c3_fail(c3_handle* h, int code, const char* msg) { if (h) h->err = msg; return code; }

// the device counter block (C3Counters, c3_args.h): zeroed and read by field
static C3Counters* dev_cnt(c3_handle* h) { return h->d_counter.as<C3Counters>(); }
template <class T> static hipError_t zero_cnt(c3_handle* h, T* field) { return hipMemsetAsync(field, 0, sizeof(T), h->stream); }
static hipError_t zero_counters(c3_handle* h) { return hipMemsetAsync(h->d_counter.p, 0, sizeof(C3Counters), h->stream); }
static hipError_t read_counters(c3_handle* h, C3Counters* c) {
  hipError_t e = hipMemcpyAsync(c, h->d_counter.p, sizeof(*c), hipMemcpyDeviceToHost, h->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(h->stream);
}

extern "C" void c3_default_config(c3_config* c) {
  memset(c, 0, sizeof(*c));
  c->device = 0;
  c->conk_match = 5; c->conk_mismatch = -4; c->conk_penalty = 20;
  c->sg_iters = 3; c->sg_window = 41; c->sg_order = 2; c->mdistcutoff = 500;
  c->poa_match = 5; c->poa_mismatch = 4; c->poa_o1 = 4; c->poa_e1 = 2; c->poa_o2 = 24; c->poa_e2 = 1;
  c->poa_band_b = 10; c->poa_band_f = 0.01;
  c->pol_match = 3; c->pol_mismatch = -5; c->pol_gap = -4; c->pol_window = 500; c->pol_q = 5; c->dang_band = 128;
  c->slots_poa = 0; c->slots_win = 0; c->zero = 1; c->zero_max_cells = 16 << 20;
}
extern "C" const char* c3_version(void) { return "c3poa_amd 0.1 (gfx950)"; }
extern "C" int c3_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }

extern "C" int c3_warm_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) { (void)hipGetLastError(); return C3_E_NO_DEVICE; }
  if (hipSetDevice(device) != hipSuccess || hipFree(nullptr) != hipSuccess) { (void)hipGetLastError(); return C3_E_HIP; }
  return C3_E_OK;
}

static thread_local std::string g_create_err;
extern "C" const char* c3_last_error(const c3_handle* h) { return h ? h->err.c_str() : g_create_err.c_str(); }
void c3_set_host_error(const char* msg) { g_create_err = msg; }     // handle-free calls (c3_demux_host) report here

extern "C" int c3_create(const c3_config* cfg, c3_handle** out) {
  if (!cfg || !out) return C3_E_ARG;
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) { g_create_err = "no HIP device: the c3poa HIP backend has no CPU fallback"; return C3_E_NO_DEVICE; }
  if (cfg->device < 0 || cfg->device >= ndev) { g_create_err = "bad device ordinal"; return C3_E_ARG; }
  if (cfg->conk_match < -127 || cfg->conk_match > 127 || cfg->conk_mismatch < -127 || cfg->conk_mismatch > 127) {
    g_create_err = "conk_match / conk_mismatch must fit a signed byte"; return C3_E_ARG;                 // k_conk keeps them in byte tables
  }
  if (cfg->dang_band > 255) { g_create_err = "dang_band must be at most 255 (k_prep holds 512 band offsets per wave)"; return C3_E_LIMIT; }
  if (cfg->sg_order != 2 && cfg->sg_order != 3) { g_create_err = "sg_order must be 2 or 3"; return C3_E_ARG; }
  if (cfg->sg_window < 5 || cfg->sg_window > 127 || !(cfg->sg_window & 1)) { g_create_err = "sg_window must be odd, 5..127"; return C3_E_ARG; }
  if (cfg->zero_max_cells < 1 || cfg->zero_max_cells > INT32_MAX) { g_create_err = "zero_max_cells must be 1..2147483647"; return C3_E_ARG; }
  c3_handle* h = new c3_handle();
  h->cfg = *cfg;
  hipDeviceProp_t prop;
  e = hipSetDevice(cfg->device);
  if (e == hipSuccess) {
    // synchronisation points sleep instead of spinning: the stages are milliseconds long, and a spinning waiter per
    // handle eats the CPU quota the reader / writer threads need (refused once the context exists: ignored)
    (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync); (void)hipGetLastError();
    e = hipGetDeviceProperties(&prop, cfg->device);
  }
  if (e == hipSuccess) e = hipStreamCreate(&h->stream);
  if (e == hipSuccess) e = hipStreamCreate(&h->stream_up);
  if (e == hipSuccess) e = hipStreamCreate(&h->stream_dn);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_dn, hipEventDisableTiming);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_tot, 64, hipHostMallocDefault);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipEventCreate(&h->ev_up[i]);
  for (int i = 0; i < EV_N && e == hipSuccess; ++i) e = hipEventCreate(&h->ev[i]);
  if (e != hipSuccess) { g_create_err = hipGetErrorString(e); c3_destroy(h); return C3_E_HIP; }
  h->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  h->mem_total = prop.totalGlobalMem;
  memset(&h->tm, 0, sizeof(h->tm));
  *out = h;
  return C3_E_OK;
}

// also takes a handle that c3_create left half made (null members); the device buffers free themselves (DBuf)
extern "C" void c3_destroy(c3_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  for (hipStream_t s : {h->stream, h->stream_up, h->stream_dn}) if (s) (void)hipStreamSynchronize(s);
  for (hipStream_t s : {h->stream, h->stream_up, h->stream_dn}) if (s) (void)hipStreamDestroy(s);
  for (hipEvent_t ev : {h->ev_dn, h->ev_up[0], h->ev_up[1], h->ev_qv[0], h->ev_qv[1]}) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : h->ev) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : h->ev_post) if (ev) (void)hipEventDestroy(ev);
  if (h->h_tot) (void)hipHostFree(h->h_tot);
  delete h;
}

static inline int code_of(char c) {
  switch (c) { case 'C': case 'c': return 1; case 'G': case 'g': return 2; case 'T': case 't': case 'U': case 'u': return 3; default: return 0; }
}

extern "C" int c3_set_splints(c3_handle* h, int n, const char* cat, const int64_t* off) {
  if (!h || n <= 0 || !cat || !off) return C3_E_ARG;
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<uint8_t> codes((size_t)n * 2 * C3_SPLINT_MAX, 0);
  h->sp_len.assign(n, 0); h->max_spl = 0;
  for (int i = 0; i < n; ++i) {
    int S = (int)(off[i + 1] - off[i]);
    if (S <= 0 || S > C3_SPLINT_MAX) return c3_fail(h, C3_E_LIMIT, "splint length must be 1..512");
    // a cell grows by the larger of the two substitution scores per splint row, whichever of them it is
    if ((long long)std::max({h->cfg.conk_match, h->cfg.conk_mismatch, 0}) * S > 32000 || h->cfg.conk_penalty < 0 || h->cfg.conk_penalty > 32000)
      return c3_fail(h, C3_E_LIMIT, "max(conk_match, conk_mismatch) * splint length and conk_penalty must stay within 32000 (16-bit score cells in k_conk)");
    h->sp_len[i] = S; h->max_spl = std::max(h->max_spl, S);
    for (int k = 0; k < S; ++k) {
      int c = code_of(cat[off[i] + k]);
      codes[((size_t)i * 2 + 0) * C3_SPLINT_MAX + k] = (uint8_t)c;
      codes[((size_t)i * 2 + 1) * C3_SPLINT_MAX + (S - 1 - k)] = (uint8_t)(3 - c);   // reverse complement (C3POa.py:234)
    }
  }
  HIPCHK(h->d_sp_codes.ensure(codes.size()));
  HIPCHK(h->d_sp_len.ensure(sizeof(int) * n));
  HIPCHK(hipMemcpyAsync(h->d_sp_codes.p, codes.data(), codes.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_sp_len.p, h->sp_len.data(), sizeof(int) * n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->n_spl = n;
  return C3_E_OK;
}

static C3Batch dev_batch(c3_handle* h) {
  C3Batch b; b.n = h->n; b.pk = h->d_pk.as<uint32_t>(); b.woff = h->d_woff.as<int64_t>(); b.qual = h->d_qual.as<uint8_t>();
  b.off = h->d_off.as<int64_t>(); b.strand = h->d_strand.as<uint8_t>(); b.splint_id = h->d_sid.as<int16_t>();
  return b;
}
static C3Params dev_params(const c3_config& c) {
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

// Stage the NEXT batch: validation, H2D copies and the 2-bit pack run on a second stream, so they overlap the kernels of
// the resident batch.  seqs / quals must stay valid until c3_batch_commit returns (page-locked buffers make the copies
// truly asynchronous); off / splint_id / strand are copied before the call returns.
extern "C" int c3_batch_stage(c3_handle* h, int n, const char* seqs, const char* quals, const int64_t* off,
                              const int16_t* splint_id, const char* strand) {
  if (!h || n <= 0 || !seqs || !quals || !off || !strand) return C3_E_ARG;
  if (h->n_spl <= 0) return c3_fail(h, C3_E_STATE, "c3_set_splints must be called first");
  if (h->st.pending) return c3_fail(h, C3_E_STATE, "a staged batch is waiting for c3_batch_commit");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (off[0] != 0) return c3_fail(h, C3_E_ARG, "off[0] must be 0");
  c3_handle::Staged& t = h->st;
  t.n = n; t.total = off[n] - off[0]; t.off.assign(off, off + n + 1); t.woff.assign(n + 1, 0); t.maxL = 0;
  t.sid.assign((size_t)n, 0); t.strand.assign(strand, (size_t)n);
  for (int i = 0; i < n; ++i) {
    int64_t L = off[i + 1] - off[i];
    if (L < 0 || L > (1 << 30)) return c3_fail(h, C3_E_ARG, "bad read length");
    t.maxL = std::max(t.maxL, L);
    t.woff[i + 1] = t.woff[i] + (L + 15) / 16 + 2;          // +2 words: aligned-window overread
    if (splint_id) { if (splint_id[i] < 0 || splint_id[i] >= h->n_spl) return c3_fail(h, C3_E_ARG, "splint_id out of range"); t.sid[i] = splint_id[i]; }
  }
  t.words = t.woff[n];
  const size_t T = (size_t)t.total;
  HIPCHK(t.d_ascii.ensure(T + 16)); HIPCHK(t.d_pk.ensure(sizeof(uint32_t) * (size_t)t.words + 64));
  HIPCHK(t.d_qual.ensure(T + 16)); HIPCHK(t.d_off.ensure(sizeof(int64_t) * (n + 1))); HIPCHK(t.d_woff.ensure(sizeof(int64_t) * (n + 1)));
  HIPCHK(t.d_strand.ensure(n)); HIPCHK(t.d_sid.ensure(sizeof(int16_t) * n));
  hipStream_t su = h->stream_up;
  HIPCHK(hipEventRecord(h->ev_up[0], su));
  HIPCHK(hipMemcpyAsync(t.d_ascii.p, seqs, T, hipMemcpyHostToDevice, su));
  HIPCHK(hipMemcpyAsync(t.d_qual.p, quals, T, hipMemcpyHostToDevice, su));
  HIPCHK(hipMemcpyAsync(t.d_off.p, t.off.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, su));
  HIPCHK(hipMemcpyAsync(t.d_woff.p, t.woff.data(), sizeof(int64_t) * (n + 1), hipMemcpyHostToDevice, su));
  HIPCHK(hipMemcpyAsync(t.d_strand.p, t.strand.data(), n, hipMemcpyHostToDevice, su));
  HIPCHK(hipMemcpyAsync(t.d_sid.p, t.sid.data(), sizeof(int16_t) * n, hipMemcpyHostToDevice, su));
  dim3 g((unsigned)std::min((n + 3) / 4, h->n_cus * 32));
  hipLaunchKernelGGL(k_pack, g, dim3(256), 0, su, t.d_ascii.as<uint8_t>(), t.d_off.as<int64_t>(), t.d_woff.as<int64_t>(), n, t.d_pk.as<uint32_t>());
  HIPCHK(hipEventRecord(h->ev_up[1], su));
  HIPCHK(hipGetLastError());
  t.pending = true;
  return C3_E_OK;
}

// Make the staged batch the resident one (after the results of the previous batch have been fetched).
extern "C" int c3_batch_commit(c3_handle* h) {
  if (!h) return C3_E_ARG;
  if (!h->st.pending) return c3_fail(h, C3_E_STATE, "no staged batch");
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));            // the previous batch is completely done
  HIPCHK(hipStreamSynchronize(h->stream_up));         // the staged copies and the pack have landed
  c3_handle::Staged& t = h->st;
  std::swap(h->d_ascii, t.d_ascii); std::swap(h->d_pk, t.d_pk); std::swap(h->d_woff, t.d_woff); std::swap(h->d_qual, t.d_qual);
  std::swap(h->d_off, t.d_off); std::swap(h->d_strand, t.d_strand); std::swap(h->d_sid, t.d_sid);
  h->off.swap(t.off); h->woff.swap(t.woff);
  h->n = t.n; h->total = t.total; h->words = t.words; h->maxL = t.maxL;
  t.pending = false;
  const int n = h->n;
  HIPCHK(h->d_info.ensure(sizeof(C3Info) * (size_t)n));
  HIPCHK(h->d_counter.ensure(sizeof(C3Counters)));
  HIPCHK(hipMemsetAsync(h->d_info.p, 0, sizeof(C3Info) * (size_t)n, h->stream));   // the unused tails of peaks[] / sub_*[] read as 0
  hipLaunchKernelGGL(k_init_info, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_info.as<C3Info>(), n);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev_up[0], h->ev_up[1]));
  memset(&h->tm, 0, sizeof(h->tm)); h->tm.ms_pack = ms; h->tm.n_reads = n; h->tm.n_bases = h->total;
  h->stages_done = 0; h->injected = false; h->n_windows = 0; h->res_prefix = 0;
  return C3_E_OK;
}

// Overwrite the splint row / strand of every read of the resident batch (after c3_scan_splints, before c3_batch_run):
// strand[i] = '+' / '-', anything else = not assigned; splint_id[i] < 0 is stored as 0 for such reads.
extern "C" int c3_batch_assign(c3_handle* h, const int16_t* splint_id, const char* strand) {
  if (!h || h->n <= 0 || !splint_id || !strand) return C3_E_ARG;
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<int16_t> sid((size_t)h->n);
  for (int i = 0; i < h->n; ++i) {
    const bool on = strand[i] == '+' || strand[i] == '-';
    if (on && (splint_id[i] < 0 || splint_id[i] >= h->n_spl)) return c3_fail(h, C3_E_ARG, "splint_id out of range");
    sid[(size_t)i] = on ? splint_id[i] : (int16_t)0;
  }
  HIPCHK(hipMemcpyAsync(h->d_strand.p, strand, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_sid.p, sid.data(), sizeof(int16_t) * (size_t)h->n, hipMemcpyHostToDevice, h->stream));
  // a read that was unassigned in an earlier run carries C3_ST_NOT_ASSIGNED: every record starts over
  hipLaunchKernelGGL(k_init_info, dim3((h->n + 255) / 256), dim3(256), 0, h->stream, h->d_info.as<C3Info>(), h->n);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipGetLastError());
  h->stages_done = 0;
  return C3_E_OK;
}

// upload = stage + commit (nothing to overlap with)
extern "C" int c3_batch_upload(c3_handle* h, int n, const char* seqs, const char* quals, const int64_t* off,
                               const int16_t* splint_id, const char* strand) {
  if (h && h->st.pending) { (void)hipStreamSynchronize(h->stream_up); h->st.pending = false; }     // an abandoned staged batch is dropped
  int rc = c3_batch_stage(h, n, seqs, quals, off, splint_id, strand);
  if (rc != C3_E_OK) return rc;
  return c3_batch_commit(h);
}

static int auto_slots(c3_handle* h, int want, size_t per_slot_bytes, int n_items, int waves_per_cu) {
  int s = want > 0 ? want : h->n_cus * waves_per_cu;
  size_t budget = h->mem_total ? h->mem_total / 3 : ((size_t)64 << 30);
  if (per_slot_bytes > 0) { size_t mx = budget / per_slot_bytes; if ((size_t)s > mx) s = (int)std::max<size_t>(mx, 1); }
  if (s > n_items) s = std::max(n_items, 1);
  return s;
}

static int run_conk(c3_handle* h) {
  HIPCHK(h->d_track.ensure(sizeof(int32_t) * (size_t)h->total + 64));
  HIPCHK(zero_cnt(h, &dev_cnt(h)->queue));
  ConkArgs a; a.b = dev_batch(h); a.sp_codes = h->d_sp_codes.as<uint8_t>(); a.sp_len = h->d_sp_len.as<int>();
  a.track = h->d_track.as<int32_t>(); a.info = h->d_info.as<C3Info>(); a.cnt = dev_cnt(h);
  a.match = h->cfg.conk_match; a.mismatch = h->cfg.conk_mismatch; a.penalty = h->cfg.conk_penalty; a.n_spl = h->n_spl; a.scan = nullptr;
  int waves = std::min(h->n, h->n_cus * 32);
  c3k_launch_conk(&a, h->max_spl, (waves + 3) / 4, 0, h->stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// closed-form Savitzky-Golay coefficients: the same expression as the oracle, evaluated on the host.  The filter is symmetric and
// k_peaks adds mirrored taps first, so only c[0 .. half] is written: PeaksArgs::coef holds 64 doubles, enough for half <= 63
// (sg_window <= 127); all 2 * half + 1 coefficients would not fit it from window 65 on
static void savgol_coeffs(int window, double* c) {
  int m = (window - 1) / 2;
  double den = (double)(2 * m - 1) * (double)(2 * m + 1) * (double)(2 * m + 3);
  for (int k = -m; k <= 0; ++k) c[k + m] = 3.0 * (double)(3 * m * m + 3 * m - 1 - 5 * k * k) / den;
}

static int run_peaks(c3_handle* h) {
  static const int blocks_per_cu = c3k_peaks_blocks_per_cu();
  const int grid = std::min(h->n, h->n_cus * blocks_per_cu);       // = the workgroups resident at once; reads come off a queue
  h->peaks_grid = grid;
  const size_t mL = (size_t)h->maxL + 8;
  HIPCHK(h->d_bufA.ensure(sizeof(double) * mL * grid)); HIPCHK(h->d_bufB.ensure(sizeof(double) * mL * grid));
  HIPCHK(h->d_cand.ensure(sizeof(int32_t) * (mL / 2 + 2) * grid)); HIPCHK(h->d_cst.ensure((mL / 2 + 2) * grid));
  HIPCHK(h->d_raw.ensure(sizeof(int32_t) * (size_t)h->n * C3_MAX_PEAKS)); HIPCHK(h->d_nraw.ensure(sizeof(int32_t) * (size_t)h->n));
  PeaksArgs a; memset(&a, 0, sizeof(a));
  a.b = dev_batch(h); a.track = h->d_track.as<int32_t>(); a.info = h->d_info.as<C3Info>();
  a.bufA = h->d_bufA.as<double>(); a.bufB = h->d_bufB.as<double>(); a.cand = h->d_cand.as<int32_t>(); a.cstate = h->d_cst.as<uint8_t>();
  a.raw_peaks = h->d_raw.as<int32_t>(); a.n_raw = h->d_nraw.as<int32_t>(); a.sp_len = h->d_sp_len.as<int>();
  savgol_coeffs(h->cfg.sg_window, a.coef);
  a.maxL = (int64_t)mL; a.window = h->cfg.sg_window; a.iters = h->cfg.sg_iters; a.min_dist = h->cfg.mdistcutoff;
  a.cnt = dev_cnt(h);
  HIPCHK(zero_cnt(h, &a.cnt->peaks_queue));
  c3k_launch_peaks(&a, grid, h->stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// summary of the split -> work list + capacities
static int copy_summary(c3_handle* h) {
  const int n = h->n;
  HIPCHK(h->d_sum.ensure(sizeof(Summary) * (size_t)n));
  hipLaunchKernelGGL(k_summary, dim3((n + 255) / 256), dim3(256), 0, h->stream, h->d_info.as<C3Info>(), h->d_off.as<int64_t>(), n, h->d_sum.as<Summary>());
  h->sum.resize(n);
  HIPCHK(hipMemcpyAsync(h->sum.data(), h->d_sum.p, sizeof(Summary) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  // This wait (k_conk + k_peaks, ~15 % of a batch) is followed by the only host section the GPU waits for: the work list.  A
  // thread that slept through it (blocking sync) wakes up on a core that has dropped its clock, and the section then takes twice
  // as long (measured: 2.0 ms against 0.9 per 100 000 reads); so THIS wait polls.
  if (!getenv("C3_NO_SPIN")) {
    hipError_t q;
    while ((q = hipStreamQuery(h->stream)) == hipErrorNotReady) { for (int k_ = 0; k_ < 64; ++k_) __builtin_ia32_pause(); }
    if (q != hipSuccess) HIPCHK(q);
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  // longest used prefix of the per-read arrays (peaks / kept subreads are final after k_peaks; the zero-repeat rescue adds two)
  int k = 2;
  for (int i = 0; i < n; ++i) k = std::max(k, std::max(h->sum[i].n_peaks, h->sum[i].n_sub));
  h->res_prefix = std::min((k + 7) & ~7, (int)C3_MAX_PEAKS);
  return 0;
}

static void fill_zero_args(c3_handle* h, ZeroArgs& z, int nz) {
  memset(&z, 0, sizeof(z));
  z.b = dev_batch(h); z.info = h->d_info.as<C3Info>(); z.p = dev_params(h->cfg); z.cnt = dev_cnt(h);
  z.work = h->d_zwork.as<int>(); z.n_work = nz;
  z.D = h->s_zero_d.as<uint8_t>(); z.zinfo = h->d_zinfo.as<int4>(); z.zflag = h->d_zflag.as<uint8_t>();
  z.draft = h->d_draft.as<uint8_t>(); z.cons = h->d_cons.as<char>();
}

// zero-repeat rescue, first half (bin/determine_consensus.py:14-18,106-128): reads whose split kept no
// subread but has both dangling pieces get their overlap located and become 2-subread POA jobs.  k_zero takes the pairs
// its LDS rows and direction matrix hold; every other pair within zero_max_cells goes to k_zero_long.
static const long long ZL_BUDGET = 1LL << 30;    // k_zero_long scratch of all slots together (at least one slot)
static int run_zero(c3_handle* h) {
  h->zwork.clear();
  HIPCHK(h->d_zflag.ensure((size_t)h->n + 16));
  HIPCHK(hipMemsetAsync(h->d_zflag.p, 0, (size_t)h->n, h->stream));
  if (!h->cfg.zero || h->injected) return 0;
  // test hooks: C3_DEBUG_ZERO_LONG=1 sends every eligible read to k_zero_long, C3_DEBUG_ZERO_K=<n> sets its checkpoint interval
  const char* ev_long = getenv("C3_DEBUG_ZERO_LONG");
  const bool force_long = ev_long && atoi(ev_long) != 0;
  const char* ev_k = getenv("C3_DEBUG_ZERO_K");
  const int zk = (ev_k && atoi(ev_k) > 0) ? atoi(ev_k) : 256;
  long long dmax = 0, smax = 0;
  std::vector<int> zlong;
  for (int i = 0; i < h->n; ++i) {
    const Summary& s = h->sum[i];
    if (s.status != C3_ST_NO_CONSENSUS || s.n_sub != 0 || s.front <= 0 || s.tail <= 0) continue;
    const long long cells = (long long)s.front * s.tail;
    if (cells > h->cfg.zero_max_cells) continue;
    if (!force_long && s.front <= 4096 && cells <= (16 << 20)) {
      h->zwork.push_back(i);
      dmax = std::max(dmax, (long long)(s.front + 1) * (s.tail + 1));
    } else {
      zlong.push_back(i);
      smax = std::max(smax, c3_zl_layout(s.front, s.tail, zk).total);
    }
  }
  const int ns = (int)h->zwork.size(), nl = (int)zlong.size();
  h->zwork.insert(h->zwork.end(), zlong.begin(), zlong.end());
  const int nz = ns + nl;
  if (nz == 0) return 0;
  HIPCHK(h->d_zwork.ensure(sizeof(int) * (size_t)nz)); HIPCHK(h->d_zinfo.ensure(sizeof(int4) * (size_t)h->n));
  if (ns) {
    const int grid = std::min(ns, 512);
    HIPCHK(h->s_zero_d.ensure((size_t)dmax * grid + 64));
  }
  int grid_l = 0;
  if (nl) {
    grid_l = (int)std::min<long long>(std::min(nl, 2 * h->n_cus), std::max(1LL, ZL_BUDGET / smax));
    HIPCHK(h->s_zero_l.ensure((size_t)smax * grid_l));
  }
  HIPCHK(hipMemcpyAsync(h->d_zwork.p, h->zwork.data(), sizeof(int) * (size_t)nz, hipMemcpyHostToDevice, h->stream));
  if (ns) {
    ZeroArgs z; fill_zero_args(h, z, ns); z.dcap = dmax;
    DBG("zero: nz=%d grid=%d dmax=%lld\n", ns, std::min(ns, 512), dmax);
    c3k_launch_zero(&z, std::min(ns, 512), h->stream);
    HIPCHK(hipGetLastError());
  }
  if (nl) {
    ZeroArgs z; fill_zero_args(h, z, nl);
    z.work = h->d_zwork.as<int>() + ns; z.S = h->s_zero_l.as<uint8_t>(); z.scap = smax; z.zk = zk;
    DBG("zero long: nz=%d grid=%d slot=%lld K=%d\n", nl, grid_l, smax, zk);
    c3k_launch_zero_long(&z, grid_l, h->stream);
    HIPCHK(hipGetLastError());
  }
  { int r_ = copy_summary(h); DBG("zero done\n"); return r_; }              // the rescued reads now carry 2 pseudo-subreads
}

static int fetch_summary(c3_handle* h) {
  int rc = copy_summary(h);                       // (waits for k_conk + k_peaks: not host time)
  DBG("summary copied\n");
  if (rc) return rc;
  const auto wl0 = std::chrono::steady_clock::now();
  struct WlTimer { c3_handle* h; std::chrono::steady_clock::time_point t0; ~WlTimer() { h->tm.ms_host_worklist = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); } } wl_timer_{h, wl0};
  HIPCHK(zero_cnt(h, &dev_cnt(h)->zero_cells));
  if ((rc = run_zero(h))) return rc;
  const int n = h->n;
  h->work.clear();
  for (int i = 0; i < n; ++i) if (h->sum[i].status == C3_ST_OK && h->sum[i].n_sub >= 1) h->work.push_back(i);
  // longest first: better tail behaviour of the dynamic work queues.  Same order as a stable sort by descending cost
  // (ties: read order), done on packed (inverted cost, read) keys -- the GPU is idle while this runs
  if (n < (1 << 24)) {
    // stable LSD radix sort of (inverted cost, read) keys, 4 passes of 10 bits over the 40 cost bits (the reads are already in
    // index order, so stability gives the tie order for free): ~0.5 ms per 100 000 reads where std::sort took ~4 ms
    const size_t m = h->work.size();
    std::vector<uint64_t> keys(m), tmp(m);
    for (size_t k = 0; k < m; ++k) {
      const int i = h->work[k];
      const uint64_t cost = (uint64_t)h->sum[i].sum_sub * (uint64_t)h->sum[i].n_sub;          // < 2^40
      keys[k] = ((((uint64_t)1 << 40) - 1 - cost) << 24) | (uint64_t)i;
    }
    uint64_t* src = keys.data(); uint64_t* dst = tmp.data();
    for (int pass = 0; pass < 4; ++pass) {
      const int sh = 24 + 10 * pass;
      size_t cnt[1025] = {0};
      for (size_t k = 0; k < m; ++k) ++cnt[((src[k] >> sh) & 1023) + 1];
      for (int b = 0; b < 1024; ++b) cnt[b + 1] += cnt[b];
      for (size_t k = 0; k < m; ++k) dst[cnt[(src[k] >> sh) & 1023]++] = src[k];
      std::swap(src, dst);
    }
    for (size_t k = 0; k < m; ++k) h->work[k] = (int)(src[k] & 0xffffff);
  } else {
    std::stable_sort(h->work.begin(), h->work.end(), [&](int x, int y) {
      long cx = (long)h->sum[x].sum_sub * h->sum[x].n_sub, cy = (long)h->sum[y].sum_sub * h->sum[y].n_sub; return cx > cy; });
  }
  HIPCHK(h->d_work.ensure(sizeof(int) * std::max<size_t>(h->work.size(), 1)));
  if (!h->work.empty()) HIPCHK(hipMemcpyAsync(h->d_work.p, h->work.data(), sizeof(int) * h->work.size(), hipMemcpyHostToDevice, h->stream));
  return 0;
}

// one launch of k_poa over `nw` reads of `d_work` with the given capacities
static int launch_poa(c3_handle* h, const int* d_work, int nw, int Ncap, int K, int Pcap, long long cells, int* d_overflow, int* d_overflow16, int waves_per_cu, int wide_ring) {
  cells = (cells + 15) & ~15LL;                   // every per-slot arena starts 16-byte aligned
  cells = (cells + 63) & ~63LL;
  // far arena (32-bit cells of rows with a successor beyond the LDS ring, rows wider than a ring slot, rows with > 4 predecessors):
  // a quarter of the cells in the first pass (a few per cent are used), all of them in the 32-bit pass, where every row is far
  const bool w32 = d_overflow16 == nullptr || getenv("C3_DEBUG_POA32");      // the pass that takes the reads beyond 16 bits (test hook: every pass)
  const PoaLayout L = c3_poa_layout(Ncap, K, (int)cells, c3_poa_far_shift(w32), Pcap);
  const int slots = auto_slots(h, h->cfg.slots_poa, L.total, nw, waves_per_cu);
  const size_t S = (size_t)slots;
  HIPCHK(h->s_poa_i.ensure(L.ints * S)); HIPCHK(h->s_poa_nk.ensure(L.edges * S));
  HIPCHK(h->s_poa_cells.ensure(L.cells * S + 256)); HIPCHK(h->s_poa_b.ensure(L.bases * S)); HIPCHK(h->s_poa_sc.ensure(L.score * S));
  HIPCHK(h->s_poa_desc.ensure(L.desc * S)); HIPCHK(h->s_poa_jump.ensure(L.jump * S)); HIPCHK(h->s_poa_path.ensure(L.path * S));
  PoaArgs a; memset(&a, 0, sizeof(a));
  a.b = dev_batch(h); a.info = h->d_info.as<C3Info>(); a.p = dev_params(h->cfg);
  a.cnt = dev_cnt(h); a.work = d_work; a.n_work = nw;
  a.ibase = h->s_poa_i.as<int>(); a.ebase = h->s_poa_nk.as<int>(); a.cellsb = h->s_poa_cells.as<char>();
  a.bbase = h->s_poa_b.as<uint8_t>(); a.score = h->s_poa_sc.as<long long>();
  a.Ncap = Ncap; a.K = K; a.Pcap = Pcap; a.cells_cap = (int)cells; a.desc = h->s_poa_desc.as<uint4>(); a.jump = h->s_poa_jump.as<int>();
  a.pbase = h->s_poa_path.as<int>(); a.overflow = d_overflow; a.overflow16 = d_overflow16;
  if (const char* e = getenv("C3_DEBUG_POA_RBSPAN")) a.rb_span = std::max(3300, atoi(e));      // (>= the 400 units below the bias + a row's growth)
  a.no2col = getenv("C3_DEBUG_POA_NO2COL") != nullptr;
  a.draft = h->d_draft.as<uint8_t>(); a.tpos = h->d_tpos.as<int32_t>();
  a.msa_dbg = nullptr; a.msa_off = nullptr; a.msa_len = nullptr;
  if (h->debug_msa) { a.msa_dbg = h->d_msa.as<uint8_t>(); a.msa_off = h->d_msa_off.as<int64_t>(); a.msa_len = h->d_msa_len.as<int>(); }
  DBG("poa: nw=%d Ncap=%d K=%d cells=%lld slots=%d (%.1f MB per slot)%s\n", nw, Ncap, K, cells, slots, L.total / 1048576.0, d_overflow ? "" : (d_overflow16 ? " [full-size pass]" : " [32-bit pass]"));
  // the pass with an overflow list runs the 16-bit rows; the final pass (no list) the 32-bit rows only (C3_DEBUG_POA32: test hook, first pass too)
  c3k_launch_poa(&a, slots, w32 ? 1 : 0, wide_ring, h->stream);
  HIPCHK(hipGetLastError());
  return 0;
}

// K3 over the work list.  The per-slot scratch (graph arrays, DP cells) is sized for the TYPICAL alignment of the batch --
// small slots mean more resident waves, and the DP kernels live on resident waves -- and the few reads that overflow it
// (ragged subread lengths widen the adaptive band; long insertions add nodes) are queued by the kernel and redone by a
// second launch with worst-case scratch, so no read is ever lost to the smaller first-pass capacity.
static int run_poa(c3_handle* h) {
  const int nw = (int)h->work.size();
  HIPCHK(h->d_draft.ensure((size_t)h->total + 64)); HIPCHK(h->d_tpos.ensure(sizeof(int32_t) * (size_t)h->total + 64));
  HIPCHK(h->d_cons.ensure((size_t)h->total + 64));
  HIPCHK(hipMemsetAsync(h->d_tpos.p, 0xff, sizeof(int32_t) * (size_t)h->total, h->stream));
  if (nw == 0) return 0;
  int max_sum = 0, max_ns = 0, max_q = 0;
  for (int i : h->work) { max_sum = std::max(max_sum, h->sum[i].sum_sub); max_ns = std::max(max_ns, h->sum[i].n_sub); max_q = std::max(max_q, h->sum[i].max_sub); }
  const int Ncap_full = max_sum + 8, K = max_ns + 1, Pcap = max_sum + 8;
  const int w = h->cfg.poa_band_b + (int)(h->cfg.poa_band_f * max_q);
  long long cells_full = (long long)(2 * max_q + 2) * (2 * w + 1 + max_q / 5);
  if (max_ns < 2) cells_full = 64;
  if (cells_full > 0x7fffff00LL) cells_full = 0x7fffff00LL;
  // typical need: every further subread adds ~12 % nodes (mismatch siblings + insertions) to a graph of max_q nodes; a row
  // holds 2w+1 cells plus the drift between the row's nominal column and the argmax of its predecessors
  const double nodes_typ = (double)max_q * (1.0 + 0.15 * std::max(0, max_ns - 1));
  int Ncap = (int)std::min<double>(Ncap_full, 1.3 * nodes_typ + 256);
  long long cells = std::min<long long>(cells_full, (long long)(1.5 * nodes_typ * (2 * w + 12)) + 4096);
  if (const char* e_ = getenv("C3_DEBUG_POA_SMALL")) { Ncap = std::min(Ncap_full, std::max(64, atoi(e_))); cells = std::min<long long>(cells_full, 16LL * Ncap); }   // test hook: forces the second pass
  if (h->debug_msa) {
    std::vector<int64_t> mo(h->n + 1, 0);
    for (int i = 0; i < h->n; ++i) mo[i + 1] = mo[i] + (int64_t)h->sum[i].n_sub * (h->sum[i].sum_sub + 2);
    HIPCHK(h->d_msa.ensure((size_t)mo[h->n] + 64)); HIPCHK(h->d_msa_off.ensure(sizeof(int64_t) * (h->n + 1))); HIPCHK(h->d_msa_len.ensure(sizeof(int) * h->n));
    HIPCHK(hipMemcpyAsync(h->d_msa_off.p, mo.data(), sizeof(int64_t) * (h->n + 1), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->d_msa_len.p, 0, sizeof(int) * h->n, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  HIPCHK(h->d_overflow.ensure(sizeof(int) * 2 * (size_t)nw));
  C3Counters* dc = dev_cnt(h);        // (zero_cells of run_zero stay: tm.cells_poa counts them)
  HIPCHK(zero_cnt(h, &dc->queue)); HIPCHK(zero_cnt(h, &dc->cells)); HIPCHK(zero_cnt(h, &dc->poa_ovf)); HIPCHK(zero_cnt(h, &dc->poa_ovf16));
  HIPCHK(zero_cnt(h, &dc->phases));
  // ring geometry of the first pass: subreads beyond the LDS query copy (1792 bases) or with bands beyond two 64-column chunks
  // (w = band_b + band_f * Q; a row holds 2w+1 columns + the drift of its predecessors' maxima) take the WIDE instance
  // (4 ring rows of 192 cells, sliding query window); C3_DEBUG_POA_WIDE = 0 / 1 forces one (test hook)
  int wide_ring = (max_q > 1792 || 2 * w + 1 + 24 > 128) ? 1 : 0;
  if (const char* e_ = getenv("C3_DEBUG_POA_WIDE")) wide_ring = atoi(e_) ? 1 : 0;
  // pass 1: scratch for the typical alignment.  Its two lists: reads the scratch was too small for -> pass 2 (the same kernel, worst-case
  // scratch); reads with a score beyond the 16-bit cells (from either pass) -> pass 3 (the 32-bit instance, worst-case scratch)
  int* ovA = h->d_overflow.as<int>(); int* ovB = h->d_overflow.as<int>() + nw;
  int rc = launch_poa(h, h->d_work.as<int>(), nw, Ncap, K, Pcap, cells, ovA, ovB, 24, wide_ring);
  if (rc) return rc;
  h->n_poa_redo = 0; h->n_poa_redo16 = 0;
  C3Counters c;
  HIPCHK(read_counters(h, &c));
  if (c.poa_ovf > 0) {
    h->n_poa_redo = c.poa_ovf;
    HIPCHK(zero_cnt(h, &dc->queue));
    if ((rc = launch_poa(h, ovA, c.poa_ovf, Ncap_full, K, Pcap, cells_full, nullptr, ovB, 24, wide_ring))) return rc;
    HIPCHK(read_counters(h, &c));
  }
  if (c.poa_ovf16 > 0) {
    h->n_poa_redo += c.poa_ovf16; h->n_poa_redo16 = c.poa_ovf16;
    HIPCHK(zero_cnt(h, &dc->queue));
    if ((rc = launch_poa(h, ovB, c.poa_ovf16, Ncap_full, K, Pcap, cells_full, nullptr, nullptr, 24, 0))) return rc;
  }
  if (!h->zwork.empty()) {             // zero-repeat rescue, second half: stitch left + overlap consensus + right
    ZeroArgs z; fill_zero_args(h, z, (int)h->zwork.size());
    c3k_launch_zero_finish(&z, std::min((int)h->zwork.size(), 512), h->stream);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemcpyAsync(h->phase_poa, dc->phases, sizeof(h->phase_poa), hipMemcpyDeviceToHost, h->stream));
  return 0;
}

static int run_polish(c3_handle* h, float* ms_prep, float* ms_win, float* ms_st) {
  const int nw = (int)h->work.size();
  DBG("polish: nw=%d\n", nw);
  HIPCHK(h->d_cons.ensure((size_t)h->total + 64));
  if (nw == 0) return 0;
  const int WL = h->cfg.pol_window;
  int max_ns = 0, max_q = 0, max_dang = 0; long long wcap = 0;
  for (int i : h->work) {
    max_ns = std::max(max_ns, h->sum[i].n_sub); max_q = std::max(max_q, h->sum[i].max_sub); max_dang = std::max(max_dang, h->sum[i].max_dang);
    wcap += (2 * h->sum[i].max_sub + WL - 1) / WL + 1;
  }
  const int NLcap = max_ns + 2, NWcap = (2 * max_q + WL - 1) / WL + 1;
  // direction tags of one piece: one dword per lane and three rows, or two rows for a band that needs the wide rows (k_polish.hip:
  // ext_dir_bytes; 5 or 8 band offsets per lane; c3_create refuses a band beyond 64 * 8 offsets)
  const int64_t ecap = (int64_t)(max_dang / (2 * h->cfg.dang_band + 1 > 320 ? 2 : 3) + 2) * 256;
  const size_t per_slot_prep = (size_t)ecap + (size_t)NLcap * NWcap * 8;
  const int slots_p = auto_slots(h, h->cfg.slots_poa, per_slot_prep, nw, getenv("C3_DEBUG_PREP_WPC") ? atoi(getenv("C3_DEBUG_PREP_WPC")) : 20);
  HIPCHK(h->s_eD.ensure((size_t)ecap * slots_p));
  HIPCHK(h->s_lw.ensure(sizeof(int) * (size_t)NLcap * NWcap * 2 * slots_p));
  HIPCHK(h->d_wrec.ensure(sizeof(WinRec) * (size_t)wcap)); HIPCHK(h->d_wlay.ensure(sizeof(WLayer) * (size_t)wcap * NLcap));
  HIPCHK(h->d_wbase.ensure(sizeof(int) * (size_t)h->n));
  PrepArgs p; memset(&p, 0, sizeof(p));
  p.b = dev_batch(h); p.info = h->d_info.as<C3Info>(); p.p = dev_params(h->cfg);
  p.cnt = dev_cnt(h); p.work = h->d_work.as<int>(); p.n_work = nw;
  p.draft = h->d_draft.as<uint8_t>(); p.tpos = h->d_tpos.as<int32_t>();
  p.eD = h->s_eD.as<uint8_t>(); p.ecap = ecap;
  p.lw_first = h->s_lw.as<int>(); p.lw_last = p.lw_first + (size_t)NLcap * NWcap * slots_p; p.NLcap = NLcap; p.NWcap = NWcap;
  p.wrec = h->d_wrec.as<WinRec>(); p.wlay = h->d_wlay.as<WLayer>(); p.win_base = h->d_wbase.as<int>();
  p.wcap = (int)std::min<long long>(wcap, 0x7fffffff);
  const int bonus4 = 4 * (h->cfg.pol_match - h->cfg.pol_mismatch);
  p.sub_shift = -1;
  for (int b = 2; b <= 12; ++b) if (bonus4 == 1 << b) p.sub_shift = b;
  if (const char* e = getenv("C3_DEBUG_PREP_ROWS")) p.rows_old = !strcmp(e, "old");      // test hook (tests/test_gpu_prep_rows.py)
  HIPCHK(zero_counters(h));
  HIPCHK(hipEventRecord(h->ev[5], h->stream));
  DBG("prep: slots=%d ecap=%lld NL=%d NW=%d wcap=%lld\n", slots_p, (long long)ecap, NLcap, NWcap, (long long)wcap);
  c3k_launch_prep(&p, slots_p, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[6], h->stream));
  C3Counters c;
  HIPCHK(read_counters(h, &c));
  h->tm.cells_polish += c.cells; h->tm.cells_polish_computed += c.cells;       // dangling-piece extensions
  // k_prep reserves windows with an atomicAdd BEFORE its capacity check: after an overflow the counter exceeds wcap, and
  // the records past wcap were never written (the reads that overflowed carry C3_ST_LIMIT and n_win = 0)
  const int n_win = (int)std::min<long long>(c.n_windows, std::min<long long>(wcap, 0x7fffffff));
  h->n_windows = n_win;
  DBG("prep done: n_win=%d\n", n_win);
  const int wout_cap = 3 * WL + 64;
  HIPCHK(hipEventRecord(h->ev[7], h->stream));
  if (n_win > 0) {
    HIPCHK(h->d_wout.ensure((size_t)n_win * wout_cap));
    const int Ncap = 3 * WL + 40 * NLcap, K = NLcap + 2;   // cfg2: 1700 nodes -> 10.2 KB of LDS per wave, 16 waves per CU
    // DP scratch per slot, in cells (4 bytes of H + 1 byte of D each).  Worst case: every node a row, 704+ columns.  The FIRST
    // launch gets what the usual layer needs -- banded rows or a matrix of at most 256 columns over a graph of a window and a
    // quarter plus the branches its layers add: 256 bytes of direction words per row (+ the index rows and some head room) -- which is
    // a fifth of the worst case; a window with a layer beyond that is queued on the device and redone by a SECOND launch with
    // worst-case scratch on a few slots (no host round trip: it reads the count from device memory).  40 GB -> 10 GB of scratch
    // at cfg2 / cfg5 on 256 CUs: that much less to allocate and to touch for the first time in a fresh process.
    const long long hcap_full = (long long)(Ncap + 1) * 64 * 12;
    const int R_typ = std::min(Ncap, WL + WL / 4 + 30 * NLcap + 64);
    long long hcap = std::min(hcap_full, (long long)(R_typ + R_typ / 2 + 4) * 256);      // (a window in the second launch runs alone on an idle device, ~1.5 ms: sized so that a usual batch has none -- at + R_typ / 4 one cfg2 window in 400 000 took it)
    if (const char* e = getenv("C3_DEBUG_HCAP_DIV")) hcap = std::max(4096LL, hcap_full / std::max(1, atoi(e)) / 64 * 64);       // test hook: smaller first-launch scratch (more windows take the second launch)
    const WinLayout L = c3_win_layout(Ncap, K, hcap), L2 = c3_win_layout(Ncap, K, hcap_full);
    const int slots = auto_slots(h, h->cfg.slots_win, L.total, n_win, 20);
    const int slots2 = hcap < hcap_full ? std::min(slots, 256) : 0;
    const size_t S = (size_t)slots, S2 = (size_t)slots2;
    HIPCHK(h->s_win_i.ensure(L.ints * S + 64)); HIPCHK(h->s_win_nk.ensure(L.edges * S));
    HIPCHK(h->s_win_h.ensure(L.H * S)); HIPCHK(h->s_win_d.ensure(L.D * S + 256));
    HIPCHK(h->s_win_b.ensure(L.bases * S)); HIPCHK(h->s_win_sc.ensure(L.score * S)); HIPCHK(h->s_win_desc.ensure(L.desc * S));
    if (slots2) {                      // the second launch: worst-case DP cells on fewer slots, the other regions shared
      HIPCHK(h->s_win_h2.ensure(L2.H * S2)); HIPCHK(h->s_win_d2.ensure(L2.D * S2 + 256));
      HIPCHK(h->d_wovf.ensure(sizeof(int) * (size_t)n_win));
    }
    WinArgs a; memset(&a, 0, sizeof(a));
    a.b = dev_batch(h); a.p = dev_params(h->cfg); a.cnt = dev_cnt(h); a.n_win = n_win;
    a.wrec_in = h->d_wrec.as<WinRec>(); a.wrec = h->d_wrec.as<WinRec>(); a.wlay = h->d_wlay.as<WLayer>(); a.NLcap = NLcap;
    a.draft = h->d_draft.as<uint8_t>();
    a.ibase = h->s_win_i.as<int>(); a.ebase = h->s_win_nk.as<int>();
    a.base = h->s_win_b.as<uint8_t>(); a.score = h->s_win_sc.as<long long>();
    a.H = h->s_win_h.as<int32_t>(); a.D = h->s_win_d.as<uint16_t>(); a.rdesc = h->s_win_desc.as<uint4>(); a.Ncap = Ncap; a.K = K; a.hcap = hcap; a.Lcap = std::min(std::min(Ncap, 2 * WL + 30 * NLcap), ((getenv("C3_DEBUG_WIN_LDS") ? atoi(getenv("C3_DEBUG_WIN_LDS")) : 6656) - 16) / 6);       // (LDS per wave capped at 6.5 KB: at cfg4 the uncapped sweep arrays took 8.5 KB and k_window ran 7 % slower; larger graphs use the global-scratch sweep)
    if (const char* e = getenv("C3_DEBUG_WIN_LCAP")) a.Lcap = std::max(64, std::min(Ncap, atoi(e)));   // test hook: forces the global-scratch consensus path
    a.wout = h->d_wout.as<uint8_t>(); a.wout_cap = wout_cap;
    HIPCHK(zero_counters(h));
    if (const char* e = getenv("C3_DEBUG_BAND")) a.band_mode = !strcmp(e, "off") ? 1 : !strcmp(e, "fail") ? 2 : !strcmp(e, "verify") ? 3 : 0;    // test hook (tests/test_gpu_band.py)
    a.ovf_list = slots2 ? h->d_wovf.as<int>() : nullptr;
    c3k_launch_window(&a, slots, h->stream);
    HIPCHK(hipGetLastError());
    if (slots2) {
      a.H = h->s_win_h2.as<int32_t>(); a.D = h->s_win_d2.as<uint16_t>(); a.hcap = hcap_full;
      a.wlist = h->d_wovf.as<int>(); a.ovf_list = nullptr;
      c3k_launch_window(&a, slots2, h->stream);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(h->phase_win, dev_cnt(h)->phases, sizeof(h->phase_win), hipMemcpyDeviceToHost, h->stream));
  }
  HIPCHK(hipEventRecord(h->ev[8], h->stream));
  StitchArgs s; memset(&s, 0, sizeof(s));
  s.b = dev_batch(h); s.info = h->d_info.as<C3Info>(); s.work = h->d_work.as<int>(); s.n_work = nw;
  s.wrec = h->d_wrec.as<WinRec>(); s.win_base = h->d_wbase.as<int>(); s.wout = h->d_wout.as<uint8_t>(); s.wout_cap = wout_cap;
  s.cons = h->d_cons.as<char>(); s.zflag = h->d_zflag.as<uint8_t>();
  DBG("stitch\n");
  c3k_launch_stitch(&s, std::min(nw, h->n_cus * 16), h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev[9], h->stream));
  HIPCHK(read_counters(h, &c));
  if (n_win > 0) {
    h->tm.n_win_redo = c.win_ovf; h->tm.cells_polish += c.cells; h->tm.cells_polish_computed += c.cells_computed;
    h->tm.n_band_layers = c.band_layers; h->tm.n_band_fallback = c.band_fallback; h->tm.n_band_mismatch = c.band_mismatch;
    if (c.band_mismatch) fprintf(stderr, "c3poa: band verify mismatch in window %d layer %d (R = %d): last differing base q = %d, band row %d, full row %d, row of q+1 = %d\n",
                                 c.verify.window, c.verify.layer, c.verify.R, c.verify.q, c.verify.band_row, c.verify.full_row, c.verify.next_row);
  }
  HIPCHK(hipEventElapsedTime(ms_prep, h->ev[5], h->ev[6]));
  HIPCHK(hipEventElapsedTime(ms_win, h->ev[7], h->ev[8]));
  HIPCHK(hipEventElapsedTime(ms_st, h->ev[8], h->ev[9]));
  h->tm.n_windows = n_win;
  return 0;
}

// QV scratch: one direction slot per wave (ceil(longest piece / 8) groups of 256 bytes; a piece is at most a read) and, when
// the batch has reads longer than the LDS holds, one S + codes slot per workgroup; the slot count is bounded by a fixed budget.
static const long long QV_BUDGET = 1LL << 30;
static int qv_scratch(c3_handle* h, long long max_m, long long max_n, int n_items, QvArgs& a, int* grid) {
  a.dir_words = (max_m + 7) / 8 * 64;
  a.lds_n = (int)std::min<long long>((max_n + 15) / 16 * 16, c3k_qv_lds_max());
  a.gcap = max_n > a.lds_n ? (max_n + 15) / 16 * 16 : 0;
  const long long per_wg = 4 * 4 * a.dir_words + 5 * a.gcap;
  *grid = (int)std::max(1LL, std::min<long long>(std::min(n_items, h->n_cus * 8), QV_BUDGET / per_wg));
  HIPCHK(h->s_qv_dirs.ensure(sizeof(uint32_t) * (size_t)a.dir_words * 4 * (size_t)*grid + 256));
  if (a.gcap) HIPCHK(h->s_qv_g.ensure((size_t)a.gcap * 5 * (size_t)*grid + 256));
  a.dirs = h->s_qv_dirs.as<uint32_t>();
  a.gS = a.gcap ? h->s_qv_g.as<int>() : nullptr; a.gcodes = a.gcap ? h->s_qv_g.as<uint8_t>() + (size_t)a.gcap * 4 * (size_t)*grid : nullptr;
  HIPCHK(h->d_qv_cnt.ensure(64));
  HIPCHK(hipMemsetAsync(h->d_qv_cnt.p, 0, 64, h->stream));
  a.cnt = h->d_qv_cnt.as<unsigned long long>();
  return 0;
}
static int qv_counts(c3_handle* h, float ms) {
  unsigned long long c[8];
  HIPCHK(hipMemcpyAsync(c, h->d_qv_cnt.p, 64, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->qtm.ms_qv = ms; h->qtm.n_reads = (int64_t)c[0]; h->qtm.n_pieces = (int64_t)c[1]; h->qtm.n_skipped = (int64_t)c[2];
  h->qtm.band_cells = (int64_t)c[3]; h->qtm.edge_hits = (int64_t)c[4];
  return 0;
}

// per-base QVs of every read with a consensus (k_qv after the polish); writes the QV arena at off[i] as d_cons
static int run_qv(c3_handle* h) {
  for (int i = 0; i < 2; ++i) if (!h->ev_qv[i]) HIPCHK(hipEventCreate(&h->ev_qv[i]));
  HIPCHK(h->d_qv.ensure((size_t)h->total + 64));
  QvArgs a; memset(&a, 0, sizeof(a));
  int grid = 0;
  int rc = qv_scratch(h, h->maxL, h->maxL, h->n, a, &grid);
  if (rc) return rc;
  a.n_reads = h->n; a.info = h->d_info.as<C3Info>(); a.pk = h->d_pk.as<uint32_t>(); a.woff = h->d_woff.as<int64_t>();
  a.qual = h->d_qual.as<uint8_t>(); a.off = h->d_off.as<int64_t>(); a.cons = h->d_cons.as<char>(); a.qv = h->d_qv.as<char>();
  a.sa_np = -1;
  DBG("qv: grid=%d dir_words=%lld lds_n=%d gcap=%lld\n", grid, a.dir_words, a.lds_n, a.gcap);
  HIPCHK(hipEventRecord(h->ev_qv[0], h->stream));
  c3k_launch_qv(&a, grid, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev_qv[1], h->stream));
  HIPCHK(hipEventSynchronize(h->ev_qv[1]));
  float ms = 0; HIPCHK(hipEventElapsedTime(&ms, h->ev_qv[0], h->ev_qv[1]));
  return qv_counts(h, ms);
}

extern "C" int c3_batch_run(c3_handle* h, int stages) {
  if (!h || h->n <= 0) return C3_E_STATE;
  if ((stages & C3_STAGE_QV) && !((stages | h->stages_done) & C3_STAGE_POLISH))
    return c3_fail(h, C3_E_STATE, "C3_STAGE_QV needs the polish stage (in this call or an earlier one on the resident batch)");
  HIPCHK(hipSetDevice(h->cfg.device));
  int rc;
  float ms;
  hipEvent_t t0 = h->ev[0], t1 = h->ev[1], t2 = h->ev[2], t3 = h->ev[3], t4 = h->ev[4];
  DBG("run: start n=%d\n", h->n);
  const auto wall0 = std::chrono::steady_clock::now();
  const double alloc0 = g_alloc_ms;
  // per-run figures start from zero: repeated runs of one resident batch (bench.py, tools/) must not accumulate
  if (stages & C3_STAGE_CONK) { h->tm.ms_conk = 0; h->tm.cells_conk = 0; }
  if (stages & C3_STAGE_PEAKS) h->tm.ms_peaks = 0;
  if (stages & C3_STAGE_POA) { h->tm.ms_poa = 0; h->tm.cells_poa = 0; }
  if (stages & C3_STAGE_POLISH) { h->tm.ms_prep = h->tm.ms_window = h->tm.ms_stitch = 0; h->tm.cells_polish = 0; h->tm.cells_polish_computed = 0; h->tm.n_band_layers = h->tm.n_band_fallback = h->tm.n_band_mismatch = 0; h->tm.n_windows = 0; h->tm.n_win_redo = 0; }
  HIPCHK(hipEventRecord(t0, h->stream));
  if (stages & C3_STAGE_CONK) { if ((rc = run_conk(h))) return rc; h->tm.cells_conk = 0; for (int i = 0; i < h->n; ++i) h->tm.cells_conk += (h->off[i + 1] - h->off[i]) * (int64_t)h->max_spl; }
  HIPCHK(hipEventRecord(t1, h->stream));
  if (stages & C3_STAGE_PEAKS) { if ((rc = run_peaks(h))) return rc; }
  HIPCHK(hipEventRecord(t2, h->stream));
  float ms_prep = 0, ms_win = 0, ms_st = 0;
  if (stages & (C3_STAGE_POA | C3_STAGE_POLISH)) {
    DBG("run: conk+peaks launched\n");
    if ((rc = fetch_summary(h))) return rc;
    DBG("run: work list ready (%zu reads)\n", h->work.size());
    HIPCHK(hipEventRecord(t3, h->stream));
    if (stages & C3_STAGE_POA) {
      if ((rc = run_poa(h))) return rc;
    }
    HIPCHK(hipEventRecord(t4, h->stream));
    if (stages & C3_STAGE_POA) {
      C3Counters c;
      HIPCHK(read_counters(h, &c));
      if (!h->work.empty()) h->tm.cells_poa = (int64_t)(c.zero_cells + c.cells);      // zero-repeat overlaps + POA
      h->tm.n_poa_redo = h->n_poa_redo; h->tm.n_poa_redo16 = h->n_poa_redo16;
      DBG("run: poa done\n");
      HIPCHK(hipEventElapsedTime(&ms, t3, t4)); h->tm.ms_poa = ms;
    }
    if (stages & C3_STAGE_POLISH) { if ((rc = run_polish(h, &ms_prep, &ms_win, &ms_st))) return rc; }
  }
  if (stages & C3_STAGE_QV) { if ((rc = run_qv(h))) return rc; }
  HIPCHK(hipStreamSynchronize(h->stream));
  DBG("run: done\n");
  HIPCHK(hipGetLastError());
  if (stages & C3_STAGE_CONK) { HIPCHK(hipEventElapsedTime(&ms, t0, t1)); h->tm.ms_conk = ms; }
  if (stages & C3_STAGE_PEAKS) { HIPCHK(hipEventElapsedTime(&ms, t1, t2)); h->tm.ms_peaks = ms; }
  if (stages & C3_STAGE_POLISH) { h->tm.ms_prep = ms_prep; h->tm.ms_window = ms_win; h->tm.ms_stitch = ms_st; }
  h->tm.ms_total = h->tm.ms_conk + h->tm.ms_peaks + h->tm.ms_poa + h->tm.ms_prep + h->tm.ms_window + h->tm.ms_stitch;
  h->tm.ms_wall = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
  h->tm.ms_alloc = (float)(g_alloc_ms - alloc0);
  h->tm.ms_host_gap = h->tm.ms_wall - h->tm.ms_total;
  if (stages & C3_STAGES_ALL) h->stages_done &= ~C3_STAGE_QV;         // a rerun of any stage without QV leaves stale QVs
  h->stages_done |= stages;
  return C3_E_OK;
}

extern "C" int c3_batch_qv_timing(c3_handle* h, c3_qv_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->qtm;
  return C3_E_OK;
}

extern "C" int c3_batch_sync(c3_handle* h) {
  if (!h) return C3_E_ARG;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipStreamSynchronize(h->stream));
  return C3_E_OK;
}

// Results of the resident batch, in two halves so that the copy can run beside the NEXT batch's kernels:
//   c3_batch_results_snapshot  (owner thread, after c3_batch_run) freezes the records and the compact consensus bytes in device
//                              buffers of their own: offsets by a device scan (one 8-byte read back for the total), one gather
//                              kernel, three strided device copies -- ~0.3 ms;
//   c3_batch_results_fetch     copies the snapshot into the caller's buffers on the handle's third stream and waits for it.  It
//                              touches nothing but the snapshot, so ANOTHER thread may call it while the owner commits and runs
//                              the next batch (the only pair of calls on one handle that may overlap).
// One snapshot exists per handle: a second _snapshot before the _fetch returns C3_E_STATE.  c3_batch_results = both, back to back.
extern "C" int c3_batch_results_snapshot(c3_handle* h) {
  if (!h || h->n <= 0) return C3_E_ARG;
  if (h->snap_pending.load(std::memory_order_acquire)) return c3_fail(h, C3_E_STATE, "c3_batch_results_snapshot: the previous snapshot has not been fetched");
  HIPCHK(hipSetDevice(h->cfg.device));
  const int n = h->n;
  DBuf& d_coff = h->d_gather_off; DBuf& d_out = h->d_gather;
  const int nb = (n + 255) / 256;
  HIPCHK(d_coff.ensure(sizeof(int64_t) * (size_t)(n + 1))); HIPCHK(h->d_coff_part.ensure(sizeof(long long) * (size_t)nb));
  hipLaunchKernelGGL(k_coff_sums, dim3(nb), dim3(256), 0, h->stream, h->d_info.as<C3Info>(), n, h->d_coff_part.as<long long>());
  hipLaunchKernelGGL(k_coff_scan, dim3(1), dim3(1024), 0, h->stream, h->d_coff_part.as<long long>(), nb, d_coff.as<int64_t>(), n);
  hipLaunchKernelGGL(k_coff_final, dim3(nb), dim3(256), 0, h->stream, h->d_info.as<C3Info>(), n, h->d_coff_part.as<long long>(), d_coff.as<int64_t>());
  long long tot = 0;
  const bool have_cons = (h->stages_done & C3_STAGE_POLISH) != 0;
  if (have_cons) {
    HIPCHK(hipMemcpyAsync(h->h_tot, d_coff.as<int64_t>() + n, sizeof(long long), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    tot = *h->h_tot;
  }
  // A record is 3 kB of which a typical read uses ~150 bytes: the header plus the first n_peaks / n_sub entries of three
  // arrays.  When the batch's longest prefix is known (after the POA / polish stages) only those bytes are kept and cross PCIe, as
  // three strided copies; array entries past a read's n_peaks / n_sub are then UNSPECIFIED in the caller's records.
  const int kp = h->res_prefix;
  const bool prefix = kp > 0 && kp * 4 < C3_MAX_PEAKS && (h->stages_done & (C3_STAGE_POA | C3_STAGE_POLISH)) && !getenv("C3_FULL_RESULTS");
  const size_t pitch = sizeof(C3Info), head = offsetof(C3Info, peaks);
  const size_t o_sb = offsetof(C3Info, sub_beg), o_se = offsetof(C3Info, sub_end);
  HIPCHK(h->d_info_snap.ensure(pitch * (size_t)n));
  const char* src = h->d_info.as<char>(); char* snap = h->d_info_snap.as<char>();
  if (prefix) {
    HIPCHK(hipMemcpy2DAsync(snap, pitch, src, pitch, head + 4 * (size_t)kp, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpy2DAsync(snap + o_sb, pitch, src + o_sb, pitch, 4 * (size_t)kp, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpy2DAsync(snap + o_se, pitch, src + o_se, pitch, 4 * (size_t)kp, (size_t)n, hipMemcpyDeviceToDevice, h->stream));
  } else {
    HIPCHK(hipMemcpyAsync(snap, src, pitch * (size_t)n, hipMemcpyDeviceToDevice, h->stream));
  }
  if (have_cons && tot > 0) {
    // gather on the device (one wave per read): the fetch is then ONE device->host copy of the compact bytes
    HIPCHK(d_out.ensure((size_t)tot + 64));
    hipLaunchKernelGGL(k_gather_cons, dim3((unsigned)std::min((n + 3) / 4, h->n_cus * 32)), dim3(256), 0, h->stream,
                       h->d_cons.as<char>(), h->d_off.as<int64_t>(), d_coff.as<int64_t>(), n, d_out.as<char>());
  }
  const bool have_qv = have_cons && (h->stages_done & C3_STAGE_QV) != 0;
  if (have_qv && tot > 0) {                                   // the QV bytes, gathered at the same offsets
    HIPCHK(h->d_gather_qv.ensure((size_t)tot + 64));
    hipLaunchKernelGGL(k_gather_cons, dim3((unsigned)std::min((n + 3) / 4, h->n_cus * 32)), dim3(256), 0, h->stream,
                       h->d_qv.as<char>(), h->d_off.as<int64_t>(), d_coff.as<int64_t>(), n, h->d_gather_qv.as<char>());
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev_dn, h->stream));
  h->snap_n = n; h->snap_kp = prefix ? kp : 0; h->snap_tot = tot; h->snap_cons = have_cons; h->snap_qv = have_qv;
  h->snap_pending.store(true, std::memory_order_release);
  return C3_E_OK;
}

// c3_batch_results_fetch and c3_batch_results_fetch_qv (qv != NULL: the QV bytes too, same offsets and cap)
static int results_fetch(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv) {
  if (!h || !res) return C3_E_ARG;
  if (!h->snap_pending.load(std::memory_order_acquire)) return C3_E_STATE;          // (h->err belongs to the owner thread: not touched here)
  if (qv && !h->snap_qv) return C3_E_STATE;                                          // (the snapshot stays pending for a plain fetch)
  hipError_t e;
#define DNCHK(x) do { if ((e = (x)) != hipSuccess) { h->snap_pending.store(false, std::memory_order_release); return C3_E_HIP; } } while (0)
  DNCHK(hipSetDevice(h->cfg.device));
  const int n = h->snap_n, kp = h->snap_kp;
  const size_t pitch = sizeof(C3Info), head = offsetof(C3Info, peaks);
  const size_t o_sb = offsetof(C3Info, sub_beg), o_se = offsetof(C3Info, sub_end);
  const char* snap = h->d_info_snap.as<char>(); char* dst = (char*)res;
  hipStream_t dn = h->stream_dn;
  DNCHK(hipStreamWaitEvent(dn, h->ev_dn, 0));
  if (kp > 0) {
    DNCHK(hipMemcpy2DAsync(dst, pitch, snap, pitch, head + 4 * (size_t)kp, (size_t)n, hipMemcpyDeviceToHost, dn));
    DNCHK(hipMemcpy2DAsync(dst + o_sb, pitch, snap + o_sb, pitch, 4 * (size_t)kp, (size_t)n, hipMemcpyDeviceToHost, dn));
    DNCHK(hipMemcpy2DAsync(dst + o_se, pitch, snap + o_se, pitch, 4 * (size_t)kp, (size_t)n, hipMemcpyDeviceToHost, dn));
  } else {
    DNCHK(hipMemcpyAsync(dst, snap, pitch * (size_t)n, hipMemcpyDeviceToHost, dn));
  }
  if (cons_off) DNCHK(hipMemcpyAsync(cons_off, h->d_gather_off.p, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, dn));
  const bool fits = !(cons_off && cons) || h->snap_tot <= cons_cap;
  if (cons_off && cons && fits && h->snap_cons && h->snap_tot > 0) DNCHK(hipMemcpyAsync(cons, h->d_gather.p, (size_t)h->snap_tot, hipMemcpyDeviceToHost, dn));
  if (qv && cons_off && cons && fits && h->snap_tot > 0) DNCHK(hipMemcpyAsync(qv, h->d_gather_qv.p, (size_t)h->snap_tot, hipMemcpyDeviceToHost, dn));
  DNCHK(hipStreamSynchronize(dn));
#undef DNCHK
  h->snap_pending.store(false, std::memory_order_release);
  return fits ? C3_E_OK : C3_E_LIMIT;                 // too small: the records and the offsets (needed size = cons_off[n]) were still delivered
}

extern "C" int c3_batch_results_fetch(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off) {
  return results_fetch(h, res, cons, cons_cap, cons_off, nullptr);
}
extern "C" int c3_batch_results_fetch_qv(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv) {
  if (!qv) return C3_E_ARG;
  return results_fetch(h, res, cons, cons_cap, cons_off, qv);
}

extern "C" int c3_batch_results_qv(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv) {
  if (!h || h->n <= 0 || !res || !qv) return C3_E_ARG;
  if (!(h->stages_done & C3_STAGE_QV) || !(h->stages_done & C3_STAGE_POLISH)) return c3_fail(h, C3_E_STATE, "the resident batch did not run C3_STAGE_QV");
  int rc = c3_batch_results_snapshot(h);
  if (rc) return rc;
  rc = c3_batch_results_fetch_qv(h, res, cons, cons_cap, cons_off, qv);
  if (rc == C3_E_LIMIT) return c3_fail(h, C3_E_LIMIT, "consensus buffer too small");
  if (rc == C3_E_HIP) return c3_fail(h, C3_E_HIP, "HIP error while copying the results");
  return rc;
}

extern "C" int c3_batch_results(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off) {
  if (!h || h->n <= 0 || !res) return C3_E_ARG;
  int rc = c3_batch_results_snapshot(h);
  if (rc) return rc;
  rc = c3_batch_results_fetch(h, res, cons, cons_cap, cons_off);
  if (rc == C3_E_LIMIT) return c3_fail(h, C3_E_LIMIT, "consensus buffer too small");
  if (rc == C3_E_HIP) return c3_fail(h, C3_E_HIP, "HIP error while copying the results");
  return rc;
}

// PMC calibration: read `bytes` with one dword per lane, write `bytes` with one dword per
// lane -- the access width the DP kernels use -- so FETCH_SIZE / WRITE_SIZE can be checked against a
// known byte count on this device before they are trusted for k_window / k_poa.
__global__ void k_calib_rw(const uint32_t* in, uint32_t* out, size_t nwords) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, st = (size_t)gridDim.x * blockDim.x;
  uint32_t acc = 0;
  for (size_t k = i; k < nwords; k += st) acc += in[k];
  for (size_t k = i; k < nwords; k += st) out[k] = acc + (uint32_t)k;
}
extern "C" int c3_debug_calibrate(c3_handle* h, long long bytes) {
  if (!h || bytes < 4096) return C3_E_ARG;
  HIPCHK(hipSetDevice(h->cfg.device));
  uint32_t *a = nullptr, *b = nullptr;
  HIPCHK(hipMalloc(&a, (size_t)bytes)); HIPCHK(hipMalloc(&b, (size_t)bytes));
  HIPCHK(hipMemsetAsync(a, 1, (size_t)bytes, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  hipLaunchKernelGGL(k_calib_rw, dim3(h->n_cus * 8), dim3(256), 0, h->stream, a, b, (size_t)bytes / 4);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipFree(a)); HIPCHK(hipFree(b));
  return C3_E_OK;
}

// diagnostic builds (-DC3_PHASE_PROF) only: per-phase cycle sums of k_poa (which=0) / k_window (which=1)
extern "C" int c3_debug_phases(c3_handle* h, int which, unsigned long long* out) {
  if (!h || !out) return C3_E_ARG;
  memcpy(out, which ? h->phase_win : h->phase_poa, 128);
  return C3_E_OK;
}

extern "C" int c3_batch_timing(c3_handle* h, c3_timing* t) { if (!h || !t) return C3_E_ARG; *t = h->tm; return C3_E_OK; }

// ---- probes -----------------------------------------------------------------------------
extern "C" int c3_fetch_track(c3_handle* h, int read, int32_t* out, int64_t cap) {
  if (!h || read < 0 || read >= h->n || !out) return C3_E_ARG;
  if (!(h->stages_done & C3_STAGE_CONK)) return c3_fail(h, C3_E_STATE, "conk stage not run");
  int64_t L = h->off[read + 1] - h->off[read];
  if (cap < L) return C3_E_LIMIT;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(hipMemcpy(out, h->d_track.as<int32_t>() + h->off[read], sizeof(int32_t) * (size_t)L, hipMemcpyDeviceToHost));
  return (int)L;
}
extern "C" int c3_fetch_smoothed(c3_handle* h, int read, double* out, int64_t cap) {
  if (!h || read < 0 || read >= h->n || !out) return C3_E_ARG;
  if (!(h->stages_done & C3_STAGE_PEAKS)) return c3_fail(h, C3_E_STATE, "peaks stage not run");
  if (h->n > h->peaks_grid) return c3_fail(h, C3_E_STATE, "smoothed tracks are only retained when the batch fits the peaks grid");
  int64_t L = h->off[read + 1] - h->off[read];
  if (cap < L) return C3_E_LIMIT;
  HIPCHK(hipSetDevice(h->cfg.device));
  // result buffer after `iters` ping-pong passes: A if iters is even, B if odd
  const double* src = ((h->cfg.sg_iters & 1) ? h->d_bufB.as<double>() : h->d_bufA.as<double>()) + (size_t)read * ((size_t)h->maxL + 8);
  HIPCHK(hipMemcpy(out, src, sizeof(double) * (size_t)L, hipMemcpyDeviceToHost));
  return (int)L;
}
extern "C" int c3_fetch_raw_peaks(c3_handle* h, int read, int32_t* out, int cap) {
  if (!h || read < 0 || read >= h->n || !out) return C3_E_ARG;
  if (!(h->stages_done & C3_STAGE_PEAKS)) return c3_fail(h, C3_E_STATE, "peaks stage not run");
  HIPCHK(hipSetDevice(h->cfg.device));
  int n = 0;
  HIPCHK(hipMemcpy(&n, h->d_nraw.as<int32_t>() + read, sizeof(int), hipMemcpyDeviceToHost));
  if (n > cap) return C3_E_LIMIT;
  if (n > 0) HIPCHK(hipMemcpy(out, h->d_raw.as<int32_t>() + (size_t)read * C3_MAX_PEAKS, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
  return n;
}
extern "C" int c3_fetch_draft(c3_handle* h, int read, char* out, int cap) {
  if (!h || read < 0 || read >= h->n || !out) return C3_E_ARG;
  if (!(h->stages_done & C3_STAGE_POA)) return c3_fail(h, C3_E_STATE, "POA stage not run");
  HIPCHK(hipSetDevice(h->cfg.device));
  C3Info inf;
  HIPCHK(hipMemcpy(&inf, h->d_info.as<C3Info>() + read, sizeof(C3Info), hipMemcpyDeviceToHost));
  int C = inf.draft_len;
  if (C > cap) return C3_E_LIMIT;
  if (C > 0) {
    std::vector<uint8_t> tmp(C);
    HIPCHK(hipMemcpy(tmp.data(), h->d_draft.as<uint8_t>() + h->off[read], C, hipMemcpyDeviceToHost));
    for (int i = 0; i < C; ++i) out[i] = "ACGT"[tmp[i] & 3];
  }
  return C;
}
static int fetch_msa_rows(c3_handle* h, int read, int nrows, char* out, int64_t cap, int* msa_len) {
  if (!h->debug_msa || !h->d_msa.p) return c3_fail(h, C3_E_STATE, "MSA rows are only kept by c3_poa_msa / debug batches");
  int ml = 0;
  HIPCHK(hipMemcpy(&ml, h->d_msa_len.as<int>() + read, sizeof(int), hipMemcpyDeviceToHost));
  *msa_len = ml;
  if (ml <= 0) return 0;
  if ((int64_t)ml * nrows > cap) return C3_E_LIMIT;
  std::vector<int64_t> mo(2);
  HIPCHK(hipMemcpy(mo.data(), h->d_msa_off.as<int64_t>() + read, sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<uint8_t> tmp((size_t)ml * nrows);
  HIPCHK(hipMemcpy(tmp.data(), h->d_msa.as<uint8_t>() + mo[0], tmp.size(), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < tmp.size(); ++i) out[i] = tmp[i] > 3 ? '-' : "ACGT"[tmp[i]];
  return 0;
}
extern "C" int c3_fetch_msa2(c3_handle* h, int read, char* rowA, char* rowB, int cap) {
  if (!h || read < 0 || read >= h->n || !rowA || !rowB) return C3_E_ARG;
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<char> tmp((size_t)cap * 2 + 2);
  int ml = 0;
  int rc = fetch_msa_rows(h, read, 2, tmp.data(), (int64_t)cap * 2, &ml);
  if (rc) return rc;
  memcpy(rowA, tmp.data(), ml); memcpy(rowB, tmp.data() + ml, ml);
  return ml;
}

// inject a pre-split "read": [front][sub0]...[subn-1][tail]; skips conk/peaks
static int inject(c3_handle* h, int n, const char* const* subs, const char* const* quals, const int* lens,
                  const char* front, const char* front_q, int front_len, const char* tail, const char* tail_q, int tail_len) {
  if (n < 1 || n > C3_MAX_SUB) return c3_fail(h, C3_E_LIMIT, "1..250 subreads");
  if (h->n_spl <= 0) { const char sp[] = "ACGT"; int64_t o[2] = {0, 4}; int rc = c3_set_splints(h, 1, sp, o); if (rc) return rc; }
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
  int64_t off[2] = {0, (int64_t)seq.size()};
  int16_t sid = 0; char st = '+';
  int rc = c3_batch_upload(h, 1, seq.data(), ql.data(), off, &sid, &st);
  if (rc) return rc;
  HIPCHK(hipMemcpy(h->d_info.p, &r, sizeof(r), hipMemcpyHostToDevice));
  h->injected = true;
  return 0;
}

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
  const long long dcap = (long long)(h->maxL + 1) * (h->max_spl + 1) + 64;
  const int grid = (int)std::min<size_t>(items, (size_t)h->n_cus * 16);
  DBuf res, dd;
  HIPCHK(res.ensure(sizeof(int32_t) * 12 * items)); HIPCHK(dd.ensure((size_t)dcap * grid));
  HIPCHK(zero_cnt(h, &dev_cnt(h)->queue));
  AdapterArgs a; memset(&a, 0, sizeof(a));
  a.b = dev_batch(h); a.p = dev_params(h->cfg); a.cnt = dev_cnt(h);
  a.ad_codes = h->d_sp_codes.as<uint8_t>(); a.ad_len = h->d_sp_len.as<int>(); a.n_ad = h->n_spl;
  a.D = dd.as<uint8_t>(); a.dcap = dcap; a.out = res.as<int32_t>();
  c3k_launch_adapter(&a, grid, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, res.p, sizeof(int32_t) * 12 * items, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
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
  HIPCHK(dp.ensure((size_t)n * 64)); HIPCHK(dl.ensure(sizeof(int) * (size_t)n)); HIPCHK(di.ensure(ib + 16));
  HIPCHK(doff.ensure(sizeof(int64_t) * (size_t)(n_idx + 1))); HIPCHK(dout.ensure(sizeof(int) * (size_t)n));
  HIPCHK(hipMemcpyAsync(dp.p, pieces, (size_t)n * 64, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dl.p, lens, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(di.p, idx_cat, ib, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(doff.p, idx_off, sizeof(int64_t) * (size_t)(n_idx + 1), hipMemcpyHostToDevice, h->stream));
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
  const int rc = c3_post_check_args("c3_post_emit", a, arena, cap, stream_off, n_kept);
  if (rc != C3_E_OK) return c3_fail(h, rc, c3_last_error(nullptr));
  HIPCHK(hipSetDevice(h->cfg.device));
  for (hipEvent_t& ev : h->ev_post) if (!ev) HIPCHK(hipEventCreate(&ev));
  PostArgs p; memset(&p, 0, sizeof(p));
  p.n = a->n; p.S = 3 * a->n_dest + 3;
  p.o.n_ad = a->n_ad; p.o.class5 = a->class5; p.o.undirectional = a->undirectional != 0; p.o.trim = a->trim != 0; p.o.barcoded = a->barcoded != 0;
  p.o.quals = a->quals != nullptr; p.o.has_index = a->has_index != 0; p.o.n_idx = a->has_index ? a->n_idx : 0; p.o.n_dest = a->n_dest;
  const int S = p.S, n = a->n, nb = (n + 255) / 256;
  const size_t sb = n ? (size_t)a->off[n] : 0, nmb = n ? (size_t)a->name_off[n] : 0, tb = sizeof(int32_t) * 24 * (size_t)n * a->n_ad;
  const size_t anb = a->n_ad ? (size_t)a->ad_name_off[a->n_ad] : 0, ib = p.o.n_idx ? (size_t)a->idx_off[p.o.n_idx] : 0;
  // every input buffer keeps 16 bytes of slack: the dword copies of k_post_emit read whole aligned dwords
  struct Up { const void* src; size_t bytes; } up[13] = {
    {a->names, nmb}, {a->name_off, sizeof(int64_t) * (n + 1)}, {a->seqs, sb}, {a->quals, a->quals ? sb : 0}, {a->off, sizeof(int64_t) * (n + 1)},
    {a->table, tb}, {a->ad_len, sizeof(int32_t) * a->n_ad}, {a->ad_class, sizeof(int32_t) * a->n_ad}, {a->ad_names, anb},
    {a->ad_name_off, a->n_ad ? sizeof(int64_t) * (a->n_ad + 1) : 0}, {a->idx_cat, ib}, {a->idx_off, p.o.n_idx ? sizeof(int64_t) * (p.o.n_idx + 1) : 0},
    {a->idx_dest, sizeof(int32_t) * p.o.n_idx}};
  DBuf* d = h->d_post;
  for (int k = 0; k < 13; ++k) {
    HIPCHK(d[k].ensure(up[k].bytes + 16));
    if (n > 0 && up[k].bytes) HIPCHK(hipMemcpyAsync(d[k].p, up[k].src, up[k].bytes, hipMemcpyHostToDevice, h->stream));
  }
  DBuf& work = d[13]; DBuf& offs = d[14]; DBuf& out = d[15];
  // work = dec [n] | len [n][6] | roff [n][6] | bsum [nb][S + 1]
  const size_t w_dec = 0, w_len = w_dec + sizeof(C3PostDec) * n, w_roff = w_len + sizeof(int64_t) * C3_POST_REC * n, w_bsum = w_roff + sizeof(int64_t) * C3_POST_REC * n;
  HIPCHK(work.ensure(w_bsum + sizeof(long long) * (size_t)(nb + 1) * (S + 1)));
  HIPCHK(offs.ensure(sizeof(int64_t) * (S + 2)));
  p.names = d[0].as<uint8_t>(); p.name_off = d[1].as<int64_t>(); p.seqs = d[2].as<uint8_t>(); p.quals = a->quals ? d[3].as<uint8_t>() : nullptr;
  p.off = d[4].as<int64_t>(); p.table = d[5].as<int32_t>(); p.ad_len = d[6].as<int32_t>(); p.ad_class = d[7].as<int32_t>();
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
  std::vector<int64_t> so((size_t)S + 2);
  HIPCHK(hipMemcpyAsync(so.data(), offs.p, sizeof(int64_t) * (S + 2), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int64_t need = 0;                                              // the sums come from lengths the rule bounds: anything else is a kernel fault
  for (int s = 0; s <= S; ++s) { if (so[s] < need) return c3_fail(h, C3_E_HIP, "k_post: stream offsets out of order"); need = so[s]; }
  if (so[0] != 0 || so[S + 1] < 0 || so[S + 1] > n) return c3_fail(h, C3_E_HIP, "k_post: header out of range");
  memcpy(stream_off, so.data(), sizeof(int64_t) * (S + 1));
  *n_kept = so[S + 1];
  h->ptm = c3_post_timing{};
  if (need > cap) return c3_fail(h, C3_E_LIMIT, "c3_post_emit: arena too small (bytes needed in stream_off[S])");
  HIPCHK(out.ensure((size_t)need + 16));
  p.arena = out.as<uint8_t>();
  HIPCHK(hipEventRecord(h->ev_post[3], h->stream));
  c3k_launch_post_emit(&p, h->stream);
  HIPCHK(hipEventRecord(h->ev_post[4], h->stream));
  HIPCHK(hipGetLastError());
  if (need) HIPCHK(hipMemcpyAsync(arena, out.p, (size_t)need, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipEventElapsedTime(&h->ptm.ms_classify, h->ev_post[0], h->ev_post[1]));
  HIPCHK(hipEventElapsedTime(&h->ptm.ms_scan, h->ev_post[1], h->ev_post[2]));
  HIPCHK(hipEventElapsedTime(&h->ptm.ms_emit, h->ev_post[3], h->ev_post[4]));
  h->ptm.n_reads = n; h->ptm.n_kept = so[S + 1]; h->ptm.in_bytes = (int64_t)(nmb + sb * (a->quals ? 2 : 1) + tb); h->ptm.out_bytes = need;
  h->ptm.ms_call = (float)(dbg_now_ms() - t_call);
  return C3_E_OK;
}
extern "C" int c3_post_emit_timing(c3_handle* h, c3_post_timing* t) {
  if (!h || !t) return C3_E_ARG;
  *t = h->ptm;
  return C3_E_OK;
}

// sample demultiplexer (paper/Demultiplex_R2C2_reads.py, demultiplex): k_demux over n heads of 300 bytes; the host
// statement is c3_demux_host (c3_io.cpp), which also holds the checks both share (c3_demux_prepare).
int c3_demux_prepare(int n_a, const char* a_cat, const int64_t* a_off, int n_b, const char* b_cat, const int64_t* b_off,
                     uint8_t* tab, int* n_codes, const char** msg);
extern "C" int c3_demux_indexes(c3_handle* h, int n, const char* heads, int n_a, const char* a_cat, const int64_t* a_off,
                                int n_b, const char* b_cat, const int64_t* b_off, int32_t* win, uint8_t* dist) {
  if (!h) return C3_E_ARG;
  if (n < 0 || (n > 0 && (!heads || !win))) return c3_fail(h, C3_E_ARG, "heads / win missing");
  uint8_t tab[256]; int K = 0; const char* msg = "";
  const int rc = c3_demux_prepare(n_a, a_cat, a_off, n_b, b_cat, b_off, tab, &K, &msg);
  if (rc != C3_E_OK) return c3_fail(h, rc, msg);
  if (n == 0) return C3_E_OK;
  // meta = Peq [I][K+1] words (bit j of Peq[k][c]: byte j of index k has code c), lengths [I] words, byte codes [256]
  const int I = n_a + n_b, K1 = K + 1;
  std::vector<uint32_t> meta((size_t)I * K1 + I + 64, 0u);
  for (int k = 0; k < I; ++k) {
    const char* cat = k < n_a ? a_cat : b_cat;
    const int64_t* off = k < n_a ? a_off + k : b_off + (k - n_a);
    const int m = (int)(off[1] - off[0]);
    for (int j = 0; j < m; ++j) meta[(size_t)k * K1 + tab[(uint8_t)cat[off[0] + j]]] |= 1u << j;
    meta[(size_t)I * K1 + k] = (uint32_t)m;
  }
  memcpy(&meta[(size_t)I * K1 + I], tab, 256);
  const size_t hb = (size_t)n * C3_DEMUX_HEAD, wb = sizeof(int32_t) * 2 * (size_t)n, db = dist ? (size_t)n * I : 0;
  HIPCHK(hipSetDevice(h->cfg.device));
  HIPCHK(h->d_dmx_heads.ensure(hb)); HIPCHK(h->d_dmx_meta.ensure(sizeof(uint32_t) * meta.size())); HIPCHK(h->d_dmx_out.ensure(wb + db));
  HIPCHK(hipMemcpyAsync(h->d_dmx_heads.p, heads, hb, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->d_dmx_meta.p, meta.data(), sizeof(uint32_t) * meta.size(), hipMemcpyHostToDevice, h->stream));
  uint8_t* d_out = h->d_dmx_out.as<uint8_t>();
  c3k_launch_demux(h->d_dmx_heads.as<uint8_t>(), n, h->d_dmx_meta.as<uint8_t>(), n_a, n_b, K1, (int32_t*)d_out,
                   dist ? d_out + wb : nullptr, h->stream);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(win, d_out, wb, hipMemcpyDeviceToHost, h->stream));
  if (dist) HIPCHK(hipMemcpyAsync(dist, d_out + wb, db, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));      // meta is a host vector of this frame
  return C3_E_OK;
}

// stand-alone QVs of one consensus (k_qv on one workgroup); the host statement and the shared refusals are in c3_qv.cpp.
// The pieces are 2-bit packed here the way c3_batch_stage packs reads (every piece starts on a word).
int c3_qv_check(const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat, const int64_t* piece_off,
                const int32_t* modes, const char* qv_out, const char** msg);
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
  const int rc = qv_scratch(h, max_m, n, 1, a, &grid);
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
  HIPCHK(d_rows.ensure((size_t)2 * msa_len)); HIPCHK(d_qa.ensure((size_t)lenA + 16)); HIPCHK(d_qb.ensure((size_t)lenB + 16));
  HIPCHK(d_scr.ensure((size_t)2 * msa_len + 16)); HIPCHK(d_out.ensure((size_t)msa_len + 16)); HIPCHK(d_len.ensure(16));
  HIPCHK(hipMemcpyAsync(d_rows.p, rows.data(), rows.size(), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d_qa.p, same ? qualB : qualA, (size_t)lenA, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(d_qb.p, qualB, (size_t)lenB, hipMemcpyHostToDevice, h->stream));
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
  if (h->n_spl <= 0) { const char sp[] = "ACGT"; int64_t o[2] = {0, 4}; int rc = c3_set_splints(h, 1, sp, o); if (rc) return rc; }
  std::string seq((size_t)n, 'A'), ql((size_t)n, 'I');
  int64_t off[2] = {0, n};
  int16_t sid = 0; char st = '+';
  int rc = c3_batch_upload(h, 1, seq.data(), ql.data(), off, &sid, &st);
  if (rc) return rc;
  HIPCHK(h->d_track.ensure(sizeof(int32_t) * (size_t)n + 64));
  HIPCHK(hipMemcpy(h->d_track.p, scores, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
  h->stages_done |= C3_STAGE_CONK;
  const int md0 = h->cfg.mdistcutoff;
  h->cfg.mdistcutoff = min_dist;
  rc = c3_batch_run(h, C3_STAGE_PEAKS);
  h->cfg.mdistcutoff = md0;
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
  const bool dbg0 = h->debug_msa; h->debug_msa = (msa != nullptr);
  rc = c3_batch_run(h, C3_STAGE_POA);
  if (rc == 0 && cons) {
    // pyabpoa semantics: the consensus is the heaviest bundle also for n == 2; the batch path gives the
    // pairwise-merged draft there, so only n != 2 is served from the draft
    if (n == 2) { h->debug_msa = dbg0; return c3_fail(h, C3_E_ARG, "out_cons with exactly 2 sequences is not a reference call shape"); }
    int C = c3_fetch_draft(h, 0, cons, cons_cap);
    if (C < 0) rc = C; else if (cons_len) *cons_len = C;
  }
  if (rc == 0 && msa) { int ml = 0; rc = fetch_msa_rows(h, 0, n, msa, msa_cap, &ml); if (rc == 0 && msa_len) *msa_len = ml; }
  h->debug_msa = dbg0;
  return rc;
}

extern "C" int c3_zero_repeats(c3_handle* h, const char* d0, const char* q0, int n0, const char* d1, const char* q1, int n1,
                               int min_len, char* out, int cap, int* out_len) {
  if (!h || !d0 || !d1 || n0 <= 0 || n1 <= 0 || !out || !out_len) return C3_E_ARG;
  *out_len = 0;
  if (h->n_spl <= 0) { const char sp[] = "ACGT"; int64_t o[2] = {0, 4}; int rc = c3_set_splints(h, 1, sp, o); if (rc) return rc; }
  std::string seq(d0, n0), ql;
  seq.append(d1, n1);
  if (q0) ql.append(q0, n0); else ql.append(n0, 'I');
  if (q1) ql.append(q1, n1); else ql.append(n1, 'I');
  int64_t off[2] = {0, (int64_t)seq.size()};
  int16_t sid = 0; char st = '+';
  int rc = c3_batch_upload(h, 1, seq.data(), ql.data(), off, &sid, &st);
  if (rc) return rc;
  c3_read_result r; memset(&r, 0, sizeof(r));
  r.status = C3_ST_NO_CONSENSUS; r.n_peaks = 1; r.has_front = 1; r.has_tail = 1; r.front_end = n0; r.tail_beg = n0;
  HIPCHK(hipMemcpy(h->d_info.p, &r, sizeof(r), hipMemcpyHostToDevice));
  const int md0 = h->cfg.mdistcutoff, z0 = h->cfg.zero;
  h->cfg.mdistcutoff = min_len; h->cfg.zero = 1;
  rc = c3_batch_run(h, C3_STAGE_POA | C3_STAGE_POLISH);
  h->cfg.mdistcutoff = md0; h->cfg.zero = z0;
  if (rc) return rc;
  std::vector<c3_read_result> res(1);
  int64_t co[2];
  rc = c3_batch_results(h, res.data(), out, cap, co);
  if (rc) return rc;
  *out_len = (res[0].status == C3_ST_OK) ? res[0].cons_len : 0;
  return C3_E_OK;
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
  std::vector<c3_read_result> res(1);
  int64_t co[2];
  rc = c3_batch_results(h, res.data(), out, cap, co);
  if (rc) return rc;
  *out_len = (res[0].status == C3_ST_OK) ? res[0].cons_len : 0;
  return C3_E_OK;
}

// ---- BGZF output (k_bgzf.hip; host statement c3_bgzf.cpp) ---------------------------------
// Input goes to the device in chunks of BGZF_CHUNK_BLOCKS blocks: copy in (the pieces land back to back), k_bgzf + k_bgzf_pack,
// the member sizes back, then one copy of the packed members straight into the caller's buffer.
#define BGZF_CHUNK_BLOCKS 2048
struct c3_bgzf {
  int device = 0; hipStream_t stream = nullptr; int* h_sizes = nullptr;
  DBuf d_in, d_slots, d_sizes, d_packed;
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
  hipStream_t copy_stream = nullptr;
};

extern "C" int c3_bgzf_create(int device, c3_bgzf** out) {
  if (!out) return C3_E_ARG;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); g_create_err = "no HIP device: the c3poa HIP backend has no CPU fallback"; return C3_E_NO_DEVICE; }
  if (device < 0 || device >= ndev) { g_create_err = "bad device ordinal"; return C3_E_ARG; }
  c3_bgzf* z = new c3_bgzf();
  z->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&z->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipHostMalloc((void**)&z->h_sizes, BGZF_CHUNK_BLOCKS * sizeof(int), hipHostMallocDefault);
  if (e != hipSuccess) { g_create_err = hipGetErrorString(e); c3_bgzf_destroy(z); return C3_E_HIP; }
  *out = z;
  return C3_E_OK;
}

extern "C" void c3_bgzf_destroy(c3_bgzf* z) {
  if (!z) return;
  (void)hipSetDevice(z->device);
  if (z->stream) { (void)hipStreamSynchronize(z->stream); (void)hipStreamDestroy(z->stream); }
  if (z->h_sizes) (void)hipHostFree(z->h_sizes);
  if (z->h_mem) (void)hipHostFree(z->h_mem);
  if (z->h_res) (void)hipHostFree(z->h_res);
  if (z->copy_stream) { (void)hipStreamSynchronize(z->copy_stream); (void)hipStreamDestroy(z->copy_stream); }
  if (z->h_hdr) (void)hipHostFree(z->h_hdr);
  for (auto& f : z->fq) { if (f.h_off) (void)hipHostFree(f.h_off); if (f.h_name_off) (void)hipHostFree(f.h_name_off); }
  delete z;
}

static int bgzf_fail(hipError_t e, const char* what) {
  char buf[256];
  snprintf(buf, sizeof buf, "HIP error %d (%s): %s", (int)e, hipGetErrorString(e), what);
  g_create_err = buf;
  return C3_E_HIP;
}

// the concatenation of pieces p[0..np) compressed as one text (the writers' formatter slices, c3_io.cpp)
extern "C" int c3_bgzf_compress_pieces(c3_bgzf* z, const char* const* p, const int64_t* len, int np, char* dst, int64_t cap, int64_t* out_len) {
  if (!z || !out_len || np < 0 || (np > 0 && (!p || !len))) { g_create_err = "c3_bgzf_compress: bad arguments"; return C3_E_ARG; }
  int64_t n = 0;
  for (int i = 0; i < np; ++i) { if (len[i] < 0 || (len[i] > 0 && !p[i])) { g_create_err = "c3_bgzf_compress: bad piece"; return C3_E_ARG; } n += len[i]; }
  if (cap < c3_bgzf_bound(n) || (n > 0 && !dst)) { g_create_err = "c3_bgzf_compress: cap < c3_bgzf_bound(n)"; return C3_E_ARG; }
  *out_len = 0;
  if (n == 0) return C3_E_OK;
  hipError_t e = hipSetDevice(z->device);
  if (e != hipSuccess) return bgzf_fail(e, "hipSetDevice");
  const int64_t CH = (int64_t)BGZF_CHUNK_BLOCKS * BGZF_BLOCK;
  const int64_t first = std::min(CH, n);
  const int nb_max = (int)((first + BGZF_BLOCK - 1) / BGZF_BLOCK);
  // k_bgzf reads up to 8 bytes past a chunk's end (realigned dword loads): the input buffer has 256 bytes of slack
  if ((e = z->d_in.ensure((size_t)first + 256)) != hipSuccess) return bgzf_fail(e, "input buffer");
  if ((e = z->d_slots.ensure((size_t)nb_max * BGZF_SLOT)) != hipSuccess) return bgzf_fail(e, "slots");
  if ((e = z->d_sizes.ensure((size_t)nb_max * sizeof(int))) != hipSuccess) return bgzf_fail(e, "sizes");
  if ((e = z->d_packed.ensure((size_t)nb_max * BGZF_MAX_MEMBER)) != hipSuccess) return bgzf_fail(e, "packed members");
  int64_t o = 0;
  int pi = 0; int64_t pin = 0;                                  // piece index / bytes of it already sent
  for (int64_t c0 = 0; c0 < n; c0 += CH) {
    const int64_t cn = std::min(CH, n - c0);
    const int nb = (int)((cn + BGZF_BLOCK - 1) / BGZF_BLOCK);
    int64_t at = 0;
    while (at < cn) {
      while (pi < np && pin == len[pi]) { ++pi; pin = 0; }
      const int64_t k = std::min(len[pi] - pin, cn - at);
      e = hipMemcpyAsync(z->d_in.as<char>() + at, p[pi] + pin, (size_t)k, hipMemcpyHostToDevice, z->stream);
      if (e != hipSuccess) return bgzf_fail(e, "copy in");
      at += k; pin += k;
    }
    c3k_launch_bgzf(z->d_in.as<uint8_t>(), (long long)cn, nb, z->d_slots.as<uint8_t>(), z->d_sizes.as<int>(), z->d_packed.as<uint8_t>(), z->stream);
    if ((e = hipGetLastError()) != hipSuccess) return bgzf_fail(e, "k_bgzf launch");
    e = hipMemcpyAsync(z->h_sizes, z->d_sizes.p, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, z->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
    if (e != hipSuccess) return bgzf_fail(e, "k_bgzf");
    int64_t tot = 0;
    for (int b = 0; b < nb; ++b) {
      const int s = z->h_sizes[b];
      if (s < BGZF_HDR + 13 || s > BGZF_MAX_MEMBER) { g_create_err = "k_bgzf: member size out of range"; return C3_E_HIP; }
      tot += s;
    }
    e = hipMemcpyAsync(dst + o, z->d_packed.p, (size_t)tot, hipMemcpyDeviceToHost, z->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
    if (e != hipSuccess) return bgzf_fail(e, "copy out");
    o += tot;
  }
  *out_len = o;
  return C3_E_OK;
}

extern "C" int c3_bgzf_compress(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!z || !out_len || n < 0 || (n > 0 && !src)) { g_create_err = "c3_bgzf_compress: bad arguments"; return C3_E_ARG; }
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
int c3_bgzf_data_error(const char* who, int64_t member, int st);      // c3_inflate.cpp

// nm members of src (all accepted by c3_bgzf_scan) inflated into the caller's dst, or -- d_dst != null -- left on the device
// at d_dst (the reader's device parse); either way every member's CRC is compared here before the call returns
static int bgzf_inflate_members(c3_bgzf* z, const char* src, int64_t n, int64_t nm, uint8_t* d_dst, char* dst, int64_t* out_len) {
  hipError_t e = hipSetDevice(z->device);
  if (e != hipSuccess) return bgzf_fail(e, "hipSetDevice");
  const int CH = inflate_chunk();
  if (!z->h_mem) e = hipHostMalloc((void**)&z->h_mem, CH * sizeof(C3BgzfMember), hipHostMallocDefault);
  if (e == hipSuccess && !z->h_res) e = hipHostMalloc((void**)&z->h_res, CH * sizeof(int2), hipHostMallocDefault);
  if (e != hipSuccess) return bgzf_fail(e, "descriptor buffers");
  if ((e = z->d_mem.ensure(CH * sizeof(C3BgzfMember))) != hipSuccess) return bgzf_fail(e, "descriptors");
  if ((e = z->d_res.ensure(CH * sizeof(int2))) != hipSuccess) return bgzf_fail(e, "statuses");
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
    if ((e = z->d_in.ensure((size_t)cn + 256)) != hipSuccess) return bgzf_fail(e, "input buffer");
    if (!d_dst && (e = z->d_out.ensure((size_t)oo + 256)) != hipSuccess) return bgzf_fail(e, "output buffer");
    e = hipMemcpyAsync(z->d_in.p, src + c0, (size_t)cn, hipMemcpyHostToDevice, z->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(z->d_mem.p, z->h_mem, (size_t)k * sizeof(C3BgzfMember), hipMemcpyHostToDevice, z->stream);
    if (e != hipSuccess) return bgzf_fail(e, "copy in");
    c3k_launch_inflate(z->d_in.as<uint8_t>(), z->d_mem.as<C3BgzfMember>(), k, d_dst ? d_dst + o : z->d_out.as<uint8_t>(), z->d_res.as<int2>(), z->stream);
    if ((e = hipGetLastError()) != hipSuccess) return bgzf_fail(e, "k_inflate launch");
    e = hipMemcpyAsync(z->h_res, z->d_res.p, (size_t)k * sizeof(int2), hipMemcpyDeviceToHost, z->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
    if (e != hipSuccess) return bgzf_fail(e, "k_inflate");
    for (int i = 0; i < k; ++i) {
      int st = z->h_res[i].x;
      if (st == C3_INF_OK && (uint32_t)z->h_res[i].y != z->h_mem[i].crc) st = C3_INF_CRC;
      if (st != C3_INF_OK) return c3_bgzf_data_error("c3_bgzf_decompress", done + i, st);
    }
    if (oo && !d_dst) {
      e = hipMemcpyAsync(dst + o, z->d_out.p, (size_t)oo, hipMemcpyDeviceToHost, z->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
      if (e != hipSuccess) return bgzf_fail(e, "copy out");
    }
    o += oo; done += k;
  }
  *out_len = o;
  return C3_E_OK;
}

extern "C" int c3_bgzf_decompress(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len) {
  if (!z || !out_len || n < 0 || (n > 0 && !src)) { g_create_err = "c3_bgzf_decompress: bad arguments"; return C3_E_ARG; }
  *out_len = 0;
  int64_t nm = 0, ob = 0;
  const int rc = c3_bgzf_scan(src, n, &nm, &ob);
  if (rc) return rc;
  if (cap < ob || (ob > 0 && !dst)) { g_create_err = "c3_bgzf_decompress: cap < inflated size (c3_bgzf_scan)"; return C3_E_ARG; }
  if (nm == 0) return C3_E_OK;
  return bgzf_inflate_members(z, src, n, nm, nullptr, dst, out_len);
}

// ---- FASTQ records on the GPU (k_fastq.hip; host statement c3_fastq.cpp) -------------------
// One parse = three waits: the line count (sizes nl[] and the record tables), the header (sizes the outputs, answers the
// capacity question before any byte is gathered), the finished arrays.
int c3_fastq_check_args(const char* who, const char* text, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                        const char* seqs, const char* quals, int64_t bases_cap, const int64_t* off, int64_t max_records,
                        c3_fastq_info* info);                         // c3_fastq.cpp

static int fq_prepare(c3_bgzf* z) {
  hipError_t e = hipSetDevice(z->device);
  if (e != hipSuccess) return bgzf_fail(e, "hipSetDevice");
  if (!z->h_hdr) e = hipHostMalloc((void**)&z->h_hdr, sizeof(C3FqHdr), hipHostMallocDefault);
  if (e == hipSuccess && !z->copy_stream) e = hipStreamCreateWithFlags(&z->copy_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = z->d_hdr.ensure(sizeof(C3FqHdr));
  if (e != hipSuccess) return bgzf_fail(e, "k_fastq buffers");
  return C3_E_OK;
}

// the text [lo, lo + n) of sl.text parsed: tables and header on the device, *info filled; no byte gathered yet
static int fq_parse_device(c3_bgzf* z, c3_bgzf::FqSlot& sl, uint32_t lo, int64_t n, int at_eof, int min_len, c3_fastq_info* info) {
  memset(info, 0, sizeof *info);
  sl.n_rec = 0;
  if (n == 0) return C3_E_OK;
  hipError_t e;
  const uint32_t hi = lo + (uint32_t)n;
  const size_t tiles = ((size_t)hi + 65535) / 65536;
  const uint8_t* buf = sl.text.as<uint8_t>();
  C3FqHdr* hdr = z->d_hdr.as<C3FqHdr>();
  if ((e = z->d_cnt.ensure(tiles * 4 * sizeof(int32_t))) != hipSuccess) return bgzf_fail(e, "k_fastq counts");
  c3k_launch_fastq_count(buf, lo, hi, z->d_cnt.as<int32_t>(), at_eof, hdr, z->stream);
  if ((e = hipGetLastError()) != hipSuccess) return bgzf_fail(e, "k_fastq_count launch");
  e = hipMemcpyAsync(z->h_hdr, hdr, sizeof(C3FqHdr), hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
  if (e != hipSuccess) return bgzf_fail(e, "k_fastq_count");
  const int L = z->h_hdr->n_lines, Lv = z->h_hdr->n_lines_v;
  if (L < 0 || (int64_t)L > n || Lv < L || Lv > L + 1) { g_create_err = "k_fastq: line count out of range"; return C3_E_HIP; }
  const int n_full = Lv / 4, partial = (at_eof && (Lv & 3)) ? 1 : 0;
  if (n_full == 0 && !partial) return C3_E_OK;                        // no whole record yet: everything stays unconsumed
  const size_t nr = (size_t)n_full + 1, nb = ((size_t)n_full + 255) / 256;
  if ((e = z->d_nl.ensure(((size_t)L + 4) * sizeof(int32_t))) != hipSuccess) return bgzf_fail(e, "k_fastq lines");
  if ((e = z->d_slen.ensure(nr * sizeof(int32_t))) != hipSuccess) return bgzf_fail(e, "k_fastq records");
  if ((e = z->d_nlen.ensure(nr * sizeof(int32_t))) != hipSuccess) return bgzf_fail(e, "k_fastq records");
  if ((e = z->d_bsum.ensure((nb + 1) * 3 * sizeof(long long))) != hipSuccess) return bgzf_fail(e, "k_fastq sums");
  if ((e = sl.off.ensure(nr * sizeof(int64_t))) != hipSuccess) return bgzf_fail(e, "k_fastq offsets");
  if ((e = sl.name_off.ensure(nr * sizeof(int64_t))) != hipSuccess) return bgzf_fail(e, "k_fastq offsets");
  if ((e = sl.src.ensure(nr * sizeof(int4))) != hipSuccess) return bgzf_fail(e, "k_fastq sources");
  c3k_launch_fastq_lines(buf, lo, hi, z->d_cnt.as<int32_t>(), z->d_nl.as<int32_t>(), z->stream);
  c3k_launch_fastq_records(buf, lo, hi, z->d_nl.as<int32_t>(), L, n_full, partial, min_len, z->d_slen.as<int32_t>(), z->d_nlen.as<int32_t>(),
                           z->d_bsum.as<long long>(), hdr, sl.off.as<int64_t>(), sl.name_off.as<int64_t>(), sl.src.as<int4>(), z->stream);
  if ((e = hipGetLastError()) != hipSuccess) return bgzf_fail(e, "k_fastq_records launch");
  e = hipMemcpyAsync(z->h_hdr, hdr, sizeof(C3FqHdr), hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
  if (e != hipSuccess) return bgzf_fail(e, "k_fastq_records");
  const C3FqHdr& h = *z->h_hdr;
  if (h.n_records < 0 || h.n_records > n_full || h.n_kept < 0 || h.n_kept > h.n_records || h.consumed < 0 || h.consumed > n ||
      h.base_bytes < 0 || h.base_bytes > n || h.name_bytes < 0 || h.name_bytes > n) { g_create_err = "k_fastq: header out of range"; return C3_E_HIP; }
  info->n_records = h.n_records; info->n_kept = h.n_kept; info->n_short = h.n_short; info->consumed = h.consumed;
  info->name_bytes = h.name_bytes; info->base_bytes = h.base_bytes; info->departed = h.departed;
  sl.n_rec = h.n_kept;
  return C3_E_OK;
}

// the kept records of the parse that fq_parse_device just made, gathered into sl.names / sl.seqs / sl.quals (queued, not waited for)
static int fq_gather_device(c3_bgzf* z, c3_bgzf::FqSlot& sl, const c3_fastq_info& info) {
  if (info.n_kept == 0) return C3_E_OK;
  hipError_t e;
  if ((e = sl.names.ensure((size_t)info.name_bytes + 256)) != hipSuccess) return bgzf_fail(e, "k_fastq names");
  if ((e = sl.seqs.ensure((size_t)info.base_bytes + 256)) != hipSuccess) return bgzf_fail(e, "k_fastq bases");
  if ((e = sl.quals.ensure((size_t)info.base_bytes + 256)) != hipSuccess) return bgzf_fail(e, "k_fastq qualities");
  c3k_launch_fastq_gather(sl.text.as<uint8_t>(), sl.src.as<int4>(), sl.off.as<int64_t>(), sl.name_off.as<int64_t>(), (long long)info.n_kept,
                          sl.names.as<uint8_t>(), sl.seqs.as<uint8_t>(), sl.quals.as<uint8_t>(), z->stream);
  if ((e = hipGetLastError()) != hipSuccess) return bgzf_fail(e, "k_fastq_gather launch");
  return C3_E_OK;
}

extern "C" int c3_fastq_parse(c3_bgzf* z, const char* text, int64_t n, int at_eof, int min_len, char* names, int64_t names_cap,
                              int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off, int64_t max_records,
                              c3_fastq_info* info) {
  int rc = c3_fastq_check_args("c3_fastq_parse", text, n, names, names_cap, name_off, seqs, quals, bases_cap, off, max_records, info);
  if (rc) return rc;
  if (!z) { g_create_err = "c3_fastq_parse: null handle"; return C3_E_ARG; }
  if (n == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  if ((rc = fq_prepare(z)) != C3_E_OK) return rc;
  c3_bgzf::FqSlot& sl = z->fq[0];
  const uint32_t lo = (uint32_t)((uintptr_t)text & 3u);               // the text keeps its place inside a dword: the kernels see the caller's misalignment
  hipError_t e;
  if ((e = sl.text.ensure((size_t)lo + (size_t)n + 256)) != hipSuccess) return bgzf_fail(e, "k_fastq text");
  e = hipMemcpyAsync(sl.text.as<char>() + lo, text, (size_t)n, hipMemcpyHostToDevice, z->stream);
  if (e != hipSuccess) return bgzf_fail(e, "copy in");
  if ((rc = fq_parse_device(z, sl, lo, n, at_eof, min_len, info)) != C3_E_OK) return rc;
  if (info->n_kept > max_records || info->name_bytes > names_cap || info->base_bytes > bases_cap) {
    g_create_err = "c3_fastq_parse: capacity too small (needed sizes in info)";
    return C3_E_LIMIT;
  }
  if (info->n_kept == 0) { name_off[0] = 0; off[0] = 0; return C3_E_OK; }
  if ((rc = fq_gather_device(z, sl, *info)) != C3_E_OK) return rc;
  const size_t nt = ((size_t)info->n_kept + 1) * sizeof(int64_t);
  e = hipMemcpyAsync(off, sl.off.p, nt, hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(name_off, sl.name_off.p, nt, hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess && info->name_bytes) e = hipMemcpyAsync(names, sl.names.p, (size_t)info->name_bytes, hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess && info->base_bytes) e = hipMemcpyAsync(seqs, sl.seqs.p, (size_t)info->base_bytes, hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess && info->base_bytes) e = hipMemcpyAsync(quals, sl.quals.p, (size_t)info->base_bytes, hipMemcpyDeviceToHost, z->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
  if (e != hipSuccess) return bgzf_fail(e, "k_fastq_gather");
  return C3_E_OK;
}

// ---- the reader's device stretches (c3_io.cpp; not part of the public interface) ----------
// Stretch = `carry_len` bytes of the other slot's text from `carry_from` on (the record its end cut), then the inflated
// members of comp; it stays on the device, is parsed there with min_len 0 (the group rule, min_len included, is the
// reader's), and the record tables come back.  On return the slot holds the finished records until it is loaded again.
struct c3_fq_stretch { c3_fastq_info info; const int64_t* off; const int64_t* name_off; int64_t text_bytes; };

extern "C" int c3_bgzf_stretch_parse(c3_bgzf* z, int slot, const char* comp, int64_t ncomp, int64_t carry_from, int64_t carry_len,
                                     int at_eof, c3_fq_stretch* out) {
  if (!z || !out || slot < 0 || slot > 1 || ncomp < 0 || (ncomp > 0 && !comp) || carry_len < 0) { g_create_err = "c3_bgzf_stretch_parse: bad arguments"; return C3_E_ARG; }
  memset(out, 0, sizeof *out);
  int64_t nm = 0, ob = 0;
  int rc = c3_bgzf_scan(comp, ncomp, &nm, &ob);
  if (rc) return rc;
  const int64_t total = carry_len + ob;
  if (total > C3_FASTQ_MAX_TEXT) { g_create_err = "c3_bgzf_stretch_parse: stretch longer than C3_FASTQ_MAX_TEXT"; return C3_E_LIMIT; }
  if ((rc = fq_prepare(z)) != C3_E_OK) return rc;
  c3_bgzf::FqSlot& sl = z->fq[slot];
  const c3_bgzf::FqSlot& other = z->fq[slot ^ 1];
  if (carry_len > 0 && (carry_from < 0 || carry_from + carry_len > other.text_n)) { g_create_err = "c3_bgzf_stretch_parse: carry outside the other stretch"; return C3_E_ARG; }
  hipError_t e;
  if ((e = sl.text.ensure((size_t)total + 256)) != hipSuccess) return bgzf_fail(e, "stretch text");
  sl.text_n = 0;
  if (carry_len > 0) {
    e = hipMemcpyAsync(sl.text.p, other.text.as<char>() + carry_from, (size_t)carry_len, hipMemcpyDeviceToDevice, z->stream);
    if (e != hipSuccess) return bgzf_fail(e, "carry");
  }
  if (nm > 0) {
    int64_t got = 0;
    rc = bgzf_inflate_members(z, comp, ncomp, nm, sl.text.as<uint8_t>() + carry_len, nullptr, &got);
    if (rc) return rc;
    if (got != ob) { g_create_err = "c3_bgzf_stretch_parse: inflated size differs from the headers"; return C3_E_DATA; }
  }
  sl.text_n = total;
  out->text_bytes = total;
  if ((rc = fq_parse_device(z, sl, 0, total, at_eof, 0, &out->info)) != C3_E_OK) return rc;
  const int64_t nk = out->info.n_kept;
  if (nk > 0) {
    if ((rc = fq_gather_device(z, sl, out->info)) != C3_E_OK) return rc;
    if (sl.h_cap < (size_t)nk + 1) {
      if (sl.h_off) (void)hipHostFree(sl.h_off);
      if (sl.h_name_off) (void)hipHostFree(sl.h_name_off);
      sl.h_off = sl.h_name_off = nullptr; sl.h_cap = 0;
      const size_t want = (size_t)nk + 1 + (size_t)nk / 8 + 1024;
      e = hipHostMalloc((void**)&sl.h_off, want * sizeof(int64_t), hipHostMallocDefault);
      if (e == hipSuccess) e = hipHostMalloc((void**)&sl.h_name_off, want * sizeof(int64_t), hipHostMallocDefault);
      if (e != hipSuccess) return bgzf_fail(e, "stretch tables");
      sl.h_cap = want;
    }
    e = hipMemcpyAsync(sl.h_off, sl.off.p, ((size_t)nk + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, z->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sl.h_name_off, sl.name_off.p, ((size_t)nk + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, z->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(z->stream);
    if (e != hipSuccess) return bgzf_fail(e, "k_fastq_gather");
    if (sl.h_off[0] != 0 || sl.h_name_off[0] != 0 || sl.h_off[nk] != out->info.base_bytes || sl.h_name_off[nk] != out->info.name_bytes) {
      g_create_err = "k_fastq: offsets do not match the header"; return C3_E_HIP;
    }
    out->off = sl.h_off; out->name_off = sl.h_name_off;
  }
  return C3_E_OK;
}

// records [r0, r1) of the slot's stretch copied to the host (names / seqs / quals point at the place of record r0; seqs and
// quals may be null: names only).  Runs on copy_stream: the other slot may be being loaded on another thread meanwhile.
extern "C" int c3_bgzf_stretch_fetch(c3_bgzf* z, int slot, int64_t r0, int64_t r1, char* names, char* seqs, char* quals) {
  if (!z || slot < 0 || slot > 1 || !names) { g_create_err = "c3_bgzf_stretch_fetch: bad arguments"; return C3_E_ARG; }
  const c3_bgzf::FqSlot& sl = z->fq[slot];
  if (r0 < 0 || r1 < r0 || r1 > sl.n_rec) { g_create_err = "c3_bgzf_stretch_fetch: records outside the stretch"; return C3_E_ARG; }
  if (r0 == r1) return C3_E_OK;
  hipError_t e = hipSetDevice(z->device);
  if (e != hipSuccess) return bgzf_fail(e, "hipSetDevice");
  const int64_t nb = sl.h_name_off[r0], ne = sl.h_name_off[r1], sb = sl.h_off[r0], se = sl.h_off[r1];
  if (ne > nb) e = hipMemcpyAsync(names, sl.names.as<char>() + nb, (size_t)(ne - nb), hipMemcpyDeviceToHost, z->copy_stream);
  if (e == hipSuccess && seqs && se > sb) e = hipMemcpyAsync(seqs, sl.seqs.as<char>() + sb, (size_t)(se - sb), hipMemcpyDeviceToHost, z->copy_stream);
  if (e == hipSuccess && quals && se > sb) e = hipMemcpyAsync(quals, sl.quals.as<char>() + sb, (size_t)(se - sb), hipMemcpyDeviceToHost, z->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(z->copy_stream);
  if (e != hipSuccess) return bgzf_fail(e, "stretch fetch");
  return C3_E_OK;
}

// text [from, from + len) of the slot's stretch copied to the host (a departure: the host parser takes over from there)
extern "C" int c3_bgzf_stretch_text(c3_bgzf* z, int slot, int64_t from, int64_t len, char* dst) {
  if (!z || slot < 0 || slot > 1 || from < 0 || len < 0 || (len > 0 && !dst)) { g_create_err = "c3_bgzf_stretch_text: bad arguments"; return C3_E_ARG; }
  const c3_bgzf::FqSlot& sl = z->fq[slot];
  if (from + len > sl.text_n) { g_create_err = "c3_bgzf_stretch_text: bytes outside the stretch"; return C3_E_ARG; }
  if (len == 0) return C3_E_OK;
  hipError_t e = hipSetDevice(z->device);
  if (e == hipSuccess) e = hipMemcpyAsync(dst, sl.text.as<char>() + from, (size_t)len, hipMemcpyDeviceToHost, z->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(z->copy_stream);
  if (e != hipSuccess) return bgzf_fail(e, "stretch text");
  return C3_E_OK;
}

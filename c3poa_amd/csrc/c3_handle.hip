// c3_handle.hip -- the batch handle of the C ABI (include/c3poa.h): create / destroy, splints, staging and commit of a batch,
// results and formatted records (snapshot + fetch), probes.  The stages themselves are c3_stages.hip.
// No CPU fallback exists in this library: without a gfx950 device c3_create fails.
#include "c3_host.h"
#include "c3_bgzf.h"

thread_local double c3h::g_alloc_ms = 0.0;      // (DBuf::ensure adds to it, c3_batch_run reads it)

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
// the 2-bit pack of n reads that lie on the device (c3_batch_stage; the text path of the post-processing step, c3_text.hip)
extern "C" void c3k_launch_pack(const uint8_t* ascii, const int64_t* off, const int64_t* woff, int n, uint32_t* pk, int grid, hipStream_t s) {
  hipLaunchKernelGGL(k_pack, dim3((unsigned)grid), dim3(256), 0, s, ascii, off, woff, n, pk);
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

// POA scoring k_poa's 16-bit cells hold exactly or hand to the 32-bit pass (DESIGN.md 4.3 derives every bound from the constants
// of k_poa.hip).  Pure arithmetic on the configuration: checked before a device is looked for.
static int check_poa_scoring(const c3_config* cfg) {
  const struct { const char* name; int v, lo, hi; } f[6] = {
    {"poa_match", cfg->poa_match, 1, 64}, {"poa_mismatch", cfg->poa_mismatch, 0, 64},
    {"poa_o1", cfg->poa_o1, 0, 64}, {"poa_e1", cfg->poa_e1, 0, 16}, {"poa_o2", cfg->poa_o2, 0, 64}, {"poa_e2", cfg->poa_e2, 0, 16}};
  for (const auto& x : f) {
    if (x.v < x.lo || x.v > x.hi) {
      char buf[160];
      snprintf(buf, sizeof buf, "%s = %d: must be %d..%d (the 16-bit cells of k_poa and their guard are exact in that range only)", x.name, x.v, x.lo, x.hi);
      return host_fail(C3_E_ARG, buf);
    }
  }
  return C3_E_OK;
}

// Polish scoring the 32-bit rows of k_window and k_prep hold exactly (DESIGN.md 4.6a derives the bound from the constants of
// k_polish.hip; the 16-bit rows guard themselves per layer, the pieces and layers of a batch are checked against the scoring in
// run_polish).  Every sign is admitted, one relation is not.  Pure arithmetic on the configuration: checked before a device is
// looked for.
static int check_pol_scoring(const c3_config* cfg) {
  const struct { const char* name; int v; } f[3] = {{"pol_match", cfg->pol_match}, {"pol_mismatch", cfg->pol_mismatch}, {"pol_gap", cfg->pol_gap}};
  for (const auto& x : f) {
    if (x.v < -C3_POL_MAX || x.v > C3_POL_MAX) {
      char buf[160];
      snprintf(buf, sizeof buf, "%s = %d: must be %d..%d (the 32-bit cells of the polish rows and their sentinels are exact in that range only)", x.name, x.v, -C3_POL_MAX, C3_POL_MAX);
      return host_fail(C3_E_ARG, buf);
    }
  }
  // a matched pair has to beat two gaps: otherwise no layer aligns to the backbone, every layer adds all its bases as new nodes
  // and no window fits the graph k_window has room for (3 * window + 40 per layer): every read would end as C3_ST_LIMIT
  if (cfg->pol_match <= 2 * cfg->pol_gap) {
    char buf[200];
    snprintf(buf, sizeof buf, "pol_match = %d: must be above 2 * pol_gap = %d (a match that scores no more than two gaps makes every layer a chain of new nodes, beyond the window graph's capacity)",
             cfg->pol_match, 2 * cfg->pol_gap);
    return host_fail(C3_E_ARG, buf);
  }
  return C3_E_OK;
}

// Window length and extension band: run_polish divides by pol_window and sizes every capacity of the polish from
// it; beyond C3_POL_WINDOW_MAX the node ids of a window graph leave the 16 bits k_window's consensus keeps them in.  A negative
// dang_band is a band of negative width.  Pure arithmetic on the configuration: checked before a device is looked for.
static int check_pol_window(const c3_config* cfg) {
  char buf[200];
  if (cfg->pol_window < 1 || cfg->pol_window > C3_POL_WINDOW_MAX) {
    snprintf(buf, sizeof buf, "pol_window = %d: must be %d..%d (a window graph of 3 * pol_window + 40 nodes per layer has to stay below the 65535 node ids k_window's consensus holds)",
             cfg->pol_window, 1, C3_POL_WINDOW_MAX);
    return host_fail(C3_E_ARG, buf);
  }
  if (cfg->dang_band < 0) {
    snprintf(buf, sizeof buf, "dang_band = %d: must be %d..%d (the half width of the extension band; 0 is the diagonal alone)", cfg->dang_band, 0, 255);
    return host_fail(C3_E_ARG, buf);
  }
  return C3_E_OK;
}

extern "C" int c3_create(const c3_config* cfg, c3_handle** out) {
  if (!cfg || !out) return C3_E_ARG;
  *out = nullptr;
  if (int rc = check_poa_scoring(cfg)) return rc;
  if (int rc = check_pol_scoring(cfg)) return rc;
  if (int rc = check_pol_window(cfg)) return rc;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) return host_fail(C3_E_NO_DEVICE, "no HIP device: the c3poa HIP backend has no CPU fallback");
  if (cfg->device < 0 || cfg->device >= ndev) return host_fail(C3_E_ARG, "bad device ordinal");
  if (cfg->conk_match < -127 || cfg->conk_match > 127 || cfg->conk_mismatch < -127 || cfg->conk_mismatch > 127) {
    return host_fail(C3_E_ARG, "conk_match / conk_mismatch must fit a signed byte");                 // k_conk keeps them in byte tables
  }
  if (cfg->dang_band > 255) return host_fail(C3_E_LIMIT, "dang_band must be at most 255 (k_prep holds 512 band offsets per wave)");
  if (cfg->sg_order != 2 && cfg->sg_order != 3) return host_fail(C3_E_ARG, "sg_order must be 2 or 3");
  if (cfg->sg_window < 5 || cfg->sg_window > 127 || !(cfg->sg_window & 1)) return host_fail(C3_E_ARG, "sg_window must be odd, 5..127");
  if (cfg->zero_max_cells < 1 || cfg->zero_max_cells > INT32_MAX) return host_fail(C3_E_ARG, "zero_max_cells must be 1..2147483647");
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
  if (e != hipSuccess) { c3_destroy(h); return host_fail(C3_E_HIP, hipGetErrorString(e)); }
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
  for (hipEvent_t ev : {h->ev_dn, h->ev_up[0], h->ev_up[1], h->ev_qv[0], h->ev_qv[1], h->ev_pair[0], h->ev_pair[1]}) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : h->ev) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : h->ev_post) if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : h->ev_fa) if (ev) (void)hipEventDestroy(ev);
  for (c3h::EmitBufs* eb : {&h->emit_sa, &h->emit_snap}) for (hipEvent_t ev : eb->ev) if (ev) (void)hipEventDestroy(ev);
  if (h->ev_emit_dn) (void)hipEventDestroy(h->ev_emit_dn);
  if (h->h_fa_hdr) (void)hipHostFree(h->h_fa_hdr);
  c3h::post_text_free(h);
  c3h::demux_text_free(h);
  if (h->h_tot) (void)hipHostFree(h->h_tot);
  delete h;
}

extern "C" int c3_set_splints(c3_handle* h, int n, const char* cat, const int64_t* off) {
  if (!h || n <= 0 || !cat || !off) return C3_E_ARG;
  HIPCHK(hipSetDevice(h->cfg.device));
  std::vector<uint8_t> codes((size_t)n * 2 * C3_SPLINT_MAX, 0);
  // a refused table changes nothing: sp_len / max_spl size the scratch of the scans that run against the table on the device
  std::vector<int> sp_len((size_t)n, 0); int max_spl = 0;
  for (int i = 0; i < n; ++i) {
    int S = (int)(off[i + 1] - off[i]);
    if (S <= 0 || S > C3_SPLINT_MAX) return c3_fail(h, C3_E_LIMIT, "splint length must be 1..512");
    // a cell grows by the larger of the two substitution scores per splint row, whichever of them it is
    if ((long long)std::max({h->cfg.conk_match, h->cfg.conk_mismatch, 0}) * S > 32000 || h->cfg.conk_penalty < 0 || h->cfg.conk_penalty > 32000)
      return c3_fail(h, C3_E_LIMIT, "max(conk_match, conk_mismatch) * splint length and conk_penalty must stay within 32000 (16-bit score cells in k_conk)");
    sp_len[(size_t)i] = S; max_spl = std::max(max_spl, S);
    for (int k = 0; k < S; ++k) {
      int c = code_of(cat[off[i] + k]);
      codes[((size_t)i * 2 + 0) * C3_SPLINT_MAX + k] = (uint8_t)c;
      codes[((size_t)i * 2 + 1) * C3_SPLINT_MAX + (S - 1 - k)] = (uint8_t)(3 - c);   // reverse complement (C3POa.py:234)
    }
  }
  HIPCHK(h->d_sp_codes.put(codes.data(), codes.size(), h->stream));
  HIPCHK(h->d_sp_len.put(sp_len.data(), sizeof(int) * n, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->sp_len.swap(sp_len); h->max_spl = max_spl; h->n_spl = n;
  return C3_E_OK;
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
  c3k_launch_pack(t.d_ascii.as<uint8_t>(), t.d_off.as<int64_t>(), t.d_woff.as<int64_t>(), n, t.d_pk.as<uint32_t>(), std::min((n + 3) / 4, h->n_cus * 32), su);
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
  // gather on the device (one wave per read): the fetch is then ONE device->host copy of the compact bytes
  auto gather = [&](const DBuf& arena, DBuf& out) {
    const hipError_t e = out.ensure((size_t)tot + 64);
    if (e == hipSuccess) hipLaunchKernelGGL(k_gather_cons, dim3((unsigned)std::min((n + 3) / 4, h->n_cus * 32)), dim3(256), 0, h->stream,
                                            arena.as<char>(), h->d_off.as<int64_t>(), d_coff.as<int64_t>(), n, out.as<char>());
    return e;
  };
  if (have_cons && tot > 0) HIPCHK(gather(h->d_cons, d_out));
  const bool have_qv = have_cons && (h->stages_done & C3_STAGE_QV) != 0;
  if (have_qv && tot > 0) HIPCHK(gather(h->d_qv, h->d_gather_qv));      // the QV bytes, gathered at the same offsets
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

// snapshot + fetch back to back; the fetch's bare codes get their text here, on the owner thread
static int results_now(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv) {
  int rc = c3_batch_results_snapshot(h);
  if (rc) return rc;
  rc = results_fetch(h, res, cons, cons_cap, cons_off, qv);
  if (rc == C3_E_LIMIT) return c3_fail(h, C3_E_LIMIT, "consensus buffer too small");
  if (rc == C3_E_HIP) return c3_fail(h, C3_E_HIP, "HIP error while copying the results");
  return rc;
}
extern "C" int c3_batch_results_qv(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv) {
  if (!h || h->n <= 0 || !res || !qv) return C3_E_ARG;
  if (!(h->stages_done & C3_STAGE_QV) || !(h->stages_done & C3_STAGE_POLISH)) return c3_fail(h, C3_E_STATE, "the resident batch did not run C3_STAGE_QV");
  return results_now(h, res, cons, cons_cap, cons_off, qv);
}
extern "C" int c3_batch_results(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off) {
  if (!h || h->n <= 0 || !res) return C3_E_ARG;
  return results_now(h, res, cons, cons_cap, cons_off, nullptr);
}

// The records of the resident batch as file bytes, in two halves like the results above (include/c3poa.h "Records formatted on
// the GPU"; the three steps are c3h::emit_run, c3_scans.hip):
//   c3_batch_emit_snapshot  (owner thread, after c3_batch_run) uploads the names -- the only input that is not on the device --
//                           and formats from the resident buffers into the snapshot's own arena: the consensus and QV bytes of
//                           read i lie at d_cons / d_qv + off[i], their length is the record's.  One 8 * (S + 2)-byte read back.
//   c3_batch_emit_fetch     copies the streams out on the download stream; with C3_EMIT_BGZF each stream goes through k_bgzf
//                           first (c3h::bgzf_chunks, c3_stream.hip; the packed members of the last chunks land at the wait that ends the call).
extern "C" int c3_batch_emit_snapshot(c3_handle* h, const char* names, const int64_t* name_off, int zero, int flags) {
  if (!h || h->n <= 0 || !names || !name_off || (flags & ~(C3_EMIT_BGZF | C3_EMIT_BAM))) return C3_E_ARG;
  if (h->emit_pending.load(std::memory_order_acquire)) return c3_fail(h, C3_E_STATE, "c3_batch_emit_snapshot: the previous emit snapshot has not been fetched");
  if (h->n_spl > C3_EMIT_MAX_SPLINTS) return c3_fail(h, C3_E_LIMIT, "c3_batch_emit_snapshot: more than 64 splints");
  const double t_call = dbg_now_ms();
  const int n = h->n;
  if (name_off[0] != 0) return c3_fail(h, C3_E_ARG, "c3_batch_emit_snapshot: name_off must start at 0");
  for (int i = 0; i < n; ++i) if (name_off[i + 1] < name_off[i]) return c3_fail(h, C3_E_ARG, "c3_batch_emit_snapshot: name_off not ascending");
  for (int i = 0; i < n; ++i) if (name_off[i + 1] - name_off[i] >= (1ll << 31)) return c3_fail(h, C3_E_LIMIT, "c3_batch_emit_snapshot: a name of 2^31 bytes or more");
  const int bam = (flags & C3_EMIT_BAM) != 0;
  if (bam) { const int nrc = c3_bamout_check_names("c3_batch_emit_snapshot", names, name_off, n); if (nrc != C3_E_OK) return c3_fail(h, nrc, c3_last_error(nullptr)); }
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->ev_emit_dn) HIPCHK(hipEventCreateWithFlags(&h->ev_emit_dn, hipEventDisableTiming));
  const size_t nmb = (size_t)name_off[n];
  HIPCHK(h->d_emit_names.put(names, nmb, h->stream, 16));
  HIPCHK(h->d_emit_noff.put(name_off, sizeof(int64_t) * (size_t)(n + 1), h->stream));
  const bool have_cons = (h->stages_done & C3_STAGE_POLISH) != 0, have_qv = have_cons && (h->stages_done & C3_STAGE_QV) != 0;
  EmitArgs p; memset(&p, 0, sizeof(p));
  p.n = n; p.n_splints = h->n_spl; p.K = have_qv && !bam ? 3 : 2; p.zero = zero; p.bam = bam;
  p.names = h->d_emit_names.as<uint8_t>(); p.name_off = h->d_emit_noff.as<int64_t>();
  p.seqs = h->d_ascii.as<uint8_t>(); p.quals = h->d_qual.as<uint8_t>(); p.off = h->d_off.as<int64_t>();
  p.info = h->d_info.as<C3Info>(); p.sid = h->d_sid.as<int16_t>();
  p.cons = have_cons ? h->d_cons.as<uint8_t>() : nullptr; p.qv = have_qv ? h->d_qv.as<uint8_t>() : nullptr;
  p.cons_at = h->d_off.as<int64_t>(); p.cons_off = nullptr;
  const int rc = c3h::emit_run(h, p, h->emit_snap, h->stream, h->emit_so, -1);
  if (rc != C3_E_OK) return rc;
  HIPCHK(hipEventRecord(h->ev_emit_dn, h->stream));
  const int SK = p.n_splints * p.K;
  c3_emit_timing& t = h->emit_tm;
  t = c3_emit_timing{};
  HIPCHK(hipEventElapsedTime(&t.ms_len, h->emit_snap.ev[0], h->emit_snap.ev[1]));
  HIPCHK(hipEventElapsedTime(&t.ms_scan, h->emit_snap.ev[1], h->emit_snap.ev[2]));
  t.n_reads = n; t.n_records = h->emit_so[(size_t)SK + 1]; t.in_bytes = (int64_t)nmb + 2 * h->total;
  t.ms_call = (float)(dbg_now_ms() - t_call);
  h->emit_S = SK; h->emit_flags = flags;
  h->emit_pending.store(true, std::memory_order_release);
  return C3_E_OK;
}

extern "C" int c3_batch_emit_fetch(c3_handle* h, char* arena, int64_t cap, int64_t* stream_off) {
  if (!h || !stream_off || cap < 0 || (cap > 0 && !arena)) return C3_E_ARG;
  if (!h->emit_pending.load(std::memory_order_acquire)) return C3_E_STATE;          // (h->err belongs to the owner thread: not touched here)
  const double t_call = dbg_now_ms();
  const int S = h->emit_S;
  const std::vector<int64_t>& so = h->emit_so;
  const bool z = (h->emit_flags & C3_EMIT_BGZF) != 0;
  // capacity first: the plain total, or the sum of the compressed bounds
  int64_t need = 0;
  for (int x = 0; x < S; ++x) { stream_off[x] = need; const int64_t len = so[(size_t)x + 1] - so[(size_t)x]; need += z ? (len ? c3_bgzf_bound(len) : 0) : len; }
  stream_off[S] = need;
  if (need > cap) return C3_E_LIMIT;                                                 // (the snapshot stays: fetch again with a larger arena)
  hipError_t e;
#define DNCHK(x) do { if ((e = (x)) != hipSuccess) { h->emit_pending.store(false, std::memory_order_release); return C3_E_HIP; } } while (0)
  DNCHK(hipSetDevice(h->cfg.device));
  hipStream_t dn = h->stream_dn;
  DNCHK(hipStreamWaitEvent(dn, h->ev_emit_dn, 0));
  const char* src = h->emit_snap.arena.as<char>();
  int64_t out = 0;
  float ms_bgzf = 0.f;
  if (!z) {
    if (need) DNCHK(hipMemcpyAsync(arena, src, (size_t)need, hipMemcpyDeviceToHost, dn));
    out = need;
  } else {
    const double t_z = dbg_now_ms();
    int64_t longest = 0;
    for (int x = 0; x < S; ++x) longest = std::max(longest, so[(size_t)x + 1] - so[(size_t)x]);
    DNCHK(h->emit_zs.reserve(longest));
    for (int x = 0; x < S; ++x) {
      stream_off[x] = out;
      const char* sx = src + so[(size_t)x];
      const c3h::ZStatus st = c3h::bgzf_chunks(h->emit_zs, dn, so[(size_t)x + 1] - so[(size_t)x], [&](char* d_zin, int64_t c0, int64_t cn) {
        return hipMemcpyAsync(d_zin, sx + c0, (size_t)cn, hipMemcpyDeviceToDevice, dn); }, arena, cap, &out, false);
      if (st.e != hipSuccess || st.bad) { h->emit_pending.store(false, std::memory_order_release); return C3_E_HIP; }
    }
    stream_off[S] = out;
    DNCHK(hipStreamSynchronize(dn));
    ms_bgzf = (float)(dbg_now_ms() - t_z);
  }
  DNCHK(hipStreamSynchronize(dn));
  c3_emit_timing t = h->emit_tm;
  DNCHK(hipEventElapsedTime(&t.ms_write, h->emit_snap.ev[3], h->emit_snap.ev[4]));
#undef DNCHK
  t.ms_bgzf = ms_bgzf; t.out_bytes = out; t.ms_call += (float)(dbg_now_ms() - t_call);
  h->etm = t;
  h->emit_pending.store(false, std::memory_order_release);
  return C3_E_OK;
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
int c3h::fetch_msa_rows(c3_handle* h, int read, int nrows, char* out, int64_t cap, int* msa_len) {
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
  int rc = c3h::fetch_msa_rows(h, read, 2, tmp.data(), (int64_t)cap * 2, &ml);
  if (rc) return rc;
  memcpy(rowA, tmp.data(), ml); memcpy(rowB, tmp.data() + ml, ml);
  return ml;
}

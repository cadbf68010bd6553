// c3_stages.hip -- c3_batch_run: the stage drivers of the resident batch (conk, peaks, work list, zero-repeat rescue, POA,
// polish, QVs), their scratch sizing and timing.
#include "c3_host.h"

// what the host needs of every record to build the work list and size the scratch (Summary, c3_host.h)
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

static hipError_t zero_counters(c3_handle* h) { return hipMemsetAsync(h->d_counter.p, 0, sizeof(C3Counters), h->stream); }

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
static int launch_poa(c3_handle* h, const int* d_work, int nw, int Ncap, int K, int Pcap, long long cells, int* d_overflow, int* d_overflow16, int waves_per_cu, int wide_ring, bool first_pass = false) {
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
  // k_poa_pair ahead of the first pass when that pass is the default-scoring, NARROW, 16-bit instance: it aligns subread 1 to the
  // chain of subread 0 in this pass's slots and leaves vq, cells and a flag per read (C3_DEBUG_POA_PAIR=0: test hook, not launched);
  // every other pass gets null pointers and recomputes
  const bool def = c3_poa_default_scoring(a.p);
  const char* pe = getenv("C3_DEBUG_POA_PAIR");
  if (first_pass && def && !w32 && !wide_ring && !(pe && atoi(pe) == 0)) {
    HIPCHK(h->d_pair_vq.ensure(sizeof(uint16_t) * (size_t)h->total + 64)); HIPCHK(h->d_pair_cells.ensure(sizeof(int) * (size_t)h->n));
    HIPCHK(h->d_pair_done.ensure((size_t)h->n));
    for (int i = 0; i < 2; ++i) if (!h->ev_pair[i]) HIPCHK(hipEventCreate(&h->ev_pair[i]));
    HIPCHK(hipMemsetAsync(h->d_pair_done.p, 0, (size_t)h->n, h->stream));
    PoaPairArgs q; memset(&q, 0, sizeof(q));
    q.b = a.b; q.info = a.info; q.p = a.p; q.cnt = a.cnt; q.work = d_work; q.n_work = nw;
    q.ibase = a.ibase; q.cellsb = a.cellsb; q.dstride = L.cells; q.dbytes = (int)std::min<size_t>(L.cells, (size_t)1 << 30);
    q.Ncap = Ncap; q.cells_cap = (int)cells; q.rb_span = a.rb_span;
    q.vq = h->d_pair_vq.as<uint16_t>(); q.cells = h->d_pair_cells.as<int>(); q.done = h->d_pair_done.as<uint8_t>();
    HIPCHK(hipEventRecord(h->ev_pair[0], h->stream));
    c3k_launch_poa_pair(&q, slots, h->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(h->ev_pair[1], h->stream));
    a.pair_done = q.done; a.pair_vq = q.vq; a.pair_cells = q.cells;
    h->pair_ran = true;
  }
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
  // typical need: every further subread adds ~12 % nodes (mismatch siblings + insertions) to a graph of max_q nodes; a row
  // holds 2w+1 cells plus the drift between the row's nominal column and the argmax of its predecessors
  const double nodes_typ = (double)max_q * (1.0 + 0.15 * std::max(0, max_ns - 1));
  // rows of the full-size arena: one per node.  Twice the longest subread holds the graph of a few subreads; a deep read's graph
  // grows with every subread (250 subreads of 240 bases at 12 % errors: 845 rows per alignment on average), so 1.3 x the typical
  // node count where that is more (from five subreads per read on), within the node capacity of the pass.  At 2 * max_q + 2
  // alone, reads of 200 and more subreads overflowed every pass and ended as C3_ST_LIMIT: DESIGN.md 3, tests/test_gpu_deep_reads.py
  const long long rows_full = std::max<long long>(2LL * max_q + 2, std::min<long long>(Ncap_full, (long long)(1.3 * nodes_typ)));
  long long cells_full = rows_full * (2 * w + 1 + max_q / 5);
  if (max_ns < 2) cells_full = 64;
  if (cells_full > 0x7fffff00LL) cells_full = 0x7fffff00LL;
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
  HIPCHK(zero_cnt(h, &dc->pair_queue)); HIPCHK(zero_cnt(h, &dc->n_pair)); HIPCHK(zero_cnt(h, &dc->n_pair_declined));
  h->pair_ran = false; h->n_pair = 0; h->n_pair_declined = 0;
  // ring geometry of the first pass: subreads beyond the LDS query copy (1792 bases) or with bands beyond two 64-column chunks
  // (w = band_b + band_f * Q; a row holds 2w+1 columns + the drift of its predecessors' maxima) take the WIDE instance
  // (4 ring rows of 192 cells, sliding query window); C3_DEBUG_POA_WIDE = 0 / 1 forces one (test hook)
  int wide_ring = (max_q > 1792 || 2 * w + 1 + 24 > 128) ? 1 : 0;
  if (const char* e_ = getenv("C3_DEBUG_POA_WIDE")) wide_ring = atoi(e_) ? 1 : 0;
  // pass 1: scratch for the typical alignment.  Its two lists: reads the scratch was too small for -> pass 2 (the same kernel, worst-case
  // scratch); reads with a score beyond the 16-bit cells (from either pass) -> pass 3 (the 32-bit instance, worst-case scratch)
  int* ovA = h->d_overflow.as<int>(); int* ovB = h->d_overflow.as<int>() + nw;
  int rc = launch_poa(h, h->d_work.as<int>(), nw, Ncap, K, Pcap, cells, ovA, ovB, 24, wide_ring, true);
  if (rc) return rc;
  h->n_poa_redo = 0; h->n_poa_redo16 = 0;
  C3Counters c;
  HIPCHK(read_counters(h, &c));
  h->n_pair = c.n_pair; h->n_pair_declined = c.n_pair_declined;
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
  {
    // the 32-bit keys of the extension rows and of the linear window rows against the longest piece and layer of this batch
    // (DESIGN.md 4.6a): a cell is at most 2 * length + band steps of at most `kstep` from the origin, and every valid key has
    // to stay 2^28 above the rows' sentinels.  The default scoring (kstep 23) passes up to 5.8 million bases.
    const int pm = std::max({std::abs(h->cfg.pol_match), std::abs(h->cfg.pol_mismatch), std::abs(h->cfg.pol_gap)});
    const long long kstep = 4LL * pm + 3, bw = 2LL * h->cfg.dang_band + 1;
    if (kstep * (2LL * std::max(max_q, max_dang) + 4 * bw) >= C3_POL_KEY_RANGE)
      return c3_fail(h, C3_E_LIMIT, "polish scoring times the longest subread or dangling piece of the batch leaves the 32-bit cells of the polish rows: "
                                    "(4 * max|pol_*| + 3) * (2 * length + 4 * (2 * dang_band + 1)) must stay below 2^28");
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
    // (the worst case's columns: a layer of one window and a half of bases in one window, 12 groups of 64 at the default 500 --
    // at a fixed 12 groups a window of thousands of bases had rows, but no columns, for its own layers: DESIGN.md 4.6b)
    const long long hcap_full = (long long)(Ncap + 1) * 64 * std::max(12, (WL + WL / 2 + 64) / 64);
    const int R_typ = std::min(Ncap, WL + WL / 4 + 30 * NLcap + 64);
    long long hcap = std::min(hcap_full, (long long)(R_typ + R_typ / 2 + 4) * 256);      // (a window in the second launch runs alone on an idle device, ~1.5 ms: sized so that a usual batch has none -- at + R_typ / 4 one cfg2 window in 400 000 took it)
    if (const char* e = getenv("C3_DEBUG_HCAP_DIV")) hcap = std::max(4096LL, hcap_full / std::max(1, atoi(e)) / 64 * 64);       // test hook: smaller first-launch scratch (more windows take the second launch)
    const WinLayout L = c3_win_layout(Ncap, K, hcap), L2 = c3_win_layout(Ncap, K, hcap_full);
    const int slots = auto_slots(h, h->cfg.slots_win, L.total, n_win, 20);
    // (the second launch's worst-case cells grow with the square of the window length: its slots stay within a twelfth of the
    // device memory -- 256 slots need 1.7 GB at the default -- and, where that is fewer than 256, within half of what is free;
    // a window length whose single slot does not fit is refused here with a text, not by an allocation failing further down --
    // DESIGN.md 4.6b)
    const size_t budget = h->mem_total ? h->mem_total / 3 : ((size_t)64 << 30), per2 = L2.H + L2.D;
    size_t budget2 = budget / 4;
    if (hcap < hcap_full && per2 * 256 > budget2) {
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget2 = std::min(budget2, fr / 2); else (void)hipGetLastError();
    }
    if (L.total > budget || (hcap < hcap_full && per2 > budget2))
      return c3_fail(h, C3_E_NOMEM, "pol_window: the scratch of one window (DP cells for 3 * pol_window + 40 nodes per layer, 1.5 * pol_window columns) does not fit the device memory set aside for it");
    const int slots2 = hcap < hcap_full ? (int)std::min<size_t>(std::min(slots, 256), budget2 / per2) : 0;
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
    if (const char* e = getenv("C3_DEBUG_WIN_CHAIN")) a.no_chain = !strcmp(e, "0");      // test hook (tests/test_gpu_win_chain.py)
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
int c3h::qv_scratch(c3_handle* h, long long max_m, long long max_n, int n_items, QvArgs& a, int* grid) {
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
  int rc = c3h::qv_scratch(h, h->maxL, h->maxL, h->n, a, &grid);
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
  const double alloc0 = c3h::g_alloc_ms;
  // per-run figures start from zero: repeated runs of one resident batch (bench.py, tools/) must not accumulate
  if (stages & C3_STAGE_CONK) { h->tm.ms_conk = 0; h->tm.cells_conk = 0; }
  if (stages & C3_STAGE_PEAKS) h->tm.ms_peaks = 0;
  if (stages & C3_STAGE_POA) { h->tm.ms_poa = 0; h->tm.cells_poa = 0; h->tm.ms_poa_pair = 0; h->tm.n_pair = h->tm.n_pair_declined = 0; h->pair_ran = false; h->n_pair = h->n_pair_declined = 0; }
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
      h->tm.n_pair = h->n_pair; h->tm.n_pair_declined = h->n_pair_declined;
      if (h->pair_ran) { HIPCHK(hipEventElapsedTime(&ms, h->ev_pair[0], h->ev_pair[1])); h->tm.ms_poa_pair = ms; }
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
  h->tm.ms_alloc = (float)(c3h::g_alloc_ms - alloc0);
  h->tm.ms_host_gap = h->tm.ms_wall - h->tm.ms_total;
  if (stages & C3_STAGES_ALL) h->stages_done &= ~C3_STAGE_QV;         // a rerun of any stage without QV leaves stale QVs
  h->stages_done |= stages;
  return C3_E_OK;
}

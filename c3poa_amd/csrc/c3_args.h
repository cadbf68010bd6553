// c3_args.h -- kernel argument blocks shared by the host units (c3_host.h) and the kernels;
// PostArgs lives with its rule in c3_post.h.
#pragma once
#include "c3_dev.h"
#include <cstddef>

// Device counter block of a handle (c3_host.h: d_counter).  Every field has one purpose; the host zeroes a stage's fields
// before its launch and reads them by name.
struct C3Counters {
  int queue;                            // work queue of k_conk, k_adapter, k_poa, k_prep and the first k_window launch
  int peaks_queue;                      // k_peaks: read queue
  unsigned long long cells;             // DP cells counted by the last k_poa, k_prep or k_window stage
  unsigned long long cells_computed;    // k_window: cells actually computed (a banded row counts its band only)
  unsigned long long zero_cells;        // k_zero / k_zero_long: overlap cells of the zero-repeat rescue
  int poa_ovf;                          // k_poa: reads whose scratch overflowed (list PoaArgs::overflow)
  int poa_ovf16;                        // k_poa: reads with a score beyond the 16-bit cells (list PoaArgs::overflow16)
  int pair_queue;                       // k_poa_pair: work queue
  int n_pair, n_pair_declined;          // k_poa_pair: reads it aligned and flagged / reads with >= 2 subreads it declined (k_poa aligns those)
  int n_windows;                        // k_prep: windows reserved (may exceed PrepArgs::wcap)
  int win_ovf;                          // first k_window launch: windows queued for the second one (WinArgs::ovf_list)
  int win_queue2;                       // second k_window launch: work queue
  int band_layers, band_fallback;       // k_window: layers aligned with banded rows / band certificates that failed
  int band_mismatch;                    // k_window (test hook C3_DEBUG_BAND=verify): layers whose band and full tracebacks differ
  struct { int window, layer, R, q, band_row, full_row, next_row; } verify;   // ... the last such layer (q = last differing base)
  unsigned long long phases[16];        // diagnostic builds (-DC3_PHASE_PROF): per-phase cycle sums of k_poa / k_window
};
static_assert(offsetof(C3Counters, cells) % 8 == 0 && offsetof(C3Counters, cells_computed) % 8 == 0 &&
              offsetof(C3Counters, zero_cells) % 8 == 0 && offsetof(C3Counters, phases) % 8 == 0, "u64 counters must be 8-byte aligned");

struct ConkArgs {
  C3Batch b; const uint8_t* sp_codes; const int* sp_len; int32_t* track; C3Info* info; C3Counters* cnt;
  int match, mismatch, penalty;
  int n_spl; int32_t* scan;      // scan mode: [n * n_spl * 2][4] = max, argmax, mean, L
};
struct PeaksArgs {
  C3Batch b; const int32_t* track; C3Info* info; double* bufA; double* bufB; int32_t* cand; uint8_t* cstate;
  int32_t* raw_peaks; int32_t* n_raw; const int* sp_len; double coef[64]; int64_t maxL; int window, iters, min_dist;
  C3Counters* cnt;
};
struct PoaArgs {
  C3Batch b; C3Info* info; C3Params p; C3Counters* cnt; const int* work; int n_work;
  // per-slot scratch, one block per kind strided by slot (c3_poa_layout; the kernel derives every array from these bases: few live SGPRs)
  int* ibase; int* ebase; char* cellsb; uint8_t* bbase; long long* score;
  int Ncap, K, Pcap, cells_cap;
  uint8_t* draft; int32_t* tpos; uint8_t* msa_dbg; const int64_t* msa_off; int* msa_len;
  int rb_span;              // 0 = default; test hook C3_DEBUG_POA_RBSPAN: width of the window a row maximum may move in before the 16-bit base follows it
  int no2col;               // test hook C3_DEBUG_POA_NO2COL: no two-column rows (those rows take the near rows, as before them)
  uint4* desc; int* jump;
  int* pbase;               // [slots][Pcap] node of every fused base
  int* overflow;            // reads whose scratch overflowed (count in cnt->poa_ovf): redone with worst-case scratch; nullptr in the passes that have it
  int* overflow16;          // reads with a score beyond the 16-bit cells (count in cnt->poa_ovf16): redone by the 32-bit instance; nullptr in that pass
  // what k_poa_pair left (PoaPairArgs); nullptr in every pass but the first DEF, NARROW, 16-bit one: those recompute
  const uint8_t* pair_done; const uint16_t* pair_vq; const int* pair_cells;
};
// k_poa_pair (k_poa_pair.hip): subread 1 against the chain of subread 0, ahead of the first k_poa pass, in that pass's slots
struct PoaPairArgs {
  C3Batch b; const C3Info* info; C3Params p; C3Counters* cnt; const int* work; int n_work;
  int* ibase; char* cellsb;             // k_poa's per-slot int block (row records go to its rowm) and cell arena (direction bytes, 128 per row)
  size_t dstride; int dbytes;           // bytes between the arenas of two slots / usable bytes of one
  int Ncap, cells_cap, rb_span;         // as in PoaArgs: a read k_poa's slot would be too small for is declined
  uint16_t* vq;                         // per base of the batch (at off[rid] + sub_beg[1] + q): node aligned to base q of subread 1, 0xffff = insertion
  int* cells; uint8_t* done;            // per read: counted cells / 1 = vq and cells are valid (zeroed by the host per batch)
};
// k_poa scratch of one slot, bytes per region (each region is one buffer strided by slot):
//   ints  C3_POA_NI * Ncap ints (n_in n_out grp order order2 index gfirst glast rem mpl mpr rowm[3N] anchor col col2t nxt foff)
//   edges 3 * Ncap * K ints (in_from out_to out_w)
//   cells 2 bytes per cell (direction bytes D8, predecessor bytes P8) + 16 bytes per far cell (32-bit H E1 E2 D of the few rows
//         that keep them): cells_cap >> far_shift far cells, a quarter in the 16-bit instance, all of them in the 32-bit one
//   bases 5 * Ncap bytes (base rows2[4N]); score Ncap long longs; desc 2 * Ncap uint4; jump C3_JUMP_LEVELS * Ncap ints; path Pcap ints
#define C3_POA_NI 19
#define C3_POA_I_ROWM 11              // block of rowm in the int region (3 blocks: 11..13); k_poa's Ctx and k_poa_pair's row records use it
// abPOA's default scoring with match 5: what the DEF instances of k_poa and k_poa_pair are compiled for
__host__ __device__ inline bool c3_poa_default_scoring(const C3Params& p) {
  return p.poa_match == 5 && p.poa_mismatch == 4 && p.o1 == 4 && p.e1 == 2 && p.o2 == 24 && p.e2 == 1;
}
__host__ __device__ inline int c3_poa_far_shift(bool w32) { return w32 ? 0 : 2; }
struct PoaLayout { size_t ints, edges, cells, bases, score, desc, jump, path, total; };
__host__ __device__ inline PoaLayout c3_poa_layout(size_t Ncap, size_t K, int cells_cap, int far_shift, size_t Pcap) {
  PoaLayout l;
  l.ints = sizeof(int) * C3_POA_NI * Ncap; l.edges = sizeof(int) * 3 * Ncap * K;
  l.cells = 2 * (size_t)cells_cap + 16 * (size_t)(cells_cap >> far_shift);
  l.bases = 5 * Ncap; l.score = sizeof(long long) * Ncap; l.desc = sizeof(uint4) * 2 * Ncap;
  l.jump = sizeof(int) * C3_JUMP_LEVELS * Ncap; l.path = sizeof(int) * Pcap;
  l.total = l.ints + l.edges + l.cells + l.bases + l.score + l.desc + l.jump + l.path;
  return l;
}

struct WLayer { int qbeg, len, begin, end; };
struct WinRec { int rid, w, n_layers, blen, tgs, out_len, polished, pad_; };
struct PrepArgs {
  C3Batch b; C3Info* info; C3Params p; C3Counters* cnt; const int* work; int n_work;
  const uint8_t* draft; int32_t* tpos; int wcap; uint8_t* eD; int64_t ecap; int* lw_first; int* lw_last; int NLcap, NWcap;
  WinRec* wrec; WLayer* wlay; int* win_base;
  int sub_shift;                          // log2(4 * (pol_match - pol_mismatch)) when that is a power of two (the rows' one-and match flags), else -1
  int rows_old;                           // test hook C3_DEBUG_PREP_ROWS=old: every extension row takes the masked body
};
struct WinArgs {
  C3Batch b; C3Params p; C3Counters* cnt; int n_win; const WinRec* wrec_in; WinRec* wrec; const WLayer* wlay; int NLcap;
  const uint8_t* draft;
  uint8_t* base; int* ibase; int* ebase; long long* score;
  int32_t* H; uint16_t* D; uint4* rdesc; int Ncap, K; long long hcap; uint8_t* wout; int wout_cap;
  int Lcap;                               // nodes the LDS consensus sweep can hold (<= Ncap)
  int band_mode;                          // 0 = banded rows with certificate (default), 1 = never banded, 2 = every certificate counts as failed (test hook: C3_DEBUG_BAND)
  // two launches: the first with DP scratch for the typical layer (hcap small); a window one of whose layers does not fit is
  // dropped untouched into `ovf_list` (count in cnt->win_ovf) and redone by the second launch, which has worst-case scratch,
  // takes its windows from `wlist`, their number from device memory (cnt->win_ovf) and its queue from cnt->win_queue2
  // (k_window<true>: the first launch's code carries none of this)
  const int* wlist; int* ovf_list;
  int no_chain;                           // test hook C3_DEBUG_WIN_CHAIN=0: the first layer of a window takes the general graph phases too
};
// k_window scratch of one slot, bytes per region (each region is one buffer strided by slot): ints W_INTS * Ncap ints (WCtx::I,
// 18 * Ncap + 9 used), edges 4 * Ncap * K ints, bases 2 * Ncap bytes (base, mask), score Ncap long longs, DP cells hcap * (4 bytes
// of H + 1 direction byte), row descriptors Ncap + 1 uint4
#define W_INTS 19
struct WinLayout { size_t ints, edges, bases, score, H, D, desc, total; };
__host__ __device__ inline WinLayout c3_win_layout(size_t Ncap, size_t K, size_t hcap) {
  WinLayout l;
  l.ints = sizeof(int) * W_INTS * Ncap; l.edges = sizeof(int) * 4 * Ncap * K; l.bases = 2 * Ncap; l.score = sizeof(long long) * Ncap;
  l.H = sizeof(int32_t) * hcap; l.D = hcap; l.desc = sizeof(uint4) * (Ncap + 1);
  l.total = l.ints + l.edges + l.bases + l.score + l.H + l.D + l.desc;
  return l;
}
struct StitchArgs {
  C3Batch b; C3Info* info; const int* work; int n_work; const WinRec* wrec; const int* win_base; const uint8_t* wout; int wout_cap; char* cons;
  const uint8_t* zflag;
};
// adapter finder (k_adapter): every read x every entry of the splint table x both strands
struct AdapterArgs {
  C3Batch b; C3Params p; C3Counters* cnt;
  const uint8_t* ad_codes; const int* ad_len; int n_ad;
  uint8_t* D; long long dcap;           // [grid][dcap] direction bytes
  int32_t* out;                         // [n * n_ad * 2][12]
};

struct ZeroArgs {
  C3Batch b; C3Info* info; C3Params p; C3Counters* cnt; const int* work; int n_work;
  uint8_t* D; long long dcap;           // [grid][dcap] direction bytes
  int4* zinfo; uint8_t* zflag;          // per read: r_st, r_en, q_st, q_en; rescue in progress / done
  const uint8_t* draft; char* cons;
  uint8_t* S; long long scap; int zk;   // k_zero_long: [grid][scap] scratch (checkpoint rows, direction block, row carries); checkpoint interval
};

// k_zero_long scratch of one read (d0 = n0 columns, d1 = n1 rows, checkpoint every K rows), laid out from the slot base:
// checkpoint rows ceil(n1/K) * (n0+1) * int2 (H, E) | direction block min(K, n1) * (n0+1) bytes | row carries n1 * 3 ints
struct ZlLayout { long long ck, dir, car, total; };
__host__ __device__ inline ZlLayout c3_zl_layout(long long n0, long long n1, long long K) {
  ZlLayout l;
  l.ck = 0;
  l.dir = (n1 + K - 1) / K * (n0 + 1) * 8;
  l.car = (l.dir + (n1 < K ? n1 : K) * (n0 + 1) + 15) & ~15LL;
  l.total = (l.car + n1 * 12 + 255) & ~255LL;
  return l;
}
// k_qv (k_qv.hip): per-base consensus QVs.  Batch form (sa_np < 0): every read of the resident batch with status OK and
// cons_len > 0; stand-alone form (sa_np >= 0): one consensus cons[0..sa_n) with sa_np pieces packed like reads.
struct QvArgs {
  int n_reads; const C3Info* info; const uint32_t* pk; const int64_t* woff; const uint8_t* qual; const int64_t* off;
  const char* cons; char* qv;                      // consensus / QV bytes at off[r] (batch) or at 0 (stand-alone)
  int sa_np, sa_n; const int64_t* sa_woff; const int64_t* sa_off; const int32_t* sa_mode;
  uint32_t* dirs; long long dir_words;             // [grid * 4][dir_words] packed direction dwords, one slot per wave
  int* gS; uint8_t* gcodes; long long gcap;        // [grid][gcap]: S and codes of a consensus longer than lds_n
  int lds_n;                                       // consensus columns held in LDS (S int32 + code byte each)
  unsigned long long* cnt;                         // [0] reads, [1] pieces, [2] skipped, [3] band cells, [4] edge hits
};

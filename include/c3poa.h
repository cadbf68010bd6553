/*
 * c3poa.h -- C ABI of the MI355X-native R2C2 consensus hot path (libc3poa_hip.so).
 *
 * The reference (rvolden/C3POa v2.2.3) has no FFI layer of its own: its seams are plain Python
 * call sites into un-vendored native dependencies.  Every entry point below names the reference
 * call site(s) it replaces (paths relative to the reference repository root); INTEGRATION.md
 * shows the ctypes stub a maintainer of the reference would add at each site.
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; all functions return 0 or a negative c3_err
 *   - one c3_handle per GPU, not thread-safe; create once per worker, never per batch
 *   - a per-read failure is a status code in c3_read_result, never a batch failure
 *   - sequences are ASCII; A/C/G/T/U in either case are coded 0..3, every other byte is coded
 *     as 'A' for alignment purposes (2-bit packing)
 *   - the library FAILS LOUDLY without a GPU: there is no CPU fallback anywhere in it
 */
#ifndef C3POA_H
#define C3POA_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define C3_MAX_PEAKS 256   /* peaks / kept subreads recorded per read */

typedef enum {
  C3_E_OK = 0,
  C3_E_NO_DEVICE = -1,
  C3_E_HIP = -2,
  C3_E_ARG = -3,
  C3_E_NOMEM = -4,
  C3_E_STATE = -5,
  C3_E_LIMIT = -6,
  C3_E_DATA = -7                                /* damaged input: a BGZF member that does not inflate to what its trailer says */
} c3_err;

/* per-read status (same numbering as the oracle's) */
typedef enum {
  C3_ST_OK = 0,
  C3_ST_NOT_ASSIGNED = 1,  /* C3POa.py:115 */
  C3_ST_NO_PEAKS = 2,      /* C3POa.py:125,131 */
  C3_ST_NO_CONSENSUS = 3,  /* repeats == 0, or polish emitted nothing (determine_consensus.py:44-47,97-99) */
  C3_ST_TOO_SHORT = 4,     /* shorter than the smoothing half-window */
  C3_ST_LIMIT = 5          /* capacity limit (subreads > 250, band arena, window graph) */
} c3_status;

/* algorithm constants of the reference call sites; c3_default_config fills them */
typedef struct {
  int device;                                   /* HIP device ordinal */
  int conk_match, conk_mismatch, conk_penalty;  /* conk.conk(splint, seq, 20): C3POa.py:111,123 */
  int sg_iters, sg_window, sg_order;            /* call_peaks(scores, d, 3, 41, 2): C3POa.py:111,124 */
  int mdistcutoff;                              /* -d: C3POa.py:45 */
  int poa_match, poa_mismatch;                  /* poa.msa_aligner(match=5): determine_consensus.py:30 */
  int poa_o1, poa_e1, poa_o2, poa_e2;           /* abPOA defaults 4,2,24,1.  All six POA scores are penalties / rewards given as
                                                   non-negative numbers.  Admitted: poa_match 1..64, poa_mismatch 0..64,
                                                   poa_o1 and poa_o2 0..64, poa_e1 and poa_e2 0..16, no order between the two gap
                                                   pieces; anything else makes c3_create fail with C3_E_ARG (the message names the
                                                   field and its bounds).  Inside these ranges the result is the 32-bit result:
                                                   the 16-bit cells of k_poa hold every value or hand the read to the 32-bit
                                                   pass (DESIGN.md 4.3 derives the bounds).  That pass carries score * 512 in
                                                   32 bits: alignment scores must stay inside (-524288, 4194304), which is
                                                   poa_match * subread length < 4194304 at the top (65535 bases at match 64) */
  int poa_band_b; double poa_band_f;            /* abPOA defaults 10, 0.01 */
  int pol_match, pol_mismatch, pol_gap;         /* racon 3,-5,-4.  Scores as racon takes them (signed; a gap of zero or more, a
                                                   match of zero or less and a mismatch above the match are admitted).  Admitted:
                                                     pol_match    -8191..8191, and above 2 * pol_gap
                                                     pol_mismatch -8191..8191
                                                     pol_gap      -8191..8191 (so at most 4095, under pol_match 8191)
                                                   anything else makes c3_create fail with C3_E_ARG (the message names the field
                                                   and its bounds).  A match that scores no more than two gaps aligns no layer to
                                                   its backbone: the window graphs outgrow their capacity and every read would
                                                   end as C3_ST_LIMIT.  Inside the range the result is the exact one as long as
                                                   (4 * max|pol_*| + 3) * (2 * length + 4 * (2 * dang_band + 1)) < 2^28 for the
                                                   longest subread and dangling piece of a batch (5.8 million bases at the
                                                   default scoring, 3 580 at 8191); c3_batch_run refuses a batch beyond that with
                                                   C3_E_LIMIT.  The 16-bit rows of the window polish guard themselves per layer
                                                   and hand what they cannot hold to the 32-bit rows. */
  int pol_window, pol_q;                        /* racon window 500; -q 5: determine_consensus.py:92.  Admitted: pol_window
                                                   1..18458; anything else makes c3_create fail with C3_E_ARG (the message names
                                                   the field and its bounds).  Below 1 there is no window to cut; above 18458 a
                                                   window graph (3 * pol_window + 40 nodes per layer) outgrows the 16-bit node ids
                                                   of the window consensus.  The scratch of the polish grows with
                                                   the square of the window length: a run whose worst-case window does not fit
                                                   the device memory ends with C3_E_NOMEM. */
  int dang_band;                                /* half band of the dangling-piece extension, 128.  Admitted: 0 (the diagonal
                                                   alone) .. 255; below 0 c3_create fails with C3_E_ARG, above 255 with C3_E_LIMIT */
  int slots_poa, slots_win;                     /* resident wave slots (0 = auto) */
  int zero;                                     /* args.zero (C3POa.py:48-49): attempt the zero-repeat rescue (default 1) */
  int64_t zero_max_cells;                       /* zero-repeat rescue only for pieces with front * tail <= this (default 16777216;
                                                   1 .. 2147483647, else c3_create fails with C3_E_ARG).  The reference has no cap. */
} c3_config;

typedef struct {
  int32_t status;
  int32_t n_peaks;                 /* after shift by len(splint)//2 and clip (C3POa.py:127-132) */
  int32_t n_sub;                   /* kept subreads = "repeats" (determine_consensus.py:12) */
  int32_t has_front, has_tail;     /* dangling pieces read[:front_end], read[tail_beg:] (C3POa.py:145-155) */
  int32_t front_end, tail_beg;
  int32_t cons_len, draft_len;
  int32_t n_win;
  int32_t peaks[C3_MAX_PEAKS];
  int32_t sub_beg[C3_MAX_PEAKS], sub_end[C3_MAX_PEAKS];   /* pure slices of the read (C3POa.py:141-144) */
} c3_read_result;
/* ARRAY TAILS ARE UNSPECIFIED: c3_batch_results copies only the used prefix of peaks / sub_beg / sub_end across PCIe, so in the
 * caller's records peaks[k] for k >= n_peaks and sub_beg[k] / sub_end[k] for k >= n_sub hold whatever the buffer held before
 * (never read them; set C3_FULL_RESULTS=1 in the environment to get whole records, e.g. when diffing raw buffers). */

/* kernel time of the last c3_batch_run, measured with hipEvents on the library's own stream */
typedef struct {
  float ms_pack, ms_conk, ms_peaks, ms_poa, ms_prep, ms_window, ms_stitch, ms_total;
  int64_t n_reads, n_bases, n_windows;
  int64_t cells_conk, cells_poa, cells_polish;
  int64_t n_poa_redo;      /* reads whose POA scratch (sized for the typical alignment) overflowed and were redone full-size, plus n_poa_redo16 */
  float ms_wall;           /* host wall time of the whole c3_batch_run call; ms_wall - ms_total = time the GPU waited for the host */
  float ms_host_worklist;  /* of which: building + uploading the POA work list on the host (timer starts AFTER the wait for k_conk / k_peaks) */
  float ms_alloc;          /* of which: growing device scratch buffers (only while batch shapes are still growing) */
  float ms_host_gap;       /* ms_wall - ms_total: time the GPU was not running one of the six timed kernels during the call */
  int64_t cells_polish_computed;   /* polish DP cells actually computed: banded layers fill 64*CB columns per row, a layer whose band
                                      certificate failed counts band + full matrix.  cells_polish stays the full-matrix count (= oracle) */
  int64_t n_band_layers, n_band_fallback;   /* window layers aligned in a band and accepted / redone unbanded after a failed certificate */
  int64_t n_band_mismatch;                  /* C3_DEBUG_BAND=verify only: accepted band layers whose traceback differs from the full matrix's (must be 0) */
  int64_t n_win_redo;                       /* windows with a layer beyond the first launch's DP scratch, redone by the full-size second launch of k_window */
  int64_t n_poa_redo16;                     /* of n_poa_redo: reads redone by the 32-bit POA pass -- a score did not fit the 16-bit cells of the first passes, or the 32-bit cells of its wide / far rows did not fit the arena of the full-size pass (0 on the config shapes) */
  int64_t n_pair, n_pair_declined;          /* k_poa_pair: reads whose second subread it aligned to the chain of the first ahead of k_poa / reads with >= 2 subreads it left to k_poa (both 0 when it does not run: non-default scoring, WIDE or 32-bit first pass) */
  float ms_poa_pair;                        /* its kernel time (part of ms_poa) */
} c3_timing;

typedef struct c3_handle c3_handle;

void c3_default_config(c3_config* cfg);
const char* c3_version(void);
/* GPUs visible to the process (0 without a GPU); -n of the CLI is clamped to it (C3POa.py:236 sized a process pool) */
int c3_device_count(void);
/* Creates the HIP context of device `device` on the calling thread and returns (hipSetDevice + an empty hipFree): the CLI calls it
 * on a thread of its own per GPU at start-up so that the workers' c3_create finds the context ready (C3POa.py:236-248 paid the
 * start-up of every worker process instead).  0 or a negative c3_status. */
int c3_warm_device(int device);

/* lifecycle.  Replaces the per-task worker process of C3POa.py:236 (mp.Pool, maxtasksperchild=1). */
int c3_create(const c3_config* cfg, c3_handle** out);
void c3_destroy(c3_handle* h);
const char* c3_last_error(const c3_handle* h);

/* splint table (C3POa.py:231-234: splint_dict[name] = [seq, revcomp(seq)]); the library makes the
 * reverse complements itself.  cat = concatenated ASCII, off[n+1]. */
/* k_conk keeps its score cells in 16 bits: max(conk_match, conk_mismatch, 0) * splint length must not exceed 32000 and
 * conk_penalty must lie in 0..32000, for every splint; otherwise C3_E_LIMIT with a c3_last_error text.  A splint of 0 or of more
 * than 512 bases is C3_E_LIMIT as well.  A refused call leaves the table of the last successful call in force. */
int c3_set_splints(c3_handle* h, int n, const char* cat, const int64_t* off);

/* batch = the `reads` argument of analyze_reads (C3POa.py:110) in SoA form.
 *   seqs/quals: concatenated ASCII, off[n+1]; splint_id[i] = row of c3_set_splints;
 *   strand[i] = '+' / '-' (adapter_dict[name][1], C3POa.py:117-122), anything else = not assigned.
 * Copies to the device and packs to 2 bit; the caller may free its buffers on return. */
int c3_batch_upload(c3_handle* h, int n, const char* seqs, const char* quals, const int64_t* off,
                    const int16_t* splint_id, const char* strand);

/* double buffering: c3_batch_stage copies (and 2-bit packs) the NEXT batch on a second stream while the resident batch
 * is being processed; c3_batch_commit makes it resident once the results of the previous batch have been fetched.
 * seqs / quals must stay valid until c3_batch_commit returns; c3_batch_upload = stage + commit. */
int c3_batch_stage(c3_handle* h, int n, const char* seqs, const char* quals, const int64_t* off,
                   const int16_t* splint_id, const char* strand);
int c3_batch_commit(c3_handle* h);

/* overwrite the splint row / strand of the resident batch (e.g. with the output of c3_scan_splints) before c3_batch_run */
int c3_batch_assign(c3_handle* h, const int16_t* splint_id, const char* strand);

/* run the resident batch through the hot path.  The call returns when the batch is done: the stage sizes (work lists,
 * window count) are read back on the host between the kernels.  Overlap comes from c3_batch_stage on the second stream.
 * stages: bit0 conk, bit1 peaks+split, bit2 POA/draft, bit3 polish.  C3_STAGES_ALL = whole path
 * = one call of analyze_reads (C3POa.py:110-173) minus file I/O. */
#define C3_STAGE_CONK 1
#define C3_STAGE_PEAKS 2
#define C3_STAGE_POA 4
#define C3_STAGE_POLISH 8
#define C3_STAGES_ALL 15
int c3_batch_run(c3_handle* h, int stages);
int c3_batch_sync(c3_handle* h);

/* results of the resident batch.  cons receives the consensus bytes of read i at cons_off[i]
 * (cons_off[n+1] is written by the call; capacity cons_cap bytes; returns C3_E_LIMIT and the
 * needed size in cons_off[n] if too small).  Pass cons=NULL to fetch only the per-read records.
 * After the POA / polish stages only the used part of every record is copied: peaks[k >= n_peaks] and
 * sub_beg / sub_end[k >= n_sub] of the caller's records are then unspecified (left as they were). */
int c3_batch_results(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off);
/* The same in two halves, so that the device->host copy runs beside the NEXT batch's kernels (the reference overlaps nothing:
 * analyze_reads writes its files before the worker takes the next group, C3POa.py:110-173).
 * c3_batch_results_snapshot (owner thread, after c3_batch_run) freezes the records and the compact consensus bytes in device
 * buffers of their own; afterwards the owner may c3_batch_commit and c3_batch_run the next batch.
 * c3_batch_results_fetch copies the snapshot into the caller's buffers (same arguments and C3_E_LIMIT rule as c3_batch_results)
 * and returns when they have landed; it touches nothing but the snapshot and MAY BE CALLED FROM ANOTHER THREAD while the owner
 * works on the next batch -- the only two calls on one handle that may overlap (it does not set c3_last_error).
 * One snapshot per handle: _snapshot before the previous one was fetched, or _fetch without a snapshot, returns C3_E_STATE. */
int c3_batch_results_snapshot(c3_handle* h);
int c3_batch_results_fetch(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off);
int c3_batch_timing(c3_handle* h, c3_timing* t);

/* ---- stage probes (tests / per-stage shims), all operate on the resident batch ---- */
/* conk.conk(splint, seq, penalty) score track of read i (C3POa.py:123): L int32 */
int c3_fetch_track(c3_handle* h, int read, int32_t* out, int64_t cap);
/* 3x Savitzky-Golay smoothed track (bin/call_peaks.py:10-11): L doubles.  Only valid for the last
 * `slots` reads processed, so tests call it with single-read batches. */
int c3_fetch_smoothed(c3_handle* h, int read, double* out, int64_t cap);
/* raw call_peaks() indices before the shift (bin/call_peaks.py:15) */
int c3_fetch_raw_peaks(c3_handle* h, int read, int32_t* out, int cap);
/* draft consensus before polish (abpoa_cons, determine_consensus.py:32,41,47) */
int c3_fetch_draft(c3_handle* h, int read, char* out, int cap);
/* 2-row MSA of a 2-subread read (res.msa_seq, determine_consensus.py:34); returns msa_len */
int c3_fetch_msa2(c3_handle* h, int read, char* rowA, char* rowB, int cap);

/* stand-alone stage entry points used by the per-stage Python shims.  Each one uploads its
 * arguments, runs the corresponding kernels and returns the result. */
/* call_peaks(scores, min_dist, iters, window, order) (bin/call_peaks.py:8-16; iters/window/order are the
 * handle's sg_* settings): returns the number of peaks written to `peaks` (0 = gated / none);
 * smoothed (optional, n doubles) receives the smoothed track.
 * Capacity: a track keeps at most C3_MAX_PEAKS - 1 = 255 peaks.  With more, the call fails with C3_E_LIMIT and a
 * c3_last_error text instead of returning a count (in a batch such a read gets C3_ST_LIMIT and n_peaks = 0); the reference
 * has no such limit.
 * Too short: a track of fewer than (sg_window - 1) / 2 + 1 points (or of 1 point) is not smoothed: 0 peaks here,
 * C3_ST_TOO_SHORT in a batch.  The reference has no defined answer there: its padding slices (bin/savitzky_golay.py:33-34)
 * come up short, and the filtered track it returns has another length than the input (18 points for 20 at window 41). */
int c3_call_peaks(c3_handle* h, const int32_t* scores, int n, int min_dist, int32_t* peaks, int cap, double* smoothed);
/* pyabpoa.msa_aligner(match=5).msa(seqs, out_cons, out_msa) (determine_consensus.py:30,34,43):
 * msa receives n rows of *msa_len chars (row-major).  quals may be NULL. */
int c3_poa_msa(c3_handle* h, int n, const char* const* seqs, const int* lens,
               char* cons, int cons_cap, int* cons_len, char* msa, int64_t msa_cap, int* msa_len);
/* pairwise_consensus(msa_rows, subreads, quals) (bin/consensus.py:76-81; call site determine_consensus.py:36-40): rowA/rowB
 * are the two MSA rows ('-' = gap), msa_len columns each.  *out_len <= msa_len bases are written to out. */
int c3_pairwise_consensus(c3_handle* h, const char* rowA, const char* rowB, int msa_len,
                          const char* subA, int lenA, const char* qualA, const char* subB, int lenB, const char* qualB,
                          char* out, int cap, int* out_len);
/* determine_consensus for repeats >= 1 (determine_consensus.py:29-99): draft + polish.
 * front/tail may be NULL.  returns consensus length in *out_len (0 = nothing emitted). */
int c3_determine_consensus(c3_handle* h, int n, const char* const* subs, const char* const* quals,
                           const int* lens, const char* front, const char* front_q, int front_len,
                           const char* tail, const char* tail_q, int tail_len,
                           char* out, int cap, int* out_len, char* draft, int draft_cap, int* draft_len);

/* splint / strand assignment of the resident batch (replaces the blat step of bin/preprocess.py:12-45,61-77):
 * every read is scored against every splint on both strands with the conk kernel.
 * out (optional) [n][n_splints][2][4] = {max of the track, its offset, mean of the track, read length};
 * assign_splint[i] = best splint (-1 = none), assign_strand[i] = '+', '-' or '?'; a candidate is accepted when
 * max >= 6 * mean (the contrast call_peaks demands later, bin/call_peaks.py:13) and max >= match*51*52/2
 * (the diagonal sum of a perfect 51-base match: `matches > 50`, bin/preprocess.py:32). */
int c3_scan_splints(c3_handle* h, int32_t* out, int16_t* assign_splint, char* assign_strand);

/* adapter finder of the post-processing step (replaces the blat call of C3POa_postprocessing.py:229-236; fields as
 * read by parse_blat, :238-264): best local affine alignment of every read of the resident batch against every entry
 * of the splint table (load the adapters with c3_set_splints) on both strands.
 * out[(i*n_adapters + a)*2 + rc][12] = score, qStart, qEnd, tStart, tEnd (PSL conventions, forward coordinates),
 * matches, misMatches, qBaseInsert, tBaseInsert, qNumInsert, tNumInsert, read length; score 0 = no alignment. */
int c3_scan_adapters(c3_handle* h, int32_t* out);

/* zero_repeats(name, seq, qual, dangling, qual_dangling, subread_file) (determine_consensus.py:106-136):
 * d0 = first dangling piece, d1 = second; *out_len = 0 when there is no acceptable overlap or the
 * stitched sequence is shorter than min_len (args.mdistcutoff, determine_consensus.py:17). */
int c3_zero_repeats(c3_handle* h, const char* d0, const char* q0, int n0, const char* d1, const char* q1, int n1,
                    int min_len, char* out, int cap, int* out_len);

/* ---- host I/O either side of the path; host code only, works without a GPU ---- */

/* one group of reads in structure-of-arrays form; the buffers belong to the reader (page-locked when a GPU is
 * present, so c3_batch_upload(h, b.n, b.seqs, b.quals, b.off, ...) copies them by DMA) */
typedef struct {
  int32_t n;                 /* reads in the group */
  int64_t n_short;           /* records skipped because they were shorter than min_len */
  const char* names;         /* concatenated names, name_off[n+1] (name = header up to the first blank) */
  const int64_t* name_off;
  const char* seqs;          /* concatenated bases / qualities, off[n+1] */
  const char* quals;         /* FASTA records get '!' */
  const int64_t* off;
} c3_host_batch;

/* host buffers for callers that assemble their own batches: page-locked when a GPU is present (DMA copies in
 * c3_batch_stage / c3_batch_upload), plain memory otherwise.  The reference builds Python lists (C3POa.py:239-244). */
int c3_host_alloc(int64_t bytes, void** out);
void c3_host_free(void* p);

typedef struct c3_reader c3_reader;
/* mm.fastx_read(path, read_comment=False) (C3POa.py:201,239): FASTA or FASTQ, multi-line, plain or .gz.
 * n_sets = how many groups stay valid at once (the buffers of a group are reused n_sets calls later). */
int c3_reader_open(const char* path, int n_sets, c3_reader** out);
/* the same over the byte range [beg, end) of a plain FASTA / 4-line FASTQ file: begins at the first record starting at or
 * after beg, ends before the first record starting at or after end (end < 0: end of file), so ranges that tile the file
 * read every record exactly once -- one reader per GPU worker (C3POa.py:236-256 sharded 1000-read groups over a pool) */
int c3_reader_open_range(const char* path, int n_sets, int64_t beg, int64_t end, c3_reader** out);
void c3_reader_close(c3_reader* r);
const char* c3_reader_error(const c3_reader* r);
/* records without a quality line seen so far (FASTA).  The reference cannot process them (C3POa.py:167 takes ord() of every
 * quality character; racon runs with -q 5), so the CLI refuses such input */
int64_t c3_reader_noqual(const c3_reader* r);
/* bytes of (page-locked) host buffers the reader holds: sized by what its file / byte range can still deliver, never by max_reads alone */
int64_t c3_reader_reserved_bytes(const c3_reader* r);
/* 1 when c3_reader_open_range found bytes but no 4-line FASTQ / FASTA record start in its range (multi-line FASTQ): the caller
 * must read the file with ONE reader (c3_reader_open), or the records of that range are lost */
int c3_reader_range_lost(const c3_reader* r);
/* names_only != 0: parse but do not store sequences/qualities (first pass of C3POa.py:200-207: names + counts) */
void c3_reader_names_only(c3_reader* r, int names_only);
/* next group: at most max_reads reads of length >= min_len (C3POa.py:202-204,240-241), stops early once max_bases
 * bases are held (0 = no limit).  out->n == 0 at end of file. */
int c3_reader_next(c3_reader* r, int max_reads, int64_t max_bases, int min_len, c3_host_batch* out);
/* the same into buffer set `set` (0 .. n_sets-1) named by the caller instead of round-robin: a pipeline whose consumers
 * finish out of order (several GPUs) keeps a free list of sets and reuses one only after its group has been written */
int c3_reader_next_set(c3_reader* r, int set, int max_reads, int64_t max_bases, int min_len, c3_host_batch* out);

/* file side effects of analyze_reads + determine_consensus for one group (C3POa.py:141-173,
 * bin/determine_consensus.py:57-77,108-114): appends the consensus FASTA records to cons_paths[splint_id[i]] and the
 * subread FASTQ records to sub_paths[splint_id[i]].  cons/cons_off as returned by c3_batch_results; zero = args.zero. */
int c3_write_group(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                   const int16_t* splint_id, int n_splints, const char* const* cons_paths,
                   const char* const* sub_paths, int zero);

/* c3_write_group may be called from several threads on the same files (one writer per GPU worker): every call reserves its
 * byte range at the end of each file under a lock.  Reservations are keyed by the file itself (device, inode) and live only
 * while a writer of that file is in flight: a file truncated or replaced between two calls is appended to from its real end.
 * c3_writer_reset forgets all reservations (start of a run; never while c3_write_group calls are in flight). */
void c3_writer_reset(void);

/* splint assignment from the PSL (bin/preprocess.py:22-45) without per-read host objects: rows with qBaseInsert < 50 and
 * matches > 50 count, per read the row with the most matches wins (the earliest on ties).  Host code. */
typedef struct c3_assign c3_assign;
int c3_assign_open(const char* psl_path, int n_splints, const char* const* splint_names, c3_assign** out);
void c3_assign_close(c3_assign* a);
/* splint row / strand ('+', '-'; -1 / '?' = no counted row) of every read of the group; returns how many are assigned */
int c3_assign_batch(const c3_assign* a, const c3_host_batch* b, int16_t* splint_id, char* strand);
/* adapter_set (bin/preprocess.py:34,43): flags[s] = 1 when a counted row names splint s; *rows_kept = counted rows */
int c3_assign_seen(const c3_assign* a, uint8_t* flags, int64_t* rows_kept);

/* PSL rows of the GPU splint finder, appended to `path` (one 21-column row per assigned read of the group; table /
 * splint_id / strand as returned by c3_scan_splints; the row format is stated by psl_row() in c3poa_amd/preprocess.py) */
int c3_write_splint_psl(const c3_host_batch* b, const int32_t* table, const int16_t* splint_id, const char* strand,
                        int n_splints, const char* const* splint_names, const int32_t* splint_lens, int match,
                        const char* path, int64_t* rows_written);

/* match_index for a whole batch on the GPU (one lane per piece): pieces = n slots of 64 bytes, lens[n] <= 64, at most
 * 16 indexes of at most 32 bases; out[i] = winning index number or -1.  Same function as c3_match_index below. */
int c3_match_index_batch(c3_handle* h, int n, const char* pieces, const int32_t* lens, int n_idx,
                         const char* idx_cat, const int64_t* idx_off, int32_t* out);

/* match_index(seq, seq_to_idx) of C3POa_postprocessing.py:266-285 (oligo-dT demultiplexing): sliding Levenshtein
 * distance of seq against every index (file order, idx_off[n_idx+1] into idx_cat); returns the winning index number or
 * -1 for '-'.  Host code. */
int c3_match_index(const char* seq, int n, int n_idx, const char* idx_cat, const int64_t* idx_off);

/* Sample demultiplexer (paper/Demultiplex_R2C2_reads.py, demultiplex): per read and per index set (A = Nextera,
 * B = TSO), the minimum Levenshtein distance of every index (length m) to head[i : i+m] for i in 0 .. 299-m (the window
 * at 300-m is not searched); sets are decided separately: stable sort by distance, the first index wins when its
 * distance is < 4 and the runner-up's is more than 1 further away.  Byte-exact (case-sensitive, N matches only N).
 *   heads: n slots of C3_DEMUX_HEAD bytes (the first 300 bases of reads longer than 300; shorter reads are not searched)
 *   set A: n_a indexes, a_off[n_a+1] into a_cat; set B likewise.  2 .. C3_DEMUX_MAX_IDX indexes per set, each of
 *          0 .. C3_DEMUX_MAX_LEN bytes (an empty index has distance 0), at most C3_DEMUX_MAX_BYTES distinct bytes over
 *          both sets; otherwise C3_E_LIMIT / C3_E_ARG with a c3_last_error text
 *   win[2n]: (A, B) winning index number per read (file order within the set) or -1
 *   dist[n * (n_a + n_b)]: minimum distances, A's columns then B's, or NULL to skip
 * c3_demux_indexes runs on the handle's device (k_demux); c3_demux_host is its host statement (textbook DP over every
 * window) and reports its error text through c3_last_error(NULL). */
#define C3_DEMUX_HEAD 300
#define C3_DEMUX_MAX_IDX 128
#define C3_DEMUX_MAX_LEN 32
#define C3_DEMUX_MAX_BYTES 31
int c3_demux_indexes(c3_handle* h, int n, const char* heads, int n_a, const char* a_cat, const int64_t* a_off,
                     int n_b, const char* b_cat, const int64_t* b_off, int32_t* win, uint8_t* dist);
int c3_demux_host(int n, const char* heads, int n_a, const char* a_cat, const int64_t* a_off,
                  int n_b, const char* b_cat, const int64_t* b_off, int32_t* win, uint8_t* dist);

/* ---- per-base consensus quality values (opt-in; the reference writes FASTA only) ----
 * Every consensus base C[j] gets a SUPPORT score from the pieces the polish used, realigned to the consensus:
 *   kept subread k < n_sub     read[sub_beg[k]:sub_end[k]]  mode 0 (global: whole piece against whole C)
 *   tail piece (has_tail)      read[tail_beg:L]             mode 1 (anchored at start: begins at C[0] / piece[0], ends at the best cell)
 *   front piece (has_front)    read[0:front_end]            mode 2 (anchored at end: mode 1 on both sequences reversed, mapped back)
 * Alignment: piece rows i = 0..m against C columns j = 0..n, 2-bit codes (c3poa.h conventions), linear scores match
 * +C3_QV_MATCH, mismatch C3_QV_MISMATCH, gap C3_QV_GAP, H maximised, H[0][0] = 0.  Only C3_QV_BAND cells per row exist:
 * c(i) - 64 <= j <= c(i) + 63 with c(i) = floor((i*n + floor(m/2)) / m) in mode 0 and c(i) = i in modes 1 / 2.  The end
 * cell is (m, n) in mode 0, else the band cell of largest H (smallest i, then smallest j).  Traceback priority: diagonal,
 * deletion (consumes C[j-1]), insertion.  With q(b) = Phred byte - 33 clamped to 0..93, each piece adds to S[j] of the
 * columns it covers (all in mode 0, else the consumed ones): +q(b) for a matching diagonal, -q(b) for a mismatching one,
 * -q(last piece base consumed before it, else piece[0]) for a deletion, -max q of every maximal insertion run to the column
 * after it (or to the last covered column).  QV[j] = min(C3_QV_MAX, max(0, S[j])), written as QV + 33; uncovered columns get 0.
 * A mode-0 pair with max(m, n) > C3_QV_SKEW * min(m, n) is not aligned.  These values measure SUPPORT: they are not calibrated
 * error probabilities.  DESIGN.md "Consensus quality values" has the full statement. */
#define C3_STAGE_QV 16            /* c3_batch_run(h, C3_STAGES_ALL | C3_STAGE_QV): k_qv after the polish (C3_STAGES_ALL stays 15) */
#define C3_QV_BAND 128            /* band cells per DP row */
#define C3_QV_MAX 60              /* QV clamp */
#define C3_QV_MATCH 2
#define C3_QV_MISMATCH (-4)
#define C3_QV_GAP (-4)
#define C3_QV_SKEW 4              /* mode-0 pairs beyond this length ratio are refused (stand-alone) / skipped (batch) */
#define C3_QV_MAX_PIECES 252      /* C3_MAX_SUB subreads + the two dangling pieces */
#define C3_QV_GLOBAL 0
#define C3_QV_ANCHOR_START 1
#define C3_QV_ANCHOR_END 2

/* kernel figures of the last c3_batch_run with C3_STAGE_QV (c3_timing is not extended: its size is part of the ABI) */
typedef struct {
  float ms_qv;               /* k_qv, hipEvents on the library's stream */
  int64_t n_reads;           /* reads given QVs (status OK, cons_len > 0) */
  int64_t n_pieces;          /* pieces aligned */
  int64_t n_skipped;         /* mode-0 pieces beyond the skew limit (cover no column) */
  int64_t band_cells;        /* C3_QV_BAND * DP rows computed, row 0 included */
  int64_t edge_hits;         /* pieces whose traceback touched an interior band edge (band adequacy diagnostic, not an error) */
} c3_qv_timing;
int c3_batch_qv_timing(c3_handle* h, c3_qv_timing* t);

/* c3_batch_results + the QV bytes: qv[cons_off[i] ..] receives read i's QVs, same offsets and cap as cons.
 * _fetch_qv follows the rules of c3_batch_results_fetch (may overlap the next batch's run); c3_batch_results_qv = snapshot +
 * fetch_qv.  C3_E_STATE when the resident batch (at snapshot time) did not run C3_STAGE_QV. */
int c3_batch_results_fetch_qv(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv);
int c3_batch_results_qv(c3_handle* h, c3_read_result* res, char* cons, int64_t cons_cap, int64_t* cons_off, char* qv);

/* stand-alone QVs of one consensus cons[0..n) from n_pieces pieces (seq_cat / qual_cat, piece_off[n_pieces+1], modes[k] =
 * C3_QV_GLOBAL / _ANCHOR_START / _ANCHOR_END); qv_out[n] receives Phred+33 bytes.  c3_consensus_qv runs k_qv on the
 * handle's device; c3_consensus_qv_host is its host statement (full band DP per piece), errors through c3_last_error(NULL).
 * Both refuse an empty consensus, an empty piece, more than C3_QV_MAX_PIECES pieces, an unknown mode and a mode-0 pair beyond
 * the skew limit. */
int c3_consensus_qv(c3_handle* h, const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat,
                    const int64_t* piece_off, const int32_t* modes, char* qv_out);
int c3_consensus_qv_host(const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat,
                         const int64_t* piece_off, const int32_t* modes, char* qv_out);

/* R2C2_Consensus.fastq: @<header>\n<cons>\n+\n<qv>\n for exactly the reads c3_write_group gives a FASTA record (same header,
 * same order), appended to fq_paths[splint_id[i]] with c3_write_group's per-file reservation and locking.  Host code. */
int c3_write_consensus_fastq(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                             const char* qv, const int16_t* splint_id, int n_splints, const char* const* fq_paths, int zero);

/* ---- BGZF output (--bgzf) ----
 * Text is cut into blocks of 65 280 bytes (the last one shorter); each block becomes one BGZF member holding one final
 * deflate block: dynamic Huffman with literals and end-of-block only (optimal length-limited codes), or a stored block
 * where that is not smaller.  Output = the members back to back (no EOF member; n = 0 gives no bytes).
 * c3_bgzf_compress runs k_bgzf on the device of a c3_bgzf (device buffers and a stream of its own; one per thread, not
 * thread-safe); c3_bgzf_compress_host is its host statement, byte for byte.  cap < c3_bgzf_bound(n) and null arguments
 * return C3_E_ARG before anything is launched.  Errors of the handle-free calls through c3_last_error(NULL). */
typedef struct c3_bgzf c3_bgzf;
int c3_bgzf_create(int device, c3_bgzf** out);
void c3_bgzf_destroy(c3_bgzf* z);
int64_t c3_bgzf_bound(int64_t n);
int c3_bgzf_compress(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len);
int c3_bgzf_compress_host(const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len);
/* ---- BGZF input (--inflate gpu) ----
 * replaces the zlib threads of the reader (mm.fastx_read on a .gz file, C3POa.py:201,239) for BGZF files.  A member is
 * accepted exactly when its raw deflate stream (all of RFC 1951, zlib's rules for code sets) ends inside the payload,
 * yields ISIZE <= 65536 bytes and their CRC-32 is the trailer's; bytes after the stream's end are ignored.  Any other
 * member fails the whole call with C3_E_DATA and a c3_last_error(NULL) text naming the first bad member and the reason;
 * never a short or altered result.
 * c3_bgzf_scan walks the member headers of a buffer that holds whole members: count (empty members included) and total
 * ISIZE; C3_E_DATA when it is not BGZF.  c3_bgzf_decompress runs k_inflate on the device of a c3_bgzf;
 * c3_bgzf_decompress_host is its host statement (the same decoder, c3_inflate.h, on one CPU thread; no zlib).
 * cap < out_bytes, null arguments and a null handle return C3_E_ARG; n == 0 is success with out_len = 0. */
int c3_bgzf_scan(const char* src, int64_t n, int64_t* n_members, int64_t* out_bytes);
int c3_bgzf_decompress(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len);
int c3_bgzf_decompress_host(const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len);
/* ---- gzip input ----
 * A plain gzip file (RFC 1952: any header fields, members back to back, stored, fixed and dynamic blocks; no BC size field
 * needed) inflated in parallel: the compressed bytes are cut into pieces of C3_GUNZIP_PIECE bytes (environment, read at
 * every call; default 4 096, at least 64), every piece but the first looks for the first bit at which a dynamic-Huffman
 * block header parses and decodes from there into 16-bit symbols (a byte, or 0x8000 | p = byte p of the unknown 32 KiB in
 * front of it), a piece is accepted exactly when the accepted piece before it stopped at its first bit, the 32 KiB windows
 * go down the chain, and the symbols become bytes.  A wrong guess costs time, never a byte: where the chain breaks one
 * piece is decoded again from the true position (at most 16 times per stretch of 32 MiB; past that, and in a stretch
 * without any candidate, the rest of the stretch is decoded serially on the host; both are counted).  The output is what
 * zlib delivers, member after member; CRC-32 and ISIZE of every member are compared.  Damage is C3_E_DATA with a
 * c3_last_error(NULL) text naming the member, its file offset and the reason; never a short or altered result.
 * c3_gunzip runs the k_gunzip kernels on the device of a c3_bgzf with the whole file in memory; c3_gunzip_host is its host
 * statement (the same procedure and decoder by plain loops on one CPU thread, no zlib; piece > 0 overrides the
 * environment).  Null arguments, a null handle and a cap below the inflated size return C3_E_ARG -- before anything is
 * launched where the last member's ISIZE already shows it, otherwise when the stretch that would cross cap is reached;
 * n == 0 is success with out_len = 0.  (The early answer trusts the file's last four bytes: a file whose only damage is an
 * ISIZE above cap gets C3_E_ARG, and C3_E_DATA once cap has grown past it.)
 * c3_gunzip_stats: the first n of the calling thread's counters of its last c3_gunzip / c3_gunzip_host call, in this
 * order: pieces, pieces with a candidate, candidates accepted, candidates rejected (accepted + rejected = candidates),
 * relaunches, full slabs, bytes inflated by the serial fallback, stretches. */
int c3_gunzip(c3_bgzf* z, const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len);
int c3_gunzip_host(const char* src, int64_t n, char* dst, int64_t cap, int64_t* out_len, int64_t piece);
int c3_gunzip_stats(int64_t* v, int n);
/* c3_reader_open, but a BGZF file's stretches are inflated by k_inflate on `device` (a c3_bgzf owned by the reader)
 * instead of zlib threads; a file that is not BGZF (plain gzip, plain text) is read exactly as c3_reader_open reads it.
 * C3_E_NO_DEVICE without a usable GPU: asking for the device never falls back to zlib. */
int c3_reader_open_inflate(const char* path, int n_sets, int device, c3_reader** out);
/* c3_reader_gunzip_on_device(r, 1): a plain gzip file (not BGZF) opened by c3_reader_open_inflate is inflated by the k_gunzip
 * kernels on that device instead of gzread: the file is read and inflated stretch by stretch (C3_GUNZIP_PIECE and the other
 * variables are read here), the next stretch on a thread of its own while the parser works, and the groups are the ones the
 * plain reader delivers.  With it c3_reader_parse_on_device and c3_reader_stage_on_device are valid on such a reader too: the
 * inflated text stays on the device for k_fastq, departures as on BGZF.  c3_reader_inflate_wait counts for it.  Damage fails
 * c3_reader_next with C3_E_DATA and c3_gunzip's text.  Before the first group, and not taken back; anything else is
 * C3_E_STATE with a text.  Without the call every reader is as before.  c3_reader_gunzip_stats: the counters of
 * c3_gunzip_stats summed over the stretches inflated so far. */
int c3_reader_gunzip_on_device(c3_reader* r, int on);
int c3_reader_gunzip_stats(const c3_reader* r, int64_t* v, int n);
/* seconds the parser has waited for inflated bytes of a BGZF file so far, with either inflater (C3_STREAM_STATS); 0 for other files */
double c3_reader_inflate_wait(const c3_reader* r);
/* c3_write_group / c3_write_consensus_fastq with each file's text of the call (all records, in record order) compressed
 * through z and appended (compressed size reserved as in c3_write_group) to the paths, which name the .gz files.  The
 * caller appends the 28-byte BGZF EOF member once the last writer of a file is done. */
int c3_write_group_bgzf(c3_bgzf* z, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                        const int16_t* splint_id, int n_splints, const char* const* cons_paths, const char* const* sub_paths, int zero);
int c3_write_consensus_fastq_bgzf(c3_bgzf* z, const c3_host_batch* b, const c3_read_result* res, const char* cons,
                                  const int64_t* cons_off, const char* qv, const int16_t* splint_id, int n_splints,
                                  const char* const* fq_paths, int zero);

/* ---- FASTQ records on the GPU (--parse gpu) ----
 * A text is STRICT when, from its first byte, it is a sequence of records of exactly four lines: line 0 begins with '@';
 * line 1 is not empty and does not begin with '@', '>' or '+'; line 2 begins with '+'; line 3 is as long as line 1.  A line
 * ends at '\n'; one '\r' directly before it is not part of the line (all four lines).  The name is line 0 after the '@', up
 * to the first blank or tab (what c3_reader_next_set does).  With at_eof != 0 the last line of the last record may lack its
 * '\n' (a '\r' at its end is dropped all the same).
 * The call parses the longest prefix of whole strict records: info->consumed is its byte length.  A record that is merely
 * incomplete at the end of the text (at_eof == 0) is left unconsumed; that is no error.  The first record that is not
 * strict is a DEPARTURE (a blank line, a FASTA record, multi-line sequence or quality, unequal lengths, a missing '+', an
 * incomplete record with at_eof set): parsing stops in front of it, consumed ends there, departed = 1, and the records
 * before it are delivered as usual.  Records with a sequence shorter than min_len are counted in n_short and not stored;
 * n_records = n_kept + n_short.  names / name_off[n_kept + 1], seqs / quals / off[n_kept + 1] of the kept records mean what
 * they mean in c3_host_batch.
 * c3_fastq_parse runs k_fastq on the device of a c3_bgzf; c3_fastq_parse_host is its host statement.  n_kept > max_records,
 * name_bytes > names_cap or base_bytes > bases_cap return C3_E_LIMIT with the needed sizes in info and nothing written to
 * the arrays; n > C3_FASTQ_MAX_TEXT returns C3_E_LIMIT (line positions are 32-bit on the device); null arguments and a null
 * handle return C3_E_ARG before anything is launched (text may be null when n == 0); n == 0 is success with all counts
 * zero.  Errors through c3_last_error(NULL). */
#define C3_FASTQ_MAX_TEXT 0x7FF00000
typedef struct { int64_t n_records, n_kept, n_short, consumed, name_bytes, base_bytes; int32_t departed; } c3_fastq_info;
int c3_fastq_parse(c3_bgzf* z, const char* text, int64_t n, int at_eof, int min_len,
                   char* names, int64_t names_cap, int64_t* name_off, char* seqs, char* quals, int64_t bases_cap,
                   int64_t* off, int64_t max_records, c3_fastq_info* info);
int c3_fastq_parse_host(const char* text, int64_t n, int at_eof, int min_len,
                        char* names, int64_t names_cap, int64_t* name_off, char* seqs, char* quals, int64_t bases_cap,
                        int64_t* off, int64_t max_records, c3_fastq_info* info);
/* on != 0: a reader opened by c3_reader_open_inflate on a BGZF file keeps every inflated stretch on the device, parses it
 * there (k_fastq) and copies only the finished names / bases / qualities of each group into its buffer sets; the groups are
 * the ones the host parser delivers.  From the first departure on the rest of the file is parsed on the host (the existing
 * parser, so multi-line records, blank lines, FASTA records and every error text are as ever).  C3_E_STATE on any other
 * reader and after the first c3_reader_next.  Environment: C3_INFLATE_STRETCH_MEMBERS = BGZF members per device stretch
 * (default 4096; read when the reader is opened). */
int c3_reader_parse_on_device(c3_reader* r, int on);
/* stretches parsed on the device / on the host since c3_reader_parse_on_device(r, 1), and records that entered groups (or
 * were counted short) from the device: proof that the device path ran and nothing fell back silently */
int c3_reader_parse_stats(const c3_reader* r, int64_t* stretches_device, int64_t* stretches_host, int64_t* records_device);

/* ---- Unaligned BAM records on the GPU (-r reads.bam) ----
 * The inflated bytes of a BAM file: the file header (magic "BAM\1", l_text, the text, n_ref, per reference l_name, name, l_ref;
 * skipped, not interpreted; a wrong magic, a negative length or n_ref > C3_BAM_MAX_REFS is a departure, reason HEADER; a
 * header whose n_ref exceeds an eighth of the bytes behind it cannot end inside the data and is incomplete), then records.  All fields are
 * little-endian.  The record at byte p: block_size (u32) at +0, l_read_name (u8) at +12, n_cigar_op (u16) at +16, flag (u16)
 * at +18, l_seq (u32) at +20, read_name at +36, then 4 * n_cigar_op cigar bytes, (l_seq + 1) / 2 packed bases, l_seq
 * qualities, and tags up to p + 4 + block_size, where the next record begins (the rule is c3poa_amd/csrc/c3_bam.h).
 * A record is STRICT when none of these holds; they are tested in this order and the first that holds is the reason (the
 * values of c3_bam_info.reason, 0 = none):
 *   1 BLOCK   block_size outside [34, C3_BAM_MAX_RECORD]
 *   2 NAME    l_read_name == 0, or read_name[l_read_name - 1] != 0 (looked at where that byte lies inside the record)
 *   3 FIELDS  32 + l_read_name + 4 * n_cigar_op + (l_seq + 1) / 2 + l_seq > block_size (in 64 bits)
 *   4 FLAG    flag & (0x10 | 0x100 | 0x800): a reverse-strand, secondary or supplementary record; such a file is aligned
 *             (convert it with samtools fastq)
 *   5 EMPTY   l_seq == 0
 *   6 NOQUAL  qual[0] == 0xFF
 * n_cigar_op > 0 and every other flag bit are accepted and ignored; tags are skipped.  Delivered: the name = read_name up to
 * the first NUL, blank or tab (the cut of the FASTQ rule); the bases "=ACMGRSVTWYHKDBN"[code], high nibble first; the
 * qualities min(q, 93) + 33.
 * The call parses the longest prefix of whole strict records: info->consumed is its byte length.  With at_start != 0 the
 * data begins with the file header, which is consumed first and reported in header_bytes; a header that is merely incomplete
 * gives consumed = 0 and is no error.  A record that does not end inside the data is left unconsumed; that is no error
 * unless at_eof != 0, which makes it (and an incomplete header) a departure with reason 7, TRUNCATED.  The first record that
 * is not strict is a DEPARTURE: parsing stops in front of it, consumed ends there, departed = 1, reason and bad_at (its byte
 * offset in data) are set, and the records before it are delivered as usual (reason 8, HEADER: bad_at = 0, nothing
 * delivered).  Records with fewer than min_len bases are counted in n_short and not stored; n_records = n_kept + n_short.
 * names / name_off[n_kept + 1], seqs / quals / off[n_kept + 1] of the kept records mean what they mean in c3_host_batch.
 * c3_bam_parse runs k_bam on the device of a c3_bgzf; c3_bam_parse_host is its host statement.  n_kept > max_records,
 * name_bytes > names_cap or base_bytes > bases_cap return C3_E_LIMIT with the needed sizes in info and nothing written to
 * the arrays; n > C3_FASTQ_MAX_TEXT returns C3_E_LIMIT (positions are 32-bit on the device); null arguments and a null handle
 * return C3_E_ARG before anything is launched (data may be null when n == 0); n == 0 is success with all counts zero.
 * Errors through c3_last_error(NULL).
 * The reader: c3_reader_open / c3_reader_open_inflate on a path ending in ".bam" read it as BGZF (C3_NO_BGZF is not looked at;
 * a .bam that is not BGZF fails at the first c3_reader_next with a text) and form the groups of the group rule from these
 * records; c3_reader_parse_on_device and c3_reader_stage_on_device are valid on such a reader (k_bam in place of k_fastq).
 * A departure is an error of c3_reader_next on either path, BAM has no second parser: the c3_reader_error text names the
 * record's index, its inflated byte offset and the reason.  The call that meets it returns the error at once: the groups of
 * the earlier calls were delivered, the records that this call had collected in front of the departure are not (unlike
 * c3_bam_parse, which delivers the records before it).  c3_reader_noqual stays 0; c3_reader_open_range refuses ".bam"
 * with C3_E_ARG. */
#define C3_BAM_TILE 65536            /* bytes of data per chain tile on the device (the tests place records against it) */
#define C3_BAM_MAX_RECORD (1 << 28)
#define C3_BAM_MAX_REFS (1 << 20)    /* references in the file header (an unaligned BAM has none) */
typedef struct { int64_t n_records, n_kept, n_short, consumed, name_bytes, base_bytes, header_bytes, bad_at;
                 int32_t departed, reason; } c3_bam_info;
int c3_bam_parse(c3_bgzf* z, const char* data, int64_t n, int at_start, int at_eof, int min_len,
                 char* names, int64_t names_cap, int64_t* name_off, char* seqs, char* quals, int64_t bases_cap,
                 int64_t* off, int64_t max_records, c3_bam_info* info);
int c3_bam_parse_host(const char* data, int64_t n, int at_start, int at_eof, int min_len,
                      char* names, int64_t names_cap, int64_t* name_off, char* seqs, char* quals, int64_t bases_cap,
                      int64_t* off, int64_t max_records, c3_bam_info* info);

/* ---- Post-processing on the GPU (C3POa_postprocessing.py --emit gpu) ----
 * One batch of consensus reads and its adapter table in, finished file bytes out: classification (parse_blat), trimming,
 * orientation, oligo-dT demultiplexing and record formatting of write_fasta_file (C3POa_postprocessing.py:238-398), and the
 * PSL text find_adapters_gpu writes.  The per-read rule is c3poa_amd/csrc/c3_post.h.
 *   names / name_off[n+1], seqs / off[n+1]: as in c3_host_batch; quals (same offsets) or NULL.  With quals the main, left and
 *       right records are FASTQ (@name_len, SEQ, +, QUAL; QUAL reversed wherever SEQ is reverse-complemented)
 *   table[n][n_ad][2][12]: as c3_scan_adapters returns it; taken as data, whatever its values
 *   ad_len[n_ad]; ad_class[n_ad] >= 0: equal names share a class; class5 = class of "5Prime_adapter" or -1; ad_names /
 *       ad_name_off[n_ad+1]: the names for the PSL rows
 *   has_index: an index set is given (-x); idx_cat / idx_off[n_idx+1]: its distinct sequences in file order (at most 16 of at
 *       most 32 bases, else C3_E_LIMIT); idx_dest[n_idx]: destination of each (same name = same destination); n_dest
 *       destinations, no_index_found being the last (n_dest = 1 without an index set)
 * Output: S = 3 * n_dest + 3 streams back to back in arena, stream s at [stream_off[s], stream_off[s+1]): per destination d
 * main, left, right = 3d, 3d+1, 3d+2; then the 10x file, the oligo-dT TSV, the PSL.  Records within a stream are in input
 * order.  *n_kept = reads written.  When the streams need more than cap bytes: C3_E_LIMIT, stream_off is filled all the same
 * (stream_off[S] = bytes needed) and the arena is left alone.  The total of seqs must stay below 2^31 bytes (C3_E_LIMIT).
 * c3_post_emit runs k_post on the handle's device; c3_post_emit_host is its host statement, byte for byte (errors through
 * c3_last_error(NULL)). */
typedef struct c3_post_args {
  int32_t n;
  const char* names; const int64_t* name_off;
  const char* seqs; const char* quals; const int64_t* off;
  const int32_t* table;
  int32_t n_ad; const int32_t* ad_len; const int32_t* ad_class; int32_t class5;
  const char* ad_names; const int64_t* ad_name_off;
  int32_t has_index, n_idx; const char* idx_cat; const int64_t* idx_off; const int32_t* idx_dest; int32_t n_dest;
  int32_t undirectional, trim, barcoded;
} c3_post_args;
/* kernel time of the last c3_post_emit on the handle (hipEvents on its stream) and of the call with its copies */
typedef struct { float ms_classify, ms_scan, ms_emit, ms_call; int64_t n_reads, n_kept, in_bytes, out_bytes; } c3_post_timing;
int c3_post_emit(c3_handle* h, const c3_post_args* a, char* arena, int64_t cap, int64_t* stream_off, int64_t* n_kept);
int c3_post_emit_host(const c3_post_args* a, char* arena, int64_t cap, int64_t* stream_off, int64_t* n_kept);
int c3_post_emit_timing(c3_handle* h, c3_post_timing* t);

/* ---- Sample demultiplexer, text in / file bytes out (C3POa_demux.py --emit gpu) ----
 * FASTA text as read_fasta of paper/Demultiplex_R2C2_reads.py reads it, for ASCII bytes (the rule is c3poa_amd/csrc/c3_fasta.h):
 * a line ends at every '\n' and every '\r' (the last line may lack one); the bytes 9..13 and 28..32 are stripped at its end,
 * nothing at its front; a stripped-empty line is ignored; a line whose first byte is '>' opens a record, its name being
 * everything behind the '>' (may be empty); every other line is appended, stripped, to the sequence of the open record (which
 * may stay empty).
 * With at_eof == 0 the last record of the text is left unconsumed (its sequence may continue): info->consumed is the offset of
 * the last header line's first byte, 0 when the text holds no header; with at_eof != 0 everything is consumed.  A text starts
 * at the start of the file or at a header line.  DEPARTURES deliver only the records that lie wholly in front of the first
 * offending byte, with consumed at the header line of the first record not delivered: departed = 1, a byte >= 0x80;
 * departed = 2, a non-blank sequence line in front of the first header (nothing delivered, consumed = 0).
 * c3_fasta_parse delivers every record: names / name_off[n_records + 1], seqs / off[n_records + 1] as in c3_host_batch, and
 * name_hash[n_records], the 64-bit FNV-1a hash of each name.  It runs k_fasta on the handle's device; c3_fasta_parse_host is
 * its host statement.  n_records > max_records, name_bytes > names_cap or base_bytes > bases_cap return C3_E_LIMIT with the
 * needed sizes in info and nothing written; n > C3_FASTA_MAX_TEXT returns C3_E_LIMIT; null arguments and a null handle return
 * C3_E_ARG (text may be null when n == 0); n == 0 is success with all counts zero.
 * c3_demux_emit runs parse -> heads -> k_demux -> format on the device and returns the bytes of Indexed_reads.fasta for the
 * delivered records in out: per record with more than C3_DEMUX_HEAD sequence bytes, in input order,
 * '>' name '|' A '_' B '\n' sequence '\n', A / B being the name of the winning index of each set (c3_demux_indexes) or empty;
 * shorter records are dropped.  Index sets as in c3_demux_indexes (same limits, same error texts), their names as
 * a_names / a_name_off[n_a + 1] and b_names / b_name_off[n_b + 1].  name_hash[n_records] as above, for every delivered record,
 * kept or not.  out_bytes > cap returns C3_E_LIMIT with info->out_bytes = the need and out left alone; n_records > max_records
 * likewise.  c3_demux_emit_host is the host statement, byte for byte.  Errors of the host statements through
 * c3_last_error(NULL). */
#define C3_FASTA_MAX_TEXT 0x7FF00000
typedef struct { int64_t n_records, consumed, name_bytes, base_bytes; int32_t departed; } c3_fasta_info;
typedef struct { int64_t n_records, n_kept, consumed, out_bytes; int32_t departed; } c3_demux_info;
int c3_fasta_parse(c3_handle* h, const char* text, int64_t n, int at_eof, char* names, int64_t names_cap, int64_t* name_off,
                   char* seqs, int64_t bases_cap, int64_t* off, uint64_t* name_hash, int64_t max_records, c3_fasta_info* info);
int c3_fasta_parse_host(const char* text, int64_t n, int at_eof, char* names, int64_t names_cap, int64_t* name_off,
                        char* seqs, int64_t bases_cap, int64_t* off, uint64_t* name_hash, int64_t max_records, c3_fasta_info* info);
int c3_demux_emit(c3_handle* h, const char* text, int64_t n, int at_eof,
                  int n_a, const char* a_cat, const int64_t* a_off, const char* a_names, const int64_t* a_name_off,
                  int n_b, const char* b_cat, const int64_t* b_off, const char* b_names, const int64_t* b_name_off,
                  char* out, int64_t cap, uint64_t* name_hash, int64_t max_records, c3_demux_info* info);
int c3_demux_emit_host(const char* text, int64_t n, int at_eof,
                       int n_a, const char* a_cat, const int64_t* a_off, const char* a_names, const int64_t* a_name_off,
                       int n_b, const char* b_cat, const int64_t* b_off, const char* b_names, const int64_t* b_name_off,
                       char* out, int64_t cap, uint64_t* name_hash, int64_t max_records, c3_demux_info* info);
/* kernel times of the last c3_demux_emit on the handle (hipEvents on its stream) and of the call with its copies */
typedef struct { float ms_parse, ms_demux, ms_emit, ms_call; int64_t n_records, n_kept, in_bytes, out_bytes; } c3_demux_timing;
int c3_demux_emit_timing(c3_handle* h, c3_demux_timing* t);

/* ---- Records formatted on the GPU (C3POa.py --emit gpu) ----
 * The file bytes of c3_write_group (and of c3_write_consensus_fastq when qv is given) for one group, as streams in one arena
 * instead of appended to files.  The per-read rule is c3poa_amd/csrc/c3_emit.h (emit_of and the record order of the writer, the
 * average-quality text by integer arithmetic).  b / res / cons / cons_off / qv / splint_id / n_splints / zero mean what they
 * mean in c3_write_group and c3_write_consensus_fastq; cons may be NULL (no consensus records), qv needs cons.
 * Output: K kinds per splint, K = 2 without qv (consensus FASTA, subread FASTQ), K = 3 with it (+ consensus FASTQ); stream
 * s * K + kind at [stream_off[x], stream_off[x + 1]), x = 0 .. n_splints * K - 1; records within a stream are in read order.
 * *n_records = records written over all streams.  When the streams need more than cap bytes: C3_E_LIMIT, stream_off is filled
 * all the same (stream_off[n_splints * K] = bytes needed) and the arena is left alone.
 * Every record is validated before anything is formatted (on the host, before any launch): offsets ascending from 0 (a
 * group may hold any number of bytes; one read, name or consensus must stay below 2^31: C3_E_LIMIT), and for each read that writes something n_sub in 0 .. 250, 0 <= sub_beg <= sub_end <= L for its kept
 * subreads, front_end / tail_beg of the pieces it writes inside the read, L > 0 where a consensus record is due; otherwise
 * C3_E_ARG with a text naming the read.  More than 64 splints: C3_E_LIMIT.
 * c3_emit_group uploads its arguments, runs k_emit on the handle's device and copies the arena down; c3_emit_group_host is
 * its host statement, byte for byte (errors through c3_last_error(NULL)). */
#define C3_EMIT_BGZF 1            /* flags of c3_batch_emit_snapshot: the fetch delivers BGZF members instead of text */
int c3_emit_group(c3_handle* h, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                  const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                  int64_t* stream_off, int64_t* n_records);
int c3_emit_group_host(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                       const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                       int64_t* stream_off, int64_t* n_records);
/* The same for the RESIDENT batch, in two halves like c3_batch_results_snapshot / _fetch, so that the finished bytes leave the
 * device beside the next batch's kernels and the host formats nothing.
 * c3_batch_emit_snapshot (owner thread, after c3_batch_run with C3_STAGE_POLISH, before the next c3_batch_commit) uploads the
 * names of the resident batch (name_off[n + 1] from 0), formats its records from the resident buffers (splint ids as uploaded,
 * n_splints = rows of c3_set_splints; K = 3 when the batch ran C3_STAGE_QV) into a grow-only device arena of its own and
 * records an event.  It does not replace the results snapshot.  One emit snapshot per handle: a second one before the fetch
 * returns C3_E_STATE, as does a fetch without a snapshot.
 * c3_batch_emit_fetch copies the streams into arena / stream_off[n_splints * K + 1] on the handle's download stream and returns
 * when they have landed; it touches nothing but the emit snapshot and may run on another thread beside the owner's next
 * c3_batch_commit / c3_batch_run (it does not set c3_last_error).  cap too small: C3_E_LIMIT with stream_off filled
 * (stream_off[n_splints * K] = bytes needed) and THE SNAPSHOT KEPT, so the caller can fetch again with a larger arena.
 * With C3_EMIT_BGZF set at snapshot time every non-empty stream is compressed by k_bgzf before it leaves the device (as one
 * text, exactly the members c3_write_group_bgzf / c3_write_consensus_fastq_bgzf append for the same group); stream_off then
 * describes the compressed streams, and the bytes needed are the sum of c3_bgzf_bound over the streams. */
int c3_batch_emit_snapshot(c3_handle* h, const char* names, const int64_t* name_off, int zero, int flags);
int c3_batch_emit_fetch(c3_handle* h, char* arena, int64_t cap, int64_t* stream_off);
/* kernel times (hipEvents) of the last c3_emit_group, or of the snapshot that the last c3_batch_emit_fetch delivered: k_emit_len,
 * the scans, k_emit_write, k_bgzf inside the fetch (host time of the compression loop), host time of the call(s) with their
 * copies; bytes read (names, bases, qualities, consensus) and bytes delivered.  Ask on the thread that made that call. */
typedef struct { float ms_len, ms_scan, ms_write, ms_bgzf, ms_call; int64_t n_reads, n_records, in_bytes, out_bytes; } c3_emit_timing;
int c3_emit_timing_get(c3_handle* h, c3_emit_timing* t);
/* Appends stream x (arena + stream_off[x], stream_off[x + 1] - stream_off[x] bytes) to paths[x] for every non-empty stream
 * whose path is not NULL, with c3_write_group's per-file reservation and locking (several workers may share the files).
 * A file that cannot be opened or written fails the call with the writers' code for that, C3_E_ARG, and a c3_last_error(NULL)
 * text naming the path and the system's reason.  Host code. */
int c3_append_streams(const char* const* paths, const char* arena, const int64_t* stream_off, int n_streams);

/* ---- Records written as unaligned BAM (C3POa.py --emit gpu --bam) ----
 * The records of "Records formatted on the GPU" as BAM records instead of text.  Which reads write which records, in which
 * order and from which slice is the same rule (c3poa_amd/csrc/c3_emit.h); what a record is made of is
 * c3poa_amd/csrc/c3_bamout.h.  K = 2 kinds per splint whatever qv is: stream s * 2 + kind, kind 0 = consensus records, kind 1 =
 * subread records, records within a stream in read order.  One record, every field little-endian and none aligned:
 *   block_size (bytes behind it), refID -1, pos -1, l_read_name (name bytes + the NUL), mapq 0, bin 4680, n_cigar_op 0, flag 4,
 *   l_seq, next_refID -1, next_pos -1, tlen 0, read_name NUL, seq ((l_seq + 1) / 2 bytes, high nibble first, an unused low
 *   nibble 0), qual (l_seq bytes), tags (consensus records only).
 * A subread record is named <name>_<idx> (the FASTQ record's text between '@' and the newline), holds the bases and qualities of
 * its piece and no tags; a piece of 0 bases is a record with l_seq = 0.  A consensus record is named
 * <name>_<avgQ>_<L>_<ns>_<clen> (the FASTA header's text), holds the consensus, the QV bytes as qualities when qv is given and
 * l_seq bytes of 0xFF when not, and three tags in this order: np:i = ns as the name prints it, rl:i = L, aq:f =
 * (float)((double)tot / (double)L) with the tot the name's avgQ is made from.  A base is stored as its index in
 * "=ACMGRSVTWYHKDBN", a lower-case letter as its upper-case form, every other byte as 15; a quality byte b as
 * min(max(b - 33, 0), 93).
 * Limits, checked on the host before any launch, beside those of c3_emit_group: a read name of more than 219 bytes is
 * C3_E_LIMIT (254 name bytes fit a record; the longest suffix takes 35 of them; decided from the names alone, for every read of
 * the group), a name that holds a NUL is C3_E_ARG; both texts name the read.  Unaligned records only, no index, no @RG.
 * c3_emit_group_bam / c3_emit_group_bam_host deliver the UNCOMPRESSED record bytes per stream; arena, cap,
 * stream_off[n_splints * 2 + 1], n_records and C3_E_LIMIT with the bytes needed work as in c3_emit_group.  The host call is the
 * statement of the device call, byte for byte (errors through c3_last_error(NULL)).
 * c3_batch_emit_snapshot takes C3_EMIT_BAM in its flags: the streams of the fetch are then the two BAM kinds (K = 2), with the
 * QVs as consensus qualities when the batch ran C3_STAGE_QV; with C3_EMIT_BGZF beside it every non-empty stream is compressed by
 * k_bgzf as for text (a record may straddle two members).  The name limits are checked there as well.
 * c3_bam_out_header writes the file header: "BAM\1", l_text, the text
 * "@HD\tVN:1.6\tSO:unknown\n@PG\tID:c3poa_amd\tPN:c3poa_amd\tVN:<c3_version()>\n", n_ref = 0; *len = its bytes, C3_E_LIMIT with
 * *len set when cap is smaller.  A file is that header as BGZF member(s), the members of the record streams in any order of
 * arrival, and the BGZF EOF member.  Host code. */
#define C3_EMIT_BAM 2             /* c3_batch_emit_snapshot: BAM records instead of text; K = 2 */
int c3_emit_group_bam(c3_handle* h, const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                      const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                      int64_t* stream_off, int64_t* n_records);
int c3_emit_group_bam_host(const c3_host_batch* b, const c3_read_result* res, const char* cons, const int64_t* cons_off,
                           const char* qv, const int16_t* splint_id, int n_splints, int zero, char* arena, int64_t cap,
                           int64_t* stream_off, int64_t* n_records);
int c3_bam_out_header(char* dst, int64_t cap, int64_t* len);

/* ---- Strict FASTA / FASTQ records (the input of C3POa_postprocessing.py) ----
 * A text is STRICT of kind 4 (the four-line FASTQ rule of "FASTQ records on the GPU") or of kind 2, the two-line FASTA that
 * C3POa.py writes: line 0 begins with '>'; line 1 is not empty and does not begin with '>', '@' or '+'.  The kind of a file is
 * announced by its first byte ('@' = 4, '>' = 2; any other byte is a departure) and is an argument here.  Lines, the '\r' rule
 * and the name rule (line 0 after its first byte, up to the first blank or tab) are those of the FASTQ rule; with
 * at_eof != 0 the last line may lack its '\n'.  The rule is c3poa_amd/csrc/c3_fastx.h.
 * The call parses the longest prefix of whole strict records: info->consumed is its byte length, always a record boundary.
 * A record that is merely incomplete at the end of the text (at_eof == 0) is left unconsumed.  The first record that is not
 * strict is a DEPARTURE: a blank line, an empty sequence line, a record of the other kind, a byte >= 0x80 anywhere in the
 * record, an incomplete record with at_eof set, and a sequence of several lines (kind 2: the line behind the first sequence
 * line stands where a header is due, so the departure lies behind that record's first two lines).  Parsing stops in front of
 * it, departed = 1, and the records before it are delivered.  Every record is delivered (no minimum length):
 * names / name_off[n_records + 1], seqs / quals / off[n_records + 1] as in c3_host_batch (quals may be NULL for kind 2 and is
 * then not written; kind 4 needs it), name_hash[n_records] = the 64-bit FNV-1a of each name, as c3_fasta_parse gives it.
 * n_records > max_records, name_bytes > names_cap or base_bytes > bases_cap return C3_E_LIMIT with the needed sizes in info
 * and nothing written to the arrays; n > C3_FASTX_MAX_TEXT returns C3_E_LIMIT; null arguments and a kind other than 2 or 4
 * return C3_E_ARG (text may be null when n == 0); n == 0 is success with all counts zero.  Host code; errors through
 * c3_last_error(NULL). */
#define C3_FASTX_MAX_TEXT 0x7FF00000
typedef struct { int64_t n_records, consumed, name_bytes, base_bytes; int32_t departed; } c3_fastx_info;
int c3_fastx_strict_parse_host(const char* text, int64_t n, int at_eof, int kind, char* names, int64_t names_cap,
                               int64_t* name_off, char* seqs, char* quals, int64_t bases_cap, int64_t* off,
                               uint64_t* name_hash, int64_t max_records, c3_fastx_info* info);

/* ---- Post-processing, text in / file bytes out (C3POa_postprocessing.py --emit gpu --parse gpu) ----
 * c3_post_emit_text (C3POa_postprocessing.py:145,218-227,229-398): consecutive pieces of one consensus file in, the streams of
 * c3_post_emit out, with no text, base, adapter table or record visiting the host in between.  src holds plain text, or with
 * C3_POST_IN_BGZF whole BGZF members (inflated by k_inflate under the rules of "BGZF input": C3_E_DATA on a damaged member).
 * The handle keeps the unconsumed tail of the (inflated) text on the device and puts it in front of the next piece;
 * at_eof != 0 ends the file; c3_post_text_reset drops the tail and forgets the file's kind.  The kind (2 or 4) is the one the
 * file's first byte announces ("Strict FASTA / FASTQ records"); any other first byte is a departure.
 * The text is parsed by the strict rule (k_fastx), its bases packed for k_adapter where they lie, aligned against the rows of
 * c3_set_splints (which must equal plan->n_ad in number), classified, cut and formatted by k_post.  plan carries the adapter,
 * index and option fields of c3_post_args; its batch fields (n, names .. off) and table are ignored.  Qualities reach the
 * records only with C3_POST_KEEP_QUALS (kind 4; with kind 2: C3_E_ARG).
 * Output: the S = 3 * n_dest + 3 streams of c3_post_emit for the delivered records, stream_off[S + 1].  With C3_POST_OUT_BGZF
 * every non-empty stream among the 3 * n_dest read streams and the 10x stream is compressed by k_bgzf as one text (byte for
 * byte c3_bgzf_compress_host of that stream); the TSV and PSL streams stay plain; stream_off describes what is delivered.
 * Too small a cap: C3_E_LIMIT with stream_off filled (stream_off[S] = bytes needed; with C3_POST_OUT_BGZF the sum of
 * c3_bgzf_bound over the compressed streams plus the plain ones) and the arena left alone.  name_hash[n_records]: the 64-bit
 * FNV-1a of every delivered record's name; n_records > max_records: C3_E_LIMIT with info->n_records = the need.
 * info: n_records delivered, n_kept written, text_bytes = tail + (inflated) piece, consumed = how many of them the delivered
 * records cover, out_bytes, departed.  A departure delivers the records in front of it.  Whatever c3_batch_upload or
 * c3_post_emit would refuse for such a batch is refused here with the same code.  Every refusal happens before anything is
 * written to arena and leaves the kept tail as it was, so the same piece can be passed again.
 * c3_post_text_timing: times of the last call -- host time of the inflation and of the compression loop, hipEvent times of
 * the parse (with its two read-backs), gather + pack, k_adapter and k_post, host time of the call with its copies. */
#define C3_POST_IN_BGZF   1   /* src holds whole BGZF members; inflated on the device (k_inflate rules, C3_E_DATA on damage) */
#define C3_POST_OUT_BGZF  2   /* the read-file streams leave as BGZF members */
#define C3_POST_KEEP_QUALS 4  /* kind 4 only; kind 2 with it: C3_E_ARG */
typedef struct { int64_t n_records, n_kept, consumed, text_bytes, out_bytes; int32_t departed; } c3_post_text_info;
typedef struct { float ms_inflate, ms_parse, ms_gather, ms_adapter, ms_post, ms_bgzf, ms_call;
                 int64_t n_records, n_kept, in_bytes, text_bytes, out_bytes; } c3_post_text_timing;
int c3_post_emit_text(c3_handle* h, const char* src, int64_t n, int at_eof, int flags, const c3_post_args* plan,
                      char* arena, int64_t cap, int64_t* stream_off, uint64_t* name_hash, int64_t max_records,
                      c3_post_text_info* info);
int c3_post_text_reset(c3_handle* h);
int c3_post_text_timing_get(c3_handle* h, c3_post_text_timing* t);

/* ---- Sample demultiplexer, pieces of text in / per-sample streams out (C3POa_demux.py --parse gpu) ----
 * c3_demux_emit_text: consecutive pieces of one read file in, the renamed records out, with nothing visiting the host in
 * between.  src holds plain text, or with C3_DEMUX_IN_BGZF whole BGZF members (inflated by k_inflate under the rules of "BGZF
 * input": C3_E_DATA on a damaged member).  The handle keeps the unconsumed tail of the (inflated) text on the device and puts
 * it in front of the next piece; at_eof != 0 ends the file; c3_demux_text_reset drops the tail and forgets the file's kind.
 * The kind is the one the first byte of the text announces: '>' = 2, FASTA under the rule of c3_demux_emit (whole-line names,
 * wrapped sequences, the strip set, departures 1 and 2); '@' = 4, FASTQ under the strict four-line rule ("Strict FASTA /
 * FASTQ records": name = header up to the first blank or tab, departed = 1); any other first byte is a departure (departed = 1,
 * nothing consumed).  Every record with more than C3_DEMUX_HEAD sequence bytes is searched (c3_demux_indexes) and written as
 * '>' name '|' A '_' B '\n' sequence '\n', or with C3_DEMUX_KEEP_QUALS (kind 4 only; on kind 2: C3_E_ARG) as
 * '@' name '|' A '_' B '\n' sequence '\n' '+' '\n' quality '\n'.
 * Output: S streams in arena, stream s at [stream_off[s], stream_off[s + 1]).  S = 1 without C3_DEMUX_SPLIT: every record in
 * input order (for a FASTA text exactly the bytes of c3_demux_emit).  With C3_DEMUX_SPLIT S = (n_a + 1) * (n_b + 1) and a record
 * goes to stream a * (n_b + 1) + b, a = the winner of set A (n_a where there is none), b likewise; records keep their input
 * order within a stream.  S > C3_DEMUX_MAX_STREAMS: C3_E_LIMIT.  With C3_DEMUX_OUT_BGZF every non-empty stream is compressed
 * by k_bgzf as one text (byte for byte c3_bgzf_compress_host of that stream; no EOF member) and stream_off describes what is
 * delivered.  Too small a cap: C3_E_LIMIT with stream_off filled (stream_off[S] = bytes needed; with C3_DEMUX_OUT_BGZF the sum
 * of c3_bgzf_bound over the non-empty streams) and the arena left alone.  name_hash[n_records]: the 64-bit FNV-1a of every
 * delivered record's name, kept or not; n_records > max_records: C3_E_LIMIT with info->n_records = the need.
 * info: n_records delivered, n_kept written, text_bytes = tail + (inflated) piece, consumed = how many of them the delivered
 * records cover, out_bytes, departed, kind (0 while no byte was seen), n_streams = S.  A departure delivers the records in front
 * of it.  Every refusal happens before anything is written to arena and leaves the kept tail as it was, so the same piece can be
 * passed again.
 * c3_demux_emit_text_host is the host statement for ONE plain text of a stated kind (no tail, no inflation):
 * c3_fasta_parse_host or c3_fastx_strict_parse_host, then c3_demux_host, then the same streams, with C3_DEMUX_OUT_BGZF through
 * c3_bgzf_compress_host; C3_DEMUX_IN_BGZF and a kind other than 2 or 4 are C3_E_ARG.  Errors through c3_last_error(NULL).
 * c3_demux_text_timing_get: times of the last call -- host time of the inflation and of the compression loop, hipEvent times of
 * the parse (with its read-backs and the gather), k_demux (with the head copies), the placement (k_dsplit_key, _tile, _cols,
 * _offs) and k_dsplit_emit, host time of the call with its copies, and the number of stream waits of the call. */
#define C3_DEMUX_IN_BGZF 1
#define C3_DEMUX_OUT_BGZF 2
#define C3_DEMUX_KEEP_QUALS 4
#define C3_DEMUX_SPLIT 8
#define C3_DEMUX_MAX_STREAMS 4096
typedef struct {                  /* the ten index arguments of c3_demux_emit */
  int n_a; const char* a_cat; const int64_t* a_off; const char* a_names; const int64_t* a_name_off;
  int n_b; const char* b_cat; const int64_t* b_off; const char* b_names; const int64_t* b_name_off;
} c3_demux_sets;
typedef struct { int64_t n_records, n_kept, consumed, text_bytes, out_bytes; int32_t departed, kind, n_streams; } c3_demux_text_info;
typedef struct { float ms_inflate, ms_parse, ms_demux, ms_split, ms_emit, ms_bgzf, ms_call;
                 int64_t n_records, n_kept, in_bytes, text_bytes, out_bytes; int32_t n_streams, n_waits; } c3_demux_text_timing;
int c3_demux_emit_text(c3_handle* h, const char* src, int64_t n, int at_eof, int flags, const c3_demux_sets* sets,
                       char* arena, int64_t cap, int64_t* stream_off, uint64_t* name_hash, int64_t max_records,
                       c3_demux_text_info* info);
int c3_demux_emit_text_host(const char* text, int64_t n, int at_eof, int kind, int flags, const c3_demux_sets* sets,
                            char* arena, int64_t cap, int64_t* stream_off, uint64_t* name_hash, int64_t max_records,
                            c3_demux_text_info* info);
int c3_demux_text_reset(c3_handle* h);
int c3_demux_text_timing_get(c3_handle* h, c3_demux_text_timing* t);

/* ---- Groups kept on the device ----
 * With c3_reader_parse_on_device the bases and qualities of every read are gathered on the device, copied down into the
 * reader's page-locked sets, from where a caller that works on the device has to copy them straight back up.  These calls leave
 * them where they are and hand out device pointers.
 *
 * c3_reader_stage_on_device(r, on != 0): valid only on a reader with c3_reader_parse_on_device(r, 1) in force that has not
 * delivered its first group; otherwise C3_E_STATE with a c3_reader_error text (null reader: C3_E_ARG).  Such a reader keeps
 * one DEVICE buffer set per host set (owned, grow-only, on the reader's device, sized as the host sets are); the page-locked
 * seqs / quals blocks of its host sets are not allocated while its groups stay on the device (c3_reader_reserved_bytes counts
 * host memory only and shows that).  A DEVICE GROUP is formed by the group rule of c3_reader_next_set, unchanged; each run of
 * records that enters it is copied device to device into the set named by the call, at the group's fill offsets, and the
 * copies have landed when the call returns.  names, name_off, off, n and n_short come to the host as ever; seqs == quals ==
 * NULL in the c3_host_batch.  c3_reader_device_group(r, set, out) describes the group set `set` holds: d_seqs / d_quals
 * (off[] of the c3_host_batch indexes them), the device ordinal and bytes = off[n].  For a set that holds a host group, or none,
 * it returns C3_E_OK with d_seqs == d_quals == NULL, device = -1 and bytes = 0.  A set is overwritten only when the caller names
 * it again.
 * DEPARTURE (see "FASTQ records on the GPU"): a device group that meets the first record that is not strict ends in front of
 * it when it holds at least one record -- group boundaries may therefore differ from the host parser's there; the
 * concatenation of all groups does not.  When it holds none the same call goes on as an ordinary HOST GROUP (non-NULL seqs /
 * quals in the page-locked set), so n == 0 still means the end of the file.  From then on every group is
 * a host group.  The text that the last stretch leaves over at the end of the file (a record without its final newline) is
 * handed over in the same way.  names_only readers deliver no bases either way and are not affected.
 * c3_reader_stage_stats: groups (n > 0) delivered on the device / on the host since c3_reader_stage_on_device(r, 1), and the
 * bytes of bases and qualities that host groups brought to the host (0 while no departure occurred).
 * A caller reads a device group with kernels or copies of its own on the group's device; the group's set must stay unnamed
 * for as long as it does. */
typedef struct {
  const char* d_seqs;        /* device pointers; read i at [off[i], off[i + 1]) of both */
  const char* d_quals;
  int32_t device;            /* HIP device ordinal the group lies on */
  int64_t bytes;             /* bytes of each array = off[n] */
} c3_device_batch;
int c3_reader_stage_on_device(c3_reader* r, int on);
int c3_reader_device_group(const c3_reader* r, int set, c3_device_batch* out);
int c3_reader_stage_stats(const c3_reader* r, int64_t* groups_device, int64_t* groups_host, int64_t* host_bytes);

#ifdef __cplusplus
}
#endif
#endif

// c3_checks.h -- what the host statements (*.cpp, plain C++) and the HIP host units (c3_host.h) share: the handle-free error
// text, the argument checks that a device call and its host statement both apply, and the reader's private calls into the
// stream unit.  No hip_runtime.h here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/c3poa.h"

void c3_set_host_error(const char* msg);        // c3_handle.hip: the text of c3_last_error(NULL)

int c3_demux_prepare(int n_a, const char* a_cat, const int64_t* a_off, int n_b, const char* b_cat, const int64_t* b_off,
                     uint8_t* tab, int* n_codes, const char** msg);                                                  // c3_index.cpp
int c3_qv_check(const char* cons, int n, int n_pieces, const char* seq_cat, const char* qual_cat, const int64_t* piece_off,
                const int32_t* modes, const char* qv_out, const char** msg);                                          // c3_qv.cpp
int c3_fastq_check_args(const char* who, const char* text, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                        const char* seqs, const char* quals, int64_t bases_cap, const int64_t* off, int64_t max_records,
                        c3_fastq_info* info);                                                                         // c3_fastq.cpp
int c3_bam_check_args(const char* who, const char* data, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                      const char* seqs, const char* quals, int64_t bases_cap, const int64_t* off, int64_t max_records,
                      c3_bam_info* info);                                                                             // c3_bam.cpp
const char* c3_bam_reason_text(int reason);                                                                           // c3_bam.cpp
int c3_fasta_check_args(const char* who, const char* text, int64_t n, const char* names, int64_t names_cap, const int64_t* name_off,
                        const char* seqs, int64_t bases_cap, const int64_t* off, const uint64_t* name_hash, int64_t max_records,
                        c3_fasta_info* info);                                                                         // c3_fasta.cpp
int c3_demux_emit_check_args(const char* who, const char* text, int64_t n, int n_a, const char* a_names, const int64_t* a_name_off,
                             int n_b, const char* b_names, const int64_t* b_name_off, const char* out, int64_t cap,
                             const uint64_t* name_hash, int64_t max_records, c3_demux_info* info);                    // c3_fasta.cpp
int c3_demux_text_check_args(const char* who, const char* src, int64_t n, int flags, const c3_demux_sets* sets, const char* arena,
                             int64_t cap, const int64_t* stream_off, const uint64_t* name_hash, int64_t max_records,
                             c3_demux_text_info* info, int* S, uint8_t* tab, int* n_codes);                          // c3_dsplit.cpp
int c3_bgzf_data_error(const char* who, int64_t member, int st);                                                      // c3_inflate.cpp

// the reader's device stretches (c3_stream.hip, called by c3_reader.cpp and c3_reader_bgzf.cpp; not part of the public interface)
// (a BAM stretch fills the same table: info as for FASTQ, plus the reason and place of a departure and the file header's bytes)
struct c3_fq_stretch { c3_fastq_info info; const int64_t* off; const int64_t* name_off; int64_t text_bytes;
                       int32_t reason; int64_t bad_at, header_bytes; };
extern "C" int c3_bgzf_stretch_parse(c3_bgzf* z, int slot, const char* comp, int64_t ncomp, int64_t carry_from, int64_t carry_len,
                                     int at_eof, c3_fq_stretch* out);
// the same for the inflated bytes of a BAM file (k_bam): at_start != 0 while the file header has not been consumed
extern "C" int c3_bgzf_stretch_parse_bam(c3_bgzf* z, int slot, const char* comp, int64_t ncomp, int64_t carry_from, int64_t carry_len,
                                         int at_start, int at_eof, c3_fq_stretch* out);
extern "C" int c3_bgzf_stretch_fetch(c3_bgzf* z, int slot, int64_t r0, int64_t r1, char* names, char* seqs, char* quals);
extern "C" int c3_bgzf_stretch_text(c3_bgzf* z, int slot, int64_t from, int64_t len, char* dst);
// the reader's device buffer sets (c3_reader_stage_on_device): n_sets pairs of grow-only device buffers; _reserve grows set
// `set` to `bytes` per array keeping its first `keep`; _stretch_stage = _stretch_fetch with the bases and qualities copied
// device to device into the set at byte `at` instead of to the host; _set_get: the set's pointers and device
extern "C" int c3_bgzf_sets_create(c3_bgzf* z, int n_sets);
extern "C" int c3_bgzf_set_reserve(c3_bgzf* z, int set, int64_t bytes, int64_t keep);
extern "C" int c3_bgzf_stretch_stage(c3_bgzf* z, int slot, int64_t r0, int64_t r1, char* names, int set, int64_t at);
extern "C" int c3_bgzf_set_get(const c3_bgzf* z, int set, const char** d_seqs, const char** d_quals, int* device);
// the --bgzf writers' private call (c3_stream.hip, called by c3_writer.cpp): pieces p[0..np) compressed as one text
extern "C" int c3_bgzf_compress_pieces(c3_bgzf* z, const char* const* p, const int64_t* len, int np, char* dst, int64_t cap, int64_t* out_len);
// the reader's gzip stream (c3_gunzip_dev.hip, called by c3_reader_bgzf.cpp): a plain gzip file read and inflated stretch by
// stretch by the k_gunzip kernels on z's device.  _next: the stretch's bytes on the host; _next_parse: the stretch left on the
// device behind the carry in the slot's text and parsed there (c3_bgzf_stretch_parse's rule and tables).  *eof: the file ends
// behind this stretch.  Damage: C3_E_DATA, text in c3_last_error(NULL).  _stats: the counters of c3_gunzip_stats summed so far
struct c3_gunzip_stream;
extern "C" int c3_gunzip_stream_open(c3_bgzf* z, const char* path, c3_gunzip_stream** out);
extern "C" int c3_gunzip_stream_next(c3_gunzip_stream* s, const char** text, int64_t* bytes, int* eof);
extern "C" int c3_gunzip_stream_next_parse(c3_gunzip_stream* s, int slot, int64_t carry_from, int64_t carry_len, int* eof, int64_t* bytes, c3_fq_stretch* fq);
extern "C" void c3_gunzip_stream_stats(const c3_gunzip_stream* s, int64_t* v, int n);
extern "C" void c3_gunzip_stream_close(c3_gunzip_stream* s);

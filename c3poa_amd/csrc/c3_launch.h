// c3_launch.h -- the one declaration of every kernel launcher and kernel query.  The host units call through it, and every k_*.hip
// that defines a launcher includes it too, so a prototype that drifts from its definition fails to compile in the kernel's own
// translation unit.  Declarations only: the argument blocks are named, not defined (c3_args.h, c3_post.h, c3_inflate.h, c3_fastq.h, c3_bam.h, c3_fasta.h, c3_emit.h, c3_fastx.h, c3_dsplit.h, c3_gunzip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct ConkArgs; struct AdapterArgs; struct PostArgs; struct PeaksArgs; struct PoaArgs; struct PoaPairArgs; struct PrepArgs; struct WinArgs; struct StitchArgs;
struct ZeroArgs; struct QvArgs; struct C3BgzfMember; struct C3FqHdr; struct C3BamHdr; struct C3BamTile; struct FaArgs; struct EmitArgs; struct FxArgs; struct DsArgs;
struct C3GzJob; struct C3GzRes; struct C3GzSeg; struct C3GzChunk;

extern "C" {
void c3k_launch_conk(const ConkArgs*, int, int, int, hipStream_t);                                                          // k_conk.hip
void c3k_launch_adapter(const AdapterArgs*, int, hipStream_t);                                                              // k_adapter.hip
void c3k_launch_match_index(const char*, const int*, int, int, const char*, const long long*, int*, hipStream_t);
void c3k_launch_pairwise(const uint8_t*, int, const uint8_t*, int, const uint8_t*, int, uint8_t*, uint8_t*, int*, hipStream_t);   // k_poa.hip
void c3k_launch_poa(const PoaArgs*, int, int, int, hipStream_t);
void c3k_launch_poa_pair(const PoaPairArgs*, int, hipStream_t);                                                             // k_poa_pair.hip
void c3k_launch_post_classify(const PostArgs*, hipStream_t);                                                                // k_post.hip
void c3k_launch_post_scan(const PostArgs*, hipStream_t);
void c3k_launch_post_emit(const PostArgs*, hipStream_t);
void c3k_launch_demux(const uint8_t*, int, const uint8_t*, int, int, int, int32_t*, uint8_t*, hipStream_t);                 // k_demux.hip
size_t c3k_demux_lds(int, int);
void c3k_launch_peaks(const PeaksArgs*, int, hipStream_t);                                                                  // k_peaks.hip
int c3k_peaks_blocks_per_cu(void);
void c3k_launch_prep(const PrepArgs*, int, hipStream_t);                                                                    // k_polish.hip
void c3k_launch_window(const WinArgs*, int, hipStream_t);
void c3k_launch_stitch(const StitchArgs*, int, hipStream_t);
void c3k_launch_zero(const ZeroArgs*, int, hipStream_t);                                                                    // k_zero.hip
void c3k_launch_zero_long(const ZeroArgs*, int, hipStream_t);
void c3k_launch_zero_finish(const ZeroArgs*, int, hipStream_t);
void c3k_launch_qv(const QvArgs*, int, hipStream_t);                                                                        // k_qv.hip
int c3k_qv_lds_max(void);
void c3k_launch_bgzf(const uint8_t*, long long, int, uint8_t*, int*, uint8_t*, hipStream_t);                                // k_bgzf.hip
void c3k_launch_inflate(const uint8_t*, const C3BgzfMember*, int, uint8_t*, int2*, hipStream_t);                            // k_inflate.hip
void c3k_launch_gunzip_find(const uint8_t*, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t*, hipStream_t);                  // k_gunzip.hip
void c3k_launch_gunzip_decode(const uint8_t*, int64_t, const C3GzJob*, int, uint16_t*, C3GzRes*, hipStream_t);
void c3k_launch_gunzip_window(const uint16_t*, const C3GzSeg*, int, uint8_t*, hipStream_t);
void c3k_launch_gunzip_resolve(const uint16_t*, const C3GzSeg*, const C3GzChunk*, int, const uint8_t*, uint8_t*, uint2*, hipStream_t);
int c3k_gunzip_chunk(void);
void c3k_launch_fastq_count(const uint8_t*, uint32_t, uint32_t, int32_t*, int, C3FqHdr*, hipStream_t);                      // k_fastq.hip
void c3k_launch_fastq_lines(const uint8_t*, uint32_t, uint32_t, const int32_t*, int32_t*, hipStream_t);
void c3k_launch_fastq_records(const uint8_t*, uint32_t, uint32_t, const int32_t*, int, int, int, int, int32_t*, int32_t*, long long*,
                              C3FqHdr*, int64_t*, int64_t*, int4*, hipStream_t);
void c3k_launch_fastq_gather(const uint8_t*, const int4*, const int64_t*, const int64_t*, long long, uint8_t*, uint8_t*, uint8_t*, hipStream_t);
void c3k_launch_bam_chain(const uint8_t*, uint32_t, uint32_t, int, C3BamTile*, C3BamHdr*, hipStream_t);                          // k_bam.hip
void c3k_launch_bam_records(const uint8_t*, uint32_t, uint32_t, const C3BamTile*, int, int, int, uint32_t*, int32_t*, int32_t*, int32_t*,
                            int4*, long long*, C3BamHdr*, int64_t*, int64_t*, int4*, hipStream_t);
void c3k_launch_bam_gather(const uint8_t*, const int4*, const int64_t*, const int64_t*, long long, uint8_t*, uint8_t*, uint8_t*, hipStream_t);
void c3k_launch_fasta_count(const FaArgs*, hipStream_t);                                                                   // k_fasta.hip
void c3k_launch_fasta_records(const FaArgs*, int, hipStream_t);
void c3k_launch_fasta_gather(const FaArgs*, hipStream_t);
void c3k_launch_demux_heads(const FaArgs*, hipStream_t);
void c3k_launch_demux_len(const FaArgs*, hipStream_t);
void c3k_launch_demux_emit(const FaArgs*, hipStream_t);
void c3k_launch_emit_len(const EmitArgs*, hipStream_t);                                                                    // k_emit.hip
void c3k_launch_emit_scan(const EmitArgs*, hipStream_t);
void c3k_launch_emit_write(const EmitArgs*, hipStream_t);
void c3k_launch_bamout_len(const EmitArgs*, hipStream_t);                                                                  // k_bamout.hip
void c3k_launch_bamout_write(const EmitArgs*, hipStream_t);
void c3k_launch_fastx_high(const FxArgs*, hipStream_t);                                                                    // k_fastx.hip
void c3k_launch_fastx_records(const FxArgs*, hipStream_t);
void c3k_launch_fastx_gather(const FxArgs*, hipStream_t);
void c3k_launch_dsplit_krec(const DsArgs*, hipStream_t);                                                                   // k_dsplit.hip
void c3k_launch_dsplit_place(const DsArgs*, hipStream_t);
void c3k_launch_dsplit_emit(const DsArgs*, hipStream_t);
void c3k_launch_pack(const uint8_t*, const int64_t*, const int64_t*, int, uint32_t*, int, hipStream_t);                    // c3_handle.hip
}

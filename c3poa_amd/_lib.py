"""ctypes binding of the HIP backend (c3poa_amd/lib/libc3poa_hip.so, C ABI in include/c3poa.h).

There is NO CPU fallback: importing this module without the built library, or creating a handle
without an MI355X, raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("C3POA_LIB", os.path.join(_HERE, "lib", "libc3poa_hip.so"))
MAX_PEAKS = 256

STAGE_CONK, STAGE_PEAKS, STAGE_POA, STAGE_POLISH, STAGES_ALL = 1, 2, 4, 8, 15
STAGE_QV = 16                   # per-base consensus QVs (k_qv), opt-in: c3_batch_run(h, STAGES_ALL | STAGE_QV)
QV_GLOBAL, QV_ANCHOR_START, QV_ANCHOR_END = 0, 1, 2
ST_OK, ST_NOT_ASSIGNED, ST_NO_PEAKS, ST_NO_CONSENSUS, ST_TOO_SHORT, ST_LIMIT = range(6)

EXPORTS = ["c3_default_config", "c3_version", "c3_device_count", "c3_warm_device", "c3_create", "c3_destroy", "c3_last_error", "c3_set_splints",
           "c3_batch_upload", "c3_batch_stage", "c3_batch_commit", "c3_batch_assign", "c3_batch_run", "c3_batch_sync", "c3_batch_results", "c3_batch_results_snapshot", "c3_batch_results_fetch", "c3_batch_timing",
           "c3_fetch_track", "c3_fetch_smoothed", "c3_fetch_raw_peaks", "c3_fetch_draft", "c3_fetch_msa2",
           "c3_call_peaks", "c3_poa_msa", "c3_pairwise_consensus", "c3_determine_consensus", "c3_zero_repeats", "c3_scan_splints",
           "c3_reader_open", "c3_reader_open_range", "c3_reader_close", "c3_reader_error", "c3_reader_names_only", "c3_reader_next", "c3_reader_next_set", "c3_reader_noqual", "c3_reader_reserved_bytes", "c3_reader_range_lost", "c3_write_group",
           "c3_scan_adapters", "c3_match_index", "c3_match_index_batch", "c3_demux_indexes", "c3_demux_host",
           "c3_assign_open", "c3_assign_close", "c3_assign_batch", "c3_assign_seen", "c3_write_splint_psl",
           "c3_host_alloc", "c3_host_free", "c3_writer_reset",
           "c3_batch_results_fetch_qv", "c3_batch_results_qv", "c3_batch_qv_timing", "c3_consensus_qv", "c3_consensus_qv_host",
           "c3_write_consensus_fastq",
           "c3_bgzf_create", "c3_bgzf_destroy", "c3_bgzf_bound", "c3_bgzf_compress", "c3_bgzf_compress_host",
           "c3_write_group_bgzf", "c3_write_consensus_fastq_bgzf",
           "c3_bgzf_scan", "c3_bgzf_decompress", "c3_bgzf_decompress_host", "c3_reader_open_inflate", "c3_reader_inflate_wait",
           "c3_fastq_parse", "c3_fastq_parse_host", "c3_reader_parse_on_device", "c3_reader_parse_stats", "c3_bam_parse", "c3_bam_parse_host",
           "c3_post_emit", "c3_post_emit_host", "c3_post_emit_timing",
           "c3_fasta_parse", "c3_fasta_parse_host", "c3_demux_emit", "c3_demux_emit_host", "c3_demux_emit_timing",
           "c3_emit_group", "c3_emit_group_host", "c3_batch_emit_snapshot", "c3_batch_emit_fetch", "c3_emit_timing_get", "c3_append_streams",
           "c3_fastx_strict_parse_host", "c3_post_emit_text", "c3_post_text_reset", "c3_post_text_timing_get",
           "c3_demux_emit_text", "c3_demux_emit_text_host", "c3_demux_text_reset", "c3_demux_text_timing_get",
           "c3_reader_stage_on_device", "c3_reader_device_group", "c3_reader_stage_stats"]


ZERO_MAX_CELLS = 16777216       # c3_default_config's zero_max_cells: largest front * tail the zero-repeat rescue takes


class Config(C.Structure):
    _fields_ = ([("device", C.c_int), ("conk_match", C.c_int), ("conk_mismatch", C.c_int), ("conk_penalty", C.c_int),
                 ("sg_iters", C.c_int), ("sg_window", C.c_int), ("sg_order", C.c_int), ("mdistcutoff", C.c_int),
                 ("poa_match", C.c_int), ("poa_mismatch", C.c_int), ("poa_o1", C.c_int), ("poa_e1", C.c_int),
                 ("poa_o2", C.c_int), ("poa_e2", C.c_int), ("poa_band_b", C.c_int), ("poa_band_f", C.c_double),
                 ("pol_match", C.c_int), ("pol_mismatch", C.c_int), ("pol_gap", C.c_int), ("pol_window", C.c_int),
                 ("pol_q", C.c_int), ("dang_band", C.c_int), ("slots_poa", C.c_int), ("slots_win", C.c_int), ("zero", C.c_int),
                 ("zero_max_cells", C.c_int64)])


class ReadResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_peaks", C.c_int32), ("n_sub", C.c_int32), ("has_front", C.c_int32),
                ("has_tail", C.c_int32), ("front_end", C.c_int32), ("tail_beg", C.c_int32), ("cons_len", C.c_int32),
                ("draft_len", C.c_int32), ("n_win", C.c_int32), ("peaks", C.c_int32 * MAX_PEAKS),
                ("sub_beg", C.c_int32 * MAX_PEAKS), ("sub_end", C.c_int32 * MAX_PEAKS)]


RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_peaks", "<i4"), ("n_sub", "<i4"), ("has_front", "<i4"),
                         ("has_tail", "<i4"), ("front_end", "<i4"), ("tail_beg", "<i4"), ("cons_len", "<i4"),
                         ("draft_len", "<i4"), ("n_win", "<i4"), ("peaks", "<i4", (MAX_PEAKS,)),
                         ("sub_beg", "<i4", (MAX_PEAKS,)), ("sub_end", "<i4", (MAX_PEAKS,))])
assert RESULT_DTYPE.itemsize == C.sizeof(ReadResult)


class Timing(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_pack", "ms_conk", "ms_peaks", "ms_poa", "ms_prep", "ms_window",
                                         "ms_stitch", "ms_total")] + \
               [(n, C.c_int64) for n in ("n_reads", "n_bases", "n_windows", "cells_conk", "cells_poa", "cells_polish", "n_poa_redo")] + \
               [(n, C.c_float) for n in ("ms_wall", "ms_host_worklist", "ms_alloc", "ms_host_gap")] + \
               [(n, C.c_int64) for n in ("cells_polish_computed", "n_band_layers", "n_band_fallback", "n_band_mismatch", "n_win_redo", "n_poa_redo16", "n_pair", "n_pair_declined")] + \
               [("ms_poa_pair", C.c_float)]


def _fields_dict(t):
    """a timing structure as a dict of its fields"""
    return {f[0]: getattr(t, f[0]) for f in t._fields_}


class _Info(C.Structure):
    """base of the *_info structures of include/c3poa.h: all integers"""

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _t in self._fields_}


class QvTiming(C.Structure):
    _fields_ = [("ms_qv", C.c_float)] + [(n, C.c_int64) for n in ("n_reads", "n_pieces", "n_skipped", "band_cells", "edge_hits")]


class FastaInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "consumed", "name_bytes", "base_bytes")] + [("departed", C.c_int32)]


class DemuxInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "consumed", "out_bytes")] + [("departed", C.c_int32)]


class DemuxTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_parse", "ms_demux", "ms_emit", "ms_call")] + \
               [(n, C.c_int64) for n in ("n_records", "n_kept", "in_bytes", "out_bytes")]


class DemuxSetsStruct(C.Structure):       # c3_demux_sets
    _fields_ = [(k + f, t) for k in "ab" for f, t in (("_n", C.c_int), ("_cat", C.c_void_p), ("_off", C.c_void_p), ("_names", C.c_void_p), ("_name_off", C.c_void_p))]


class DemuxTextInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "consumed", "text_bytes", "out_bytes")] + \
               [(k, C.c_int32) for k in ("departed", "kind", "n_streams")]


class DemuxTextTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_inflate", "ms_parse", "ms_demux", "ms_split", "ms_emit", "ms_bgzf", "ms_call")] + \
               [(n, C.c_int64) for n in ("n_records", "n_kept", "in_bytes", "text_bytes", "out_bytes")] + \
               [(n, C.c_int32) for n in ("n_streams", "n_waits")]


class FastqInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "n_short", "consumed", "name_bytes", "base_bytes")] + [("departed", C.c_int32)]


class BamInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "n_short", "consumed", "name_bytes", "base_bytes", "header_bytes", "bad_at")] + \
               [("departed", C.c_int32), ("reason", C.c_int32)]


class FastxInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "consumed", "name_bytes", "base_bytes")] + [("departed", C.c_int32)]


class PostTextInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "consumed", "text_bytes", "out_bytes")] + [("departed", C.c_int32)]


class PostTextTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_inflate", "ms_parse", "ms_gather", "ms_adapter", "ms_post", "ms_bgzf", "ms_call")] + \
               [(n, C.c_int64) for n in ("n_records", "n_kept", "in_bytes", "text_bytes", "out_bytes")]


class PostArgs(C.Structure):
    """c3_post_args of include/c3poa.h"""
    _fields_ = [("n", C.c_int32), ("names", C.c_void_p), ("name_off", C.c_void_p), ("seqs", C.c_void_p), ("quals", C.c_void_p),
                ("off", C.c_void_p), ("table", C.c_void_p), ("n_ad", C.c_int32), ("ad_len", C.c_void_p), ("ad_class", C.c_void_p),
                ("class5", C.c_int32), ("ad_names", C.c_void_p), ("ad_name_off", C.c_void_p), ("has_index", C.c_int32),
                ("n_idx", C.c_int32), ("idx_cat", C.c_void_p), ("idx_off", C.c_void_p), ("idx_dest", C.c_void_p),
                ("n_dest", C.c_int32), ("undirectional", C.c_int32), ("trim", C.c_int32), ("barcoded", C.c_int32)]


class PostTiming(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("ms_classify", "ms_scan", "ms_emit", "ms_call")] + \
               [(k, C.c_int64) for k in ("n_reads", "n_kept", "in_bytes", "out_bytes")]


class EmitTiming(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("ms_len", "ms_scan", "ms_write", "ms_bgzf", "ms_call")] + \
               [(k, C.c_int64) for k in ("n_reads", "n_records", "in_bytes", "out_bytes")]


class HostBatchStruct(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_short", C.c_int64), ("names", C.c_void_p), ("name_off", C.c_void_p),
                ("seqs", C.c_void_p), ("quals", C.c_void_p), ("off", C.c_void_p)]


class DeviceBatchStruct(C.Structure):      # c3_device_batch
    _fields_ = [("d_seqs", C.c_void_p), ("d_quals", C.c_void_p), ("device", C.c_int32), ("bytes", C.c_int64)]


_lib = None


def load():
    """Load the shared library; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("c3poa_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, ip, cp, i64p = C.c_void_p, C.POINTER(C.c_int), C.c_char_p, C.c_void_p
    lib.c3_default_config.argtypes = [C.POINTER(Config)]
    lib.c3_version.restype = C.c_char_p
    lib.c3_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.c3_destroy.argtypes = [vp]
    lib.c3_destroy.restype = None
    lib.c3_last_error.argtypes = [vp]
    lib.c3_last_error.restype = C.c_char_p
    lib.c3_set_splints.argtypes = [vp, C.c_int, cp, i64p]
    lib.c3_batch_upload.argtypes = [vp, C.c_int, vp, vp, i64p, vp, vp]
    lib.c3_batch_stage.argtypes = [vp, C.c_int, vp, vp, i64p, vp, vp]
    lib.c3_batch_commit.argtypes = [vp]
    lib.c3_batch_assign.argtypes = [vp, vp, vp]
    lib.c3_batch_run.argtypes = [vp, C.c_int]
    lib.c3_batch_sync.argtypes = [vp]
    lib.c3_batch_results.argtypes = [vp, vp, vp, C.c_int64, i64p]
    lib.c3_batch_results_snapshot.argtypes = [vp]
    lib.c3_batch_results_fetch.argtypes = [vp, vp, vp, C.c_int64, i64p]
    lib.c3_batch_timing.argtypes = [vp, C.POINTER(Timing)]
    lib.c3_fetch_track.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.c3_fetch_smoothed.argtypes = [vp, C.c_int, vp, C.c_int64]
    lib.c3_fetch_raw_peaks.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.c3_fetch_draft.argtypes = [vp, C.c_int, vp, C.c_int]
    lib.c3_fetch_msa2.argtypes = [vp, C.c_int, vp, vp, C.c_int]
    lib.c3_call_peaks.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.c3_poa_msa.argtypes = [vp, C.c_int, C.POINTER(cp), ip, vp, C.c_int, ip, vp, C.c_int64, ip]
    lib.c3_zero_repeats.argtypes = [vp, cp, cp, C.c_int, cp, cp, C.c_int, C.c_int, vp, C.c_int, ip]
    lib.c3_scan_splints.argtypes = [vp, vp, vp, vp]
    lib.c3_pairwise_consensus.argtypes = [vp, cp, cp, C.c_int, cp, C.c_int, cp, cp, C.c_int, cp, vp, C.c_int, ip]
    lib.c3_scan_adapters.argtypes = [vp, vp]
    lib.c3_match_index.argtypes = [cp, C.c_int, C.c_int, cp, vp]
    lib.c3_match_index_batch.argtypes = [vp, C.c_int, vp, vp, C.c_int, cp, vp, vp]
    lib.c3_demux_indexes.argtypes = [vp, C.c_int, vp, C.c_int, cp, vp, C.c_int, cp, vp, vp, vp]
    lib.c3_demux_host.argtypes = [C.c_int, vp, C.c_int, cp, vp, C.c_int, cp, vp, vp, vp]
    lib.c3_assign_open.argtypes = [cp, C.c_int, C.POINTER(cp), C.POINTER(vp)]
    lib.c3_assign_close.argtypes = [vp]
    lib.c3_assign_close.restype = None
    lib.c3_assign_batch.argtypes = [vp, C.POINTER(HostBatchStruct), vp, vp]
    lib.c3_assign_seen.argtypes = [vp, vp, vp]
    lib.c3_write_splint_psl.argtypes = [C.POINTER(HostBatchStruct), vp, vp, vp, C.c_int, C.POINTER(cp), vp, C.c_int, cp, vp]
    lib.c3_host_alloc.argtypes = [C.c_int64, C.POINTER(vp)]
    lib.c3_host_free.argtypes = [vp]
    lib.c3_host_free.restype = None
    lib.c3_writer_reset.restype = None
    lib.c3_reader_open.argtypes = [cp, C.c_int, C.POINTER(vp)]
    lib.c3_reader_open_range.argtypes = [cp, C.c_int, C.c_int64, C.c_int64, C.POINTER(vp)]
    lib.c3_reader_close.argtypes = [vp]
    lib.c3_reader_close.restype = None
    lib.c3_reader_error.argtypes = [vp]
    lib.c3_reader_names_only.argtypes = [vp, C.c_int]
    lib.c3_reader_names_only.restype = None
    lib.c3_reader_error.restype = C.c_char_p
    for fn in (lib.c3_reader_noqual, lib.c3_reader_reserved_bytes):
        fn.argtypes = [vp]; fn.restype = C.c_int64
    lib.c3_reader_range_lost.argtypes = [vp]
    lib.c3_reader_next.argtypes = [vp, C.c_int, C.c_int64, C.c_int, C.POINTER(HostBatchStruct)]
    lib.c3_reader_next_set.argtypes = [vp, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(HostBatchStruct)]
    lib.c3_write_group.argtypes = [C.POINTER(HostBatchStruct), vp, vp, vp, vp, C.c_int, C.POINTER(cp), C.POINTER(cp), C.c_int]
    lib.c3_determine_consensus.argtypes = [vp, C.c_int, C.POINTER(cp), C.POINTER(cp), ip, cp, cp, C.c_int,
                                           cp, cp, C.c_int, vp, C.c_int, ip, vp, C.c_int, ip]
    lib.c3_batch_results_fetch_qv.argtypes = [vp, vp, vp, C.c_int64, i64p, vp]
    lib.c3_batch_results_qv.argtypes = [vp, vp, vp, C.c_int64, i64p, vp]
    lib.c3_batch_qv_timing.argtypes = [vp, C.POINTER(QvTiming)]
    lib.c3_consensus_qv.argtypes = [vp, cp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.c3_consensus_qv_host.argtypes = [cp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.c3_write_consensus_fastq.argtypes = [C.POINTER(HostBatchStruct), vp, vp, vp, vp, vp, C.c_int, C.POINTER(cp), C.c_int]
    lib.c3_bgzf_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.c3_bgzf_destroy.argtypes = [vp]
    lib.c3_bgzf_destroy.restype = None
    lib.c3_bgzf_bound.argtypes = [C.c_int64]
    lib.c3_bgzf_bound.restype = C.c_int64
    lib.c3_bgzf_compress.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.c3_bgzf_compress_host.argtypes = [vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.c3_write_group_bgzf.argtypes = [vp, C.POINTER(HostBatchStruct), vp, vp, vp, vp, C.c_int, C.POINTER(cp), C.POINTER(cp), C.c_int]
    lib.c3_write_consensus_fastq_bgzf.argtypes = [vp, C.POINTER(HostBatchStruct), vp, vp, vp, vp, vp, C.c_int, C.POINTER(cp), C.c_int]
    lib.c3_bgzf_scan.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.c3_bgzf_decompress.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.c3_bgzf_decompress_host.argtypes = [vp, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64)]
    lib.c3_reader_open_inflate.argtypes = [cp, C.c_int, C.c_int, C.POINTER(vp)]
    lib.c3_reader_inflate_wait.argtypes = [vp]
    lib.c3_reader_inflate_wait.restype = C.c_double
    fq = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(FastqInfo)]
    lib.c3_fastq_parse.argtypes = [vp] + fq
    lib.c3_fastq_parse_host.argtypes = fq
    bam = [vp, C.c_int64, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(BamInfo)]
    lib.c3_bam_parse.argtypes = [vp] + bam
    lib.c3_bam_parse_host.argtypes = bam
    lib.c3_reader_parse_on_device.argtypes = [vp, C.c_int]
    lib.c3_reader_parse_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.c3_post_emit.argtypes = [vp, C.POINTER(PostArgs), vp, C.c_int64, vp, vp]
    lib.c3_post_emit_host.argtypes = [C.POINTER(PostArgs), vp, C.c_int64, vp, vp]
    lib.c3_post_emit_timing.argtypes = [vp, C.POINTER(PostTiming)]
    fa = [vp, C.c_int64, C.c_int, vp, C.c_int64, vp, vp, C.c_int64, vp, vp, C.c_int64, C.POINTER(FastaInfo)]
    lib.c3_fasta_parse.argtypes = [vp] + fa
    lib.c3_fasta_parse_host.argtypes = fa
    de = [vp, C.c_int64, C.c_int] + [C.c_int, vp, vp, vp, vp] * 2 + [vp, C.c_int64, vp, C.c_int64, C.POINTER(DemuxInfo)]
    lib.c3_demux_emit.argtypes = [vp] + de
    lib.c3_demux_emit_host.argtypes = de
    lib.c3_demux_emit_timing.argtypes = [vp, C.POINTER(DemuxTiming)]
    em = [C.POINTER(HostBatchStruct), vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    lib.c3_emit_group.argtypes = [vp] + em
    lib.c3_emit_group_host.argtypes = em
    lib.c3_batch_emit_snapshot.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    lib.c3_batch_emit_fetch.argtypes = [vp, vp, C.c_int64, vp]
    lib.c3_emit_timing_get.argtypes = [vp, C.POINTER(EmitTiming)]
    lib.c3_append_streams.argtypes = [C.POINTER(C.c_char_p), vp, vp, C.c_int]
    lib.c3_fastx_strict_parse_host.argtypes = [vp, C.c_int64, C.c_int, C.c_int, vp, C.c_int64, vp, vp, vp, C.c_int64, vp, vp, C.c_int64,
                                               C.POINTER(FastxInfo)]
    lib.c3_post_emit_text.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int, C.POINTER(PostArgs), vp, C.c_int64, vp, vp, C.c_int64,
                                      C.POINTER(PostTextInfo)]
    lib.c3_post_text_reset.argtypes = [vp]
    lib.c3_post_text_timing_get.argtypes = [vp, C.POINTER(PostTextTiming)]
    dt = [vp, C.c_int64, C.c_int]
    dt2 = [C.c_int, C.POINTER(DemuxSetsStruct), vp, C.c_int64, vp, vp, C.c_int64, C.POINTER(DemuxTextInfo)]
    lib.c3_demux_emit_text.argtypes = [vp] + dt + dt2
    lib.c3_demux_emit_text_host.argtypes = dt + [C.c_int] + dt2
    lib.c3_demux_text_reset.argtypes = [vp]
    lib.c3_demux_text_timing_get.argtypes = [vp, C.POINTER(DemuxTextTiming)]
    lib.c3_reader_stage_on_device.argtypes = [vp, C.c_int]
    lib.c3_reader_device_group.argtypes = [vp, C.c_int, C.POINTER(DeviceBatchStruct)]
    lib.c3_reader_stage_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    _lib = lib
    return lib


class C3Error(RuntimeError):
    code = None                 # the c3_err value, where the raising call knows it (E_DATA: damaged input)


E_ARG, E_DATA = -3, -7          # include/c3poa.h c3_err
E_STATE, E_LIMIT = -5, -6


def default_config(**kw):
    cfg = Config()
    load().c3_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode()


class Handle:
    """One per GPU (c3_create / c3_destroy)."""

    def __init__(self, **cfg):
        self.lib = load()
        self.cfg = default_config(**cfg)
        self.h = C.c_void_p()
        rc = self.lib.c3_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            e = C3Error("c3_create failed (%d): %s" % (rc, self.lib.c3_last_error(None).decode()))
            e.code = rc
            raise e
        self.n = 0
        self.lens = None

    def close(self):
        if self.h:
            self.lib.c3_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            e = C3Error("c3 error %d: %s" % (rc, self.lib.c3_last_error(self.h).decode()))
            e.code = rc
            raise e
        return rc

    def set_splints(self, splints):
        """splints: list of sequences (order defines splint_id)"""
        bs = [_b(s) for s in splints]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bs], out=off[1:])
        self._chk(self.lib.c3_set_splints(self.h, len(bs), b"".join(bs), off.ctypes.data))
        self.n_splints = len(bs)

    def upload(self, seqs, quals, strands, splint_ids=None):
        """seqs/quals: lists of str/bytes (or pre-joined bytes with `lens`), strands: '+'/'-' per read"""
        bs = [_b(s) for s in seqs]
        n = len(bs)
        lens = np.array([len(b) for b in bs], dtype=np.int64)
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        self.upload_flat(b"".join(bs), b"".join(_b(q) for q in quals), off,
                         "".join(strands) if not isinstance(strands, (bytes, bytearray)) else strands, splint_ids)

    def upload_flat(self, seq_cat, qual_cat, off, strands, splint_ids=None):
        n = len(off) - 1
        off = np.ascontiguousarray(off, dtype=np.int64)
        st = _b(strands)
        assert len(st) == n and len(seq_cat) == off[-1] == len(qual_cat)
        sid = None
        if splint_ids is not None:
            sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
        sq = np.frombuffer(seq_cat, dtype=np.uint8)
        qq = np.frombuffer(qual_cat, dtype=np.uint8)
        self._chk(self.lib.c3_batch_upload(self.h, n, sq.ctypes.data, qq.ctypes.data, off.ctypes.data,
                                           sid.ctypes.data if sid is not None else None,
                                           np.frombuffer(st, dtype=np.uint8).ctypes.data))
        self.n = n
        self.off = off

    def upload_host(self, hb, strands, splint_ids):
        """upload a HostBatch of the native reader straight from its (page-locked) buffers: no Python copies"""
        st = np.frombuffer(_b(strands), dtype=np.uint8)
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
        assert len(st) == hb.n == len(sid)
        self._chk(self.lib.c3_batch_upload(self.h, hb.n, hb.c.seqs, hb.c.quals, hb.c.off, sid.ctypes.data, st.ctypes.data))
        self.n = hb.n
        self.off = hb.off

    def stage_host(self, hb, strands, splint_ids):
        """c3_batch_stage: copy the NEXT batch on the second stream while the resident one is processed; the HostBatch
        must stay alive until commit()"""
        st = np.frombuffer(_b(strands), dtype=np.uint8)
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
        assert len(st) == hb.n == len(sid)
        self._chk(self.lib.c3_batch_stage(self.h, hb.n, hb.c.seqs, hb.c.quals, hb.c.off, sid.ctypes.data, st.ctypes.data))
        self._staged = (hb.n, hb.off, hb)

    def commit(self):
        """c3_batch_commit: the staged batch becomes the resident one"""
        self._chk(self.lib.c3_batch_commit(self.h))
        self.n, self.off, _keep = self._staged
        self._staged = None

    def assign(self, splint_ids, strands):
        """c3_batch_assign: splint row / strand of the resident batch (e.g. from scan_splints)"""
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
        st = np.frombuffer(_b(strands), dtype=np.uint8)
        assert len(sid) == len(st) == self.n
        self._chk(self.lib.c3_batch_assign(self.h, sid.ctypes.data, st.ctypes.data))

    def upload_pinned(self, pb, splint_ids=None):
        """c3_batch_upload straight from a PinnedBatch (page-locked buffers: DMA, no staging copy)"""
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16) if splint_ids is not None else None
        self._chk(self.lib.c3_batch_upload(self.h, pb.n, pb.seqs, pb.quals, pb.off.ctypes.data,
                                           sid.ctypes.data if sid is not None else None, pb.strand.ctypes.data))
        self.n, self.off = pb.n, pb.off

    def stage_pinned(self, pb, splint_ids=None):
        """c3_batch_stage from a PinnedBatch; the batch must stay alive until commit()"""
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16) if splint_ids is not None else None
        self._chk(self.lib.c3_batch_stage(self.h, pb.n, pb.seqs, pb.quals, pb.off.ctypes.data,
                                          sid.ctypes.data if sid is not None else None, pb.strand.ctypes.data))
        self._staged = (pb.n, pb.off, pb)

    def run(self, stages=STAGES_ALL, qv=False):
        """qv=True adds STAGE_QV (per-base consensus QVs after the polish)"""
        self._chk(self.lib.c3_batch_run(self.h, stages | (STAGE_QV if qv else 0)))
        self.last_timing = self.timing()         # c3_batch_commit clears the library's copy
        if qv:
            self.last_qv_timing = self.qv_timing()

    def qv_timing(self):
        """c3_batch_qv_timing: k_qv figures of the last run with STAGE_QV"""
        t = QvTiming()
        self._chk(self.lib.c3_batch_qv_timing(self.h, C.byref(t)))
        return _fields_dict(t)

    def results_raw(self, into=None):
        """(results structured array, consensus byte buffer, cons_off[n+1]) without building Python strings.
        `into`: a ResultBuffers object owned by the caller (pipelines that keep several results alive at once hand each one
        back to their own free list); without it ONE grow-only set per handle is reused, valid until the next call."""
        rb = into if into is not None else self.__dict__.setdefault("_own_rb", ResultBuffers())
        res, buf, coff = rb.fit(self.n, int(self.off[-1]) + 16)
        self._chk(self.lib.c3_batch_results(self.h, res.ctypes.data, buf.ctypes.data, len(buf), coff.ctypes.data))
        return res, buf, coff

    def results_snapshot(self):
        """first half of results_raw (c3_batch_results_snapshot): freezes the results of the resident batch on the device; the
        handle may then commit and run the next batch.  Returns what results_fetch needs to size its buffers."""
        self._chk(self.lib.c3_batch_results_snapshot(self.h))
        return self.n, int(self.off[-1]) + 16

    def results_fetch(self, into, shape, with_cons=True):
        """second half (c3_batch_results_fetch): copies the snapshot into `into` (a ResultBuffers); may run on ANOTHER thread
        while this handle's owner works on the next batch.  `shape` = the value results_snapshot returned.  with_cons=False:
        the records and offsets alone (cons = NULL), for callers that take the bytes from emit_fetch."""
        res, buf, coff = into.fit(*shape) if with_cons else into.fit(shape[0], 16)
        rc = self.lib.c3_batch_results_fetch(self.h, res.ctypes.data, buf.ctypes.data if with_cons else None, len(buf) if with_cons else 0, coff.ctypes.data)
        if rc != 0:
            raise C3Error("c3_batch_results_fetch failed (%d)" % rc)
        return res, buf, coff

    def results_fetch_qv(self, into, shape):
        """results_fetch + the QV bytes (c3_batch_results_fetch_qv): (res, cons bytes, cons_off, QV bytes at the same offsets)"""
        res, buf, coff = into.fit(*shape)
        qv = into.fit_qv(shape[1])
        rc = self.lib.c3_batch_results_fetch_qv(self.h, res.ctypes.data, buf.ctypes.data, len(buf), coff.ctypes.data, qv.ctypes.data)
        if rc != 0:
            raise C3Error("c3_batch_results_fetch_qv failed (%d)" % rc)
        return res, buf, coff, qv

    def results(self, with_consensus=True, qv=False):
        """(records, consensus strings); qv=True: (records, consensus strings, QV strings) via c3_batch_results_qv"""
        res = np.zeros(self.n, dtype=RESULT_DTYPE)
        coff = np.zeros(self.n + 1, dtype=np.int64)
        if qv:
            cap = int(self.off[-1]) + 16
            buf, qbuf = np.zeros(cap, dtype=np.uint8), np.zeros(cap, dtype=np.uint8)
            self._chk(self.lib.c3_batch_results_qv(self.h, res.ctypes.data, buf.ctypes.data, cap, coff.ctypes.data, qbuf.ctypes.data))
            raw, qraw = buf.tobytes(), qbuf.tobytes()
            return (res, [raw[coff[i]:coff[i + 1]].decode() for i in range(self.n)],
                    [qraw[coff[i]:coff[i + 1]].decode() for i in range(self.n)])
        if not with_consensus:
            self._chk(self.lib.c3_batch_results(self.h, res.ctypes.data, None, 0, coff.ctypes.data))
            return res, None
        cap = int(self.off[-1]) + 16
        buf = np.zeros(cap, dtype=np.uint8)
        self._chk(self.lib.c3_batch_results(self.h, res.ctypes.data, buf.ctypes.data, cap, coff.ctypes.data))
        raw = buf.tobytes()
        cons = [raw[coff[i]:coff[i + 1]].decode() for i in range(self.n)]
        return res, cons

    def timing(self):
        t = Timing()
        self._chk(self.lib.c3_batch_timing(self.h, C.byref(t)))
        return _fields_dict(t)

    # ---- probes
    def track(self, i):
        L = int(self.off[i + 1] - self.off[i])
        out = np.zeros(L, dtype=np.int32)
        self._chk(self.lib.c3_fetch_track(self.h, i, out.ctypes.data, L))
        return out

    def smoothed(self, i):
        L = int(self.off[i + 1] - self.off[i])
        out = np.zeros(L, dtype=np.float64)
        self._chk(self.lib.c3_fetch_smoothed(self.h, i, out.ctypes.data, L))
        return out

    def raw_peaks(self, i):
        out = np.zeros(MAX_PEAKS, dtype=np.int32)
        n = self._chk(self.lib.c3_fetch_raw_peaks(self.h, i, out.ctypes.data, MAX_PEAKS))
        return out[:n].astype(np.int64)

    def draft(self, i):
        L = int(self.off[i + 1] - self.off[i]) + 8
        buf = C.create_string_buffer(L)
        n = self._chk(self.lib.c3_fetch_draft(self.h, i, buf, L))
        return buf.raw[:n].decode()

    def call_peaks(self, scores, min_dist, return_smoothed=False):
        s = np.ascontiguousarray(scores, dtype=np.int32)
        pk = np.zeros(MAX_PEAKS, dtype=np.int32)
        sm = np.zeros(len(s), dtype=np.float64) if return_smoothed else None
        n = self._chk(self.lib.c3_call_peaks(self.h, s.ctypes.data, len(s), int(min_dist), pk.ctypes.data, MAX_PEAKS,
                                             sm.ctypes.data if sm is not None else None))
        self.n = 0
        out = pk[:n].astype(np.int64)
        return (out, sm) if return_smoothed else out

    def poa_msa(self, seqs, out_cons=True, out_msa=True):
        n = len(seqs)
        if n == 0:
            return [], []
        bs = [_b(s) for s in seqs]
        arr = (C.c_char_p * n)(*bs)
        lens = (C.c_int * n)(*[len(b) for b in bs])
        tot = sum(len(b) for b in bs) + 16
        cons = C.create_string_buffer(tot) if out_cons else None
        msa = C.create_string_buffer(tot * n) if out_msa else None
        cl, ml = C.c_int(0), C.c_int(0)
        self._chk(self.lib.c3_poa_msa(self.h, n, arr, lens, cons, tot, C.byref(cl), msa, tot * n, C.byref(ml)))
        c = [cons.raw[:cl.value].decode()] if out_cons and cl.value else []
        m = [msa.raw[i * ml.value:(i + 1) * ml.value].decode() for i in range(n)] if out_msa and ml.value else []
        return c, m

    def scan_splints(self):
        """splint/strand finder over the resident batch (replaces blat, bin/preprocess.py:61-77).
        returns (table[n][n_splints][2][4] = max, argmax, mean, L; splint_id[n] (-1 = none); strand bytes)"""
        n = self.n
        tab = np.zeros((n, self.n_splints, 2, 4), dtype=np.int32)
        sid = np.zeros(n, dtype=np.int16)
        st = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.c3_scan_splints(self.h, tab.ctypes.data, sid.ctypes.data, st.ctypes.data))
        return tab, sid, st.tobytes()

    def scan_adapters(self):
        """adapter finder over the resident batch (replaces blat in C3POa_postprocessing.py:229-236): table
        [n][n_adapters][2 strands][12] = score, qStart, qEnd, tStart, tEnd, matches, misMatches, qBaseInsert,
        tBaseInsert, qNumInsert, tNumInsert, read length"""
        tab = np.zeros((self.n, self.n_splints, 2, 12), dtype=np.int32)
        self._chk(self.lib.c3_scan_adapters(self.h, tab.ctypes.data))
        return tab

    def match_index_batch(self, pieces, index_seqs):
        """c3_match_index_batch: winning index number (or -1) for every piece (str, <= 64 bases)"""
        n = len(pieces)
        if n == 0:
            return np.zeros(0, dtype=np.int32)
        buf = np.zeros((n, 64), dtype=np.uint8)
        lens = np.zeros(n, dtype=np.int32)
        for i, pc in enumerate(pieces):
            b = _b(pc)
            lens[i] = len(b)
            buf[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        bs = [_b(x) for x in index_seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bs], out=off[1:])
        out = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.c3_match_index_batch(self.h, n, buf.ctypes.data, lens.ctypes.data, len(bs), b"".join(bs), off.ctypes.data, out.ctypes.data))
        return out

    def post_emit(self, plan, batch, table):
        """c3_post_emit (k_post): the finished file bytes of one batch.  plan: a PostPlan; batch: a PostBatch; table: what
        scan_adapters returned for the batch.  Returns (arena uint8 array, stream_off[S + 1], kept reads)."""
        return _post_call(lambda *a: self.lib.c3_post_emit(self.h, *a), lambda: self.lib.c3_last_error(self.h), plan, batch, table)

    def post_emit_text(self, plan, piece, at_eof=False, in_bgzf=False, out_bgzf=False, keep_quals=False, cap=None, max_records=None, bufs=None):
        """c3_post_emit_text: the next piece of a consensus file (bytes; whole BGZF members with in_bgzf) through parse,
        k_adapter and k_post on the device.  Returns a PostText: info (dict), arena (uint8 array), stream_off[S + 1], hashes
        (uint64 array of n_records), guards_intact.  cap / max_records: instead of sizes found by asking again; C3Error (code,
        .info, .stream_off, .guards_intact, .untouched) on a refusal.  bufs: a dict the call keeps its output arrays in from one
        piece to the next (no guard bytes then; the results are views that the next call overwrites)."""
        flags = (POST_IN_BGZF if in_bgzf else 0) | (POST_OUT_BGZF if out_bgzf else 0) | (POST_KEEP_QUALS if keep_quals else 0)
        a = _post_args(plan, 0, None, None, None, None, None, None)
        return _text_call(lambda *x: self.lib.c3_post_emit_text(self.h, *x), lambda: self.lib.c3_last_error(self.h), piece,
                          (int(bool(at_eof)), flags, C.byref(a)), plan.n_streams, PostTextInfo(), in_bgzf, cap, max_records, bufs)

    def demux_emit_text(self, sets, piece, at_eof=False, flags=0, cap=None, max_records=None, bufs=None):
        """c3_demux_emit_text: the next piece of a read file (bytes or a uint8 array; whole BGZF members with DEMUX_IN_BGZF)
        through parse, k_demux, k_dsplit and k_bgzf on the device.  sets: a DemuxSets.  Returns a DemuxText (_text_call)."""
        return _demux_text_call(lambda *a: self.lib.c3_demux_emit_text(self.h, *a), lambda: self.lib.c3_last_error(self.h), sets, piece, at_eof,
                                None, flags, cap, max_records, bufs)

    def demux_text_reset(self):
        """c3_demux_text_reset: drops the tail the demultiplexer's text path keeps between two pieces and forgets the file's kind"""
        self._chk(self.lib.c3_demux_text_reset(self.h))

    def demux_text_timing(self):
        """c3_demux_text_timing_get: times, counts and stream waits of the last demux_emit_text"""
        t = DemuxTextTiming()
        self._chk(self.lib.c3_demux_text_timing_get(self.h, C.byref(t)))
        return _fields_dict(t)

    def post_text_reset(self):
        """c3_post_text_reset: drops the tail the text path keeps between two pieces and forgets the file's kind"""
        self._chk(self.lib.c3_post_text_reset(self.h))

    def post_text_timing(self):
        """c3_post_text_timing_get: times of the last post_emit_text"""
        t = PostTextTiming()
        self._chk(self.lib.c3_post_text_timing_get(self.h, C.byref(t)))
        return _fields_dict(t)

    def post_emit_timing(self):
        """c3_post_emit_timing: event times of the three passes of the last post_emit and the call with its copies"""
        t = PostTiming()
        self._chk(self.lib.c3_post_emit_timing(self.h, C.byref(t)))
        return _fields_dict(t)

    def emit_group(self, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero=True, cap=None, arena=None):
        """c3_emit_group (k_emit): the file bytes of write_group (+ write_consensus_fastq with qv_buf) for one group, as an
        EmitStreams.  Same arguments as emit_group_host."""
        return _emit_call(lambda *a: self.lib.c3_emit_group(self.h, *a), lambda: self.lib.c3_last_error(self.h),
                          hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap, arena)

    def emit_snapshot(self, hb, zero=True, bgzf=False, qv=False):
        """c3_batch_emit_snapshot: formats the records of the resident batch (whose names are hb's) on the device and freezes
        the streams; the handle may then commit and run the next batch.  Returns the number of streams emit_fetch delivers."""
        no = np.ascontiguousarray(hb.name_off, dtype=np.int64)
        self._chk(self.lib.c3_batch_emit_snapshot(self.h, hb.c.names, no.ctypes.data, 1 if zero else 0, EMIT_BGZF if bgzf else 0))
        return self.n_splints * (3 if qv else 2)

    def emit_fetch(self, into, n_streams):
        """c3_batch_emit_fetch: (arena bytes, stream_off[n_streams + 1]) of the emit snapshot in `into` (an EmitBuffers); may run
        on ANOTHER thread while this handle's owner works on the next batch.  An arena that is too small is grown once."""
        so = np.zeros(n_streams + 1, dtype=np.int64)
        rc = self.lib.c3_batch_emit_fetch(self.h, into.ptr, into.size, so.ctypes.data)
        if rc == E_LIMIT:
            into.fit(int(so[n_streams]))
            rc = self.lib.c3_batch_emit_fetch(self.h, into.ptr, into.size, so.ctypes.data)
        if rc != 0:
            e = C3Error("c3_batch_emit_fetch failed (%d)" % rc)
            e.code = rc
            raise e
        return into, so

    def emit_timing(self):
        """c3_emit_timing_get: event times of the last emit_group, or of the snapshot the last emit_fetch delivered"""
        t = EmitTiming()
        self._chk(self.lib.c3_emit_timing_get(self.h, C.byref(t)))
        return _fields_dict(t)

    def demux_indexes(self, heads, set_a, set_b, return_dist=False):
        """c3_demux_indexes (k_demux): winners (n, 2) int32 of index sets A and B (index number or -1) for every head
        (300 bytes each, see _demux_args), and with return_dist the (n, len(A) + len(B)) uint8 minimum distances"""
        args, keep, res = _demux_args(heads, set_a, set_b, return_dist)
        self._chk(self.lib.c3_demux_indexes(self.h, *args))
        return res

    def fasta_parse(self, text, at_eof=True, caps=None):
        """c3_fasta_parse (k_fasta): the FASTA records of `text` as read_fasta reads them (a FastaParse)"""
        return _fasta_call(lambda *a: self.lib.c3_fasta_parse(self.h, *a), lambda: self.lib.c3_last_error(self.h), text, at_eof, caps)

    def demux_emit(self, text, sets, at_eof=True, cap=None, max_records=None):
        """c3_demux_emit (k_fasta, k_demux): FASTA text in, the bytes of Indexed_reads.fasta out (a DemuxEmit).  sets: a DemuxSets"""
        return _demux_emit_call(lambda *a: self.lib.c3_demux_emit(self.h, *a), lambda: self.lib.c3_last_error(self.h), text, sets, at_eof, cap, max_records)

    def demux_emit_raw(self, ptr, n, at_eof, sets, out, hashes):
        """c3_demux_emit on caller-owned buffers: text at address `ptr` (n bytes), out (uint8 array) and hashes (uint64 array)
        as capacities.  Returns (rc, info dict); nothing is raised, so that the caller can grow a buffer on E_LIMIT."""
        info = DemuxInfo()
        rc = self.lib.c3_demux_emit(self.h, ptr if n else None, n, int(bool(at_eof)), *(sets.args + (out.ctypes.data, out.size, hashes.ctypes.data, hashes.size, C.byref(info))))
        return rc, info.as_dict()

    def demux_emit_timing(self):
        """c3_demux_emit_timing: event times of the parse kernels, k_demux and the emit kernels of the last demux_emit, and
        the call with its copies"""
        t = DemuxTiming()
        self._chk(self.lib.c3_demux_emit_timing(self.h, C.byref(t)))
        return _fields_dict(t)

    def consensus_qv(self, cons, pieces):
        """c3_consensus_qv (k_qv): Phred+33 QV string of `cons` from pieces = [(seq, qual, mode)], mode QV_GLOBAL /
        QV_ANCHOR_START / QV_ANCHOR_END"""
        args, keep = _qv_args(cons, pieces)
        self._chk(self.lib.c3_consensus_qv(self.h, *args))
        return keep[-1].raw[:len(keep[0])].decode()

    def pairwise_consensus(self, msa_rows, subreads, quals):
        """pairwise_consensus(msa_rows, subreads, quals) of bin/consensus.py:76"""
        ra, rb = _b(msa_rows[0]), _b(msa_rows[1])
        sa, sb, qa, qb = _b(subreads[0]), _b(subreads[1]), _b(quals[0]), _b(quals[1])
        out = C.create_string_buffer(len(ra) + 1)
        ol = C.c_int(0)
        self._chk(self.lib.c3_pairwise_consensus(self.h, ra, rb, len(ra), sa, len(sa), qa, sb, len(sb), qb, out, len(ra) + 1, C.byref(ol)))
        return out.raw[:ol.value].decode()

    def zero_repeats(self, d0, q0, d1, q1, min_len=0):
        b0, b1 = _b(d0), _b(d1)
        cap = len(b0) + len(b1) + 16
        out = C.create_string_buffer(cap)
        ol = C.c_int(0)
        self._chk(self.lib.c3_zero_repeats(self.h, b0, _b(q0), len(b0), b1, _b(q1), len(b1), int(min_len), out, cap, C.byref(ol)))
        return out.raw[:ol.value].decode()

    def determine_consensus(self, subs, quals, front=None, tail=None, return_draft=False):
        n = len(subs)
        bs, bq = [_b(s) for s in subs], [_b(q) for q in quals]
        arr, qarr = (C.c_char_p * n)(*bs), (C.c_char_p * n)(*bq)
        lens = (C.c_int * n)(*[len(b) for b in bs])
        tot = sum(len(b) for b in bs) + (len(front[0]) if front else 0) + (len(tail[0]) if tail else 0) + 64
        out, draft = C.create_string_buffer(tot), C.create_string_buffer(tot)
        ol, dl = C.c_int(0), C.c_int(0)
        f = (_b(front[0]), _b(front[1]), len(front[0])) if front else (None, None, 0)
        t = (_b(tail[0]), _b(tail[1]), len(tail[0])) if tail else (None, None, 0)
        self._chk(self.lib.c3_determine_consensus(self.h, n, arr, qarr, lens, f[0], f[1], f[2], t[0], t[1], t[2],
                                                  out, tot, C.byref(ol), draft, tot, C.byref(dl)))
        if return_draft:
            return out.raw[:ol.value].decode(), draft.raw[:dl.value].decode()
        return out.raw[:ol.value].decode()


def match_index(seq, index_seqs):
    """c3_match_index: number of the winning index (file order) or -1 (match_index, C3POa_postprocessing.py:266-285)"""
    bs = [_b(x) for x in index_seqs]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bs], out=off[1:])
    sq = _b(seq)
    return int(load().c3_match_index(sq, len(sq), len(bs), b"".join(bs), off.ctypes.data))


class PostPlan:
    """what c3_post_emit needs besides the batch: adapters (name, sequence) in file order, the index set as
    postprocess.read_fasta(path, True) returns it (idx_to_seq, seq_to_idx) or None, and the options.  dests = the destination
    directory names in stream order ([""] without an index set; no_index_found is the last one)."""

    def __init__(self, adapters, index=None, undirectional=False, trim=False, barcoded=False):
        self.ad_names = [_b(a[0]) for a in adapters]
        self.ad_len = np.array([len(a[1]) for a in adapters], dtype=np.int32)
        cls = {}
        self.ad_class = np.array([cls.setdefault(n, len(cls)) for n in self.ad_names], dtype=np.int32)
        self.class5 = cls.get(b"5Prime_adapter", -1)
        self.ad_name_off = np.zeros(len(adapters) + 1, dtype=np.int64)
        np.cumsum([len(n) for n in self.ad_names], out=self.ad_name_off[1:])
        self.ad_name_cat = b"".join(self.ad_names)
        self.has_index = bool(index and index[1])
        self.dests, self.idx_seqs = [""], []
        if self.has_index:
            seq_to_idx = index[1]
            self.idx_seqs = [_b(s) for s in seq_to_idx]
            names = [x for x in dict.fromkeys(seq_to_idx.values()) if x != "no_index_found"] + ["no_index_found"]
            self.dests = names
            self.idx_dest = np.array([names.index(v) for v in seq_to_idx.values()], dtype=np.int32)
        else:
            self.idx_dest = np.zeros(0, dtype=np.int32)
        self.idx_off = np.zeros(len(self.idx_seqs) + 1, dtype=np.int64)
        np.cumsum([len(s) for s in self.idx_seqs], out=self.idx_off[1:])
        self.idx_cat = b"".join(self.idx_seqs)
        self.undirectional, self.trim, self.barcoded = bool(undirectional), bool(trim), bool(barcoded)
        self.n_streams = 3 * len(self.dests) + 3


class PostBatch:
    """one batch for c3_post_emit in structure-of-arrays form: pointers (int) or numpy arrays; quals may be None.  `keep`
    holds whatever owns the memory."""

    def __init__(self, n, names, name_off, seqs, quals, off, keep=None):
        self.n, self.names, self.name_off, self.seqs, self.quals, self.off, self.keep = n, names, name_off, seqs, quals, off, keep

    @classmethod
    def from_lists(cls, names, seqs, quals=None):
        nb, sb = [_b(x) for x in names], [_b(x) for x in seqs]
        no, so = np.zeros(len(nb) + 1, dtype=np.int64), np.zeros(len(sb) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in nb], out=no[1:])
        np.cumsum([len(x) for x in sb], out=so[1:])
        arr = [np.frombuffer(b"".join(nb) + b"\0", dtype=np.uint8), np.frombuffer(b"".join(sb) + b"\0", dtype=np.uint8)]
        q = None
        if quals is not None:
            q = np.frombuffer(b"".join(_b(x) for x in quals) + b"\0", dtype=np.uint8)
            assert len(q) == len(arr[1])
        return cls(len(nb), arr[0], no, arr[1], q, so)

    @classmethod
    def from_host(cls, hb, quals=False):
        return cls(hb.n, hb.c.names, hb.name_off, hb.c.seqs, hb.c.quals if quals else None, hb.off, keep=hb)


def _ptr(x):
    return None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x)


POST_IN_BGZF, POST_OUT_BGZF, POST_KEEP_QUALS = 1, 2, 4       # flags of c3_post_emit_text


class TextResult:
    """result of c3_post_emit_text, c3_demux_emit_text and c3_demux_emit_text_host: info (dict), arena (uint8 array), stream_off
    (int64 array of S + 1), hashes (uint64 array of n_records), guards_intact, untouched_beyond_results"""

    def streams(self):
        so = self.stream_off
        return [self.arena[int(so[s]):int(so[s + 1])].tobytes() for s in range(len(so) - 1)]


PostText = DemuxText = TextResult
_SO_GUARD = -0x5A5A5A5A5A5A5A5B


def _text_call(fn, err, piece, mid, S, info, in_z, cap, max_records, bufs=None, s_max=None):
    """one "text in, file bytes out" call: fn(src, n, *mid, arena, cap, stream_off, hashes, max_records, info) with S streams (the C
    side refuses more than s_max).  piece: bytes or a uint8 array.  cap / max_records: instead of sizes found by asking again;
    C3Error (code, .info, .stream_off, .guards_intact, .untouched) on a refusal.  bufs: a dict the call keeps its output arrays in
    from one piece to the next (no guard bytes then; the results are views that the next call overwrites)."""
    src = piece if isinstance(piece, np.ndarray) else np.frombuffer(_bytes(piece), dtype=np.uint8)
    n = len(src)
    s_ok = s_max is None or S <= s_max
    so = np.zeros((S if s_ok else s_max) + 1 + 2, dtype=np.int64)
    so[0] = so[-1] = _SO_GUARD                                           # a guard word either side
    ask = cap is None and max_records is None
    cap = (24 if in_z else 3) * n + 65536 if cap is None else int(cap)
    max_records = (8 if in_z else 1) * (n // 8) + 16 if max_records is None else int(max_records)
    g = FASTA_GUARD if bufs is None else 0
    for _try in range(3):
        if bufs is None:
            arena, hashes = np.full(cap + 2 * g, 0xA5, dtype=np.uint8), np.full(8 * max_records + 2 * g, 0xA5, dtype=np.uint8)
        else:
            if len(bufs.get("arena", ())) < cap:
                bufs["arena"] = np.empty(cap, dtype=np.uint8)
            if len(bufs.get("hashes", ())) < 8 * max_records:
                bufs["hashes"] = np.empty(8 * max_records, dtype=np.uint8)
            arena, hashes, cap, max_records = bufs["arena"], bufs["hashes"], len(bufs["arena"]), len(bufs["hashes"]) // 8
        rc = fn(src.ctypes.data if n else None, n, *mid, arena.ctypes.data + g, cap, so.ctypes.data + 8, hashes.ctypes.data + g, max_records,
                C.byref(info))
        if ask and rc == E_LIMIT and s_ok and (so[S + 1] > cap or info.n_records > max_records):
            cap, max_records = max(cap, int(so[S + 1])), max(max_records, int(info.n_records))
            continue
        break
    out = TextResult()
    out.info, out.stream_off = info.as_dict(), so[1:-1]
    used = {"arena": int(so[S + 1]), "hashes": 8 * int(info.n_records)} if rc == 0 else {"arena": 0, "hashes": 0}
    out.guards_intact, out.untouched_beyond_results = _guarded({"arena": arena, "hashes": hashes}, used) if bufs is None else (True, True)
    out.guards_intact = bool(out.guards_intact and so[0] == so[-1] == _SO_GUARD)
    if rc != 0:
        e = C3Error("c3 error %d: %s" % (rc, err().decode()))
        e.code, e.info, e.stream_off, e.guards_intact, e.untouched = rc, out.info, out.stream_off, out.guards_intact, out.untouched_beyond_results
        raise e
    out.arena = arena[g:g + used["arena"]]
    out.hashes = hashes[g:g + used["hashes"]].view(np.uint64).copy()
    return out


def _post_args(plan, n, names, name_off, seqs, quals, off, table):
    return PostArgs(n, names, name_off, seqs, quals, off, table, len(plan.ad_len), plan.ad_len.ctypes.data, plan.ad_class.ctypes.data,
                    plan.class5, C.cast(C.c_char_p(plan.ad_name_cat), C.c_void_p).value, plan.ad_name_off.ctypes.data,
                    int(plan.has_index), len(plan.idx_seqs), C.cast(C.c_char_p(plan.idx_cat), C.c_void_p).value,
                    plan.idx_off.ctypes.data, plan.idx_dest.ctypes.data, len(plan.dests),
                    int(plan.undirectional), int(plan.trim), int(plan.barcoded))


def _post_call(fn, err, plan, batch, table):
    tab = np.ascontiguousarray(table, dtype=np.int32)
    n_ad = len(plan.ad_len)
    assert tab.size == batch.n * n_ad * 24
    a = _post_args(plan, batch.n, _ptr(batch.names), _ptr(batch.name_off), _ptr(batch.seqs), _ptr(batch.quals), _ptr(batch.off), tab.ctypes.data)
    S = plan.n_streams
    so = np.zeros(S + 1, dtype=np.int64)
    kept = C.c_int64(0)
    total = int(batch.off[-1]) if batch.n else 0
    cap = 3 * total * (2 if batch.quals is not None else 1) + 512 * batch.n + 4096      # a guess: the call says what it needs
    for _try in range(2):
        arena = np.empty(cap, dtype=np.uint8)
        rc = fn(C.byref(a), arena.ctypes.data, cap, so.ctypes.data, C.byref(kept))
        if rc == E_LIMIT and so[S] > cap:
            cap = int(so[S])
            continue
        break
    if rc < 0:
        e = C3Error("c3 error %d: %s" % (rc, err().decode()))
        e.code = rc
        raise e
    return arena, so, int(kept.value)


def post_emit_host(plan, batch, table):
    """c3_post_emit_host: the host statement of Handle.post_emit (same arguments and results)"""
    lib = load()
    return _post_call(lib.c3_post_emit_host, lambda: lib.c3_last_error(None), plan, batch, table)


DEMUX_HEAD = 300        # C3_DEMUX_HEAD


def _demux_args(heads, set_a, set_b, return_dist):
    """heads: (n, 300) uint8 array or a sequence of 300-byte str / bytes; sets: sequences of str / bytes.
    Returns the ctypes arguments after the handle, the arrays they point into, and the result."""
    if isinstance(heads, np.ndarray):
        h = np.ascontiguousarray(heads, dtype=np.uint8)
    else:
        bs = [_b(x) for x in heads]
        if any(len(x) != DEMUX_HEAD for x in bs):
            raise ValueError("every head must be %d bytes" % DEMUX_HEAD)
        h = np.frombuffer(b"".join(bs), dtype=np.uint8)
    h = h.reshape(-1, DEMUX_HEAD)
    n = h.shape[0]
    sets = []
    for s in (set_a, set_b):
        bs = [_b(x) for x in s]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in bs], out=off[1:])
        sets += [len(bs), b"".join(bs), off]
    win = np.zeros((n, 2), dtype=np.int32)
    dist = np.zeros((n, sets[0] + sets[3]), dtype=np.uint8) if return_dist else None
    res = (win, dist) if return_dist else win
    args = (n, h.ctypes.data, sets[0], sets[1], sets[2].ctypes.data, sets[3], sets[4], sets[5].ctypes.data, win.ctypes.data,
            dist.ctypes.data if return_dist else None)
    return args, (h, sets), res


def demux_host(heads, set_a, set_b, return_dist=False):
    """c3_demux_host: the host statement of Handle.demux_indexes (same arguments and results)"""
    lib = load()
    args, keep, res = _demux_args(heads, set_a, set_b, return_dist)
    rc = lib.c3_demux_host(*args)
    if rc < 0:
        raise C3Error("c3 error %d: %s" % (rc, lib.c3_last_error(None).decode()))
    return res


def _qv_args(cons, pieces):
    cb = _b(cons)
    seqs, quals = [_b(p[0]) for p in pieces], [_b(p[1]) for p in pieces]
    off = np.zeros(len(pieces) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in seqs], out=off[1:])
    modes = np.array([int(p[2]) for p in pieces] or [0], dtype=np.int32)
    sc, qc = b"".join(seqs) + b"\0", b"".join(quals) + b"\0"
    out = C.create_string_buffer(len(cb) + 1)
    return (cb, len(cb), len(pieces), sc, qc, off.ctypes.data, modes.ctypes.data, out), (cb, sc, qc, off, modes, out)


def consensus_qv_host(cons, pieces):
    """c3_consensus_qv_host: the host statement of Handle.consensus_qv (same arguments and result)"""
    lib = load()
    args, keep = _qv_args(cons, pieces)
    rc = lib.c3_consensus_qv_host(*args)
    if rc < 0:
        raise C3Error("c3 error %d: %s" % (rc, lib.c3_last_error(None).decode()))
    return keep[-1].raw[:len(keep[0])].decode()


def device_count():
    return int(load().c3_device_count())


def warm_device(dev):
    """create the HIP context of one device on the calling thread (nothing else); returns the c3_status"""
    return int(load().c3_warm_device(int(dev)))


class ResultBuffers:
    """grow-only host buffers for one batch of results (no page faults per batch); owned by whoever holds the object.
    pinned=True takes them from c3_host_alloc (page-locked): what c3_batch_results_begin needs to copy asynchronously"""

    def __init__(self, pinned=False):
        self.res = self.buf = self.coff = self.qv = None
        self.pinned = pinned
        self._p = {}
        self._retired = []
        self.lib = load() if pinned else None

    def _alloc(self, name, count, dtype):
        if not self.pinned:
            return np.empty(count, dtype=dtype)
        nbytes = count * np.dtype(dtype).itemsize
        p = C.c_void_p()
        if self.lib.c3_host_alloc(nbytes + 64, C.byref(p)) != 0:
            raise MemoryError("c3_host_alloc(%d)" % nbytes)
        # a buffer that grows hands its predecessor back -- but not before the NEXT fit(): the arrays handed out by the previous
        # fit() are views of it (np.frombuffer owns nothing), and ResultFetcher's callers still read them while the next batch
        # is fetched into the other buffer
        old = self._p.pop(name, None)
        if old is not None:
            self._retired.append(old)
        self._p[name] = p
        return np.frombuffer((C.c_char * nbytes).from_address(p.value), dtype=dtype, count=count)

    def _release_retired(self):
        for p in self._retired:
            self.lib.c3_host_free(p)
        self._retired = []

    def fit(self, n, cons_cap):
        if self._retired:
            self._release_retired()                   # blocks replaced by the previous fit(): their views are two batches old now
        if self.buf is None or len(self.buf) < cons_cap:
            self.buf = self._alloc("buf", cons_cap + cons_cap // 4, np.uint8)
        if self.res is None or len(self.res) < n:
            self.res = self._alloc("res", n + n // 4 + 1, RESULT_DTYPE)
        if not self.pinned:
            return self.res[:n], self.buf, np.zeros(n + 1, dtype=np.int64)
        if self.coff is None or len(self.coff) < n + 1:
            self.coff = self._alloc("coff", n + n // 4 + 2, np.int64)
        return self.res[:n], self.buf, self.coff[:n + 1]

    def fit_qv(self, cons_cap):
        """the QV buffer (same capacity as the consensus buffer), allocated on first use only"""
        if self.qv is None or len(self.qv) < cons_cap:
            self.qv = self._alloc("qv", cons_cap + cons_cap // 4, np.uint8)
        return self.qv

    def close(self):
        self.res = self.buf = self.coff = self.qv = None
        self._release_retired()
        for p in self._p.values():
            self.lib.c3_host_free(p)
        self._p = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResultFetcher:
    """software pipeline for the results of one handle: after_run() freezes the resident batch's results on the device
    (c3_batch_results_snapshot) and hands the copy to a helper thread (c3_batch_results_fetch: it runs beside the next batch's
    kernels); it returns the PREVIOUS batch's (res, cons bytes, cons_off), or None the first time.  drain() returns the last."""

    def __init__(self, handle, n_buffers=2, pinned=False):
        from concurrent.futures import ThreadPoolExecutor
        self.h = handle
        self.pool = ThreadPoolExecutor(1)
        self.rbs = [ResultBuffers(pinned=pinned) for _ in range(n_buffers)]
        self.k = 0
        self.fut = None

    def after_run(self):
        prev = self.drain()
        shape = self.h.results_snapshot()
        self.fut = self.pool.submit(self.h.results_fetch, self.rbs[self.k % len(self.rbs)], shape)
        self.k += 1
        return prev

    def drain(self):
        fut, self.fut = self.fut, None
        return fut.result() if fut is not None else None

    def close(self):
        self.drain()
        self.pool.shutdown()


class PinnedBatch:
    """one batch in flat host buffers from c3_host_alloc (page-locked when a GPU is present): what the boundary is handed"""

    def __init__(self, seq_cat, qual_cat, off, strands):
        self.lib = load()
        self.off = np.ascontiguousarray(off, dtype=np.int64)
        self.n = len(self.off) - 1
        st = _b(strands)
        assert len(st) == self.n and len(seq_cat) == self.off[-1] == len(qual_cat)
        self.strand = np.frombuffer(st, dtype=np.uint8).copy()
        self._p = []
        for src in (seq_cat, qual_cat):
            p = C.c_void_p()
            if self.lib.c3_host_alloc(len(src) + 64, C.byref(p)) != 0:
                raise MemoryError("c3_host_alloc(%d)" % len(src))
            C.memmove(p, src, len(src))
            self._p.append(p)
        self.seqs, self.quals = self._p[0].value, self._p[1].value

    def close(self):
        for p in self._p:
            self.lib.c3_host_free(p)
        self._p = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HostBatch:
    """one group of reads held by the native reader (valid until the reader reuses its buffer set)"""

    def __init__(self, c, owner=None):
        self.c = c
        self.owner = owner                       # keeps the reader (and its buffers) alive
        self.n = int(c.n)
        self.n_short = int(c.n_short)
        self.off = np.ctypeslib.as_array(C.cast(c.off, C.POINTER(C.c_int64)), shape=(self.n + 1,)).copy()
        self.name_off = np.ctypeslib.as_array(C.cast(c.name_off, C.POINTER(C.c_int64)), shape=(self.n + 1,)).copy()

    @classmethod
    def from_lists(cls, names, seqs, quals):
        """a group assembled from Python bytes (tests, tools): the arrays live as long as the object"""
        nm, sq, ql = [_b(x) for x in names], [_b(x) for x in seqs], [_b(x) for x in quals]
        assert len(nm) == len(sq) == len(ql) and all(len(a) == len(b) for a, b in zip(sq, ql))
        n = len(nm)
        no, off = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(x) for x in nm], out=no[1:]); np.cumsum([len(x) for x in sq], out=off[1:])
        keep = [np.frombuffer(b"".join(x) + b"\0" * 16, dtype=np.uint8) for x in (nm, sq, ql)] + [no, off]
        c = HostBatchStruct(n, 0, keep[0].ctypes.data, no.ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, off.ctypes.data)
        return cls(c, owner=keep)

    def names(self):
        raw = C.string_at(self.c.names, int(self.name_off[-1])) if self.n else b""
        no = self.name_off
        return [raw[no[i]:no[i + 1]].decode() for i in range(self.n)]

    def read(self, i):
        """(name, seq, qual) of read i as str -- for tests and small inputs"""
        no, o = self.name_off, self.off
        return (C.string_at(self.c.names + int(no[i]), int(no[i + 1] - no[i])).decode(),
                C.string_at(self.c.seqs + int(o[i]), int(o[i + 1] - o[i])).decode(),
                C.string_at(self.c.quals + int(o[i]), int(o[i + 1] - o[i])).decode())


class Reader:
    """native streaming FASTA/FASTQ(.gz) reader (c3_reader_*): mm.fastx_read replacement that yields SoA groups; a path
    ending in .bam is read as unaligned BAM (BGZF; the groups of the FASTQ of the same records; a record it cannot take is
    a ValueError of next naming the record, its inflated byte offset and the reason)"""

    def __init__(self, path, n_sets=3, names_only=False, byte_range=None, inflate_device=None, parse_device=False, stage_device=False):
        """byte_range = (beg, end): only the records that START inside [beg, end) (plain files; c3_reader_open_range)
        inflate_device = d: a BGZF file is inflated by k_inflate on device d (c3_reader_open_inflate; whole-file readers)
        parse_device: ... and its records are parsed there too (k_fastq, k_bam for a .bam; c3_reader_parse_on_device).  C3Error with code
        E_STATE when the reader is not one of a BGZF file with inflate_device
        stage_device: ... and the bases and qualities of its groups stay there (c3_reader_stage_on_device): a device group has
        hb.dev (c3_device_batch) and no seqs / quals; after a departure the groups are host groups (hb.dev is None)"""
        self.lib = load()
        self.r = C.c_void_p()
        self.n_sets, self._cur = max(1, int(n_sets)), -1
        if inflate_device is not None:
            if byte_range is not None:
                raise ValueError("inflate_device goes with a whole-file reader")
            rc = self.lib.c3_reader_open_inflate(_b(str(path)), n_sets, int(inflate_device), C.byref(self.r))
            if rc not in (0, E_ARG):
                raise C3Error("c3_reader_open_inflate failed (%d): %s" % (rc, self.lib.c3_last_error(None).decode()))
        elif byte_range is None:
            rc = self.lib.c3_reader_open(_b(str(path)), n_sets, C.byref(self.r))
        else:
            rc = self.lib.c3_reader_open_range(_b(str(path)), n_sets, int(byte_range[0]), int(byte_range[1]), C.byref(self.r))
        if rc != 0:
            raise OSError("cannot open %s" % path)
        if names_only:
            self.lib.c3_reader_names_only(self.r, 1)
        if parse_device:
            rc = self.lib.c3_reader_parse_on_device(self.r, 1)
            if rc != 0:
                e = C3Error("c3_reader_parse_on_device failed (%d): %s" % (rc, self.lib.c3_reader_error(self.r).decode()))
                e.code = rc
                self.close()
                raise e
        self.stage_device = False
        if stage_device:
            rc = self.lib.c3_reader_stage_on_device(self.r, 1)
            if rc != 0:
                e = C3Error("c3_reader_stage_on_device failed (%d): %s" % (rc, self.lib.c3_reader_error(self.r).decode()))
                e.code = rc
                self.close()
                raise e
            self.stage_device = True

    def next(self, max_reads, min_len=0, max_bases=0, set_index=None):
        """next group; set_index names the buffer set to fill (caller-managed free list), None = round-robin"""
        c = HostBatchStruct()
        if set_index is None:
            rc = self.lib.c3_reader_next(self.r, int(max_reads), int(max_bases), int(min_len), C.byref(c))
        else:
            rc = self.lib.c3_reader_next_set(self.r, int(set_index), int(max_reads), int(max_bases), int(min_len), C.byref(c))
        cur = self._set_of(set_index)
        if rc != 0:
            raise ValueError("c3_reader_next: %s" % self.lib.c3_reader_error(self.r).decode())
        hb = HostBatch(c, self)
        hb.set_index = set_index
        hb.dev = None
        if self.stage_device and hb.n > 0 and not c.seqs:        # a device group: its bases lie in the reader's device set
            d = DeviceBatchStruct()
            if self.lib.c3_reader_device_group(self.r, cur, C.byref(d)) != 0:
                raise ValueError("c3_reader_device_group failed")
            hb.dev = d if d.d_seqs else None
        return hb

    def _set_of(self, set_index):
        """the buffer set the call just made filled: the one named, or the next one round-robin (c3_reader_next's rule)"""
        self._cur = int(set_index) if set_index is not None else (self._cur + 1) % self.n_sets
        return self._cur

    def noqual(self):
        """records without a quality line read so far (FASTA)"""
        return int(self.lib.c3_reader_noqual(self.r))

    def reserved_bytes(self):
        return int(self.lib.c3_reader_reserved_bytes(self.r))

    def inflate_wait(self):
        """seconds the parser waited for inflated bytes of a BGZF file (either inflater); 0 for other files"""
        return float(self.lib.c3_reader_inflate_wait(self.r))

    def parse_stats(self):
        """(stretches parsed on the device, stretches parsed on the host, records delivered from the device) of a
        parse_device reader: c3_reader_parse_stats"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.lib.c3_reader_parse_stats(self.r, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def stage_stats(self):
        """(groups delivered on the device, groups delivered on the host, bytes of bases + qualities brought to the host) of a
        stage_device reader: c3_reader_stage_stats"""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self.lib.c3_reader_stage_stats(self.r, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def range_lost(self):
        """a byte-range reader whose range holds bytes but no record start (multi-line FASTQ): read the file with one reader"""
        return bool(self.lib.c3_reader_range_lost(self.r))

    def close(self):
        if self.r:
            self.lib.c3_reader_close(self.r)
            self.r = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_splint_psl(hb, table, splint_id, strand, splint_names, splint_lens, match, path):
    """c3_write_splint_psl: PSL rows of the assigned reads of one group, appended to `path`; returns the row count"""
    lib = load()
    names = (C.c_char_p * len(splint_names))(*[_b(n) for n in splint_names])
    lens = np.ascontiguousarray(splint_lens, dtype=np.int32)
    tab = np.ascontiguousarray(table, dtype=np.int32)
    sid = np.ascontiguousarray(splint_id, dtype=np.int16)
    st = np.frombuffer(_b(strand), dtype=np.uint8)
    rows = C.c_int64(0)
    rc = lib.c3_write_splint_psl(C.byref(hb.c), tab.ctypes.data, sid.ctypes.data, st.ctypes.data, len(splint_names), names,
                                 lens.ctypes.data, int(match), _b(str(path)), C.byref(rows))
    if rc != 0:
        raise OSError("c3_write_splint_psl failed (%d)" % rc)
    return int(rows.value)


class Assigner:
    """native PSL -> per-read splint / strand assignment (c3_assign_*): bin/preprocess.py:22-45 without Python objects"""

    def __init__(self, psl_path, splint_names):
        self.lib = load()
        self.names = list(splint_names)
        arr = (C.c_char_p * len(self.names))(*[_b(n) for n in self.names])
        self.a = C.c_void_p()
        if self.lib.c3_assign_open(_b(str(psl_path)), len(self.names), arr, C.byref(self.a)) != 0:
            raise OSError("cannot read %s" % psl_path)

    def batch(self, hb):
        """(splint_id int16[n] with -1 = none, strand bytes, number assigned)"""
        sid = np.zeros(hb.n, dtype=np.int16)
        st = np.zeros(hb.n, dtype=np.uint8)
        k = self.lib.c3_assign_batch(self.a, C.byref(hb.c), sid.ctypes.data, st.ctypes.data)
        if k < 0:
            raise RuntimeError("c3_assign_batch failed (%d)" % k)
        return sid, st.tobytes(), int(k)

    def seen(self):
        flags = np.zeros(len(self.names), dtype=np.uint8)
        rows = C.c_int64(0)
        self.lib.c3_assign_seen(self.a, flags.ctypes.data, C.byref(rows))
        return set(n for n, f in zip(self.names, flags) if f), int(rows.value)

    def close(self):
        if self.a:
            self.lib.c3_assign_close(self.a)
            self.a = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_group(hb, res, cons_buf, cons_off, splint_ids, cons_paths, sub_paths, zero=True):
    """c3_write_group: append the consensus / subread records of one group to the per-splint files"""
    lib = load()
    n_spl = len(cons_paths)
    cp = (C.c_char_p * n_spl)(*[_b(p) for p in cons_paths])
    sp = (C.c_char_p * n_spl)(*[_b(p) for p in sub_paths])
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64)
    rc = lib.c3_write_group(C.byref(hb.c), res.ctypes.data, cons_buf.ctypes.data if cons_buf is not None else None,
                            coff.ctypes.data, sid.ctypes.data, n_spl, cp, sp, 1 if zero else 0)
    if rc != 0:
        raise OSError("c3_write_group failed (%d)" % rc)


def write_consensus_fastq(hb, res, cons_buf, cons_off, qv_buf, splint_ids, fq_paths, zero=True):
    """c3_write_consensus_fastq: append the consensus FASTQ records (c3_write_group's FASTA records + QV line) of one group"""
    lib = load()
    n_spl = len(fq_paths)
    fp = (C.c_char_p * n_spl)(*[_b(p) for p in fq_paths])
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64)
    rc = lib.c3_write_consensus_fastq(C.byref(hb.c), res.ctypes.data, cons_buf.ctypes.data, coff.ctypes.data, qv_buf.ctypes.data,
                                      sid.ctypes.data, n_spl, fp, 1 if zero else 0)
    if rc != 0:
        raise OSError("c3_write_consensus_fastq failed (%d)" % rc)


# ---- records formatted on the GPU (--emit gpu; include/c3poa.h "Records formatted on the GPU") ----
EMIT_BGZF = 1
EMIT_KINDS = ("consensus_fasta", "subread_fastq", "consensus_fastq")


class EmitStreams:
    """result of emit_group / emit_group_host: stream x = splint * K + kind lies at arena[stream_off[x]:stream_off[x + 1]]"""

    def __init__(self, arena, stream_off, n_records, K):
        self.arena, self.stream_off, self.n_records, self.K = arena, stream_off, n_records, K

    def stream(self, x):
        return self.arena[int(self.stream_off[x]):int(self.stream_off[x + 1])].tobytes()

    def streams(self):
        return [self.stream(x) for x in range(len(self.stream_off) - 1)]


def _emit_call(fn, err, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap=None, arena=None):
    """cap None: the arena is sized by a first call with no arena (C3_E_LIMIT reports the need).  An explicit cap / arena is
    handed through as it is; a C3Error then carries .code and .stream_off."""
    K = 3 if qv_buf is not None else 2
    S = n_splints * K
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64) if cons_off is not None else None
    so = np.zeros(max(S, 0) + 2, dtype=np.int64)
    nrec = C.c_int64(0)

    def call(ar, c):
        return fn(C.byref(hb.c), res.ctypes.data if len(res) else None, cons_buf.ctypes.data if cons_buf is not None else None,
                  coff.ctypes.data if coff is not None else None, qv_buf.ctypes.data if qv_buf is not None else None,
                  sid.ctypes.data if len(sid) else None, n_splints, 1 if zero else 0, ar.ctypes.data if ar is not None else None, c,
                  so.ctypes.data, C.byref(nrec))

    if cap is None:
        rc = call(None, 0)
        if rc == E_LIMIT:
            cap = int(so[S])
            arena = np.zeros(cap + 64, dtype=np.uint8)
            rc = call(arena, cap)
        elif rc == 0:
            arena = np.zeros(0, dtype=np.uint8)
    else:
        rc = call(arena, cap)
    if rc != 0:
        e = C3Error("c3_emit_group failed (%d): %s" % (rc, err().decode()))
        e.code, e.stream_off = rc, so[:max(S, 0) + 1].copy()
        raise e
    return EmitStreams(arena, so[:S + 1].copy(), int(nrec.value), K)


def emit_group_host(hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero=True, cap=None, arena=None):
    """c3_emit_group_host: the host statement of Handle.emit_group (same arguments and results).  hb: a HostBatch; res: RESULT_DTYPE
    records; cons_buf / cons_off / qv_buf as results_raw / results_fetch_qv return them (cons_buf and qv_buf may be None)"""
    lib = load()
    return _emit_call(lib.c3_emit_group_host, lambda: lib.c3_last_error(None), hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap, arena)


class EmitBuffers:
    """a grow-only page-locked arena for Handle.emit_fetch (one per batch in flight, pooled by the pipeline)"""

    def __init__(self, nbytes=1 << 16):
        self._pb = PinnedBytes(nbytes)
        self.ptr, self.size, self.arr = self._pb.ptr, self._pb.size, self._pb.arr

    def fit(self, nbytes):
        if nbytes > self.size:
            self._pb.close()
            self._pb = PinnedBytes(nbytes + nbytes // 8)
            self.ptr, self.size, self.arr = self._pb.ptr, self._pb.size, self._pb.arr

    def close(self):
        self.arr = None
        self._pb.close()


def append_streams(paths, arena_ptr, stream_off):
    """c3_append_streams: every non-empty stream appended to paths[x] (None: skipped) with write_group's reservation"""
    lib = load()
    n = len(paths)
    pp = (C.c_char_p * max(n, 1))(*[_b(p) if p is not None else None for p in paths])
    so = np.ascontiguousarray(stream_off, dtype=np.int64)
    assert len(so) == n + 1
    rc = lib.c3_append_streams(pp, arena_ptr, so.ctypes.data, n)
    if rc != 0:
        raise OSError("c3_append_streams failed (%d): %s" % (rc, lib.c3_last_error(None).decode(errors="replace")))


# ---- BGZF output (--bgzf; include/c3poa.h "BGZF output") ----
BGZF_BLOCK = 65280              # input bytes per member
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the SAM specification's EOF member


def _bgzf_call(fn, first, data):
    lib = load()
    src = _b(data) if not isinstance(data, (bytes, bytearray, memoryview)) else bytes(data)
    cap = int(lib.c3_bgzf_bound(len(src)))
    out = C.create_string_buffer(max(cap, 1))
    olen = C.c_int64(0)
    rc = fn(*(first + (src, len(src), out, cap, C.byref(olen))))
    if rc != 0:
        raise C3Error("c3 error %d: %s" % (rc, lib.c3_last_error(None).decode()))
    return out.raw[:olen.value]


def bgzf_compress_host(data):
    """c3_bgzf_compress_host: BGZF members of `data` (no EOF member), the host statement of Bgzf.compress"""
    return _bgzf_call(load().c3_bgzf_compress_host, (), data)


# ---- BGZF input (--inflate gpu; include/c3poa.h "BGZF input") ----
def _c3_fail(rc):
    e = C3Error("c3 error %d: %s" % (rc, load().c3_last_error(None).decode()))
    e.code = rc
    return e


def _bytes(data):
    return _b(data) if not isinstance(data, (bytes, bytearray, memoryview)) else bytes(data)


def bgzf_scan(data):
    """c3_bgzf_scan: (members, inflated bytes) of a buffer of whole BGZF members, from the headers alone"""
    src = _bytes(data)
    nm, ob = C.c_int64(0), C.c_int64(0)
    rc = load().c3_bgzf_scan(src, len(src), C.byref(nm), C.byref(ob))
    if rc != 0:
        raise _c3_fail(rc)
    return nm.value, ob.value


def _bgzf_inflate(fn, first, data):
    src = _bytes(data)
    cap = bgzf_scan(src)[1]
    out = C.create_string_buffer(max(cap, 1))
    olen = C.c_int64(0)
    rc = fn(*(first + (src, len(src), out, cap, C.byref(olen))))
    if rc != 0:
        raise _c3_fail(rc)
    return out.raw[:olen.value]


def bgzf_decompress_host(data):
    """c3_bgzf_decompress_host: the text of the BGZF members `data`; the host statement of Bgzf.decompress (no zlib)"""
    return _bgzf_inflate(load().c3_bgzf_decompress_host, (), data)


# ---- FASTQ records on the GPU (--parse gpu; include/c3poa.h "FASTQ records on the GPU") ----
FASTQ_GUARD = 64                # bytes of 0xA5 either side of every output array of a fastq_parse call


class FastqParse:
    """result of c3_fastq_parse / c3_fastq_parse_host: info (dict), names / seqs / quals (bytes), name_off / off (int64
    arrays of n_kept + 1), guards_intact (the FASTQ_GUARD bytes either side of every output array are untouched)"""

    def records(self):
        no, o = self.name_off, self.off
        return [(self.names[no[i]:no[i + 1]], self.seqs[o[i]:o[i + 1]], self.quals[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def _fastq_call(fn, first, text, at_eof, min_len, text_offset=0, caps=None, bam_at_start=None):
    """bam_at_start is None: a FASTQ call; else a BAM call (at_start in front of at_eof, a BamInfo, room for 2 bases per byte)"""
    src = _bytes(text)
    n = len(src)
    # the text at byte `text_offset` (0..3) of a dword
    raw = np.zeros(n + 16, dtype=np.uint8)
    at = (-raw.ctypes.data) % 4 + int(text_offset)
    raw[at:at + n] = np.frombuffer(src, dtype=np.uint8)
    fit = (n, n // 2 + 1, n // 7 + 1) if bam_at_start is None else (n, n, n // 38 + 1)
    names_cap, bases_cap, max_records = caps if caps is not None else fit
    g = FASTQ_GUARD

    def arr(nbytes):
        a = np.full(nbytes + 2 * g, 0xA5, dtype=np.uint8)
        return a

    bufs = {"names": arr(names_cap), "seqs": arr(bases_cap), "quals": arr(bases_cap),
            "name_off": arr(8 * (max_records + 1)), "off": arr(8 * (max_records + 1))}
    ptr = {k: v.ctypes.data + g for k, v in bufs.items()}
    info = FastqInfo() if bam_at_start is None else BamInfo()
    kind = () if bam_at_start is None else (int(bool(bam_at_start)),)
    rc = fn(*(first + (raw.ctypes.data + at if n else None, n) + kind + (int(bool(at_eof)), int(min_len), ptr["names"], names_cap, ptr["name_off"],
                       ptr["seqs"], ptr["quals"], bases_cap, ptr["off"], max_records, C.byref(info))))
    out = FastqParse()
    out.info = info.as_dict()
    used = {"names": 0, "seqs": 0, "quals": 0, "name_off": 0, "off": 0}
    if rc == 0:
        nk = out.info["n_kept"]
        used = {"names": out.info["name_bytes"], "seqs": out.info["base_bytes"], "quals": out.info["base_bytes"],
                "name_off": 8 * (nk + 1), "off": 8 * (nk + 1)}
    # guards, and on a refused call every byte of the arrays: nothing half written
    out.guards_intact = all(bool((v[:g] == 0xA5).all()) and bool((v[len(v) - g:] == 0xA5).all()) for v in bufs.values())
    out.untouched_beyond_results = all(bool((v[g + used[k]:] == 0xA5).all()) for k, v in bufs.items())
    if rc != 0:
        e = _c3_fail(rc)
        e.info, e.guards_intact, e.untouched = out.info, out.guards_intact, out.untouched_beyond_results
        raise e
    for k in ("names", "seqs", "quals"):
        setattr(out, k, bufs[k][g:g + used[k]].tobytes())
    for k in ("name_off", "off"):
        setattr(out, k, bufs[k][g:g + used[k]].view(np.int64).copy())
    return out


def fastq_parse_host(text, at_eof=False, min_len=0, text_offset=0, caps=None):
    """c3_fastq_parse_host: the longest prefix of whole strict records of `text`; the host statement of Bgzf.fastq_parse.
    caps = (names_cap, bases_cap, max_records) instead of sizes that always fit; C3Error (code E_LIMIT, .info) when too small"""
    return _fastq_call(load().c3_fastq_parse_host, (), text, at_eof, min_len, text_offset, caps)


# ---- Unaligned BAM records on the GPU (-r reads.bam; include/c3poa.h "Unaligned BAM records on the GPU") ----
BAM_TILE = 65536                # C3_BAM_TILE: bytes of data per chain tile of k_bam
BAM_MAX_RECORD = 1 << 28        # C3_BAM_MAX_RECORD
BAM_REASONS = ("OK", "BLOCK", "NAME", "FIELDS", "FLAG", "EMPTY", "NOQUAL", "TRUNCATED", "HEADER")      # c3_bam_info.reason


def bam_parse_host(data, at_start=True, at_eof=False, min_len=0, text_offset=0, caps=None):
    """c3_bam_parse_host: the file header (at_start) and the longest prefix of whole strict records of the inflated BAM bytes
    `data`; the host statement of Bgzf.bam_parse.  The result object, text_offset and caps of fastq_parse_host; info also has
    header_bytes, reason (an index of BAM_REASONS) and bad_at"""
    return _fastq_call(load().c3_bam_parse_host, (), data, at_eof, min_len, text_offset, caps, bam_at_start=bool(at_start))


# ---- Sample demultiplexer, text in / file bytes out (C3POa_demux.py --emit gpu) ----
FASTA_GUARD = 64                # bytes of 0xA5 either side of every output array of a fasta_parse / demux_emit call
FASTA_MAX_TEXT = 0x7FF00000


def fasta_max_records(n):
    """records a text of n bytes can hold at most (a record is at least '>' and a terminator; the last may lack it)"""
    return n // 2 + 1


class FastaParse:
    """result of c3_fasta_parse / c3_fasta_parse_host: info (dict), names / seqs (bytes), name_off / off (int64 arrays of
    n_records + 1), hashes (uint64 array), guards_intact, untouched_beyond_results"""

    def records(self):
        no, o = self.name_off, self.off
        return [(self.names[no[i]:no[i + 1]], self.seqs[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def _guarded(bufs, used):
    g = FASTA_GUARD
    intact = all(bool((v[:g] == 0xA5).all()) and bool((v[len(v) - g:] == 0xA5).all()) for v in bufs.values())
    untouched = all(bool((v[g + used[k]:] == 0xA5).all()) for k, v in bufs.items())
    return intact, untouched


def _fasta_call(fn, err, text, at_eof, caps=None):
    src = _bytes(text)
    n = len(src)
    names_cap, bases_cap, max_records = caps if caps is not None else (n, n, fasta_max_records(n))
    g = FASTA_GUARD
    sizes = {"names": names_cap, "seqs": bases_cap, "name_off": 8 * (max_records + 1), "off": 8 * (max_records + 1), "hashes": 8 * max_records}
    bufs = {k: np.full(v + 2 * g, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    ptr = {k: v.ctypes.data + g for k, v in bufs.items()}
    info = FastaInfo()
    rc = fn(src if n else None, n, int(bool(at_eof)), ptr["names"], names_cap, ptr["name_off"], ptr["seqs"], bases_cap, ptr["off"],
            ptr["hashes"], max_records, C.byref(info))
    out = FastaParse()
    out.info = info.as_dict()
    used = dict.fromkeys(sizes, 0)
    if rc == 0:
        nr = out.info["n_records"]
        used = {"names": out.info["name_bytes"], "seqs": out.info["base_bytes"], "name_off": 8 * (nr + 1), "off": 8 * (nr + 1), "hashes": 8 * nr}
    out.guards_intact, out.untouched_beyond_results = _guarded(bufs, used)
    if rc != 0:
        e = C3Error("c3 error %d: %s" % (rc, err().decode()))
        e.code, e.info, e.guards_intact, e.untouched = rc, out.info, out.guards_intact, out.untouched_beyond_results
        raise e
    for k in ("names", "seqs"):
        setattr(out, k, bufs[k][g:g + used[k]].tobytes())
    for k in ("name_off", "off"):
        setattr(out, k, bufs[k][g:g + used[k]].view(np.int64).copy())
    out.hashes = bufs["hashes"][g:g + used["hashes"]].view(np.uint64).copy()
    return out


def fasta_parse_host(text, at_eof=True, caps=None):
    """c3_fasta_parse_host: the host statement of Handle.fasta_parse.  caps = (names_cap, bases_cap, max_records) instead of
    sizes that always fit; C3Error (code E_LIMIT, .info) when too small"""
    lib = load()
    return _fasta_call(lib.c3_fasta_parse_host, lambda: lib.c3_last_error(None), text, at_eof, caps)


# ---- Strict FASTA / FASTQ records (the input of C3POa_postprocessing.py) ----
class FastxParse:
    """result of c3_fastx_strict_parse_host: info (dict), names / seqs / quals (bytes; quals None for kind 2), name_off / off
    (int64 arrays of n_records + 1), hashes (uint64 array), guards_intact, untouched_beyond_results"""

    def records(self):
        no, o = self.name_off, self.off
        q = self.quals
        return [(self.names[no[i]:no[i + 1]], self.seqs[o[i]:o[i + 1]], q[o[i]:o[i + 1]] if q is not None else None)
                for i in range(len(o) - 1)]


def fastx_kind(first_byte):
    """the kind a file's first byte announces: 4 ('@'), 2 ('>') or 0 (neither: a departure)"""
    return {b"@": 4, b">": 2}.get(bytes(first_byte[:1]), 0)


def fastx_max_records(n, kind):
    """records a text of n bytes can hold at most (a record is at least one byte and a '\n' per line; the last may lack it)"""
    return (n + 1) // (2 * kind) + 1


def fastx_strict_parse_host(text, at_eof=False, kind=2, caps=None):
    """c3_fastx_strict_parse_host: the longest prefix of whole strict records of `text` (kind 2: two-line FASTA, kind 4: FASTQ).
    caps = (names_cap, bases_cap, max_records) instead of sizes that always fit; C3Error (code E_LIMIT, .info) when too small"""
    lib = load()
    src = _bytes(text)
    n = len(src)
    names_cap, bases_cap, max_records = caps if caps is not None else (n, n, fastx_max_records(n, kind if kind in (2, 4) else 2))
    g = FASTA_GUARD
    sizes = {"names": names_cap, "seqs": bases_cap, "quals": bases_cap if kind == 4 else 0, "name_off": 8 * (max_records + 1),
             "off": 8 * (max_records + 1), "hashes": 8 * max_records}
    bufs = {k: np.full(v + 2 * g, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
    ptr = {k: v.ctypes.data + g for k, v in bufs.items()}
    info = FastxInfo()
    rc = lib.c3_fastx_strict_parse_host(src if n else None, n, int(bool(at_eof)), int(kind), ptr["names"], names_cap, ptr["name_off"],
                                        ptr["seqs"], ptr["quals"] if kind == 4 else None, bases_cap, ptr["off"], ptr["hashes"],
                                        max_records, C.byref(info))
    out = FastxParse()
    out.info = info.as_dict()
    used = dict.fromkeys(sizes, 0)
    if rc == 0:
        nr = out.info["n_records"]
        used = {"names": out.info["name_bytes"], "seqs": out.info["base_bytes"], "quals": out.info["base_bytes"] if kind == 4 else 0,
                "name_off": 8 * (nr + 1), "off": 8 * (nr + 1), "hashes": 8 * nr}
    out.guards_intact, out.untouched_beyond_results = _guarded(bufs, used)
    if rc != 0:
        e = _c3_fail(rc)
        e.info, e.guards_intact, e.untouched = out.info, out.guards_intact, out.untouched_beyond_results
        raise e
    for k in ("names", "seqs"):
        setattr(out, k, bufs[k][g:g + used[k]].tobytes())
    out.quals = bufs["quals"][g:g + used["quals"]].tobytes() if kind == 4 else None
    for k in ("name_off", "off"):
        setattr(out, k, bufs[k][g:g + used[k]].view(np.int64).copy())
    out.hashes = bufs["hashes"][g:g + used["hashes"]].view(np.uint64).copy()
    return out


class DemuxSets:
    """the two index sets of c3_demux_emit: (names, sequences) of the Nextera and the TSO indexes in file order (str or bytes)"""

    def __init__(self, a_names, a_seqs, b_names, b_seqs):
        self._keep, args = [], []
        self.max_name = [0, 0]
        for s, (names, seqs) in enumerate(((a_names, a_seqs), (b_names, b_seqs))):
            nb, sb = [_b(x) for x in names], [_b(x) for x in seqs]
            if len(nb) != len(sb):
                raise ValueError("an index set needs one name per sequence")
            self.max_name[s] = max([len(x) for x in nb] or [0])
            so, no = np.zeros(len(sb) + 1, dtype=np.int64), np.zeros(len(nb) + 1, dtype=np.int64)
            np.cumsum([len(x) for x in sb], out=so[1:])
            np.cumsum([len(x) for x in nb], out=no[1:])
            sc, nc = b"".join(sb) + b"\0", b"".join(nb) + b"\0"
            self._keep += [sc, nc, so, no]
            args += [len(sb), C.cast(C.c_char_p(sc), C.c_void_p).value, so.ctypes.data, C.cast(C.c_char_p(nc), C.c_void_p).value, no.ctypes.data]
        self.args = tuple(args)

    def out_bound(self, n):
        """bytes c3_demux_emit can return at most for a text of n bytes"""
        return n + (n // 302 + 1) * (5 + self.max_name[0] + self.max_name[1]) + 16

    @property
    def struct(self):
        """the sets as a c3_demux_sets"""
        return DemuxSetsStruct(*self.args)

    @property
    def n_split_streams(self):
        """streams of c3_demux_emit_text with DEMUX_SPLIT: (n_a + 1) * (n_b + 1)"""
        return (self.args[0] + 1) * (self.args[5] + 1)


class DemuxEmit:
    """result of c3_demux_emit / c3_demux_emit_host: info (dict), out (bytes), hashes (uint64 array of n_records),
    guards_intact, untouched_beyond_results"""


def _demux_emit_call(fn, err, text, sets, at_eof, cap=None, max_records=None):
    src = _bytes(text)
    n = len(src)
    cap = sets.out_bound(n) if cap is None else int(cap)
    max_records = fasta_max_records(n) if max_records is None else int(max_records)
    g = FASTA_GUARD
    bufs = {"out": np.full(cap + 2 * g, 0xA5, dtype=np.uint8), "hashes": np.full(8 * max_records + 2 * g, 0xA5, dtype=np.uint8)}
    info = DemuxInfo()
    rc = fn(src if n else None, n, int(bool(at_eof)), *(sets.args + (bufs["out"].ctypes.data + g, cap, bufs["hashes"].ctypes.data + g, max_records, C.byref(info))))
    res = DemuxEmit()
    res.info = info.as_dict()
    used = {"out": res.info["out_bytes"], "hashes": 8 * res.info["n_records"]} if rc == 0 else {"out": 0, "hashes": 0}
    res.guards_intact, res.untouched_beyond_results = _guarded(bufs, used)
    if rc != 0:
        e = C3Error("c3 error %d: %s" % (rc, err().decode()))
        e.code, e.info, e.guards_intact, e.untouched = rc, res.info, res.guards_intact, res.untouched_beyond_results
        raise e
    res.out = bufs["out"][g:g + used["out"]].tobytes()
    res.hashes = bufs["hashes"][g:g + used["hashes"]].view(np.uint64).copy()
    return res


def demux_emit_host(text, sets, at_eof=True, cap=None, max_records=None):
    """c3_demux_emit_host: the host statement of Handle.demux_emit (same arguments and results)"""
    lib = load()
    return _demux_emit_call(lib.c3_demux_emit_host, lambda: lib.c3_last_error(None), text, sets, at_eof, cap, max_records)


# ---- Sample demultiplexer, pieces of text in / per-sample streams out (C3POa_demux.py --parse gpu) ----
DEMUX_IN_BGZF, DEMUX_OUT_BGZF, DEMUX_KEEP_QUALS, DEMUX_SPLIT = 1, 2, 4, 8     # flags of c3_demux_emit_text
DEMUX_MAX_STREAMS = 4096


def _demux_text_call(fn, err, sets, piece, at_eof, kind, flags, cap, max_records, bufs=None):
    """one c3_demux_emit_text (kind None) or c3_demux_emit_text_host call through _text_call"""
    st = sets.struct
    mid = (int(bool(at_eof)),) + (() if kind is None else (int(kind),)) + (int(flags), C.byref(st))
    return _text_call(fn, err, piece, mid, sets.n_split_streams if flags & DEMUX_SPLIT else 1, DemuxTextInfo(), bool(flags & DEMUX_IN_BGZF),
                      cap, max_records, bufs, DEMUX_MAX_STREAMS)


def demux_emit_text_host(sets, text, at_eof=True, kind=2, flags=0, cap=None, max_records=None):
    """c3_demux_emit_text_host: the host statement of Handle.demux_emit_text for one plain text of a stated kind"""
    lib = load()
    return _demux_text_call(lib.c3_demux_emit_text_host, lambda: lib.c3_last_error(None), sets, text, at_eof, kind, flags, cap, max_records)


class PinnedBytes:
    """a page-locked byte buffer from c3_host_alloc (plain memory without a GPU): .arr is a uint8 view, .ptr its address"""

    def __init__(self, nbytes):
        self.lib = load()
        self._p = C.c_void_p()
        if self.lib.c3_host_alloc(int(nbytes) + 64, C.byref(self._p)) != 0:
            raise MemoryError("c3_host_alloc(%d)" % nbytes)
        self.ptr, self.size = self._p.value, int(nbytes)
        self.arr = np.frombuffer((C.c_uint8 * self.size).from_address(self.ptr), dtype=np.uint8)

    def close(self):
        if self._p:
            self.arr = None
            self.lib.c3_host_free(self._p)
            self._p = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bgzf:
    """c3_bgzf: k_bgzf on one device (device buffers and a stream of its own; one per thread)"""

    def __init__(self, device=0):
        self.lib = load()
        self.z = C.c_void_p()
        rc = self.lib.c3_bgzf_create(int(device), C.byref(self.z))
        if rc != 0:
            raise C3Error("c3_bgzf_create failed (%d): %s" % (rc, self.lib.c3_last_error(None).decode()))

    def compress(self, data):
        return _bgzf_call(self.lib.c3_bgzf_compress, (self.z,), data)

    def decompress(self, data):
        """c3_bgzf_decompress: the text of the BGZF members `data` (k_inflate); C3Error with code E_DATA on a damaged member"""
        return _bgzf_inflate(self.lib.c3_bgzf_decompress, (self.z,), data)

    def fastq_parse(self, text, at_eof=False, min_len=0, text_offset=0, caps=None):
        """c3_fastq_parse: the strict FASTQ records of `text` found and gathered by k_fastq (a FastqParse); text_offset
        0..3 = where the text starts inside a dword, which the device copy keeps"""
        return _fastq_call(self.lib.c3_fastq_parse, (self.z,), text, at_eof, min_len, text_offset, caps)

    def bam_parse(self, data, at_start=True, at_eof=False, min_len=0, text_offset=0, caps=None):
        """c3_bam_parse: the strict records of the inflated BAM bytes `data` found and gathered by k_bam (a FastqParse whose
        info is that of bam_parse_host); text_offset places the data at that byte (0..3) of a dword"""
        return _fastq_call(self.lib.c3_bam_parse, (self.z,), data, at_eof, min_len, text_offset, caps, bam_at_start=bool(at_start))

    def close(self):
        if self.z:
            self.lib.c3_bgzf_destroy(self.z)
            self.z = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_group_bgzf(z, hb, res, cons_buf, cons_off, splint_ids, cons_paths, sub_paths, zero=True):
    """c3_write_group_bgzf: write_group with each file's text compressed by k_bgzf; the paths name the .gz files"""
    lib = load()
    n_spl = len(cons_paths)
    cp = (C.c_char_p * n_spl)(*[_b(p) for p in cons_paths])
    sp = (C.c_char_p * n_spl)(*[_b(p) for p in sub_paths])
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64)
    rc = lib.c3_write_group_bgzf(z.z, C.byref(hb.c), res.ctypes.data, cons_buf.ctypes.data if cons_buf is not None else None,
                                 coff.ctypes.data, sid.ctypes.data, n_spl, cp, sp, 1 if zero else 0)
    if rc != 0:
        raise OSError("c3_write_group_bgzf failed (%d): %s" % (rc, lib.c3_last_error(None).decode()))


def write_consensus_fastq_bgzf(z, hb, res, cons_buf, cons_off, qv_buf, splint_ids, fq_paths, zero=True):
    """c3_write_consensus_fastq_bgzf: write_consensus_fastq with each file's text compressed by k_bgzf"""
    lib = load()
    n_spl = len(fq_paths)
    fp = (C.c_char_p * n_spl)(*[_b(p) for p in fq_paths])
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64)
    rc = lib.c3_write_consensus_fastq_bgzf(z.z, C.byref(hb.c), res.ctypes.data, cons_buf.ctypes.data, coff.ctypes.data,
                                           qv_buf.ctypes.data, sid.ctypes.data, n_spl, fp, 1 if zero else 0)
    if rc != 0:
        raise OSError("c3_write_consensus_fastq_bgzf failed (%d): %s" % (rc, lib.c3_last_error(None).decode()))

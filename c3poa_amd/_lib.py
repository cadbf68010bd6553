"""ctypes binding of the HIP backend (c3poa_amd/lib/libc3poa_hip.so, C ABI in include/c3poa.h).

There is NO CPU fallback: importing this module without the built library, or creating a handle
without an MI355X, raises.

Layout: the structures, the prototype table and load(), the helpers every wrapper shares (one error path, one owner base,
one offsets helper, one guarded-output helper), the Handle, then the handle-free calls in the section order of the header.
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
E_ARG, E_DATA = -3, -7          # include/c3poa.h c3_err
E_STATE, E_LIMIT = -5, -6

ZERO_MAX_CELLS = 16777216       # c3_default_config's zero_max_cells: largest front * tail the zero-repeat rescue takes


# ---- the structures of include/c3poa.h (tests/test_cabi.py compares their fields with the header) ----
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


class HostBatchStruct(C.Structure):
    _fields_ = [("n", C.c_int32), ("n_short", C.c_int64), ("names", C.c_void_p), ("name_off", C.c_void_p),
                ("seqs", C.c_void_p), ("quals", C.c_void_p), ("off", C.c_void_p)]


class QvTiming(C.Structure):
    _fields_ = [("ms_qv", C.c_float)] + [(n, C.c_int64) for n in ("n_reads", "n_pieces", "n_skipped", "band_cells", "edge_hits")]


class FastqInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "n_short", "consumed", "name_bytes", "base_bytes")] + [("departed", C.c_int32)]


class BamInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "n_short", "consumed", "name_bytes", "base_bytes", "header_bytes", "bad_at")] + \
               [("departed", C.c_int32), ("reason", C.c_int32)]


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


class FastaInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "consumed", "name_bytes", "base_bytes")] + [("departed", C.c_int32)]


class DemuxInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "consumed", "out_bytes")] + [("departed", C.c_int32)]


class DemuxTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_parse", "ms_demux", "ms_emit", "ms_call")] + \
               [(n, C.c_int64) for n in ("n_records", "n_kept", "in_bytes", "out_bytes")]


class EmitTiming(C.Structure):
    _fields_ = [(k, C.c_float) for k in ("ms_len", "ms_scan", "ms_write", "ms_bgzf", "ms_call")] + \
               [(k, C.c_int64) for k in ("n_reads", "n_records", "in_bytes", "out_bytes")]


class FastxInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "consumed", "name_bytes", "base_bytes")] + [("departed", C.c_int32)]


class PostTextInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "consumed", "text_bytes", "out_bytes")] + [("departed", C.c_int32)]


class PostTextTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_inflate", "ms_parse", "ms_gather", "ms_adapter", "ms_post", "ms_bgzf", "ms_call")] + \
               [(n, C.c_int64) for n in ("n_records", "n_kept", "in_bytes", "text_bytes", "out_bytes")]


class DemuxSetsStruct(C.Structure):       # c3_demux_sets
    _fields_ = [f for k in "ab" for f in [("n_" + k, C.c_int)] + [(k + f, C.c_void_p) for f in ("_cat", "_off", "_names", "_name_off")]]


class DemuxTextInfo(_Info):
    _fields_ = [(k, C.c_int64) for k in ("n_records", "n_kept", "consumed", "text_bytes", "out_bytes")] + \
               [(k, C.c_int32) for k in ("departed", "kind", "n_streams")]


class DemuxTextTiming(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("ms_inflate", "ms_parse", "ms_demux", "ms_split", "ms_emit", "ms_bgzf", "ms_call")] + \
               [(n, C.c_int64) for n in ("n_records", "n_kept", "in_bytes", "text_bytes", "out_bytes")] + \
               [(n, C.c_int32) for n in ("n_streams", "n_waits")]


class DeviceBatchStruct(C.Structure):      # c3_device_batch
    _fields_ = [("d_seqs", C.c_void_p), ("d_quals", C.c_void_p), ("device", C.c_int32), ("bytes", C.c_int64)]


# ---- the prototypes of include/c3poa.h: name -> (restype, argtypes), in the header's order.  load() applies the table and
# EXPORTS is its key list, so an export cannot lack a prototype; tests/test_cabi.py compares every entry with the header ----
def _prototypes():
    i, i64, dbl, vp, cp = C.c_int, C.c_int64, C.c_double, C.c_void_p, C.c_char_p
    P, ip, i64p = C.POINTER, C.POINTER(C.c_int), C.c_void_p
    pvp, pcp, pi64, hb = P(vp), P(cp), P(i64), P(HostBatchStruct)
    # shared tails: the device form of a call is its host form behind the handle
    up = [i, vp, vp, i64p, vp, vp]                                           # c3_batch_upload / _stage behind the handle
    res = [vp, vp, i64, i64p]                                                # c3_batch_results* behind the handle
    dx = [i, vp, i, cp, vp, i, cp, vp, vp, vp]                               # c3_demux_indexes / _host
    qv = [cp, i, i, vp, vp, vp, vp, vp]                                      # c3_consensus_qv / _host
    wg = [hb, vp, vp, vp, vp, i, pcp, pcp, i]                                # c3_write_group / _bgzf
    wq = [hb, vp, vp, vp, vp, vp, i, pcp, i]                                 # c3_write_consensus_fastq / _bgzf
    zz = [vp, i64, vp, i64, pi64]                                            # c3_bgzf_compress / _decompress / _host
    fq = [vp, i64, i, i, vp, i64, vp, vp, vp, i64, vp, i64, P(FastqInfo)]
    bam = [vp, i64, i, i, i, vp, i64, vp, vp, vp, i64, vp, i64, P(BamInfo)]
    pe = [P(PostArgs), vp, i64, vp, vp]                                      # c3_post_emit / _host
    fa = [vp, i64, i, vp, i64, vp, vp, i64, vp, vp, i64, P(FastaInfo)]
    de = [vp, i64, i] + [i, vp, vp, vp, vp] * 2 + [vp, i64, vp, i64, P(DemuxInfo)]
    em = [hb, vp, vp, vp, vp, vp, i, i, vp, i64, vp, pi64]
    dt = [vp, i64, i]
    dt2 = [i, P(DemuxSetsStruct), vp, i64, vp, vp, i64, P(DemuxTextInfo)]
    st3 = [vp, pi64, pi64, pi64]                                             # c3_reader_parse_stats / _stage_stats
    return {
        "c3_default_config": (None, [P(Config)]),
        "c3_version": (cp, []),
        "c3_device_count": (i, []),
        "c3_warm_device": (i, [i]),
        "c3_create": (i, [P(Config), pvp]),
        "c3_destroy": (None, [vp]),
        "c3_last_error": (cp, [vp]),
        "c3_set_splints": (i, [vp, i, cp, i64p]),
        "c3_batch_upload": (i, [vp] + up),
        "c3_batch_stage": (i, [vp] + up),
        "c3_batch_commit": (i, [vp]),
        "c3_batch_assign": (i, [vp, vp, vp]),
        "c3_batch_run": (i, [vp, i]),
        "c3_batch_sync": (i, [vp]),
        "c3_batch_results": (i, [vp] + res),
        "c3_batch_results_snapshot": (i, [vp]),
        "c3_batch_results_fetch": (i, [vp] + res),
        "c3_batch_timing": (i, [vp, P(Timing)]),
        "c3_fetch_track": (i, [vp, i, vp, i64]),
        "c3_fetch_smoothed": (i, [vp, i, vp, i64]),
        "c3_fetch_raw_peaks": (i, [vp, i, vp, i]),
        "c3_fetch_draft": (i, [vp, i, vp, i]),
        "c3_fetch_msa2": (i, [vp, i, vp, vp, i]),
        "c3_call_peaks": (i, [vp, vp, i, i, vp, i, vp]),
        "c3_poa_msa": (i, [vp, i, pcp, ip, vp, i, ip, vp, i64, ip]),
        "c3_pairwise_consensus": (i, [vp, cp, cp, i, cp, i, cp, cp, i, cp, vp, i, ip]),
        "c3_determine_consensus": (i, [vp, i, pcp, pcp, ip, cp, cp, i, cp, cp, i, vp, i, ip, vp, i, ip]),
        "c3_scan_splints": (i, [vp, vp, vp, vp]),
        "c3_scan_adapters": (i, [vp, vp]),
        "c3_zero_repeats": (i, [vp, cp, cp, i, cp, cp, i, i, vp, i, ip]),
        "c3_host_alloc": (i, [i64, pvp]),
        "c3_host_free": (None, [vp]),
        "c3_reader_open": (i, [cp, i, pvp]),
        "c3_reader_open_range": (i, [cp, i, i64, i64, pvp]),
        "c3_reader_close": (None, [vp]),
        "c3_reader_error": (cp, [vp]),
        "c3_reader_noqual": (i64, [vp]),
        "c3_reader_reserved_bytes": (i64, [vp]),
        "c3_reader_range_lost": (i, [vp]),
        "c3_reader_names_only": (None, [vp, i]),
        "c3_reader_next": (i, [vp, i, i64, i, hb]),
        "c3_reader_next_set": (i, [vp, i, i, i64, i, hb]),
        "c3_write_group": (i, wg),
        "c3_writer_reset": (None, []),
        "c3_assign_open": (i, [cp, i, pcp, pvp]),
        "c3_assign_close": (None, [vp]),
        "c3_assign_batch": (i, [vp, hb, vp, vp]),
        "c3_assign_seen": (i, [vp, vp, vp]),
        "c3_write_splint_psl": (i, [hb, vp, vp, vp, i, pcp, vp, i, cp, vp]),
        "c3_match_index_batch": (i, [vp, i, vp, vp, i, cp, vp, vp]),
        "c3_match_index": (i, [cp, i, i, cp, vp]),
        "c3_demux_indexes": (i, [vp] + dx),
        "c3_demux_host": (i, dx),
        "c3_batch_qv_timing": (i, [vp, P(QvTiming)]),
        "c3_batch_results_fetch_qv": (i, [vp] + res + [vp]),
        "c3_batch_results_qv": (i, [vp] + res + [vp]),
        "c3_consensus_qv": (i, [vp] + qv),
        "c3_consensus_qv_host": (i, qv),
        "c3_write_consensus_fastq": (i, wq),
        "c3_bgzf_create": (i, [i, pvp]),
        "c3_bgzf_destroy": (None, [vp]),
        "c3_bgzf_bound": (i64, [i64]),
        "c3_bgzf_compress": (i, [vp] + zz),
        "c3_bgzf_compress_host": (i, zz),
        "c3_bgzf_scan": (i, [vp, i64, pi64, pi64]),
        "c3_bgzf_decompress": (i, [vp] + zz),
        "c3_bgzf_decompress_host": (i, zz),
        "c3_gunzip": (i, [vp] + zz),
        "c3_gunzip_host": (i, zz + [i64]),
        "c3_gunzip_stats": (i, [pi64, i]),
        "c3_reader_open_inflate": (i, [cp, i, i, pvp]),
        "c3_reader_gunzip_on_device": (i, [vp, i]),
        "c3_reader_gunzip_stats": (i, [vp, pi64, i]),
        "c3_reader_inflate_wait": (dbl, [vp]),
        "c3_write_group_bgzf": (i, [vp] + wg),
        "c3_write_consensus_fastq_bgzf": (i, [vp] + wq),
        "c3_fastq_parse": (i, [vp] + fq),
        "c3_fastq_parse_host": (i, fq),
        "c3_reader_parse_on_device": (i, [vp, i]),
        "c3_reader_parse_stats": (i, st3),
        "c3_bam_parse": (i, [vp] + bam),
        "c3_bam_parse_host": (i, bam),
        "c3_post_emit": (i, [vp] + pe),
        "c3_post_emit_host": (i, pe),
        "c3_post_emit_timing": (i, [vp, P(PostTiming)]),
        "c3_fasta_parse": (i, [vp] + fa),
        "c3_fasta_parse_host": (i, fa),
        "c3_demux_emit": (i, [vp] + de),
        "c3_demux_emit_host": (i, de),
        "c3_demux_emit_timing": (i, [vp, P(DemuxTiming)]),
        "c3_emit_group": (i, [vp] + em),
        "c3_emit_group_host": (i, em),
        "c3_batch_emit_snapshot": (i, [vp, vp, vp, i, i]),
        "c3_batch_emit_fetch": (i, [vp, vp, i64, vp]),
        "c3_emit_timing_get": (i, [vp, P(EmitTiming)]),
        "c3_append_streams": (i, [pcp, vp, vp, i]),
        "c3_emit_group_bam": (i, [vp] + em),
        "c3_emit_group_bam_host": (i, em),
        "c3_bam_out_header": (i, [vp, i64, pi64]),
        "c3_fastx_strict_parse_host": (i, [vp, i64, i, i, vp, i64, vp, vp, vp, i64, vp, vp, i64, P(FastxInfo)]),
        "c3_post_emit_text": (i, [vp, vp, i64, i, i, P(PostArgs), vp, i64, vp, vp, i64, P(PostTextInfo)]),
        "c3_post_text_reset": (i, [vp]),
        "c3_post_text_timing_get": (i, [vp, P(PostTextTiming)]),
        "c3_demux_emit_text": (i, [vp] + dt + dt2),
        "c3_demux_emit_text_host": (i, dt + [i] + dt2),
        "c3_demux_text_reset": (i, [vp]),
        "c3_demux_text_timing_get": (i, [vp, P(DemuxTextTiming)]),
        "c3_reader_stage_on_device": (i, [vp, i]),
        "c3_reader_device_group": (i, [vp, i, P(DeviceBatchStruct)]),
        "c3_reader_stage_stats": (i, st3),
    }


_PROTOTYPES = _prototypes()
EXPORTS = list(_PROTOTYPES)
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
    for name, (restype, argtypes) in _PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


# ---- what every wrapper shares ----
class C3Error(RuntimeError):
    code = None                 # the c3_err value of the refused call (E_DATA: damaged input)


def _c3_error(rc, err=None, what=None, **attrs):
    """the one place a C3Error is made: the code rc with the text of its source.  err: the source, a callable that returns the
    text (Handle._err: c3_last_error(h); Reader._err: c3_reader_error(r)), None for c3_last_error(NULL), False for a call that
    leaves no text.  what: the message names the call ("<what> failed (rc)").  attrs: what the call attaches to its refusal."""
    text = "" if err is False else ": %s" % (err() if err else load().c3_last_error(None)).decode()
    e = C3Error("c3 error %d%s" % (rc, text) if what is None else "%s failed (%d)%s" % (what, rc, text))
    e.code = rc
    for k, v in attrs.items():
        setattr(e, k, v)
    return e


class _Owned:
    """base of the objects that own something native: close() frees it (_free says what; closing twice is harmless), `with`
    closes on the way out, and an object that is dropped unclosed frees it without ever raising from the collector"""
    _owns = None                # (attribute that holds the pointer, the export that frees it), for owners of one pointer

    def _free(self):
        attr, fn = self._owns
        if getattr(self, attr):
            getattr(self.lib, fn)(getattr(self, attr))
            setattr(self, attr, C.c_void_p())

    def close(self):
        self._free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _b(s):
    """str, bytes, bytearray or memoryview as bytes"""
    return s if isinstance(s, bytes) else bytes(s) if isinstance(s, (bytearray, memoryview)) else s.encode()


def _ptr(x):
    return None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x)


def _cat(items, tail=b""):
    """a list of str / bytes as the C side takes it: (the items joined + tail, their int64 offsets [len + 1])"""
    bs = [_b(x) for x in items]
    off = np.zeros(len(bs) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, bs), np.int64, len(bs)), out=off[1:])
    return b"".join(bs) + tail, off


GUARD = 64                      # bytes of 0xA5 either side of every output array of a guarded call
FASTQ_GUARD = FASTA_GUARD = GUARD


class _Outputs:
    """the named output arrays of one call, from a dict name -> byte size.  Guarded (keep is None): every array is filled with
    0xA5 and has GUARD bytes either side; ptr[name] points behind the front guard; after the call settle() says whether the guards
    are intact and whether every byte beyond the results is untouched (on a refused call: every byte), and take() / view() slice
    the results out.  keep = a dict: the arrays live in it from one call to the next, grow only, and have no guards."""

    def __init__(self, sizes, keep=None):
        self.g = GUARD if keep is None else 0
        if keep is None:
            self.arr = {k: np.full(v + 2 * GUARD, 0xA5, dtype=np.uint8) for k, v in sizes.items()}
        else:
            for k, v in sizes.items():
                if len(keep.get(k, ())) < v:
                    keep[k] = np.empty(v, dtype=np.uint8)
            self.arr = keep
        self.ptr = {k: self.arr[k].ctypes.data + self.g for k in sizes}
        self.used = {}

    def cap(self, k):
        return len(self.arr[k]) - 2 * self.g

    def check(self, used):
        """(guards_intact, untouched_beyond_results) for used = name -> bytes of results (a missing name: none)"""
        g = self.g
        if not g:
            return True, True
        intact = all(bool((v[:g] == 0xA5).all()) and bool((v[len(v) - g:] == 0xA5).all()) for v in self.arr.values())
        untouched = all(bool((v[g + used.get(k, 0):] == 0xA5).all()) for k, v in self.arr.items())
        return intact, untouched

    def settle(self, out, rc, err, info, used, intact=True, **attrs):
        """after the call: out.info, out.guards_intact (and `intact`, a guard of the caller's own) and
        out.untouched_beyond_results; a refusal (rc != 0) used nothing and raises the C3Error of source `err` with .info,
        .guards_intact, .untouched and attrs"""
        self.used = used if rc == 0 else {}
        out.info = info.as_dict()
        ok, out.untouched_beyond_results = self.check(self.used)
        out.guards_intact = bool(ok and intact)
        if rc != 0:
            raise _c3_error(rc, err, info=out.info, guards_intact=out.guards_intact, untouched=out.untouched_beyond_results, **attrs)

    def view(self, k):
        """the results of array k as a uint8 view"""
        return self.arr[k][self.g:self.g + self.used[k]]

    def take(self, out, /, **kinds):
        """out.<name> = the results of array <name>: bytes for None, else a copy of that dtype (np.int64, np.uint64)"""
        for k, dtype in kinds.items():
            setattr(out, k, self.view(k).tobytes() if dtype is None else self.view(k).view(dtype).copy())


def default_config(**kw):
    cfg = Config()
    load().c3_default_config(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def device_count():
    return int(load().c3_device_count())


def warm_device(dev):
    """create the HIP context of one device on the calling thread (nothing else); returns the c3_status"""
    return int(load().c3_warm_device(int(dev)))


class Handle(_Owned):
    """One per GPU (c3_create / c3_destroy)."""
    _owns = ("h", "c3_destroy")

    def __init__(self, **cfg):
        self.lib = load()
        self.cfg = default_config(**cfg)
        self.h = C.c_void_p()
        rc = self.lib.c3_create(C.byref(self.cfg), C.byref(self.h))
        if rc != 0:
            raise _c3_error(rc, None, "c3_create")
        self.n = 0
        self.lens = None

    def _err(self):
        return self.lib.c3_last_error(self.h)

    def _chk(self, rc):
        if rc < 0:
            raise _c3_error(rc, self._err)
        return rc

    def _timing(self, fn, Struct):
        t = Struct()
        self._chk(fn(self.h, C.byref(t)))
        return _fields_dict(t)

    def set_splints(self, splints):
        """splints: list of sequences (order defines splint_id)"""
        cat, off = _cat(splints)
        self._chk(self.lib.c3_set_splints(self.h, len(off) - 1, cat, off.ctypes.data))
        self.n_splints = len(off) - 1

    def upload(self, seqs, quals, strands, splint_ids=None):
        """seqs/quals: lists of str/bytes (or pre-joined bytes with `lens`), strands: '+'/'-' per read"""
        cat, off = _cat(seqs)
        self.upload_flat(cat, b"".join(_b(q) for q in quals), off,
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
        self._chk(self.lib.c3_batch_upload(self.h, n, sq.ctypes.data, qq.ctypes.data, off.ctypes.data, _ptr(sid),
                                           np.frombuffer(st, dtype=np.uint8).ctypes.data))
        self.n = n
        self.off = off

    def _send_host(self, fn, hb, strands, splint_ids):
        st = np.frombuffer(_b(strands), dtype=np.uint8)
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
        assert len(st) == hb.n == len(sid)
        self._chk(fn(self.h, hb.n, hb.c.seqs, hb.c.quals, hb.c.off, sid.ctypes.data, st.ctypes.data))

    def _send_pinned(self, fn, pb, splint_ids):
        sid = np.ascontiguousarray(splint_ids, dtype=np.int16) if splint_ids is not None else None
        self._chk(fn(self.h, pb.n, pb.seqs, pb.quals, pb.off.ctypes.data, _ptr(sid), pb.strand.ctypes.data))

    def upload_host(self, hb, strands, splint_ids):
        """upload a HostBatch of the native reader straight from its (page-locked) buffers: no Python copies"""
        self._send_host(self.lib.c3_batch_upload, hb, strands, splint_ids)
        self.n = hb.n
        self.off = hb.off

    def stage_host(self, hb, strands, splint_ids):
        """c3_batch_stage: copy the NEXT batch on the second stream while the resident one is processed; the HostBatch
        must stay alive until commit()"""
        self._send_host(self.lib.c3_batch_stage, hb, strands, splint_ids)
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
        self._send_pinned(self.lib.c3_batch_upload, pb, splint_ids)
        self.n, self.off = pb.n, pb.off

    def stage_pinned(self, pb, splint_ids=None):
        """c3_batch_stage from a PinnedBatch; the batch must stay alive until commit()"""
        self._send_pinned(self.lib.c3_batch_stage, pb, splint_ids)
        self._staged = (pb.n, pb.off, pb)

    def run(self, stages=STAGES_ALL, qv=False):
        """qv=True adds STAGE_QV (per-base consensus QVs after the polish)"""
        self._chk(self.lib.c3_batch_run(self.h, stages | (STAGE_QV if qv else 0)))
        self.last_timing = self.timing()         # c3_batch_commit clears the library's copy
        if qv:
            self.last_qv_timing = self.qv_timing()

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
            raise _c3_error(rc, False, "c3_batch_results_fetch")
        return res, buf, coff

    def results_fetch_qv(self, into, shape):
        """results_fetch + the QV bytes (c3_batch_results_fetch_qv): (res, cons bytes, cons_off, QV bytes at the same offsets)"""
        res, buf, coff = into.fit(*shape)
        qv = into.fit_qv(shape[1])
        rc = self.lib.c3_batch_results_fetch_qv(self.h, res.ctypes.data, buf.ctypes.data, len(buf), coff.ctypes.data, qv.ctypes.data)
        if rc != 0:
            raise _c3_error(rc, False, "c3_batch_results_fetch_qv")
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
        return self._timing(self.lib.c3_batch_timing, Timing)

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

    # ---- stand-alone stages
    def call_peaks(self, scores, min_dist, return_smoothed=False):
        s = np.ascontiguousarray(scores, dtype=np.int32)
        pk = np.zeros(MAX_PEAKS, dtype=np.int32)
        sm = np.zeros(len(s), dtype=np.float64) if return_smoothed else None
        n = self._chk(self.lib.c3_call_peaks(self.h, s.ctypes.data, len(s), int(min_dist), pk.ctypes.data, MAX_PEAKS, _ptr(sm)))
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

    def pairwise_consensus(self, msa_rows, subreads, quals):
        """pairwise_consensus(msa_rows, subreads, quals) of bin/consensus.py:76"""
        ra, rb = _b(msa_rows[0]), _b(msa_rows[1])
        sa, sb, qa, qb = _b(subreads[0]), _b(subreads[1]), _b(quals[0]), _b(quals[1])
        out = C.create_string_buffer(len(ra) + 1)
        ol = C.c_int(0)
        self._chk(self.lib.c3_pairwise_consensus(self.h, ra, rb, len(ra), sa, len(sa), qa, sb, len(sb), qb, out, len(ra) + 1, C.byref(ol)))
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

    def zero_repeats(self, d0, q0, d1, q1, min_len=0):
        b0, b1 = _b(d0), _b(d1)
        cap = len(b0) + len(b1) + 16
        out = C.create_string_buffer(cap)
        ol = C.c_int(0)
        self._chk(self.lib.c3_zero_repeats(self.h, b0, _b(q0), len(b0), b1, _b(q1), len(b1), int(min_len), out, cap, C.byref(ol)))
        return out.raw[:ol.value].decode()

    # ---- index matching and the sample demultiplexer
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
        cat, off = _cat(index_seqs)
        out = np.zeros(n, dtype=np.int32)
        self._chk(self.lib.c3_match_index_batch(self.h, n, buf.ctypes.data, lens.ctypes.data, len(off) - 1, cat, off.ctypes.data, out.ctypes.data))
        return out

    def demux_indexes(self, heads, set_a, set_b, return_dist=False):
        """c3_demux_indexes (k_demux): winners (n, 2) int32 of index sets A and B (index number or -1) for every head
        (300 bytes each, see _demux_args), and with return_dist the (n, len(A) + len(B)) uint8 minimum distances"""
        args, keep, res = _demux_args(heads, set_a, set_b, return_dist)
        self._chk(self.lib.c3_demux_indexes(self.h, *args))
        return res

    # ---- consensus quality values
    def qv_timing(self):
        """c3_batch_qv_timing: k_qv figures of the last run with STAGE_QV"""
        return self._timing(self.lib.c3_batch_qv_timing, QvTiming)

    def consensus_qv(self, cons, pieces):
        """c3_consensus_qv (k_qv): Phred+33 QV string of `cons` from pieces = [(seq, qual, mode)], mode QV_GLOBAL /
        QV_ANCHOR_START / QV_ANCHOR_END"""
        args, keep = _qv_args(cons, pieces)
        self._chk(self.lib.c3_consensus_qv(self.h, *args))
        return keep[-1].raw[:len(keep[0])].decode()

    # ---- post-processing on the GPU
    def post_emit(self, plan, batch, table):
        """c3_post_emit (k_post): the finished file bytes of one batch.  plan: a PostPlan; batch: a PostBatch; table: what
        scan_adapters returned for the batch.  Returns (arena uint8 array, stream_off[S + 1], kept reads)."""
        return _post_call(lambda *a: self.lib.c3_post_emit(self.h, *a), self._err, plan, batch, table)

    def post_emit_timing(self):
        """c3_post_emit_timing: event times of the three passes of the last post_emit and the call with its copies"""
        return self._timing(self.lib.c3_post_emit_timing, PostTiming)

    # ---- sample demultiplexer, text in / file bytes out
    def fasta_parse(self, text, at_eof=True, caps=None):
        """c3_fasta_parse (k_fasta): the FASTA records of `text` as read_fasta reads them (a FastaParse)"""
        return _fasta_call(lambda *a: self.lib.c3_fasta_parse(self.h, *a), self._err, text, at_eof, caps)

    def demux_emit(self, text, sets, at_eof=True, cap=None, max_records=None):
        """c3_demux_emit (k_fasta, k_demux): FASTA text in, the bytes of Indexed_reads.fasta out (a DemuxEmit).  sets: a DemuxSets"""
        return _demux_emit_call(lambda *a: self.lib.c3_demux_emit(self.h, *a), self._err, text, sets, at_eof, cap, max_records)

    def demux_emit_raw(self, ptr, n, at_eof, sets, out, hashes):
        """c3_demux_emit on caller-owned buffers: text at address `ptr` (n bytes), out (uint8 array) and hashes (uint64 array)
        as capacities.  Returns (rc, info dict); nothing is raised, so that the caller can grow a buffer on E_LIMIT."""
        info = DemuxInfo()
        rc = self.lib.c3_demux_emit(self.h, ptr if n else None, n, int(bool(at_eof)), *(sets.args + (out.ctypes.data, out.size, hashes.ctypes.data, hashes.size, C.byref(info))))
        return rc, info.as_dict()

    def demux_emit_timing(self):
        """c3_demux_emit_timing: event times of the parse kernels, k_demux and the emit kernels of the last demux_emit, and
        the call with its copies"""
        return self._timing(self.lib.c3_demux_emit_timing, DemuxTiming)

    # ---- records formatted on the GPU
    def emit_group(self, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero=True, cap=None, arena=None):
        """c3_emit_group (k_emit): the file bytes of write_group (+ write_consensus_fastq with qv_buf) for one group, as an
        EmitStreams.  Same arguments as emit_group_host."""
        return _emit_call(lambda *a: self.lib.c3_emit_group(self.h, *a), self._err,
                          hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap, arena)

    def emit_group_bam(self, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero=True, cap=None, arena=None):
        """c3_emit_group_bam (k_bamout): the records of emit_group as uncompressed BAM records, two streams per splint
        (consensus, subreads).  Same arguments as emit_group_bam_host."""
        return _emit_call(lambda *a: self.lib.c3_emit_group_bam(self.h, *a), self._err,
                          hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap, arena, bam=True)

    def emit_snapshot(self, hb, zero=True, bgzf=False, qv=False, bam=False):
        """c3_batch_emit_snapshot: formats the records of the resident batch (whose names are hb's) on the device and freezes
        the streams; the handle may then commit and run the next batch.  bam: BAM records (two streams per splint, the QVs as
        consensus qualities) instead of text.  Returns the number of streams emit_fetch delivers."""
        no = np.ascontiguousarray(hb.name_off, dtype=np.int64)
        self._chk(self.lib.c3_batch_emit_snapshot(self.h, hb.c.names, no.ctypes.data, 1 if zero else 0,
                                                  (EMIT_BGZF if bgzf else 0) | (EMIT_BAM if bam else 0)))
        return self.n_splints * (3 if qv and not bam else 2)

    def emit_fetch(self, into, n_streams):
        """c3_batch_emit_fetch: (arena bytes, stream_off[n_streams + 1]) of the emit snapshot in `into` (an EmitBuffers); may run
        on ANOTHER thread while this handle's owner works on the next batch.  An arena that is too small is grown once."""
        so = np.zeros(n_streams + 1, dtype=np.int64)
        rc = self.lib.c3_batch_emit_fetch(self.h, into.ptr, into.size, so.ctypes.data)
        if rc == E_LIMIT:
            into.fit(int(so[n_streams]))
            rc = self.lib.c3_batch_emit_fetch(self.h, into.ptr, into.size, so.ctypes.data)
        if rc != 0:
            raise _c3_error(rc, False, "c3_batch_emit_fetch")
        return into, so

    def emit_timing(self):
        """c3_emit_timing_get: event times of the last emit_group, or of the snapshot the last emit_fetch delivered"""
        return self._timing(self.lib.c3_emit_timing_get, EmitTiming)

    # ---- text in / file bytes out
    def post_emit_text(self, plan, piece, at_eof=False, in_bgzf=False, out_bgzf=False, keep_quals=False, cap=None, max_records=None, bufs=None):
        """c3_post_emit_text: the next piece of a consensus file (bytes; whole BGZF members with in_bgzf) through parse,
        k_adapter and k_post on the device.  Returns a PostText: info (dict), arena (uint8 array), stream_off[S + 1], hashes
        (uint64 array of n_records), guards_intact.  cap / max_records: instead of sizes found by asking again; C3Error (code,
        .info, .stream_off, .guards_intact, .untouched) on a refusal.  bufs: a dict the call keeps its output arrays in from one
        piece to the next (no guard bytes then; the results are views that the next call overwrites)."""
        flags = (POST_IN_BGZF if in_bgzf else 0) | (POST_OUT_BGZF if out_bgzf else 0) | (POST_KEEP_QUALS if keep_quals else 0)
        a = _post_args(plan, 0, None, None, None, None, None, None)
        return _text_call(lambda *x: self.lib.c3_post_emit_text(self.h, *x), self._err, piece,
                          (int(bool(at_eof)), flags, C.byref(a)), plan.n_streams, PostTextInfo(), in_bgzf, cap, max_records, bufs)

    def post_text_reset(self):
        """c3_post_text_reset: drops the tail the text path keeps between two pieces and forgets the file's kind"""
        self._chk(self.lib.c3_post_text_reset(self.h))

    def post_text_timing(self):
        """c3_post_text_timing_get: times of the last post_emit_text"""
        return self._timing(self.lib.c3_post_text_timing_get, PostTextTiming)

    def demux_emit_text(self, sets, piece, at_eof=False, flags=0, cap=None, max_records=None, bufs=None):
        """c3_demux_emit_text: the next piece of a read file (bytes or a uint8 array; whole BGZF members with DEMUX_IN_BGZF)
        through parse, k_demux, k_dsplit and k_bgzf on the device.  sets: a DemuxSets.  Returns a DemuxText (_text_call)."""
        return _demux_text_call(lambda *a: self.lib.c3_demux_emit_text(self.h, *a), self._err, sets, piece, at_eof,
                                None, flags, cap, max_records, bufs)

    def demux_text_reset(self):
        """c3_demux_text_reset: drops the tail the demultiplexer's text path keeps between two pieces and forgets the file's kind"""
        self._chk(self.lib.c3_demux_text_reset(self.h))

    def demux_text_timing(self):
        """c3_demux_text_timing_get: times, counts and stream waits of the last demux_emit_text"""
        return self._timing(self.lib.c3_demux_text_timing_get, DemuxTextTiming)


# ---- host I/O either side of the path (include/c3poa.h "host I/O either side of the path") ----
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
        (nm, no), (sq, off), (ql, qoff) = (_cat(x, b"\0" * 16) for x in (names, seqs, quals))
        assert len(no) == len(off) == len(qoff) and (off == qoff).all()
        keep = [np.frombuffer(x, dtype=np.uint8) for x in (nm, sq, ql)] + [no, off]
        c = HostBatchStruct(len(off) - 1, 0, keep[0].ctypes.data, no.ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, off.ctypes.data)
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


def _host_alloc(lib, nbytes):
    """nbytes (+ 64 spare) from c3_host_alloc as a c_void_p"""
    p = C.c_void_p()
    if lib.c3_host_alloc(int(nbytes) + 64, C.byref(p)) != 0:
        raise MemoryError("c3_host_alloc(%d)" % nbytes)
    return p


class PinnedBytes(_Owned):
    """a page-locked byte buffer from c3_host_alloc (plain memory without a GPU): .arr is a uint8 view, .ptr its address"""
    _owns = ("_p", "c3_host_free")

    def __init__(self, nbytes):
        self.lib = load()
        self._p = _host_alloc(self.lib, nbytes)
        self.ptr, self.size = self._p.value, int(nbytes)
        self.arr = np.frombuffer((C.c_uint8 * self.size).from_address(self.ptr), dtype=np.uint8)

    def _free(self):
        if self._p:
            self.arr = None
        super()._free()


class PinnedBatch(_Owned):
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
            self._p.append(_host_alloc(self.lib, len(src)))
            C.memmove(self._p[-1], src, len(src))
        self.seqs, self.quals = self._p[0].value, self._p[1].value

    def _free(self):
        for p in self._p:
            self.lib.c3_host_free(p)
        self._p = []


class ResultBuffers(_Owned):
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
        p = _host_alloc(self.lib, nbytes)
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

    def _free(self):
        self.res = self.buf = self.coff = self.qv = None
        self._release_retired()
        for p in self._p.values():
            self.lib.c3_host_free(p)
        self._p = {}


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


class Reader(_Owned):
    """native streaming FASTA/FASTQ(.gz) reader (c3_reader_*): mm.fastx_read replacement that yields SoA groups; a path
    ending in .bam is read as unaligned BAM (BGZF; the groups of the FASTQ of the same records; a record it cannot take is
    a ValueError of next naming the record, its inflated byte offset and the reason)"""
    _owns = ("r", "c3_reader_close")

    def __init__(self, path, n_sets=3, names_only=False, byte_range=None, inflate_device=None, parse_device=False, stage_device=False,
                 gunzip_device=False):
        """byte_range = (beg, end): only the records that START inside [beg, end) (plain files; c3_reader_open_range)
        inflate_device = d: a BGZF file is inflated by k_inflate on device d (c3_reader_open_inflate; whole-file readers)
        parse_device: ... and its records are parsed there too (k_fastq, k_bam for a .bam; c3_reader_parse_on_device).  C3Error with code
        E_STATE when the reader is not one of a BGZF file with inflate_device
        stage_device: ... and the bases and qualities of its groups stay there (c3_reader_stage_on_device): a device group has
        hb.dev (c3_device_batch) and no seqs / quals; after a departure the groups are host groups (hb.dev is None)
        gunzip_device: a plain gzip file (not BGZF) is inflated by the k_gunzip kernels on inflate_device instead of gzread
        (c3_reader_gunzip_on_device); C3Error with code E_STATE on any other reader"""
        self.lib = load()
        self.r = C.c_void_p()
        self.n_sets, self._cur, self.parse_device = max(1, int(n_sets)), -1, bool(parse_device)
        if inflate_device is not None:
            if byte_range is not None:
                raise ValueError("inflate_device goes with a whole-file reader")
            rc = self.lib.c3_reader_open_inflate(_b(str(path)), n_sets, int(inflate_device), C.byref(self.r))
            if rc not in (0, E_ARG):
                raise _c3_error(rc, None, "c3_reader_open_inflate")
        elif byte_range is None:
            rc = self.lib.c3_reader_open(_b(str(path)), n_sets, C.byref(self.r))
        else:
            rc = self.lib.c3_reader_open_range(_b(str(path)), n_sets, int(byte_range[0]), int(byte_range[1]), C.byref(self.r))
        if rc != 0:
            raise OSError("cannot open %s" % path)
        if names_only:
            self.lib.c3_reader_names_only(self.r, 1)
        self.stage_device = False
        for want, call in ((gunzip_device, "c3_reader_gunzip_on_device"), (parse_device, "c3_reader_parse_on_device"),
                           (stage_device, "c3_reader_stage_on_device")):
            rc = getattr(self.lib, call)(self.r, 1) if want else 0
            if rc != 0:
                e = _c3_error(rc, self._err, call)
                self.close()
                raise e
        self.stage_device = bool(stage_device)

    def _err(self):
        return self.lib.c3_reader_error(self.r)

    def next(self, max_reads, min_len=0, max_bases=0, set_index=None):
        """next group; set_index names the buffer set to fill (caller-managed free list), None = round-robin"""
        c = HostBatchStruct()
        if set_index is None:
            rc = self.lib.c3_reader_next(self.r, int(max_reads), int(max_bases), int(min_len), C.byref(c))
        else:
            rc = self.lib.c3_reader_next_set(self.r, int(set_index), int(max_reads), int(max_bases), int(min_len), C.byref(c))
        cur = self._set_of(set_index)
        if rc != 0:
            raise ValueError("c3_reader_next: %s" % self._err().decode())
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

    def range_lost(self):
        """a byte-range reader whose range holds bytes but no record start (multi-line FASTQ): read the file with one reader"""
        return bool(self.lib.c3_reader_range_lost(self.r))

    def inflate_wait(self):
        """seconds the parser waited for inflated bytes of a BGZF file (either inflater); 0 for other files"""
        return float(self.lib.c3_reader_inflate_wait(self.r))

    def gunzip_stats(self):
        """the counters of gunzip_stats() summed over the stretches a gunzip_device reader has inflated so far"""
        v = (C.c_int64 * len(GUNZIP_STATS))()
        self.lib.c3_reader_gunzip_stats(self.r, v, len(GUNZIP_STATS))
        return dict(zip(GUNZIP_STATS, (int(x) for x in v)))

    def _stats(self, fn):
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        fn(self.r, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value

    def parse_stats(self):
        """(stretches parsed on the device, stretches parsed on the host, records delivered from the device) of a
        parse_device reader: c3_reader_parse_stats"""
        return self._stats(self.lib.c3_reader_parse_stats)

    def stage_stats(self):
        """(groups delivered on the device, groups delivered on the host, bytes of bases + qualities brought to the host) of a
        stage_device reader: c3_reader_stage_stats"""
        return self._stats(self.lib.c3_reader_stage_stats)


def _write_group(call, z, hb, res, cons_buf, cons_off, qv, splint_ids, paths, zero):
    """one of the four group writers: z = a Bgzf or None (the plain files), qv = (address of the QV bytes,) for the FASTQ
    writers and () for the others, paths = one list of per-splint paths for each file kind the writer appends to"""
    lib = load()
    n_spl = len(paths[0])
    pp = [(C.c_char_p * n_spl)(*[_b(p) for p in ps]) for ps in paths]
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64)
    rc = getattr(lib, call)(*(() if z is None else (z.z,)), C.byref(hb.c), res.ctypes.data, _ptr(cons_buf), coff.ctypes.data, *qv,
                            sid.ctypes.data, n_spl, *pp, 1 if zero else 0)
    if rc != 0:
        raise OSError("%s failed (%d)" % (call, rc) + ("" if z is None else ": %s" % lib.c3_last_error(None).decode()))


def write_group(hb, res, cons_buf, cons_off, splint_ids, cons_paths, sub_paths, zero=True):
    """c3_write_group: append the consensus / subread records of one group to the per-splint files"""
    _write_group("c3_write_group", None, hb, res, cons_buf, cons_off, (), splint_ids, (cons_paths, sub_paths), zero)


class Assigner(_Owned):
    """native PSL -> per-read splint / strand assignment (c3_assign_*): bin/preprocess.py:22-45 without Python objects"""
    _owns = ("a", "c3_assign_close")

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


def match_index(seq, index_seqs):
    """c3_match_index: number of the winning index (file order) or -1 (match_index, C3POa_postprocessing.py:266-285)"""
    cat, off = _cat(index_seqs)
    sq = _b(seq)
    return int(load().c3_match_index(sq, len(sq), len(off) - 1, cat, off.ctypes.data))


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
        cat, off = _cat(s)
        sets += [len(off) - 1, cat, off]
    win = np.zeros((n, 2), dtype=np.int32)
    dist = np.zeros((n, sets[0] + sets[3]), dtype=np.uint8) if return_dist else None
    res = (win, dist) if return_dist else win
    args = (n, h.ctypes.data, sets[0], sets[1], sets[2].ctypes.data, sets[3], sets[4], sets[5].ctypes.data, win.ctypes.data,
            dist.ctypes.data if return_dist else None)
    return args, (h, sets), res


def demux_host(heads, set_a, set_b, return_dist=False):
    """c3_demux_host: the host statement of Handle.demux_indexes (same arguments and results)"""
    args, keep, res = _demux_args(heads, set_a, set_b, return_dist)
    rc = load().c3_demux_host(*args)
    if rc < 0:
        raise _c3_error(rc)
    return res


# ---- per-base consensus quality values (include/c3poa.h "per-base consensus quality values") ----
def _qv_args(cons, pieces):
    cb = _b(cons)
    sc, off = _cat([p[0] for p in pieces], b"\0")
    qc = b"".join(_b(p[1]) for p in pieces) + b"\0"
    modes = np.array([int(p[2]) for p in pieces] or [0], dtype=np.int32)
    out = C.create_string_buffer(len(cb) + 1)
    return (cb, len(cb), len(pieces), sc, qc, off.ctypes.data, modes.ctypes.data, out), (cb, sc, qc, off, modes, out)


def consensus_qv_host(cons, pieces):
    """c3_consensus_qv_host: the host statement of Handle.consensus_qv (same arguments and result)"""
    args, keep = _qv_args(cons, pieces)
    rc = load().c3_consensus_qv_host(*args)
    if rc < 0:
        raise _c3_error(rc)
    return keep[-1].raw[:len(keep[0])].decode()


def write_consensus_fastq(hb, res, cons_buf, cons_off, qv_buf, splint_ids, fq_paths, zero=True):
    """c3_write_consensus_fastq: append the consensus FASTQ records (c3_write_group's FASTA records + QV line) of one group"""
    _write_group("c3_write_consensus_fastq", None, hb, res, cons_buf, cons_off, (qv_buf.ctypes.data,), splint_ids, (fq_paths,), zero)


# ---- BGZF output and input (--bgzf, --inflate gpu; include/c3poa.h "BGZF output" / "BGZF input") ----
BGZF_BLOCK = 65280              # input bytes per member
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")   # the SAM specification's EOF member


def _bgzf_call(fn, first, data, cap_of):
    """fn(*first, src, n, dst, cap, &out_len) with cap = cap_of(src): the bytes it wrote"""
    src = _b(data)
    cap = cap_of(src)
    out = C.create_string_buffer(max(cap, 1))
    olen = C.c_int64(0)
    rc = fn(*first, src, len(src), out, cap, C.byref(olen))
    if rc != 0:
        raise _c3_error(rc)
    return out.raw[:olen.value]


def _bgzf_bound(src):
    return int(load().c3_bgzf_bound(len(src)))


def _bgzf_inflated(src):
    return bgzf_scan(src)[1]


def bgzf_compress_host(data):
    """c3_bgzf_compress_host: BGZF members of `data` (no EOF member), the host statement of Bgzf.compress"""
    return _bgzf_call(load().c3_bgzf_compress_host, (), data, _bgzf_bound)


def bgzf_scan(data):
    """c3_bgzf_scan: (members, inflated bytes) of a buffer of whole BGZF members, from the headers alone"""
    src = _b(data)
    nm, ob = C.c_int64(0), C.c_int64(0)
    rc = load().c3_bgzf_scan(src, len(src), C.byref(nm), C.byref(ob))
    if rc != 0:
        raise _c3_error(rc)
    return nm.value, ob.value


def bgzf_decompress_host(data):
    """c3_bgzf_decompress_host: the text of the BGZF members `data`; the host statement of Bgzf.decompress (no zlib)"""
    return _bgzf_call(load().c3_bgzf_decompress_host, (), data, _bgzf_inflated)


# ---- gzip input (include/c3poa.h "gzip input") ----
GUNZIP_STATS = ("pieces", "candidates", "accepted", "rejected", "relaunches", "full_slabs", "fallback_bytes", "stretches")


def gunzip_stats():
    """c3_gunzip_stats: the counters of this thread's last gunzip call, by name"""
    v = (C.c_int64 * len(GUNZIP_STATS))()
    rc = load().c3_gunzip_stats(v, len(GUNZIP_STATS))
    if rc != 0:
        raise _c3_error(rc)
    return dict(zip(GUNZIP_STATS, (int(x) for x in v)))


def _gunzip_call(fn, first, data, last):
    """fn(*first, src, n, dst, cap, &out_len, *last): the text of the gzip file `data`.  A gzip file does not say how long its
    text is (ISIZE is the last member's, modulo 2^32), so cap grows while the call answers E_ARG, up to deflate's 1032 : 1"""
    src = _b(data)
    top = 1032 * len(src) + 65536
    cap = min(top, max(1 << 16, 6 * len(src)))
    while True:
        out = C.create_string_buffer(cap)
        olen = C.c_int64(0)
        rc = fn(*first, src, len(src), out, cap, C.byref(olen), *last)
        if rc == 0:
            return out.raw[:olen.value]
        if rc != E_ARG or cap >= top or not len(src):
            raise _c3_error(rc)
        cap = min(top, 4 * cap)


def gunzip_host(data, piece=0):
    """c3_gunzip_host: the text of the gzip file `data` (any RFC 1952 file); the host statement of Bgzf.gunzip (no zlib).
    piece > 0: the piece size in compressed bytes instead of C3_GUNZIP_PIECE / the default"""
    return _gunzip_call(load().c3_gunzip_host, (), data, (int(piece),))


class Bgzf(_Owned):
    """c3_bgzf: k_bgzf on one device (device buffers and a stream of its own; one per thread)"""
    _owns = ("z", "c3_bgzf_destroy")

    def __init__(self, device=0):
        self.lib = load()
        self.z = C.c_void_p()
        rc = self.lib.c3_bgzf_create(int(device), C.byref(self.z))
        if rc != 0:
            raise _c3_error(rc, None, "c3_bgzf_create")

    def compress(self, data):
        return _bgzf_call(self.lib.c3_bgzf_compress, (self.z,), data, _bgzf_bound)

    def decompress(self, data):
        """c3_bgzf_decompress: the text of the BGZF members `data` (k_inflate); C3Error with code E_DATA on a damaged member"""
        return _bgzf_call(self.lib.c3_bgzf_decompress, (self.z,), data, _bgzf_inflated)

    def gunzip(self, data):
        """c3_gunzip: the text of the gzip file `data` inflated by the k_gunzip kernels; C3Error with code E_DATA on damage"""
        return _gunzip_call(self.lib.c3_gunzip, (self.z,), data, ())

    def fastq_parse(self, text, at_eof=False, min_len=0, text_offset=0, caps=None):
        """c3_fastq_parse: the strict FASTQ records of `text` found and gathered by k_fastq (a FastqParse); text_offset
        0..3 = where the text starts inside a dword, which the device copy keeps"""
        return _fastq_call(self.lib.c3_fastq_parse, (self.z,), text, at_eof, min_len, text_offset, caps)

    def bam_parse(self, data, at_start=True, at_eof=False, min_len=0, text_offset=0, caps=None):
        """c3_bam_parse: the strict records of the inflated BAM bytes `data` found and gathered by k_bam (a FastqParse whose
        info is that of bam_parse_host); text_offset places the data at that byte (0..3) of a dword"""
        return _fastq_call(self.lib.c3_bam_parse, (self.z,), data, at_eof, min_len, text_offset, caps, bam_at_start=bool(at_start))


def write_group_bgzf(z, hb, res, cons_buf, cons_off, splint_ids, cons_paths, sub_paths, zero=True):
    """c3_write_group_bgzf: write_group with each file's text compressed by k_bgzf; the paths name the .gz files"""
    _write_group("c3_write_group_bgzf", z, hb, res, cons_buf, cons_off, (), splint_ids, (cons_paths, sub_paths), zero)


def write_consensus_fastq_bgzf(z, hb, res, cons_buf, cons_off, qv_buf, splint_ids, fq_paths, zero=True):
    """c3_write_consensus_fastq_bgzf: write_consensus_fastq with each file's text compressed by k_bgzf"""
    _write_group("c3_write_consensus_fastq_bgzf", z, hb, res, cons_buf, cons_off, (qv_buf.ctypes.data,), splint_ids, (fq_paths,), zero)


# ---- FASTQ records on the GPU (--parse gpu; include/c3poa.h "FASTQ records on the GPU") ----
class FastqParse:
    """result of c3_fastq_parse / c3_fastq_parse_host: info (dict), names / seqs / quals (bytes), name_off / off (int64
    arrays of n_kept + 1), guards_intact (the FASTQ_GUARD bytes either side of every output array are untouched)"""

    def records(self):
        no, o = self.name_off, self.off
        return [(self.names[no[i]:no[i + 1]], self.seqs[o[i]:o[i + 1]], self.quals[o[i]:o[i + 1]]) for i in range(len(o) - 1)]


def _fastq_call(fn, first, text, at_eof, min_len, text_offset=0, caps=None, bam_at_start=None):
    """bam_at_start is None: a FASTQ call; else a BAM call (at_start in front of at_eof, a BamInfo, room for 2 bases per byte)"""
    src = _b(text)
    n = len(src)
    # the text at byte `text_offset` (0..3) of a dword
    raw = np.zeros(n + 16, dtype=np.uint8)
    at = (-raw.ctypes.data) % 4 + int(text_offset)
    raw[at:at + n] = np.frombuffer(src, dtype=np.uint8)
    fit = (n, n // 2 + 1, n // 7 + 1) if bam_at_start is None else (n, n, n // 38 + 1)
    names_cap, bases_cap, max_records = caps if caps is not None else fit
    o = _Outputs({"names": names_cap, "seqs": bases_cap, "quals": bases_cap, "name_off": 8 * (max_records + 1), "off": 8 * (max_records + 1)})
    p = o.ptr
    info = FastqInfo() if bam_at_start is None else BamInfo()
    kind = () if bam_at_start is None else (int(bool(bam_at_start)),)
    rc = fn(*first, raw.ctypes.data + at if n else None, n, *kind, int(bool(at_eof)), int(min_len), p["names"], names_cap, p["name_off"],
            p["seqs"], p["quals"], bases_cap, p["off"], max_records, C.byref(info))
    out = FastqParse()
    # guards, and on a refused call every byte of the arrays: nothing half written
    o.settle(out, rc, None, info, {"names": info.name_bytes, "seqs": info.base_bytes, "quals": info.base_bytes,
                                   "name_off": 8 * (info.n_kept + 1), "off": 8 * (info.n_kept + 1)})
    o.take(out, names=None, seqs=None, quals=None, name_off=np.int64, off=np.int64)
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


# ---- Post-processing on the GPU (C3POa_postprocessing.py --emit gpu; include/c3poa.h "Post-processing on the GPU") ----
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
        self.ad_name_cat, self.ad_name_off = _cat(self.ad_names)
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
        self.idx_cat, self.idx_off = _cat(self.idx_seqs)
        self.undirectional, self.trim, self.barcoded = bool(undirectional), bool(trim), bool(barcoded)
        self.n_streams = 3 * len(self.dests) + 3


class PostBatch:
    """one batch for c3_post_emit in structure-of-arrays form: pointers (int) or numpy arrays; quals may be None.  `keep`
    holds whatever owns the memory."""

    def __init__(self, n, names, name_off, seqs, quals, off, keep=None):
        self.n, self.names, self.name_off, self.seqs, self.quals, self.off, self.keep = n, names, name_off, seqs, quals, off, keep

    @classmethod
    def from_lists(cls, names, seqs, quals=None):
        (nc, no), (sc, so) = _cat(names, b"\0"), _cat(seqs, b"\0")
        arr = [np.frombuffer(nc, dtype=np.uint8), np.frombuffer(sc, dtype=np.uint8)]
        q = None
        if quals is not None:
            q = np.frombuffer(b"".join(_b(x) for x in quals) + b"\0", dtype=np.uint8)
            assert len(q) == len(arr[1])
        return cls(len(no) - 1, arr[0], no, arr[1], q, so)

    @classmethod
    def from_host(cls, hb, quals=False):
        return cls(hb.n, hb.c.names, hb.name_off, hb.c.seqs, hb.c.quals if quals else None, hb.off, keep=hb)


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
        raise _c3_error(rc, err)
    return arena, so, int(kept.value)


def post_emit_host(plan, batch, table):
    """c3_post_emit_host: the host statement of Handle.post_emit (same arguments and results)"""
    return _post_call(load().c3_post_emit_host, None, plan, batch, table)


# ---- Sample demultiplexer, text in / file bytes out (C3POa_demux.py --emit gpu) ----
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


def _fasta_call(fn, err, text, at_eof, caps=None):
    src = _b(text)
    n = len(src)
    names_cap, bases_cap, max_records = caps if caps is not None else (n, n, fasta_max_records(n))
    o = _Outputs({"names": names_cap, "seqs": bases_cap, "name_off": 8 * (max_records + 1), "off": 8 * (max_records + 1), "hashes": 8 * max_records})
    p = o.ptr
    info = FastaInfo()
    rc = fn(src if n else None, n, int(bool(at_eof)), p["names"], names_cap, p["name_off"], p["seqs"], bases_cap, p["off"],
            p["hashes"], max_records, C.byref(info))
    out = FastaParse()
    nr = info.n_records
    o.settle(out, rc, err, info, {"names": info.name_bytes, "seqs": info.base_bytes, "name_off": 8 * (nr + 1), "off": 8 * (nr + 1), "hashes": 8 * nr})
    o.take(out, names=None, seqs=None, name_off=np.int64, off=np.int64, hashes=np.uint64)
    return out


def fasta_parse_host(text, at_eof=True, caps=None):
    """c3_fasta_parse_host: the host statement of Handle.fasta_parse.  caps = (names_cap, bases_cap, max_records) instead of
    sizes that always fit; C3Error (code E_LIMIT, .info) when too small"""
    return _fasta_call(load().c3_fasta_parse_host, None, text, at_eof, caps)


class DemuxSets:
    """the two index sets of c3_demux_emit: (names, sequences) of the Nextera and the TSO indexes in file order (str or bytes)"""

    def __init__(self, a_names, a_seqs, b_names, b_seqs):
        self._keep, args = [], []
        self.max_name = [0, 0]
        for s, (names, seqs) in enumerate(((a_names, a_seqs), (b_names, b_seqs))):
            (nc, no), (sc, so) = _cat(names, b"\0"), _cat(seqs, b"\0")
            if len(no) != len(so):
                raise ValueError("an index set needs one name per sequence")
            self.max_name[s] = int(np.diff(no).max(initial=0))
            self._keep += [sc, nc, so, no]
            args += [len(so) - 1, C.cast(C.c_char_p(sc), C.c_void_p).value, so.ctypes.data, C.cast(C.c_char_p(nc), C.c_void_p).value, no.ctypes.data]
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
    src = _b(text)
    n = len(src)
    cap = sets.out_bound(n) if cap is None else int(cap)
    max_records = fasta_max_records(n) if max_records is None else int(max_records)
    o = _Outputs({"out": cap, "hashes": 8 * max_records})
    info = DemuxInfo()
    rc = fn(src if n else None, n, int(bool(at_eof)), *sets.args, o.ptr["out"], cap, o.ptr["hashes"], max_records, C.byref(info))
    res = DemuxEmit()
    o.settle(res, rc, err, info, {"out": info.out_bytes, "hashes": 8 * info.n_records})
    o.take(res, out=None, hashes=np.uint64)
    return res


def demux_emit_host(text, sets, at_eof=True, cap=None, max_records=None):
    """c3_demux_emit_host: the host statement of Handle.demux_emit (same arguments and results)"""
    return _demux_emit_call(load().c3_demux_emit_host, None, text, sets, at_eof, cap, max_records)


# ---- records formatted on the GPU (--emit gpu; include/c3poa.h "Records formatted on the GPU") ----
EMIT_BGZF = 1
EMIT_BAM = 2                     # c3_batch_emit_snapshot: BAM records (include/c3poa.h "Records written as unaligned BAM")
EMIT_KINDS = ("consensus_fasta", "subread_fastq", "consensus_fastq")


class EmitStreams:
    """result of emit_group / emit_group_host: stream x = splint * K + kind lies at arena[stream_off[x]:stream_off[x + 1]]"""

    def __init__(self, arena, stream_off, n_records, K):
        self.arena, self.stream_off, self.n_records, self.K = arena, stream_off, n_records, K

    def stream(self, x):
        return self.arena[int(self.stream_off[x]):int(self.stream_off[x + 1])].tobytes()

    def streams(self):
        return [self.stream(x) for x in range(len(self.stream_off) - 1)]


def _emit_call(fn, err, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap=None, arena=None, bam=False):
    """cap None: the arena is sized by a first call with no arena (C3_E_LIMIT reports the need).  An explicit cap / arena is
    handed through as it is; a C3Error then carries .code and .stream_off.  bam: the BAM form of the call (K = 2)."""
    K = 3 if qv_buf is not None and not bam else 2
    S = n_splints * K
    sid = np.ascontiguousarray(splint_ids, dtype=np.int16)
    res = np.ascontiguousarray(res)
    coff = np.ascontiguousarray(cons_off, dtype=np.int64) if cons_off is not None else None
    so = np.zeros(max(S, 0) + 2, dtype=np.int64)
    nrec = C.c_int64(0)

    def call(ar, c):
        return fn(C.byref(hb.c), res.ctypes.data if len(res) else None, _ptr(cons_buf), _ptr(coff), _ptr(qv_buf),
                  sid.ctypes.data if len(sid) else None, n_splints, 1 if zero else 0, _ptr(ar), c, so.ctypes.data, C.byref(nrec))

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
        raise _c3_error(rc, err, "c3_emit_group_bam" if bam else "c3_emit_group", stream_off=so[:max(S, 0) + 1].copy())
    return EmitStreams(arena, so[:S + 1].copy(), int(nrec.value), K)


def emit_group_host(hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero=True, cap=None, arena=None):
    """c3_emit_group_host: the host statement of Handle.emit_group (same arguments and results).  hb: a HostBatch; res: RESULT_DTYPE
    records; cons_buf / cons_off / qv_buf as results_raw / results_fetch_qv return them (cons_buf and qv_buf may be None)"""
    return _emit_call(load().c3_emit_group_host, None, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap, arena)


def emit_group_bam_host(hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero=True, cap=None, arena=None):
    """c3_emit_group_bam_host: the host statement of Handle.emit_group_bam (same arguments and results): uncompressed BAM
    records, stream splint * 2 + kind with kind 0 = consensus and 1 = subreads"""
    return _emit_call(load().c3_emit_group_bam_host, None, hb, res, cons_buf, cons_off, qv_buf, splint_ids, n_splints, zero, cap, arena, bam=True)


def bam_out_header():
    """c3_bam_out_header: the uncompressed header of a --bam file (magic, @HD and @PG text, no references)"""
    buf, n = C.create_string_buffer(512), C.c_int64(0)
    rc = load().c3_bam_out_header(buf, len(buf), C.byref(n))
    if rc != 0:
        raise _c3_error(rc, None, "c3_bam_out_header")
    return buf.raw[:n.value]


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
    src = _b(text)
    n = len(src)
    names_cap, bases_cap, max_records = caps if caps is not None else (n, n, fastx_max_records(n, kind if kind in (2, 4) else 2))
    q = kind == 4
    o = _Outputs({"names": names_cap, "seqs": bases_cap, "quals": bases_cap if q else 0, "name_off": 8 * (max_records + 1),
                  "off": 8 * (max_records + 1), "hashes": 8 * max_records})
    p = o.ptr
    info = FastxInfo()
    rc = load().c3_fastx_strict_parse_host(src if n else None, n, int(bool(at_eof)), int(kind), p["names"], names_cap, p["name_off"],
                                           p["seqs"], p["quals"] if q else None, bases_cap, p["off"], p["hashes"], max_records, C.byref(info))
    out = FastxParse()
    nr = info.n_records
    o.settle(out, rc, None, info, {"names": info.name_bytes, "seqs": info.base_bytes, "quals": info.base_bytes if q else 0,
                                   "name_off": 8 * (nr + 1), "off": 8 * (nr + 1), "hashes": 8 * nr})
    o.take(out, names=None, seqs=None, quals=None, name_off=np.int64, off=np.int64, hashes=np.uint64)
    if not q:
        out.quals = None
    return out


# ---- Text in / file bytes out: post-processing and the sample demultiplexer by pieces ----
POST_IN_BGZF, POST_OUT_BGZF, POST_KEEP_QUALS = 1, 2, 4       # flags of c3_post_emit_text
DEMUX_IN_BGZF, DEMUX_OUT_BGZF, DEMUX_KEEP_QUALS, DEMUX_SPLIT = 1, 2, 4, 8     # flags of c3_demux_emit_text
DEMUX_MAX_STREAMS = 4096


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
    src = piece if isinstance(piece, np.ndarray) else np.frombuffer(_b(piece), dtype=np.uint8)
    n = len(src)
    s_ok = s_max is None or S <= s_max
    so = np.zeros((S if s_ok else s_max) + 1 + 2, dtype=np.int64)
    so[0] = so[-1] = _SO_GUARD                                           # a guard word either side
    ask = cap is None and max_records is None
    cap = (24 if in_z else 3) * n + 65536 if cap is None else int(cap)
    max_records = (8 if in_z else 1) * (n // 8) + 16 if max_records is None else int(max_records)
    for _try in range(3):
        o = _Outputs({"arena": cap, "hashes": 8 * max_records}, keep=bufs)
        cap, max_records = o.cap("arena"), o.cap("hashes") // 8
        rc = fn(src.ctypes.data if n else None, n, *mid, o.ptr["arena"], cap, so.ctypes.data + 8, o.ptr["hashes"], max_records, C.byref(info))
        if ask and rc == E_LIMIT and s_ok and (so[S + 1] > cap or info.n_records > max_records):
            cap, max_records = max(cap, int(so[S + 1])), max(max_records, int(info.n_records))
            continue
        break
    out = TextResult()
    out.stream_off = so[1:-1]
    o.settle(out, rc, err, info, {"arena": int(so[S + 1]), "hashes": 8 * int(info.n_records)} if rc == 0 else {},
             intact=so[0] == so[-1] == _SO_GUARD, stream_off=out.stream_off)
    out.arena = o.view("arena")
    o.take(out, hashes=np.uint64)
    return out


def _demux_text_call(fn, err, sets, piece, at_eof, kind, flags, cap, max_records, bufs=None):
    """one c3_demux_emit_text (kind None) or c3_demux_emit_text_host call through _text_call"""
    st = sets.struct
    mid = (int(bool(at_eof)),) + (() if kind is None else (int(kind),)) + (int(flags), C.byref(st))
    return _text_call(fn, err, piece, mid, sets.n_split_streams if flags & DEMUX_SPLIT else 1, DemuxTextInfo(), bool(flags & DEMUX_IN_BGZF),
                      cap, max_records, bufs, DEMUX_MAX_STREAMS)


def demux_emit_text_host(sets, text, at_eof=True, kind=2, flags=0, cap=None, max_records=None):
    """c3_demux_emit_text_host: the host statement of Handle.demux_emit_text for one plain text of a stated kind"""
    return _demux_text_call(load().c3_demux_emit_text_host, None, sets, text, at_eof, kind, flags, cap, max_records)

"""Post-processing of consensus reads: adapter finding, trimming / re-orientation, oligo-dT and 10x demultiplexing.

Host-side mirror of /root/reference/C3POa_postprocessing.py.  The reference aligns the adapters to
the consensus reads with blat (:229-236) and reads six PSL columns back (:238-264); here `find_adapters_gpu` gets the
same information from k_adapter (c3_scan_adapters) and writes the same `adapter_to_consensus_alignment.psl`, which
`parse_blat` -- and a rerun -- consume exactly as upstream.  `match_index` (:266-285, the editdistance loop) is the
native c3_match_index.  Output files and record formats follow write_fasta_file (:287-398).
"""
import gzip
import json
import os
import shutil
import sys

import numpy as np

from . import _lib
from .seqio import fastx_read, revcomp

FLC = "R2C2_full_length_consensus_reads.fasta"
FLC_LEFT = "R2C2_full_length_consensus_reads_left_splint.fasta"
FLC_RIGHT = "R2C2_full_length_consensus_reads_right_splint.fasta"
FLC_10X = "R2C2_full_length_consensus_reads_10X_sequences.fasta"
MUX_TSV = "R2C2_oligodT_multiplexing.tsv"
PSL_NAME = "adapter_to_consensus_alignment.psl"
MIN_SCORE = 22          # > 10 matching bases under the 2 / -4 scoring: the `matches > 10` of parse_blat (:248)


def read_fasta(path, indexes):
    """:218-227 -- {name: seq} (and {seq: name} for the index file), file order"""
    reads, index_dict = {}, {}
    for rec in fastx_read(path):
        reads[rec[0]] = rec[1]
        if indexes:
            index_dict[rec[1]] = rec[0]
    return (reads, index_dict) if indexes else reads


def psl_line(read_name, read_len, adapter_name, adapter_len, strand, e):
    """21 PSL columns from one k_adapter record e = (score, qS, qE, tS, tE, matches, mism, qBaseIns, tBaseIns, qNumIns, tNumIns, L)"""
    cols = [e[5], e[6], 0, 0, e[9], e[7], e[10], e[8], strand, read_name, read_len, e[1], e[2],
            adapter_name, adapter_len, e[3], e[4], 1, "%d," % (e[2] - e[1]), "%d," % e[1], "%d," % e[3]]
    return "\t".join(str(int(c)) if not isinstance(c, str) else c for c in cols)


def find_adapters_gpu(reads, adapter_file, psl_path, batch=200000, handle=None):
    """writes the PSL the reference gets from blat: one row per (read, adapter, strand) whose local alignment reaches
    MIN_SCORE.  reads: {name: seq} in file order."""
    adapters = [(r[0], r[1]) for r in fastx_read(adapter_file)]
    h = handle or _lib.Handle()
    h.set_splints([a[1] for a in adapters])
    names = list(reads)
    with open(psl_path + ".part", "w") as out:
        for b0 in range(0, len(names), batch):
            chunk = names[b0:b0 + batch]
            seqs = [reads[n] for n in chunk]
            keep = [i for i, s in enumerate(seqs) if len(s) > 0]
            if not keep:
                continue
            h.upload([seqs[i] for i in keep], ["!" * len(seqs[i]) for i in keep], "?" * len(keep))
            tab = h.scan_adapters()
            hit = np.argwhere(tab[:, :, :, 0] >= MIN_SCORE)
            rows = []
            for i, a, rc in hit:
                name = chunk[keep[i]]
                rows.append(psl_line(name, len(reads[name]), adapters[a][0], len(adapters[a][1]), "-" if rc else "+", tab[i, a, rc]))
            if rows:
                out.write("\n".join(rows) + "\n")
    os.replace(psl_path + ".part", psl_path)
    if handle is None:
        h.close()


def parse_blat(psl_path, reads):
    """:238-264 -- per read and strand the list of (adapter, matches, projected position)"""
    adapter_dict = {}
    for name, sequence in reads.items():
        adapter_dict[name] = {"+": [("-", 1, 0)], "-": [("-", 1, len(sequence))]}
    with open(psl_path) as fh:
        for line in fh:
            a = line.strip().split("\t")
            if len(a) < 17:
                continue
            read_name, adapter, strand = a[9], a[13], a[8]
            if int(a[5]) < 50 and float(a[0]) > 10:
                if strand == "+":
                    position = int(a[12]) + (int(a[14]) - int(a[16]))        # projected END of the adapter on the read
                else:
                    position = int(a[11]) - (int(a[14]) - int(a[16]))        # projected START
                adapter_dict[read_name][strand].append((adapter, float(a[0]), position))
    return adapter_dict


def match_index(seq, seq_to_idx):
    """:266-285"""
    seqs = list(seq_to_idx)
    k = _lib.match_index(seq, seqs)
    return seq_to_idx[seqs[k]] if k >= 0 else "-"


class _Outputs:
    """the three (or four) FASTA streams of one destination directory, opened lazily in append mode"""

    def __init__(self):
        self.fh = {}

    def get(self, path, name):
        key = path + name
        if key not in self.fh:
            os.makedirs(path, exist_ok=True)
            self.fh[key] = open(key, "a")
        return self.fh[key]

    def close(self):
        for f in self.fh.values():
            f.close()
        self.fh = {}


def match_batch_host(pieces, index_seqs):
    """one native c3_match_index call per piece (host; what the CPU tests use)"""
    return np.array([_lib.match_index(p, index_seqs) for p in pieces], dtype=np.int32)


def match_batch_gpu(pieces, index_seqs, handle=None):
    """c3_match_index_batch: one lane per piece on the GPU"""
    h = handle or _lib.Handle()
    out = h.match_index_batch(pieces, index_seqs)
    if handle is None:
        h.close()
    return out


def write_fasta_file(args, path, adapter_dict, reads, seq_to_idx, idx_to_seq, match_batch=match_batch_gpu):
    """:287-398 -- classification, trimming, orientation, demultiplexing; returns the number of reads written.
    Two passes instead of the reference's one: the reads that pass the adapter rules are collected first so that all
    oligo-dT pieces are matched in one batch (match_index, :266-285), then the records are written in read order."""
    undirectional, barcoded, trim = args.undirectional, args.barcoded, args.trim
    odt = bool(seq_to_idx)
    keep = []                                              # (name, p_pos, m_pos, direction)
    for name, sequence in reads.items():
        plus = sorted((x for x in adapter_dict[name]["+"] if x[0] != "-"), key=lambda x: x[2])
        minus = sorted((x for x in adapter_dict[name]["-"] if x[0] != "-"), key=lambda x: x[2])
        if len(plus) != 1 or len(minus) != 1:
            continue
        p_pos, m_pos = plus[0][2], minus[0][2]
        if m_pos <= p_pos:
            continue
        if undirectional:
            direction = "+"
        elif plus[0][0] != minus[0][0]:
            direction = "+" if plus[0][0] == "5Prime_adapter" else "-"
        else:
            continue
        keep.append((name, p_pos, m_pos, direction))
    fwd_pieces, rev_pieces, fwd_idx, rev_idx = [], [], [], []
    if odt:
        index_seqs = list(seq_to_idx)
        for name, p_pos, m_pos, _d in keep:
            sequence = reads[name]
            fwd_pieces.append(sequence[p_pos - 4:p_pos + 16])
            rev_pieces.append(revcomp(sequence[m_pos - 16:m_pos + 4]))
        hits = match_batch(fwd_pieces + rev_pieces, index_seqs) if keep else np.zeros(0, dtype=np.int32)
        names = [seq_to_idx[x] for x in index_seqs]
        fwd_idx = [names[k] if k >= 0 else "-" for k in hits[:len(keep)]]
        rev_idx = [names[k] if k >= 0 else "-" for k in hits[len(keep):]]
    outs = _Outputs()
    if odt:
        for idx in idx_to_seq:
            if os.path.exists(path + idx):
                shutil.rmtree(path + idx)
        mux = open(path + MUX_TSV, "w")
    else:
        for nm in (FLC, FLC_LEFT, FLC_RIGHT):
            open(path + nm, "w").close()
    if barcoded:
        open(path + FLC_10X, "w").close()
    for k, (name, p_pos, m_pos, direction) in enumerate(keep):
        sequence = reads[name]
        dest = path
        if odt:
            mux.write("%s\t%s\t%s\n" % (name, rev_pieces[k], fwd_pieces[k]))
            forward_index, reverse_index = fwd_idx[k], rev_idx[k]
            idx_name = "no_index_found"
            if forward_index in idx_to_seq and reverse_index not in idx_to_seq:
                direction, idx_name = "-", forward_index
            if reverse_index in idx_to_seq and forward_index not in idx_to_seq:
                direction, idx_name = "+", reverse_index
            dest = path + idx_name + "/"
        seq = sequence[p_pos:m_pos]
        ada = sequence[max(p_pos - 40, 0):m_pos + 40]
        out_name = name + "_" + str(len(seq))
        out, out3, out5 = outs.get(dest, FLC), outs.get(dest, FLC_LEFT), outs.get(dest, FLC_RIGHT)
        if direction == "+":
            out.write(">%s\n%s\n" % (out_name, seq if trim else ada))
            out5.write(">%s\n%s\n" % (out_name, revcomp(sequence[:p_pos])))
            out3.write(">%s\n%s\n" % (out_name, sequence[m_pos:]))
            if barcoded:
                outs.get(path, FLC_10X).write(">%s\n%splus\n" % (out_name, revcomp(sequence[m_pos - 40:m_pos])))
        else:
            out.write(">%s\n%s\n" % (out_name, revcomp(seq) if trim else revcomp(ada)))
            out3.write(">%s\n%s\n" % (out_name, revcomp(sequence[:p_pos + 40])))
            out5.write(">%s\n%s\n" % (out_name, sequence[m_pos:]))
            if barcoded:
                outs.get(path, FLC_10X).write(">%s\n%sminus\n" % (out_name, sequence[p_pos:p_pos + 40]))
    outs.close()
    if odt:
        mux.close()
    return len(keep)


def _gzip_in_place(path):
    with open(path, "rb") as src, gzip.open(path + ".gz", "wb") as dst:
        shutil.copyfileobj(src, dst, 1 << 24)
    os.remove(path)


def run(args):
    """main() of the reference (:400-426) with the blat step on the GPU.  -n > 1 keeps the reference's multi-process
    output conventions (every index directory exists, -co compresses); the work itself is one GPU pass either way."""
    if not args.output_path.endswith("/"):
        args.output_path += "/"
    os.makedirs(args.output_path, exist_ok=True)
    if args.undirectional and args.barcoded:
        print("Error: undirectional and barcoded are mutually exclusive.")
        sys.exit(1)
    if args.index_file:
        idx_to_seq, seq_to_idx = read_fasta(args.index_file, True)
    else:
        idx_to_seq, seq_to_idx = {}, {}
    psl = args.output_path + PSL_NAME
    keep_quals = bool(getattr(args, "keep_quals", False))
    bgzf = bool(getattr(args, "bgzf", False))
    if getattr(args, "emit", "host") == "gpu":
        n = run_emit_text(args, idx_to_seq, seq_to_idx, psl, keep_quals) if getattr(args, "parse", "host") == "gpu" else None
        if n is None:
            n = run_emit_gpu(args, idx_to_seq, seq_to_idx, psl, keep_quals)
        if n is not None:
            _multiprocess_conventions(args, idx_to_seq, ".fastq" if keep_quals else ".fasta", ".gz" if bgzf else "")
            return n
        if keep_quals:
            sys.exit("--keep-quals needs the device path (--emit gpu), which this run cannot take (see the note above)")
    reads = read_fasta(args.input_fasta_file, False)
    if not os.path.exists(psl) or os.stat(psl).st_size == 0:
        if getattr(args, "adapter_finder", "gpu") == "gpu":
            find_adapters_gpu(reads, args.adapter_file, psl)
        else:
            raise RuntimeError("no %s: run with --adapter-finder gpu (blat is not bundled)" % psl)
    else:
        print("Reading existing psl file", file=sys.stderr)
    adapter_dict = parse_blat(psl, reads)
    n = write_fasta_file(args, args.output_path, adapter_dict, reads, seq_to_idx, idx_to_seq)
    if bgzf:                                                    # the files of the fallback leave as BGZF all the same
        _bgzf_tree(args.output_path, idx_to_seq)
    _multiprocess_conventions(args, idx_to_seq, ".fasta", ".gz" if bgzf else "")
    return n


BGZF_PIECE = 1024 * _lib.BGZF_BLOCK                            # text bytes per c3_bgzf_compress call of _bgzf_file: whole members


def _bgzf_finish(paths):
    """the EOF member behind every member chain of --bgzf (a file that got no record holds nothing else)"""
    for p in paths:
        with open(p, "ab") as fh:
            fh.write(_lib.BGZF_EOF)


def _bgzf_file(z, path):
    """path -> path.gz: its text through c3_bgzf_compress piece by piece, then the EOF member; the plain file goes"""
    with open(path, "rb") as src, open(path + ".gz", "wb") as dst:
        while True:
            piece = src.read(BGZF_PIECE)
            if not piece:
                break
            dst.write(z.compress(piece))
        dst.write(_lib.BGZF_EOF)
    os.remove(path)


def _bgzf_tree(path, idx_to_seq):
    """--bgzf after a fallback to the host path: every read file it wrote (three per destination, the 10x file) compressed
    by k_bgzf file by file; the TSV and the PSL stay plain"""
    dirs = [path + idx + "/" for idx in list(idx_to_seq) + ["no_index_found"]] if idx_to_seq else [path]
    found = [d + nm for d in dirs for nm in (FLC, FLC_LEFT, FLC_RIGHT)] + [path + FLC_10X]
    found = [p for p in found if os.path.exists(p)]
    if found:
        z = _lib.Bgzf()
        for p in found:
            _bgzf_file(z, p)
        z.close()


def _multiprocess_conventions(args, idx_to_seq, suffix, gz=""):
    """the end of main() with -n > 1 (:165-214): every destination holds every file, -co compresses them.  suffix: .fasta, or
    .fastq for the three read files under --keep-quals; gz: ".gz" under --bgzf, where a missing file is the EOF member alone"""
    if args.threads > 1:
        names = [nm[:-len(".fasta")] + suffix for nm in (FLC, FLC_LEFT, FLC_RIGHT)]
        dirs = [args.output_path]
        if idx_to_seq:
            dirs = [args.output_path + idx + "/" for idx in list(idx_to_seq) + ["no_index_found"]]
        elif args.barcoded:
            names = names + [FLC_10X]
        for d in dirs:                                          # chunk_process cats into every destination (:165-214)
            os.makedirs(d, exist_ok=True)
            for nm in names:
                if gz:
                    if not os.path.exists(d + nm + gz):
                        _bgzf_finish([d + nm + gz])
                    continue
                if not os.path.exists(d + nm):
                    open(d + nm, "w").close()
                if args.compress_output:
                    _gzip_in_place(d + nm)


def _np_bytes(ptr, nbytes):
    """a copy of nbytes at ptr as a uint8 array with slack behind it"""
    import ctypes as C
    out = np.zeros(nbytes + 16, dtype=np.uint8)
    if nbytes:
        C.memmove(out.ctypes.data, ptr, nbytes)
    return out


def _name_hashes(names, name_off):
    """one 64-bit hash per name, without a Python loop over reads (equal names give equal hashes; a collision of different
    names only sends the run to the host path)"""
    n = len(name_off) - 1
    lens = np.diff(name_off)
    total = int(name_off[-1])
    h = np.zeros(n, dtype=np.uint64)
    if total:
        pos = np.arange(total, dtype=np.int64) - np.repeat(name_off[:-1], lens)
        w = (pos.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)) | np.uint64(1)
        v = (names[:total].astype(np.uint64) + np.uint64(1)) * w
        v ^= v >> np.uint64(29)
        v *= np.uint64(0xBF58476D1CE4E5B9)
        nz = lens > 0
        h[nz] = np.add.reduceat(v, name_off[:-1][nz])
    return h ^ (lens.astype(np.uint64) * np.uint64(0x94D049BB133111EB))


def run_emit_gpu(args, idx_to_seq, seq_to_idx, psl, keep_quals):
    """--emit gpu: classification, trimming, orientation, demultiplexing, record formatting and the PSL text on the device
    (c3_post_emit); only finished file bytes come back.  Returns the number of reads written, or None after a one-line note on
    stderr when the run has to take the host path (which gives the same files): a PSL to reuse, two records with one name
    (the host's dict collapses them), a byte >= 0x80 (Python cuts characters, the device bytes), or index sets beyond the
    device limits.  Under --bgzf the read streams (three per destination, the 10x file) are compressed by k_bgzf
    (c3_bgzf_compress) before they are appended to <name>.gz, and every such file ends in one EOF member."""
    def fallback(why):
        print("--emit gpu: %s; using the host path" % why, file=sys.stderr)

    path = args.output_path
    if os.path.exists(psl) and os.stat(psl).st_size > 0:
        return fallback("%s exists and is reused" % PSL_NAME)
    adapters = [(r[0], r[1]) for r in fastx_read(args.adapter_file)]
    if any(a[0] == "-" for a in adapters) or "-" in idx_to_seq:
        return fallback("an adapter or index is named '-' (the host path's placeholder)")
    plan = _lib.PostPlan(adapters, (idx_to_seq, seq_to_idx) if seq_to_idx else None, undirectional=args.undirectional,
                         trim=args.trim, barcoded=args.barcoded)
    try:                                                    # an empty batch: the library's own verdict on the index set
        _lib.post_emit_host(plan, _lib.PostBatch.from_lists([], []), np.zeros(0, dtype=np.int32))
    except _lib.C3Error as e:
        if e.code != _lib.E_LIMIT:
            raise
        return fallback(str(e).split(": ", 2)[-1])
    # the input, once, in structure-of-arrays batches (the host path holds every read as well)
    per = max(1, int(getattr(args, "post_batch", 200000) or 200000))
    rd = _lib.Reader(args.input_fasta_file, n_sets=1)
    batches, hashes, high = [], [], False
    while True:
        hb = rd.next(per, min_len=0)
        if hb.n == 0:
            break
        nb, sb = int(hb.name_off[-1]), int(hb.off[-1])
        b = (hb.n, _np_bytes(hb.c.names, nb), hb.name_off, _np_bytes(hb.c.seqs, sb), _np_bytes(hb.c.quals, sb), hb.off)
        high = high or bool((b[1] & 0x80).any()) or bool((b[3] & 0x80).any())
        hashes.append(_name_hashes(b[1], b[2]))
        batches.append(b)
    noqual = rd.noqual()
    rd.close()
    if keep_quals and noqual:
        sys.exit("--keep-quals: %d records of %s have no quality line" % (noqual, args.input_fasta_file))
    if high:
        return fallback("the input holds a byte >= 0x80")
    if hashes and len(np.unique(np.concatenate(hashes))) < sum(b[0] for b in batches):
        return fallback("two records share a name")
    # the files as write_fasta_file opens them
    suffix = ".fastq" if keep_quals else ".fasta"
    gz = ".gz" if getattr(args, "bgzf", False) else ""
    files = [nm[:-len(".fasta")] + suffix + gz for nm in (FLC, FLC_LEFT, FLC_RIGHT)]
    if plan.has_index:
        for idx in idx_to_seq:
            if os.path.exists(path + idx):
                shutil.rmtree(path + idx)
        open(path + MUX_TSV, "w").close()
    else:
        for nm in files:
            open(path + nm, "w").close()
    if args.barcoded:
        open(path + FLC_10X + gz, "w").close()
    targets = [path + (d + "/" if plan.has_index else "") + nm for d in plan.dests for nm in files] + [path + FLC_10X + gz, path + MUX_TSV, psl + ".part"]
    n_read_streams = len(targets) - 2                       # everything but the TSV and the PSL
    open(psl + ".part", "w").close()
    z = _lib.Bgzf() if gz else None
    h = _lib.Handle()
    h.set_splints([a[1] for a in adapters])
    kept = 0
    for n, names, name_off, seqs, quals, off in batches:
        lens = np.diff(off)
        full = lens > 0
        tab = np.zeros((n, len(adapters), 2, 12), dtype=np.int32)
        if full.any():                                      # empty reads are not aligned (find_adapters_gpu): their rows stay zero
            off_up = off if full.all() else np.concatenate([off[:-1][full], off[-1:]])
            h.upload_flat(seqs[:int(off[-1])], quals[:int(off[-1])], off_up, b"?" * int(full.sum()))
            tab[full] = h.scan_adapters()
        arena, so, k = h.post_emit(plan, _lib.PostBatch(n, names, name_off, seqs, quals if keep_quals else None, off), tab)
        kept += k
        for s, target in enumerate(targets):
            if so[s + 1] > so[s]:
                os.makedirs(os.path.dirname(target), exist_ok=True)
                with open(target, "ab") as fh:
                    if z is not None and s < n_read_streams:
                        fh.write(z.compress(arena[int(so[s]):int(so[s + 1])].tobytes()))
                    else:
                        fh.write(arena[int(so[s]):int(so[s + 1])].data)
    h.close()
    if z is not None:
        z.close()
        _bgzf_finish([t for t in targets[:n_read_streams] if os.path.exists(t)])
    os.replace(psl + ".part", psl)
    return kept


def _is_bgzf(head):
    """the first 18 bytes of a file are a BGZF member header (gzip with the 'BC' extra field first)"""
    return len(head) >= 18 and head[:4] == b"\x1f\x8b\x08\x04" and head[10:12] == b"\x06\x00" and head[12:16] == b"BC\x02\x00"


def _bgzf_whole_members(buf):
    """bytes of buf that are whole BGZF members (walked by the BSIZE field; c3_bgzf_scan then vouches for them)"""
    at = 0
    while at + 18 <= len(buf):
        size = int.from_bytes(buf[at + 16:at + 18], "little") + 1
        if not _is_bgzf(buf[at:at + 18]) or at + size > len(buf):
            break
        at += size
    return at


def _text_pieces(path, chunk, inflate_gpu):
    """(piece, at_eof, in_bgzf) of the input in pieces of about `chunk` bytes: plain text as it stands; a BGZF file cut at member
    boundaries when the device inflates; any other .gz (and BGZF without --inflate gpu) through zlib on the host"""
    with open(path, "rb") as fh:
        head = fh.read(18)
    gz = head[:2] == b"\x1f\x8b"
    in_bgzf = gz and inflate_gpu and _is_bgzf(head)
    fh = gzip.open(path, "rb") if gz and not in_bgzf else open(path, "rb")
    with fh:
        buf, done = b"", False
        while not done:
            more = fh.read(chunk)
            done = not more
            buf += more
            if in_bgzf:
                k = _bgzf_whole_members(buf)
                if done and k != len(buf):
                    raise _lib.C3Error("%s: the BGZF file ends inside a member" % path)
                if k == 0 and not done:
                    continue                                    # a member longer than the chunk: read on
                if not done:
                    nxt = fh.read(1)                            # is anything left?  (at_eof goes with the last members)
                    if nxt:
                        rest = buf[k:] + nxt
                    else:
                        done, rest = True, buf[k:]
                        if rest:
                            raise _lib.C3Error("%s: the BGZF file ends inside a member" % path)
                    piece, buf = buf[:k], rest
                else:
                    piece, buf = buf, b""
                yield piece, done, True
            else:
                if not done:
                    nxt = fh.read(1)
                    if not nxt:
                        done = True
                    piece, buf = buf, nxt
                else:
                    piece, buf = buf, b""
                yield piece, done, False


def run_emit_text(args, idx_to_seq, seq_to_idx, psl, keep_quals):
    """--emit gpu --parse gpu: the input goes to the device as text (or, with --inflate gpu, as BGZF members) in pieces of
    --post-chunk bytes; c3_post_emit_text parses, aligns, classifies and formats there and returns file bytes, which are
    appended to .part files that take their names at the end.  Returns the number of reads written, or None after a one-line
    note on stderr when the run has to take the batch path of --emit gpu instead (which gives the same files and keeps its own
    fallbacks): a departure from the strict record rule, two records with one name hash, a refusal of the call, a PSL to
    reuse, a plain-gzip input under --inflate gpu."""
    stats = {"records_device": 0, "calls": 0, "inflated_bytes": 0, "fallback": True}

    def fallback(why):
        print("--parse gpu: %s; using the batch path of --emit gpu" % why, file=sys.stderr)
        if getattr(args, "emit_stats", False):
            print(json.dumps(stats), file=sys.stderr)

    path = args.output_path
    inflate_gpu = getattr(args, "inflate", "host") == "gpu"
    if os.path.exists(psl) and os.stat(psl).st_size > 0:
        return fallback("%s exists and is reused" % PSL_NAME)
    adapters = [(r[0], r[1]) for r in fastx_read(args.adapter_file)]
    if any(a[0] == "-" for a in adapters) or "-" in idx_to_seq:
        return fallback("an adapter or index is named '-' (the host path's placeholder)")
    with open(args.input_fasta_file, "rb") as fh:
        head = fh.read(18)
    if inflate_gpu and head[:2] == b"\x1f\x8b" and not _is_bgzf(head):
        return fallback("%s is gzip but not BGZF, which the device does not inflate" % args.input_fasta_file)
    plan = _lib.PostPlan(adapters, (idx_to_seq, seq_to_idx) if seq_to_idx else None, undirectional=args.undirectional,
                         trim=args.trim, barcoded=args.barcoded)
    suffix = ".fastq" if keep_quals else ".fasta"
    gz = ".gz" if getattr(args, "bgzf", False) else ""
    files = [nm[:-len(".fasta")] + suffix + gz for nm in (FLC, FLC_LEFT, FLC_RIGHT)]
    targets = [path + (d + "/" if plan.has_index else "") + nm for d in plan.dests for nm in files] + [path + FLC_10X + gz, path + MUX_TSV, psl]
    n_read_streams = len(targets) - 2
    if plan.has_index:
        for idx in idx_to_seq:
            if os.path.exists(path + idx):
                shutil.rmtree(path + idx)
    always = [psl] + ([path + MUX_TSV] if plan.has_index else [path + nm for nm in files]) + ([path + FLC_10X + gz] if args.barcoded else [])
    parts = set()

    def discard():
        for t in parts:
            if os.path.exists(t + ".part"):
                os.remove(t + ".part")

    h = _lib.Handle()
    kept, hashes, why, bufs = 0, [], None, {}
    try:
        h.set_splints([a[1] for a in adapters])
        for piece, at_eof, in_bgzf in _text_pieces(args.input_fasta_file, max(1, int(getattr(args, "post_chunk", 64 << 20))), inflate_gpu):
            try:
                res = h.post_emit_text(plan, piece, at_eof=at_eof, in_bgzf=in_bgzf, out_bgzf=bool(gz), keep_quals=keep_quals, bufs=bufs)
            except _lib.C3Error as e:
                if keep_quals and "C3_POST_KEEP_QUALS on a FASTA text" in str(e):
                    discard()
                    sys.exit("--keep-quals: the records of %s have no quality line" % args.input_fasta_file)
                why = "the device call was refused (%s)" % str(e).split(": ", 1)[-1]
                break
            stats["calls"] += 1
            stats["records_device"] += res.info["n_records"]
            stats["inflated_bytes"] += res.info["text_bytes"] - (0 if stats["calls"] == 1 else tail)
            tail = res.info["text_bytes"] - res.info["consumed"]
            if res.info["departed"]:
                why = "the input departs from the strict record rule behind record %d" % stats["records_device"]
                break
            kept += res.info["n_kept"]
            hashes.append(res.hashes)
            so = res.stream_off
            for s, target in enumerate(targets):
                if so[s + 1] > so[s]:
                    os.makedirs(os.path.dirname(target), exist_ok=True)
                    parts.add(target)
                    with open(target + ".part", "ab") as fh:
                        fh.write(res.arena[int(so[s]):int(so[s + 1])].data)
    except _lib.C3Error as e:                                   # (the piece cutter: a BGZF file that ends inside a member)
        why = str(e)
    finally:
        h.close()
    if why is None and hashes and len(np.unique(np.concatenate(hashes))) < stats["records_device"]:
        why = "two records share a name hash"
    if why is not None:
        discard()
        return fallback(why)
    for t in always:
        if t not in parts:
            parts.add(t)
            open(t + ".part", "wb").close()
    if gz:
        _bgzf_finish([t + ".part" for t in parts if t in targets[:n_read_streams]])
    for t in parts:
        os.replace(t + ".part", t)
    stats["fallback"] = False
    if getattr(args, "emit_stats", False):
        print(json.dumps(stats), file=sys.stderr)
    return kept

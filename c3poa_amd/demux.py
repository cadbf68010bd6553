"""Sample demultiplexer: paper/Demultiplex_R2C2_reads.py of the reference, with the index search on the GPU.

Every consensus read longer than 300 bases is searched in its first 300 bases for each Nextera and each TSO index
(minimum Levenshtein distance over the windows head[i : i+m], i < 300 - m) and renamed `name|<Nextera>_<TSO>`; shorter
reads are dropped.  Each set is decided on its own: the first index of smallest distance (file order breaks ties) wins
when its distance is < 4 and the runner-up's is more than 1 further away, otherwise the field stays empty.  The search
is k_demux (c3_demux_indexes) in batches of bounded size; c3_demux_host is its host statement.  read_fasta,
demultiplex and write_fasta_file keep the reference's function shapes.
"""
import os
import sys

import numpy as np

from c3poa_amd import _lib

HEAD = _lib.DEMUX_HEAD
MAX_INDEXES = 128       # C3_DEMUX_MAX_IDX, per set
MAX_INDEX_LEN = 32      # C3_DEMUX_MAX_LEN
BATCH = 65536           # reads per device call


class DemuxError(ValueError):
    """an input the reference cannot process (it crashes on all of these)"""


def read_fasta(path):
    """{header: sequence} as the reference's read_fasta: the header is the whole line after '>' (rstrip only), sequence
    lines are rstrip-ped and joined, blank lines are skipped, a repeated header keeps its first position and takes the
    last record's sequence.  Text mode with universal newlines, as the reference opens the file.  A sequence line before
    the first header raises DemuxError."""
    reads = {}
    last = None
    with open(path) as f:
        for n, line in enumerate(f, 1):
            line = line.rstrip()
            if not line:
                continue
            if line.startswith(">"):
                last = line[1:]
                reads[last] = ""
            elif last is None:
                raise DemuxError("%s:%d: sequence line before the first '>' header" % (path, n))
            else:
                reads[last] += line
    return reads


def load_indexes(path):
    """(names, sequences) of an index file in file order, checked against the limits of the search"""
    d = read_fasta(path)
    if len(d) < 2:
        raise DemuxError("%s: %d index(es); an index set needs at least 2 (the best is compared with the runner-up)" % (path, len(d)))
    if len(d) > MAX_INDEXES:
        raise DemuxError("%s: %d indexes; at most %d are supported" % (path, len(d), MAX_INDEXES))
    for name, seq in d.items():
        if len(seq) > MAX_INDEX_LEN:
            raise DemuxError("%s: index %r has %d bases; at most %d are supported (the reference cannot search an index of "
                             "%d or more)" % (path, name, len(seq), MAX_INDEX_LEN, HEAD))
    return list(d.keys()), list(d.values())


class _Encoder:
    """str -> bytes for the byte-exact search.  Latin-1 text maps one to one; text beyond it is remapped so that the
    distinct index characters get bytes 1..K and every other character 0, which keeps equality with the indexes exact."""

    def __init__(self, index_seqs):
        chars = set("".join(index_seqs))
        self.latin1 = all(ord(c) < 256 for c in chars)
        if self.latin1:
            self.spare = next(chr(b) for b in range(256) if chr(b) not in chars)
        else:
            self.table = {c: i + 1 for i, c in enumerate(sorted(chars))}

    def __call__(self, s):
        if self.latin1:
            try:
                return s.encode("latin-1")
            except UnicodeEncodeError:
                return "".join(c if ord(c) < 256 else self.spare for c in s).encode("latin-1")
        return bytes(self.table.get(c, 0) for c in s)


def demultiplex(reads, nextera_file, tso_file, handle=None, batch=BATCH, host=False):
    """The reference's demultiplex(reads, Nextera_Indexes, TSO_Indexes): {renamed header: full sequence} in input order.
    handle: a _lib.Handle to search on (None: one is opened on GPU 0 for this call); host=True uses the host statement
    c3_demux_host instead (tests).  The result does not depend on batch."""
    a_names, a_seqs = load_indexes(nextera_file)
    b_names, b_seqs = load_indexes(tso_file)
    enc = _Encoder(a_seqs + b_seqs)
    set_a, set_b = [enc(s) for s in a_seqs], [enc(s) for s in b_seqs]
    a_names, b_names = a_names + [""], b_names + [""]          # winner -1 -> empty field
    own = None
    if not host and handle is None:
        handle = own = _lib.Handle(device=0)
    try:
        kept = [(name, seq) for name, seq in reads.items() if len(seq) > HEAD]
        out = {}
        for b0 in range(0, len(kept), max(1, int(batch))):
            part = kept[b0:b0 + max(1, int(batch))]
            heads = np.frombuffer(b"".join(enc(seq[:HEAD]) for _, seq in part), dtype=np.uint8).reshape(-1, HEAD)
            win = _lib.demux_host(heads, set_a, set_b) if host else handle.demux_indexes(heads, set_a, set_b)
            for (name, seq), (wa, wb) in zip(part, win.tolist()):
                out[name + "|" + a_names[wa] + "_" + b_names[wb]] = seq
        return out
    finally:
        if own is not None:
            own.close()


def write_fasta_file(path, reads):
    """<path>/Indexed_reads.fasta: one '>name\\nsequence\\n' record per read, in dict order"""
    with open(os.path.join(path, "Indexed_reads.fasta"), "w") as out:
        items = list(reads.items())
        for i in range(0, len(items), 4096):
            out.write("".join(">%s\n%s\n" % kv for kv in items[i:i + 4096]))


# ---- --emit gpu: FASTA text up, Indexed_reads.fasta bytes down (c3_demux_emit) --------------------------
EMIT_CHUNK = 64 << 20   # bytes of input per device call (--demux-chunk); far below C3_FASTA_MAX_TEXT, large enough that the
                        # three waits of a call do not show


def _plain(strings):
    """no byte >= 0x80 and no '|': what the device path needs of index names and sequences"""
    return all(ord(c) < 0x80 and c != "|" for s in strings for c in s)


def run_emit_gpu(input_fasta, output_path, nextera_file, tso_file, chunk=EMIT_CHUNK, handle=None, stats=None):
    """C3POa_demux.py --emit gpu: the input file goes to the device in chunks of raw bytes, each chunk is parsed, searched
    and formatted there (c3_demux_emit) and the returned bytes are appended to <output_path>/Indexed_reads.fasta.part, renamed
    at the end.  No Python loop over reads.  Returns (reads written, reads in the file), or None after a one-line note on
    stderr where only the host path gives the reference's result (nothing is left behind then); stats (a dict) receives
    chunks, records_device and fallback.  Index files are loaded by load_indexes: the same DemuxErrors, before any GPU work."""
    stats = {} if stats is None else stats
    stats.update(chunks=0, records_device=0, fallback=None)
    a_names, a_seqs = load_indexes(nextera_file)
    b_names, b_seqs = load_indexes(tso_file)
    final = os.path.join(output_path, "Indexed_reads.fasta")
    part = final + ".part"
    made_dir = [False]
    state = {"out": None, "buf": None, "own": None}

    def fallback(reason):
        if state["out"] is not None:
            state["out"].close()
            state["out"] = None
        if os.path.exists(part):
            os.remove(part)
        if made_dir[0]:
            try:
                os.rmdir(output_path)
            except OSError:
                pass
        stats["fallback"] = reason
        print("C3POa_demux: --emit gpu falls back to the host path: %s" % reason, file=sys.stderr)
        return None

    if not _plain(a_names + a_seqs + b_names + b_seqs):
        return fallback("an index name or sequence holds '|' or a byte >= 0x80")
    sets = _lib.DemuxSets(a_names, a_seqs, b_names, b_seqs)
    size = max(1, min(int(chunk), _lib.FASTA_MAX_TEXT))
    if handle is None:
        handle = state["own"] = _lib.Handle(device=0)
    try:
        buf = state["buf"] = _lib.PinnedBytes(size)
        out = np.empty(sets.out_bound(size), dtype=np.uint8)
        hashes = np.empty(size // 64 + 1024, dtype=np.uint64)
        collected, written, have, at_eof = [], 0, 0, False
        with open(input_fasta, "rb") as f:
            while not at_eof:
                got = f.readinto(memoryview(buf.arr)[have:size]) if have < size else 0
                at_eof = have < size and got < size - have
                n = have + got
                while True:
                    rc, info = handle.demux_emit_raw(buf.ptr, n, at_eof, sets, out, hashes)
                    if rc == _lib.E_LIMIT and info["n_records"] > hashes.size:
                        hashes = np.empty(info["n_records"] + info["n_records"] // 8, dtype=np.uint64)
                    elif rc == _lib.E_LIMIT and info["out_bytes"] > out.size:
                        out = np.empty(info["out_bytes"] + info["out_bytes"] // 8, dtype=np.uint8)
                    else:
                        break
                if rc != 0:
                    return fallback("c3_demux_emit: %s" % handle.lib.c3_last_error(handle.h).decode())
                if info["departed"]:
                    return fallback("a byte >= 0x80 in the input" if info["departed"] == 1 else "a sequence line in front of the first header")
                stats["chunks"] += 1
                stats["records_device"] += info["n_records"]
                written += info["n_kept"]
                if info["n_records"]:
                    collected.append(hashes[:info["n_records"]].copy())
                if info["out_bytes"]:
                    if state["out"] is None:
                        made_dir[0] = not os.path.isdir(output_path)
                        os.makedirs(output_path, exist_ok=True)
                        state["out"] = open(part, "wb")
                    state["out"].write(memoryview(out)[:info["out_bytes"]])
                used = info["consumed"]
                if used == 0 and not at_eof and n == size:           # one record longer than the chunk: grow it
                    if size >= _lib.FASTA_MAX_TEXT:
                        return fallback("a record longer than C3_FASTA_MAX_TEXT")
                    size = min(2 * size, _lib.FASTA_MAX_TEXT)
                    grown = _lib.PinnedBytes(size)
                    grown.arr[:n] = buf.arr[:n]
                    buf.close()
                    buf = state["buf"] = grown
                    out = np.empty(sets.out_bound(size), dtype=np.uint8)
                elif used:
                    buf.arr[:n - used] = buf.arr[used:n]
                have = n - used
        allh = np.concatenate(collected) if collected else np.empty(0, dtype=np.uint64)
        if np.unique(allh).size != allh.size:
            return fallback("repeated headers in the input (the host path keeps one record per header)")
        if state["out"] is None:
            os.makedirs(output_path, exist_ok=True)
            state["out"] = open(part, "wb")
        state["out"].close()
        state["out"] = None
        os.replace(part, final)
        return written, int(allh.size)
    finally:
        if state["out"] is not None:
            state["out"].close()
        if state["buf"] is not None:
            state["buf"].close()
        if state["own"] is not None:
            state["own"].close()

"""Sample demultiplexer: paper/Demultiplex_R2C2_reads.py of the reference, with the index search on the GPU.

Every consensus read longer than 300 bases is searched in its first 300 bases for each Nextera and each TSO index
(minimum Levenshtein distance over the windows head[i : i+m], i < 300 - m) and renamed `name|<Nextera>_<TSO>`; shorter
reads are dropped.  Each set is decided on its own: the first index of smallest distance (file order breaks ties) wins
when its distance is < 4 and the runner-up's is more than 1 further away, otherwise the field stays empty.  The search
is k_demux (c3_demux_indexes) in batches of bounded size; c3_demux_host is its host statement.  read_fasta,
demultiplex and write_fasta_file keep the reference's function shapes.
"""
import os

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

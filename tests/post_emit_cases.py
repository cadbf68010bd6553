"""Shared cases of test_post_emit_host.py and test_gpu_post_emit.py: reads with HAND-MADE adapter tables (positions do not
depend on alignments), the expected streams from the existing Python path (psl_line -> parse_blat -> write_fasta_file,
pinned to the reference by tests/golden/post_cases.json), and the quality model (the same Python slices and [::-1]).
Nothing here calls the code under test."""
import os
import types

import numpy as np

from c3poa_amd import postprocess as PP
from c3poa_amd.seqio import revcomp

AD_DIR = [("3Prime_adapter", 36), ("5Prime_adapter", 33)]                       # (name, length): the sequences never matter here
AD_UND = [("Adapter", 40)]
AD_NO5 = [("left_ad", 30), ("right_ad", 35)]
AD_DUP = [("3Prime_adapter", 36), ("5Prime_adapter", 33), ("5Prime_adapter", 31)]
ODD = "ACGTNacgtnRYKMBDHVrykmbdhvUu*-"
IDX = [("dT_A", "GAGGTAAAGCAGGGAA"), ("dT_B", "TCATCCGCGTACTTCC"), ("dT_A", "CTCAAAATCTGAATTC"), ("dT_C", "ATGCGTTCAGGACTGA")]
IDX_UNUSED = IDX + [("dT_never", "TTTTGGGGCCCCAAAA")]                           # a destination no read goes to

# option combinations of the issue's table (+ one with every kind of stream at once: the main case)
COMBOS = {
    "none": dict(adapters=AD_DIR),
    "t": dict(adapters=AD_DIR, trim=True),
    "u": dict(adapters=AD_UND, undirectional=True),
    "ut": dict(adapters=AD_UND, undirectional=True, trim=True),
    "b": dict(adapters=AD_DIR, barcoded=True),
    "bt": dict(adapters=AD_DIR, barcoded=True, trim=True),
    "x_ut": dict(adapters=AD_UND, undirectional=True, trim=True, index=IDX),
    "x_dir": dict(adapters=AD_DIR, index=IDX),
    "main": dict(adapters=AD_DIR, barcoded=True, trim=True, index=IDX),
    "no5": dict(adapters=AD_NO5, trim=True),
    "dup": dict(adapters=AD_DUP, trim=True),
    "x_unused": dict(adapters=AD_DIR, trim=True, index=IDX_UNUSED),
}

# (L, p_pos, m_pos) of reads that pass the adapter rule: the slice and position cases of the issue
SPECIAL = [
    (300, 1, 200), (300, 2, 250), (300, 3, 120),                                # p in 1..3: seq[p-4:p+16] wraps
    (300, 1, 2), (200, 0, 9), (200, 5, 15), (300, 10, 20), (300, 3, 39), (100, 2, 16), (90, 7, 25),      # m in 2..15 and 16..39
    (100, 30, 70), (100, 50, 98), (100, 100, 150), (100, 120, 130), (50, 20, 51), (77, 76, 77),          # m+40 > L, m+4 > L, p >= L, m > L
    (16, 2, 10), (12, 1, 11), (5, 1, 3), (16, 3, 14), (1, 0, 1), (10, -3, 8), (15, 2, 13), (3, -1, 2),   # short reads: wrapped slices are not empty
    (200, 50, 59), (200, 50, 60), (300, 100, 199), (300, 100, 200), (1100, 50, 1049),                    # len(seq) 9, 10, 99, 100, 999
    (100, -5, 60), (100, -200, -100), (100, -30, -10), (100, -2 ** 31 + 40, 2 ** 31 - 100), (0, 0, 1), (0, -1, 5),
] + [(bl + 90 + k, 44 + k, 44 + k + bl) for k, bl in enumerate([1, 63, 64, 65, 255, 256, 257])] \
  + [(bl + 61, 30, 30 + bl) for bl in [63, 64, 65, 255, 256, 257]]              # copy-tail lengths at other alignments


def _entry(rng, score=60, matches=30, qbi=0):
    e = [int(x) for x in rng.integers(0, 9, 12)]
    e[0], e[5], e[7] = score, matches, qbi
    return e


def _hit(rng, ad_len, rc, pos, **kw):
    """a table row whose projected position is pos: '+' qEnd + (adLen - tEnd), '-' qStart - (adLen - tEnd)"""
    e = _entry(rng, **kw)
    delta = int(rng.integers(0, 4)) if abs(pos) < 2 ** 30 else 0
    e[4] = ad_len - delta
    e[3] = max(0, e[4] - 25)
    if rc == 0:
        e[2] = pos - delta
        e[1] = e[2] - 24
    else:
        e[1] = pos + delta
        e[2] = e[1] + 24
    return e


def make_reads(combo, seed=7, n_random=260):
    """names, seqs, quals, table [n][n_ad][2][12] for one option combination"""
    c = COMBOS[combo]
    adapters = c["adapters"]
    n_ad = len(adapters)
    rng = np.random.default_rng(seed)
    names, seqs, quals, rows = [], [], [], []

    def add(L, tab, odd=None, seq=None):
        i = len(names)
        alpha = ODD if (i % 3 == 1 if odd is None else odd) else "ACGT"
        names.append("r%04d_%d.%d_%d_%d_%d" % (i, 10 + i % 5, i % 10, 3000 + i, 1 + i % 7, L))
        seqs.append(seq if seq is not None else "".join(alpha[k] for k in rng.integers(0, len(alpha), L)))
        quals.append("".join(chr(33 + int(k)) for k in rng.integers(0, 61, L)))
        rows.append(tab)

    def blank():
        t = np.zeros((n_ad, 2, 12), dtype=np.int64)
        for a in range(n_ad):
            for rc in (0, 1):
                if rng.random() < 0.3:                                          # below MIN_SCORE: no PSL row, whatever else it says
                    t[a, rc] = _entry(rng, score=int(rng.integers(0, 22)), matches=int(rng.integers(0, 40)))
        return t

    def pair(i):
        """(plus adapter, minus adapter) of read i: different names where the adapter set has them"""
        return (0, 0) if n_ad == 1 else ((1, 0) if i % 2 == 0 else (0, 1))

    def kept(L, p, m, **kw):
        t = blank()
        ap, am = pair(len(names))
        t[ap, 0] = _hit(rng, adapters[ap][1], 0, p)
        t[am, 1] = _hit(rng, adapters[am][1], 1, m)
        add(L, t, **kw)

    for L, p, m in SPECIAL:
        kept(L, p, m)
    # drop rules, each between two kept reads
    for rule in ("two", "none", "order", "class"):
        kept(240, 40, 200)
        t = blank()
        ap, am = pair(len(names))
        t[ap, 0] = _hit(rng, adapters[ap][1], 0, 40)
        t[am, 1] = _hit(rng, adapters[am][1], 1, 200)
        if rule == "two":
            if n_ad > 1:
                t[am, 0] = _hit(rng, adapters[am][1], 0, 60)
            else:
                t[0, 0, 0] = 0                                                  # one adapter: the strand cannot hold two hits; none instead
        elif rule == "none":
            t[am, 1] = _entry(rng, score=0, matches=0)
        elif rule == "order":
            t[am, 1] = _hit(rng, adapters[am][1], 1, 40 if len(names) % 2 else 39)          # m == p, m < p
        elif n_ad > 1:
            t[am, 1] = _entry(rng, score=0, matches=0)
            t[ap, 1] = _hit(rng, adapters[ap][1], 1, 200)                       # both hits name the same adapter
        add(240, t)
        kept(240, 41, 201)
    # the three filters at their edges: an extra '+' row that must not count (kept) and one that counts (two hits: dropped)
    for kw, counts in ((dict(qbi=50), False), (dict(qbi=49), True), (dict(matches=10), False), (dict(matches=11), True),
                       (dict(score=21), False), (dict(score=22), True)):
        t = blank()
        ap, am = pair(len(names))
        t[ap, 0] = _hit(rng, adapters[ap][1], 0, 30)
        t[am, 1] = _hit(rng, adapters[am][1], 1, 180)
        if n_ad > 1:
            t[am, 0] = _hit(rng, adapters[am][1], 0, 50, **kw)
        else:
            t[0, 0] = _hit(rng, adapters[0][1], 0, 30, **kw)                     # one adapter: the only '+' row itself
        add(220, t)
    if n_ad == 3:                                                               # duplicate names: hits of the two namesakes are one class
        for ap, am in ((1, 2), (2, 1), (0, 2), (2, 0)):
            t = blank()
            t[ap, 0] = _hit(rng, adapters[ap][1], 0, 35)
            t[am, 1] = _hit(rng, adapters[am][1], 1, 190)
            add(230, t)
    # planted oligo-dT indexes: forward at seq[p : p+16], reverse-complemented at seq[m-16 : m], both, neither
    if c.get("index"):
        idx = [s for _n, s in IDX]
        for k in range(48):
            L, p, m = 260 + k, 30 + k % 5, 220 + k % 7
            s = list("".join("ACGT"[j] for j in rng.integers(0, 4, L)))
            mode = k % 4
            tag = idx[(k // 4) % 4]
            if k % 8 == 7:
                tag = tag[:5] + ("A" if tag[5] != "A" else "C") + tag[6:]        # one mismatch still wins
            if mode in (0, 2):
                s[p:p + 16] = tag
            if mode in (1, 2):
                s[m - 16:m] = revcomp(idx[(k // 4 + 1) % 4])
            kept(L, p, m, seq="".join(s))
    for _ in range(n_random):
        L = int(rng.integers(20, 600))
        p = int(rng.integers(-10, L + 10))
        m = int(rng.integers(-10, L + 60)) if rng.random() < 0.2 else p + int(rng.integers(1, max(2, L - p + 40)))
        if rng.random() < 0.85:
            kept(L, p, m)
        else:                                                                   # anything: counted rows anywhere, PSL rows that do not count
            t = blank()
            for a in range(n_ad):
                for rc in (0, 1):
                    if rng.random() < 0.5:
                        t[a, rc] = _hit(rng, adapters[a][1], rc, int(rng.integers(-50, L + 50)), matches=int(rng.integers(5, 40)),
                                        qbi=int(rng.integers(0, 80)), score=int(rng.integers(15, 90)))
            add(L, t)
    tab = np.array(rows, dtype=np.int64)
    assert tab.min() >= -2 ** 31 and tab.max() < 2 ** 31
    return names, seqs, quals, tab.astype(np.int32)


def opts_of(combo):
    c = COMBOS[combo]
    return types.SimpleNamespace(undirectional=bool(c.get("undirectional")), trim=bool(c.get("trim")), barcoded=bool(c.get("barcoded")))


def index_of(combo):
    """(idx_to_seq, seq_to_idx) exactly as read_fasta(index_file, True) builds them, or ({}, {})"""
    idx_to_seq, seq_to_idx = {}, {}
    for n, s in COMBOS[combo].get("index") or []:
        idx_to_seq[n] = s
        seq_to_idx[s] = n
    return idx_to_seq, seq_to_idx


def classify(opts, adapter_dict, reads, seq_to_idx, idx_to_seq):
    """the kept reads as write_fasta_file decides them: [(name, p_pos, m_pos, direction, destination directory)]"""
    keep = []
    for name, sequence in reads.items():
        plus = [x for x in adapter_dict[name]["+"] if x[0] != "-"]
        minus = [x for x in adapter_dict[name]["-"] if x[0] != "-"]
        if len(plus) != 1 or len(minus) != 1 or minus[0][2] <= plus[0][2]:
            continue
        p, m = plus[0][2], minus[0][2]
        if opts.undirectional:
            d = "+"
        elif plus[0][0] != minus[0][0]:
            d = "+" if plus[0][0] == "5Prime_adapter" else "-"
        else:
            continue
        dest = ""
        if seq_to_idx:
            f, r = PP.match_index(sequence[p - 4:p + 16], seq_to_idx), PP.match_index(revcomp(sequence[m - 16:m + 4]), seq_to_idx)
            dest = "no_index_found"
            if f in idx_to_seq and r not in idx_to_seq:
                d, dest = "-", f
            if r in idx_to_seq and f not in idx_to_seq:
                d, dest = "+", r
        keep.append((name, p, m, d, dest))
    return keep


def fastq_model(opts, keep, reads, quals):
    """{(destination, file kind 0 main / 1 left / 2 right): text}: write_fasta_file's slices applied to the quality string as
    well, reversed wherever the sequence is reverse-complemented"""
    out = {}
    for name, p, m, d, dest in keep:
        s, q = reads[name], quals[name]
        hdr = "@%s_%d\n" % (name, len(s[p:m]))
        main = slice(p, m) if opts.trim else slice(max(p - 40, 0), m + 40)

        def rec(sl, rc):
            return hdr + (revcomp(s[sl]) if rc else s[sl]) + "\n+\n" + (q[sl][::-1] if rc else q[sl]) + "\n"
        if d == "+":
            recs = (rec(main, False), rec(slice(m, None), False), rec(slice(None, p), True))
        else:
            recs = (rec(main, True), rec(slice(None, p + 40), True), rec(slice(m, None), False))
        for k in range(3):
            out[(dest, k)] = out.get((dest, k), "") + recs[k]
    return out


def _fasta_of(fq):
    lines = fq.split("\n")
    return "".join(">" + lines[i][1:] + "\n" + lines[i + 1] + "\n" for i in range(0, len(lines) - 1, 4))


def expected_streams(combo, names, seqs, quals, table, tmpdir, with_quals):
    """the streams the Python path writes for this batch, in c3_post_emit's order, and the kept reads (classify).  dests = the
    destination names of the plan ([""] without an index set)."""
    from c3poa_amd._lib import PostPlan
    c = COMBOS[combo]
    adapters = c["adapters"]
    opts = opts_of(combo)
    idx_to_seq, seq_to_idx = index_of(combo)
    reads = dict(zip(names, seqs))
    assert len(reads) == len(names)
    out = os.path.join(str(tmpdir), combo + ("_q" if with_quals else "")) + "/"
    os.makedirs(out)
    psl = out + PP.PSL_NAME
    rows = [PP.psl_line(names[i], len(seqs[i]), adapters[a][0], adapters[a][1], "-" if rc else "+", table[i, a, rc])
            for i, a, rc in np.argwhere(table[:, :, :, 0] >= PP.MIN_SCORE)]
    with open(psl, "w") as fh:
        if rows:
            fh.write("\n".join(rows) + "\n")
    adapter_dict = PP.parse_blat(psl, reads)
    n = PP.write_fasta_file(opts, out, adapter_dict, reads, seq_to_idx, idx_to_seq, match_batch=PP.match_batch_host)
    keep = classify(opts, adapter_dict, reads, seq_to_idx, idx_to_seq)
    assert n == len(keep)

    def rd(path):
        return open(path, "rb").read() if os.path.exists(path) else b""
    dests = PostPlan([(a[0], "A" * a[1]) for a in adapters], (idx_to_seq, seq_to_idx) if seq_to_idx else None).dests
    streams = []
    model = fastq_model(opts, keep, reads, dict(zip(names, quals)))
    for d in dests:
        base = out + (d + "/" if seq_to_idx else "")
        for k, f in enumerate((PP.FLC, PP.FLC_LEFT, PP.FLC_RIGHT)):
            fa = rd(base + f)
            fq = model.get((d if seq_to_idx else "", k), "")
            assert _fasta_of(fq).encode() == fa                                  # the model's sequences are the Python path's
            streams.append(fq.encode() if with_quals else fa)
    streams += [rd(out + PP.FLC_10X), rd(out + PP.MUX_TSV), rd(psl)]
    return streams, keep, dests


def plan_of(combo):
    from c3poa_amd._lib import PostPlan
    c = COMBOS[combo]
    idx_to_seq, seq_to_idx = index_of(combo)
    return PostPlan([(a[0], "A" * a[1]) for a in c["adapters"]], (idx_to_seq, seq_to_idx) if seq_to_idx else None,
                    undirectional=c.get("undirectional"), trim=c.get("trim"), barcoded=c.get("barcoded"))


def split(arena, so):
    return [arena[int(so[s]):int(so[s + 1])].tobytes() for s in range(len(so) - 1)]

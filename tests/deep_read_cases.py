"""Deep reads: 31 to 250 kept subreads per read, both capacity limits (250 kept subreads, 255 peaks) and POA graphs with nodes
of 16 and more predecessors / successors.  A short insert in a 50 - 100 kb read gives such reads; everything the consensus
path sizes by the subread count (k_poa's edge slots and many-predecessor rows, the first-pass scratch, run_polish's NLcap /
K / Ncap / Lcap, k_prep's layer tables, k_peaks' length median, the window edge weights) is exercised by them alone.

Shared by tests/test_deep_reads_host.py (the oracle side: every case has the shape it claims) and
tests/test_gpu_deep_reads.py (the device against the oracle).  Everything here is built once per process and cached;
nothing needs a GPU.  The generator of tests/test_gpu_edge_cases.py and tests/low_complexity_cases.py lives here."""
import collections
import ctypes as C

import numpy as np

from c3poa_amd import synth

MAX_SUB = 250                   # C3_MAX_SUB (c3_dev.h): kept subreads of one read
MAX_KEPT_PEAKS = 255            # C3_MAX_PEAKS - 1 (include/c3poa.h): peaks of one track
ST_OK, ST_NO_PEAKS, ST_NO_CONSENSUS, ST_LIMIT = 0, 2, 3, 5


def rand_seq(rng, L):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, L))


def concatemer(rng, splint, insert, n, k0, k1, err=0.1):
    """k0 bases of insert, n times (splint + insert), splint, k1 bases of insert, with `err` errors (40 % substitutions,
    25 % insertions, 35 % deletions).  insert: a sequence, or a length (then drawn from rng first).  -> (seq, qual)"""
    ins = rand_seq(rng, insert) if isinstance(insert, (int, np.integer)) else insert
    clean = ins[len(ins) - k0:] + (splint + ins) * n + splint + ins[:k1]
    s, q = synth._mutate(rng, np.frombuffer(clean.encode(), dtype=np.uint8), sub=err * 0.4, ins=err * 0.25, dele=err * 0.35)
    return s.decode(), q.decode()


SPLINT = rand_seq(np.random.default_rng(20270), 120)

# one read: its sequence, qualities, splint, the mdistcutoff it runs under and the subreads it was built with
Read = collections.namedtuple("Read", "name seq qual splint mdist built")

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- case 1: the depth sweep.  Seeds picked so that the oracle keeps every subread that was built (the host test asserts it).
DEPTH_SEEDS = {31: 0, 64: 0, 128: 0, 249: 0, 250: 0}
DEPTHS = tuple(sorted(DEPTH_SEEDS))
DEPTH120_SEED = 0


def depth_read(n):
    """splint 120, insert 120, n subreads, dangling pieces of 110, 12 % errors, mdistcutoff 150"""
    def make():
        s, q = concatemer(np.random.default_rng([20271, n, DEPTH_SEEDS[n]]), SPLINT, 120, n, 110, 110, err=0.12)
        return Read("depth%d" % n, s, q, SPLINT, 150, n)
    return _once(("depth", n), make)


def depth120_read():
    """the shape of test_many_repeats_and_long_read at four times its depth: SPLINT1, insert 250, 120 subreads, mdistcutoff 400"""
    def make():
        s, q = concatemer(np.random.default_rng([20272, DEPTH120_SEED]), synth.SPLINT1, 250, 120, 120, 120)
        return Read("depth120_splint1", s, q, synth.SPLINT1, 400, 120)
    return _once("depth120", make)


def sweep_reads():
    return tuple(depth_read(n) for n in DEPTHS) + (depth120_read(),)


# ---- case 2: the caps.  A read of `units` times (splint + insert) has units + 1 peaks; `odd` of the units carry an insert of
# twice the length, so their subread falls outside 0.8 .. 1.2 of the median length and is not kept.
#   name: (units, odd units, errors, seed) -> peaks = units + 1, kept subreads = units - odd
CAP_SHAPES = collections.OrderedDict([
    ("sub250", (250, 0, 0.12, 0)),          # the last admitted depth (the read of the depth sweep)
    ("sub251", (251, 0, 0.12, 0)),          # one kept subread too many
    ("sub254", (254, 0, 0.12, 0)),          # 255 peaks, all kept: still the subread cap
    ("peaks255", (254, 6, 0.12, 0)),        # 255 peaks, 248 kept subreads: both counts admitted
    ("peaks256", (255, 8, 0.12, 0)),        # one peak too many, although only 247 subreads would be kept
    ("clean250", (250, 0, 0.0, 0)),         # error-free: every layer identical, every merge a tie
])


def cap_read(name):
    units, odd, err, seed = CAP_SHAPES[name]
    if name == "sub250":
        return depth_read(250)

    def make():
        rng = np.random.default_rng([20273, units, odd, seed])
        ins = rand_seq(rng, 120)
        long_ins = ins + rand_seq(rng, 120)
        at = set(int(x) for x in np.linspace(20, units - 20, odd).round()) if odd else set()
        assert len(at) == odd
        clean = ins[len(ins) - 110:] + "".join(SPLINT + (long_ins if u in at else ins) for u in range(units)) + SPLINT + ins[:110]
        s, q = synth._mutate(rng, np.frombuffer(clean.encode(), dtype=np.uint8), sub=err * 0.4, ins=err * 0.25, dele=err * 0.35)
        return Read(name, s.decode(), q.decode(), SPLINT, 150, units - odd)
    return _once(("cap", name), make)


def cap_reads():
    return tuple(cap_read(k) for k in CAP_SHAPES)


def neighbours(n=2):
    """ordinary cfg1 reads (SPLINT1, three subreads of 1 216 bases) that share a batch, and so its mdistcutoff of 150, with
    the deep reads: (read, strand) pairs"""
    return _once(("cfg1", n), lambda: tuple((Read(r[0], r[1], r[2], synth.SPLINT1, 150, 3), r[3])
                                            for r in synth.generate("cfg1", n_reads=n)))


# ---- case 3: high-degree nodes by construction
#   (kind, copies with a deletion): largest in-degree, largest out-degree of the oracle's graph (tests/test_deep_reads_host.py
#   asserts them from the oracle's MSA, with the floors of 30 predecessors and 16 successors)
LADDERS = collections.OrderedDict([(("in", 40), (32, 4)), (("in", 100), (31, 4)), (("in", 200), (34, 4)),
                                   (("out", 100), (4, 21)), (("out", 200), (4, 33))])


def ladder(kind, N, quals="mixed"):
    """three copies of a 300-base sequence plus N copies with one deletion each.  kind "in": 1 + k % 40 bases that all END at
    position 200, so the node of base 200 collects a predecessor per deletion length.  kind "out": 1 + 7 k % 80 bases that all
    START at position 100, so the node of base 99 gets a successor per length.  (The mirror image of "in", 1 + k % 40 from
    position 100, stops at 11 to 14 successors on the oracle: the aligner reaches base 100 + d over the edge an earlier copy
    left, matches a base on the way by chance and opens a second gap, which is cheaper than one long gap.  Lengths that
    arrive far from the ones already in the graph leave fewer such detours.)  -> (subreads, qualities)"""
    def make():
        rng = np.random.default_rng([20274, N])
        base = rand_seq(rng, 300)
        subs = [base] * 3
        for k in range(N):
            d = 1 + k % 40 if kind == "in" else 1 + 7 * k % 80
            subs.append(base[:200 - d] + base[200:] if kind == "in" else base[:100] + base[100 + d:])
        if quals == "equal":
            qs = ["I" * len(s) for s in subs]
        else:
            qs = ["".join(chr(33 + int(v)) for v in rng.integers(2, 41, len(s))) for s in subs]
        return tuple(subs), tuple(qs)
    return _once(("ladder", kind, N, quals), make)


def msa_degrees(msa):
    """largest in- and out-degree of the POA graph an MSA came from: nodes are (column, base), an edge joins the nodes of
    two consecutive bases of a row; distinct predecessors / successors per node"""
    pred, succ = collections.defaultdict(set), collections.defaultdict(set)
    for row in msa:
        last = None
        for c, b in enumerate(row):
            if b == "-":
                continue
            if last is not None:
                pred[(c, b)].add(last); succ[last].add((c, b))
            last = (c, b)
    return max(len(v) for v in pred.values()), max(len(v) for v in succ.values())


# ---- case 4: extreme qualities on the 128-subread read
def quality_variants():
    """the 128-subread read at qualities all '~', all '!' and alternating; the 250-subread read at '~', where a window edge
    shared by every layer weighs 2 * 93 * 252 = 46 872, beyond a signed 16-bit value"""
    r, deep = depth_read(128), depth_read(250)
    L = len(r.seq)
    return tuple(r._replace(name="depth128_" + k, qual=q) for k, q in
                 (("q93", "~" * L), ("q0", "!" * L), ("q0_q93", "".join("!~"[i & 1] for i in range(L))))) + \
        (deep._replace(name="depth250_q93", qual="~" * len(deep.seq)),)


# ---- the oracle side, computed once
def oracle(read, strand="+", rowstats=False, capture=False):
    """(record fields as a dict, consensus, row statistics or None, captured windows or None) of one read on the CPU oracle.
    Row statistics: the c3o_poa_rowstats counters tools/poa_row_stats.py prints (0 rows, 4 general rows, 24 rows with more
    than four predecessors, 25 rows with a far predecessor)."""
    def make():
        from oracle import oracle_py as O
        lib = O.lib()
        S = (C.c_int64 * 64).in_dll(lib, "c3o_poa_rowstats")
        on = C.c_int.in_dll(lib, "c3o_poa_rowstats_on")
        stats = wins = None
        if rowstats:
            for i in range(64):
                S[i] = 0
            on.value = 1
        if capture:
            O.win_capture(True)
        try:
            res, cons = O.process_batch(read.splint, [(read.seq, read.qual)], [strand], params=O.default_params(mdistcutoff=read.mdist), threads=1)
            if rowstats:
                stats = tuple(int(x) for x in S)
            if capture:
                wins = [dict(win=a["win"], layer=a["layer"], n=a["n"], Q=a["Q"]) for a in O.win_captured()]
        finally:
            on.value = 0
            if capture:
                O.win_capture(False)
        r = res[0]
        rec = dict(status=int(r.status), n_peaks=int(r.n_peaks), n_sub=int(r.n_sub), cons_len=int(r.cons_len),
                   peaks=tuple(r.peaks[:r.n_peaks]) if 0 <= r.n_peaks <= 256 else (),
                   sub_beg=tuple(r.sub_beg[:r.n_sub]) if 0 <= r.n_sub <= 256 else (),
                   sub_end=tuple(r.sub_end[:r.n_sub]) if 0 <= r.n_sub <= 256 else (),
                   has_front=int(r.has_front), has_tail=int(r.has_tail), front_end=int(r.front_end), tail_beg=int(r.tail_beg),
                   cells_poa=int(r.cells_poa), cells_polish=int(r.cells_polish))
        return rec, cons[0], stats, wins
    return _once(("oracle", read.name, strand, rowstats, capture), make)

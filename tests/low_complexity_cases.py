"""Low-complexity inserts for the consensus kernels (CPU: test_low_complexity_host.py, GPU: test_gpu_low_complexity.py).  A plain
module, no fixtures, no GPU: every case is a pure function of a fixed seed, so both files see the same inputs.

Every other comparison of k_poa, k_poa_pair, k_prep and k_window with the oracle draws its inserts from uniformly random
A/C/G/T, where a row maximum is tied in well under one row in a hundred.  Here the inserts hold homopolymers, short tandem
repeats and poly-A tails, where ties decide: the adaptive band of the POA follows the first and the last column of a tied row
maximum, H / E1 / E2 / F tie in most cells of a tract, every phase shift of a repeat is co-optimal for the seam traceback of
k_prep and for the banded rows of k_window, and with equal qualities every decision of the pairwise merge is a tie.

A case is Case(name, subs, quals, front, tail, cfg, group, tract): the first six go through the pre-split determine_consensus
probe (front / tail: (seq, qual) or None; cfg: keyword arguments of the handle and of the oracle's parameters); group names the
family group whose tie shares the host test puts a floor under; tract is the (first, last + 1) span of the tract in the
insert where a test needs it, else None.  Families are noisy copies of one insert (synth._mutate) unless said otherwise, and no
subread is longer than 1 792 bases, so k_poa_pair and the fast / near rows take them.

  tracts    a tract between random flanks: a poly-A tail of 120, homopolymer blocks (runs of 5 - 40 of all four bases), AC x 150,
            CAG x 100, a random heptamer x 70, a random 64-mer x 10 and a random 65-mer x 10 (periods at the lane count and one
            past it; these two have flanks of 200 so that their drafts cut into more than fifteen windows of 64); in the same
            group the 64-mer and 65-mer families under pol_window = 64, where the window equals the period
  noflank   no flanks at all: A x 500, AC x 300, a random two-letter insert of 600
  runlen    subreads that differ from the insert ONLY in the lengths of its runs of three and more, by up to 2 or up to 15 bases:
            no substitutions, random qualities
  drift     three subreads, subread 1 with 30 AC units, 8 heptamer units or 40 A more or fewer than the other two: the band
            drifts, the pair kernel gets rows of 65 - 128 columns, the polish a layer much longer or shorter than its window
  seam      insert 1 300 = 400 random + 700 of tract + 200 random: the window seams at 500 and 1 000 fall inside the tract
  equalq    every quality equal: a pair over random + A x 60 + random + AC x 40 + random at 'I' and at '5', three subreads at 'I'
  dangling  a poly-A-tail and a heptamer family with a front and a tail cut from further noisy copies (the front a suffix, the
            tail a prefix, as tests/test_gpu_parity.py cuts them) so that the cut, the free end of the piece's anchored
            extension, lies inside the tract
  control   one random insert of 600: the contrast

BATCH: concatemers of such inserts for one run of the whole pipeline (splitter, work lists, many slots, the cost-sorted queue)."""
import collections

import numpy as np

from c3poa_amd import synth
from c3poa_amd.seqio import revcomp

from deep_read_cases import concatemer

Case = collections.namedtuple("Case", "name subs quals front tail cfg group tract")

QMAX = 1792                     # longest subread k_poa_pair takes
COUNTS = (2, 3, 6, 12)          # subreads per family: tracts and noflank
SEAM_COUNTS = (2, 3, 6)


def _acgt(rng, n):
    return synth._ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _noisy(rng, clean):
    s, q = synth._mutate(rng, np.frombuffer(clean.encode(), dtype=np.uint8))
    return s.decode(), q.decode()


def _qual(rng, n):
    return "".join(chr(33 + int(v)) for v in rng.integers(2, 41, n))


def _family(rng, insert, n):
    subs, quals = [], []
    for _ in range(n):
        s, q = _noisy(rng, insert)
        subs.append(s); quals.append(q)
    return subs, quals


def _unit(rng, k):
    """a random unit of k bases that is no repeat of a shorter one and does not end on its first base"""
    while True:
        u = _acgt(rng, k)
        if u[0] != u[-1] and all(u != (u[:p] * k)[:k] for p in range(1, k)):
            return u


def _blocks(rng, n):
    """homopolymer blocks of 5 - 40 bases over all four bases, neighbours different, n bases in all"""
    out, last = [], -1
    while sum(len(b) for b in out) < n:
        c = int(rng.integers(0, 4))
        if c == last:
            continue
        out.append("ACGT"[c] * int(rng.integers(5, 41)))
        last = c
    return "".join(out)[:n]


def _between(rng, tract, left, right):
    """(insert, span of the tract): the tract between random flanks that do not continue it"""
    while True:
        a, b = _acgt(rng, left), _acgt(rng, right)
        if (not a or a[-1] != tract[0]) and (not b or b[0] != tract[-1]):
            return a + tract + b, (left, left + len(tract))


def tract_inserts(rng):
    """name -> (insert, span of the tract)"""
    u7, u64, u65 = _unit(rng, 7), _unit(rng, 64), _unit(rng, 65)
    return collections.OrderedDict([
        ("polyA_tail", _between(rng, "A" * 120, 250, 60)),
        ("hp_blocks", _between(rng, _blocks(rng, 300), 100, 100)),
        ("AC150", _between(rng, "AC" * 150, 100, 100)),
        ("CAG100", _between(rng, "CAG" * 100, 100, 100)),
        ("hept70", _between(rng, u7 * 70, 80, 80)),
        ("p64x10", _between(rng, u64 * 10, 200, 200)),
        ("p65x10", _between(rng, u65 * 10, 200, 200)),
    ])


def _runs(s):
    """[(base, length)] of s"""
    out = []
    for c in s:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return out


def _runlen_copy(rng, insert, d):
    """the insert with every run of three and more bases changed in length by -d .. d (never below one base): nothing else"""
    out = []
    for c, n in _runs(insert):
        if n >= 3:
            n = max(1, n + int(rng.integers(-d, d + 1)))
        out.append(c * n)
    s = "".join(out)
    return s, _qual(rng, len(s))


def _drift(rng, unit, n_units, delta):
    """(subs, quals, span): three noisy copies of random 200 + unit x n_units + random 200; subread 1 has delta units more"""
    tract = unit * n_units
    ins, span = _between(rng, tract, 200, 200)
    alt = ins[:span[0]] + unit * (n_units + delta) + ins[span[1]:]
    subs, quals = [], []
    for k in range(3):
        s, q = _noisy(rng, alt if k == 1 else ins)
        subs.append(s); quals.append(q)
    return subs, quals, span


def _build():
    cases = []

    def add(name, subs, quals, group, front=None, tail=None, cfg=None, tract=None):
        assert all(0 < len(s) <= QMAX and len(s) == len(q) for s, q in zip(subs, quals)), name
        cases.append(Case(name, tuple(subs), tuple(quals), front, tail, dict(cfg or {}), group, tract))

    rng = np.random.default_rng(20260)
    tracts = tract_inserts(rng)
    for name, (ins, span) in tracts.items():
        for n in COUNTS:
            add("%s_n%d" % (name, n), *_family(rng, ins, n), group="tracts", tract=span)

    rng = np.random.default_rng(20261)
    two = "".join("AT"[i] for i in rng.integers(0, 2, 600))
    for name, ins in (("A500", "A" * 500), ("AC300", "AC" * 300), ("two_letter600", two)):
        for n in COUNTS:
            add("%s_n%d" % (name, n), *_family(rng, ins, n), group="noflank", tract=(0, len(ins)))

    rng = np.random.default_rng(20262)
    for name in ("hp_blocks", "polyA_tail"):
        for d, n in ((2, 3), (15, 6)):
            copies = [_runlen_copy(rng, tracts[name][0], d) for _ in range(n)]
            add("runlen_%s_d%d_n%d" % (name, d, n), [c[0] for c in copies], [c[1] for c in copies], group="runlen")

    rng = np.random.default_rng(20263)
    u7 = _unit(rng, 7)
    for name, unit, n_units, delta in (("AC", "AC", 100, 30), ("hept", u7, 30, 8), ("A", "A", 80, 40)):
        for sign in (1, -1):
            subs, quals, span = _drift(rng, unit, n_units, sign * delta)
            add("drift_%s_%+d" % (name, sign * delta), subs, quals, group="drift", tract=span)

    rng = np.random.default_rng(20264)
    u7, u64 = _unit(rng, 7), _unit(rng, 64)
    for name, unit in (("A", "A"), ("AC", "AC"), ("CAG", "CAG"), ("hept", u7), ("p64", u64)):
        ins, span = _between(rng, (unit * (700 // len(unit) + 1))[:700], 400, 200)
        for n in SEAM_COUNTS:
            add("seam_%s_n%d" % (name, n), *_family(rng, ins, n), group="seam", tract=span)

    rng = np.random.default_rng(20265)
    for name in ("p64x10", "p65x10"):
        ins, span = tracts[name]
        add("window64_%s" % name, *_family(rng, ins, 3), group="tracts", cfg={"pol_window": 64}, tract=span)

    rng = np.random.default_rng(20266)
    ins = _acgt(rng, 50) + "A" * 60 + _acgt(rng, 50) + "AC" * 40 + _acgt(rng, 50)
    for name, n, ch in (("pair_I", 2, "I"), ("pair_5", 2, "5"), ("three_I", 3, "I")):
        subs, _ = _family(rng, ins, n)
        add("equalq_%s" % name, subs, [ch * len(s) for s in subs], group="equalq")

    rng = np.random.default_rng(20267)
    for name, k_front, k_tail in (("polyA_tail", 60 + 60, 250 + 60), ("hept70", 80 + 200, 80 + 250)):
        ins, span = tracts[name]
        subs, quals = _family(rng, ins, 3)
        fs, fq = _family(rng, ins, 2)
        # the cut of the front (its first base) and of the tail (its last base) lie inside the tract, up to the copy's indels
        assert span[0] + 20 < len(ins) - k_front < span[1] - 20 and span[0] + 20 < k_tail < span[1] - 20
        front = (fs[0][len(fs[0]) - k_front:], fq[0][len(fs[0]) - k_front:])
        tail = (fs[1][:k_tail], fq[1][:k_tail])
        add("dangling_%s" % name, subs, quals, group="dangling", front=front, tail=tail, tract=span)

    rng = np.random.default_rng(20268)
    add("control_random600", *_family(rng, _acgt(rng, 600), 3), group="control")
    return tuple(cases)


CASES = _build()
GROUPS = tuple(collections.OrderedDict((c.group, None) for c in CASES))


_concatemer = concatemer            # over a given insert (tests/deep_read_cases.py)


def _build_batch():
    """24 reads: (seq, qual) and strands.  Inserts of the tract, no-flank and seam families, SPLINT1, three to six repeats,
    dangling pieces of 150, every third read reverse-complemented"""
    rng = np.random.default_rng(20269)
    tracts = tract_inserts(rng)
    u7 = _unit(rng, 7)
    inserts = [v[0] for v in tracts.values()]
    inserts += ["A" * 500, "AC" * 300, "".join("AT"[i] for i in rng.integers(0, 2, 600))]
    for unit in ("A", "AC", "CAG", u7):
        inserts.append(_between(rng, (unit * (700 // len(unit) + 1))[:700], 400, 200)[0])
    reads, strands = [], []
    for k in range(24):
        s, q = _concatemer(rng, synth.SPLINT1, inserts[k % len(inserts)], 3 + k % 4, 150, 150)
        if k % 3 == 2:
            s, q, st = revcomp(s), q[::-1], "-"
        else:
            st = "+"
        reads.append((s, q)); strands.append(st)
    return tuple(reads), tuple(strands)


BATCH = _build_batch()


_ref = {}


def reference():
    """the oracle's (consensus, draft, (cells_poa, cells_polish)) of every case, computed once"""
    from oracle import oracle_py as O
    if "cases" not in _ref:
        _ref["cases"] = tuple(O.determine_consensus(c.subs, c.quals, c.front, c.tail, params=O.default_params(**c.cfg), return_draft=True)
                              for c in CASES)
    return _ref["cases"]


def batch_reference():
    """the oracle's (records, consensi) of BATCH, computed once"""
    from oracle import oracle_py as O
    if "batch" not in _ref:
        _ref["batch"] = O.process_batch(synth.SPLINT1, list(BATCH[0]), list(BATCH[1]), threads=8)
    return _ref["batch"]

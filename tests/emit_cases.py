"""Shared cases of test_emit_host.py and test_gpu_emit.py: small groups with HAND-WRITTEN c3_read_result records (nothing
here depends on an alignment), their consensus / QV bytes, and the files the existing writer (c3_write_group,
c3_write_consensus_fastq) makes of them, which is the yardstick of both tests.  Nothing here calls the code under test."""
import os

import numpy as np

from c3poa_amd import _lib

N_SPLINTS = 2
ST = dict(ok=0, not_assigned=1, no_peaks=2, no_cons=3, too_short=4, limit=5)
# (tot, L) whose quotient is a tie or near one at two decimals (the issue's pins, Python's str(round(tot / L, 2)))
AVGQ_PINS = [(107, 40, "2.67"), (1, 8, "0.12"), (3, 8, "0.38"), (5, 8, "0.62"), (1, 200, "0.01"), (3, 200, "0.01"),
             (1, 400, "0.0"), (0, 5, "0.0"), (13, 1, "13.0"), (25, 2, "12.5"), (-1, 8, "-0.12"), (-1, 400, "-0.0")]
ALPHA = np.frombuffer(b"ACGTacgtNn\x80\xff*-", dtype=np.uint8)


class Group:
    """one group: lists per read, turned into the arrays the C calls take"""

    def __init__(self, seed=1):
        self.rng = np.random.default_rng(seed)
        self.names, self.seqs, self.quals, self.cons, self.qv, self.sid, self.recs, self.what = [], [], [], [], [], [], [], []

    def add(self, what, L, sid, status=0, subs=(), front=None, tail=None, clen=0, name=None, qual=None):
        rng = self.rng
        i = len(self.names)
        self.what.append(what)
        self.names.append(name if name is not None else b"read%d_%s" % (i, what.encode()))
        self.seqs.append(ALPHA[rng.integers(0, len(ALPHA), L)].tobytes())
        self.quals.append(qual if qual is not None else rng.integers(33, 127, L).astype(np.uint8).tobytes())
        assert len(self.quals[-1]) == L
        ok = status == 0
        self.cons.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, clen if ok else 0)].tobytes())
        self.qv.append(rng.integers(33, 94, clen if ok else 0).astype(np.uint8).tobytes())
        self.sid.append(sid)
        self.recs.append(dict(status=status, subs=list(subs), front=front, tail=tail, clen=clen))

    def arrays(self):
        n = len(self.names)
        res = np.zeros(n, dtype=_lib.RESULT_DTYPE)
        rng = np.random.default_rng(7)
        for k in ("peaks", "sub_beg", "sub_end"):                 # array tails are unspecified: fill them with rubbish
            res[k] = rng.integers(-2 ** 31, 2 ** 31 - 1, (n, _lib.MAX_PEAKS))
        for i, r in enumerate(self.recs):
            res["status"][i] = r["status"]; res["n_sub"][i] = len(r["subs"]); res["n_peaks"][i] = len(r["subs"]) + 1
            for k, (b, e) in enumerate(r["subs"]):
                res["sub_beg"][i, k], res["sub_end"][i, k] = b, e
            res["has_front"][i] = r["front"] is not None; res["front_end"][i] = r["front"] or 0
            res["has_tail"][i] = r["tail"] is not None; res["tail_beg"][i] = r["tail"] or 0
            res["cons_len"][i] = r["clen"]
        coff = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(c) for c in self.cons], out=coff[1:])
        cons = np.frombuffer(b"".join(self.cons) + b"\0" * 16, dtype=np.uint8)
        qv = np.frombuffer(b"".join(self.qv) + b"\0" * 16, dtype=np.uint8)
        hb = _lib.HostBatch.from_lists(self.names, self.seqs, self.quals)
        return hb, res, cons, coff, qv, np.array(self.sid, dtype=np.int16)


def qual_with(tot, L):
    """L quality bytes whose sum - 33 * L is tot"""
    base, extra = divmod(tot + 33 * L, L)
    q = np.full(L, base, dtype=np.int64)
    q[:extra] += 1
    assert q.min() >= 0 and q.max() <= 255 and int(q.sum()) - 33 * L == tot
    return q.astype(np.uint8).tobytes()


def _tiles(n, L, length):
    """n subreads of `length` bases spread over a read of L bases (they may overlap: pure slices)"""
    return [((k * 37) % max(1, L - length), (k * 37) % max(1, L - length) + length) for k in range(n)]


def main_group():
    g = Group(seed=11)
    s = [0]

    def sid():                                                    # the splints interleave
        s[0] ^= 1
        return s[0]

    for name, st in ST.items():                                   # every status, with subreads and with none
        g.add("st_" + name, 300, sid(), status=st, subs=[(10, 100), (100, 190), (190, 280)], front=10, tail=280, clen=95)
        g.add("st0_" + name, 300, sid(), status=st, subs=[], front=120, tail=150, clen=40)
    g.add("sid_minus", 200, -1, subs=[(5, 90), (90, 180)], clen=80)
    g.add("sid_high", 200, N_SPLINTS, subs=[(5, 90), (90, 180)], clen=80)
    g.add("ok_no_cons", 200, sid(), subs=[(5, 90), (90, 180)], front=5, clen=0)
    g.add("zero_front_only", 200, sid(), status=ST["no_cons"], front=90)
    g.add("zero_tail_only", 200, sid(), status=ST["no_cons"], tail=90)
    g.add("zero_neither", 200, sid(), status=ST["no_cons"])
    g.add("zero_both_empty", 200, sid(), status=ST["no_cons"], front=0, tail=200)
    g.add("front_only", 250, sid(), subs=_tiles(3, 250, 60), front=17, clen=61)
    g.add("tail_only", 250, sid(), subs=_tiles(3, 250, 60), tail=201, clen=61)
    g.add("both", 250, sid(), subs=_tiles(3, 250, 60), front=17, tail=201, clen=61)
    g.add("neither", 250, sid(), subs=_tiles(3, 250, 60), clen=61)
    for ns in (1, 2, 9, 10, 99, 100, 250):                        # digit counts of the record index
        g.add("ns%d" % ns, 400 + ns, sid(), subs=_tiles(ns, 400 + ns, 11 + ns % 7), front=3, tail=390, clen=50 + ns)
    # subreads of 0 .. 9 bases at every source alignment
    subs = [(40 + 16 * (4 * ln + rep) + sa, 40 + 16 * (4 * ln + rep) + sa + ln) for ln in range(10) for sa in range(4) for rep in range(4)]
    g.add("short_subs_a", 40 + 16 * 44, sid(), subs=subs, front=7, tail=701, clen=33, name=b"a")
    g.add("short_subs_b", 40 + 16 * 44, sid(), subs=subs[::-1], clen=34, name=b"bcd")
    # (four records of one length and source alignment follow each other: with a record length that is odd -- an odd name
    # length for 1- and 3-digit indexes, an even one for 2-digit indexes -- they land on the four destination alignments)
    g.add("short_subs_c", 40 + 16 * 44, sid(), subs=subs, clen=35, name=b"ef")
    g.add("long_40001", 40001, sid(), subs=[(100, 13000), (13000, 26001), (26001, 39000)], front=100, tail=39000, clen=12950)
    g.add("long_33000", 33000, sid(), subs=[(3, 32999)], tail=32999, clen=32000)
    g.add("name_empty", 150, sid(), subs=[(1, 70), (70, 140)], front=1, tail=140, clen=66, name=b"")
    g.add("name_200", 150, sid(), subs=[(1, 70), (70, 140)], front=1, tail=140, clen=66, name=b"N" * 199 + b"x")
    g.add("name_odd", 150, sid(), subs=[(1, 70), (70, 140)], clen=66, name=b"r\xc3\xa9ad\x80\xfe-lower_UPPER")
    for tot, L, _txt in AVGQ_PINS:
        g.add("avgq_%d_%d" % (tot, L), L, sid(), subs=[(0, L)], clen=5 + L % 3, qual=qual_with(tot, L))
    g.add("low_quals", 64, sid(), subs=[(0, 30), (30, 64)], clen=20, qual=bytes(range(64)))
    return g


def empty_group():
    return Group()


def nothing_kept_group():
    g = Group(seed=3)
    for k, st in enumerate((ST["not_assigned"], ST["no_peaks"], ST["too_short"], ST["limit"])):
        g.add("drop%d" % k, 120, k & 1, status=st, subs=[(0, 50), (50, 100)], clen=40)
    g.add("drop_sid", 120, -1, subs=[(0, 50)], clen=40)
    g.add("drop_zero", 120, 1, status=ST["no_cons"], front=30)
    return g


GROUPS = {"main": main_group, "empty": empty_group, "nothing_kept": nothing_kept_group}


def written_files(tmp, hb, res, cons, coff, qv, sid, zero, n_splints=N_SPLINTS):
    """the yardstick: what c3_write_group (and c3_write_consensus_fastq with qv) append to empty files; streams in the order of
    c3_emit_group: per splint consensus FASTA, subread FASTQ[, consensus FASTQ]"""
    K = 3 if qv is not None else 2
    paths = [[os.path.join(str(tmp), "s%d_k%d" % (s, k)) for k in range(K)] for s in range(n_splints)]
    for row in paths:
        for p in row:
            open(p, "wb").close()
    _lib.write_group(hb, res, cons, coff, sid, [r[0] for r in paths], [r[1] for r in paths], zero)
    if qv is not None:
        _lib.write_consensus_fastq(hb, res, cons, coff, qv, sid, [r[2] for r in paths], zero)
    return [open(p, "rb").read() for row in paths for p in row]

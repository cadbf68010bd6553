"""Host statement of the per-base consensus QVs (c3_consensus_qv_host) against a slow pure-Python restatement of the
specification in include/c3poa.h, its properties, and the consensus FASTQ writer (c3_write_consensus_fastq) against
c3_write_group's FASTA records.  CPU only."""
import random

import numpy as np
import pytest

from c3poa_amd import _lib

NEG = -(1 << 40)
CODE = {c: i for i, c in enumerate("ACGT")}
CODE.update({"a": 0, "c": 1, "g": 2, "t": 3, "U": 3, "u": 3})


def code(c):
    return CODE.get(c, 0)


def spec_align(C, P, Q, mode, S, info=None):
    """mode 0 / 1 in the frame given (mode 2 is handled by the caller).  info: a dict that receives what the edge tests assert
    on -- "end" (the end cell), "maxima" (the band cells of largest H, in scan order), "d" (the set of band steps
    lo(i) - lo(i-1)), "edge0" / "edge127" (the path touched band offset 0 with j > 0 / offset 127 with j < n)"""
    n, m = len(C), len(P)
    lo = [((i * n + m // 2) // m if mode == 0 else i) - 64 for i in range(m + 1)]
    H = {}

    def cell(i, j):
        if i < 0 or j < 0 or j > n or not (lo[i] <= j < lo[i] + 128):
            return NEG
        return H[(i, j)]

    for i in range(m + 1):
        for j in range(max(0, lo[i]), min(n, lo[i] + 127) + 1):
            if i == 0 and j == 0:
                H[(i, j)] = 0
                continue
            h = NEG
            if i > 0 and j > 0:
                h = max(h, cell(i - 1, j - 1) + (2 if P[i - 1] == C[j - 1] else -4))
            if j > 0:
                h = max(h, cell(i, j - 1) - 4)
            if i > 0:
                h = max(h, cell(i - 1, j) - 4)
            H[(i, j)] = h
    if mode == 0:
        ei, ej = m, n
    else:
        best = None
        for (i, j), h in sorted(H.items()):
            if best is None or h > best:
                best, ei, ej = h, i, j
    path = []
    i, j = ei, ej
    while i > 0 or j > 0:
        h = cell(i, j)
        if i > 0 and j > 0 and h == cell(i - 1, j - 1) + (2 if P[i - 1] == C[j - 1] else -4):
            path.append(("D", i, j)); i -= 1; j -= 1
        elif j > 0 and h == cell(i, j - 1) - 4:
            path.append(("X", i, j)); j -= 1
        else:
            path.append(("I", i, j)); i -= 1
    if info is not None:
        top = max(H.values())
        info.update(end=(ei, ej), maxima=sorted(k for k, h in H.items() if h == top), d={lo[i] - lo[i - 1] for i in range(1, m + 1)},
                    edge0=any(j - lo[i] == 0 and j > 0 for _k, i, j in path), edge127=any(j - lo[i] == 127 and j < n for _k, i, j in path))
    path.reverse()
    J = n if mode == 0 else ej
    if J == 0:
        return
    run = None
    for kind, i, j in path:
        if kind == "I":
            run = (max(run[0], Q[i - 1]) if run else Q[i - 1], j)
            continue
        if run:
            S[min(run[1], J - 1)] -= run[0]; run = None
        if kind == "D":
            S[j - 1] += Q[i - 1] if P[i - 1] == C[j - 1] else -Q[i - 1]
        else:
            S[j - 1] -= Q[i - 1] if i > 0 else Q[0]
    if run:
        S[min(run[1], J - 1)] -= run[0]


def _info(infos):
    if infos is None:
        return None
    infos.append({})
    return infos[-1]


def spec_qv(cons, pieces, infos=None):
    """infos: a list that receives one spec_align info dict per piece (mode 2: in the reversed frame)"""
    n = len(cons)
    C = [code(c) for c in cons]
    S = [0] * n
    for seq, qual, mode in pieces:
        P = [code(c) for c in seq]
        Q = [min(93, max(0, ord(c) - 33)) for c in qual]
        if mode == 2:
            Sr = [0] * n
            spec_align(C[::-1], P[::-1], Q[::-1], 1, Sr, _info(infos))
            for j in range(n):
                S[j] += Sr[n - 1 - j]
        else:
            spec_align(C, P, Q, mode, S, _info(infos))
    return "".join(chr(33 + min(60, max(0, s))) for s in S)


def rand_seq(rng, n, alpha="ACGT"):
    return "".join(rng.choice(alpha) for _ in range(n))


def mutate(rng, s, rate=0.1):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
        elif r < rate:
            out.append(c); out.append(rng.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out) or "A"


def rand_qual(rng, n):
    return "".join(chr(33 + rng.randrange(0, 60)) for _ in range(n))


def check(cons, pieces):
    assert _lib.consensus_qv_host(cons, pieces) == spec_qv(cons, pieces)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_random_pieces_match_spec(mode):
    rng = random.Random(100 + mode)
    for _ in range(6):
        n = rng.randrange(1, 300)
        cons = rand_seq(rng, n)
        pieces = []
        for _k in range(rng.randrange(1, 4)):
            if mode == 0:
                seq = mutate(rng, cons, 0.15)
                while max(len(seq), n) > 4 * min(len(seq), n):
                    seq = mutate(rng, cons, 0.05)
            else:
                a = rng.randrange(0, n)
                seq = mutate(rng, cons[:a + 1] if mode == 1 else cons[a:], 0.15) + rand_seq(rng, rng.randrange(0, 20))
                if mode == 2:
                    seq = rand_seq(rng, rng.randrange(0, 20)) + seq
            pieces.append((seq, rand_qual(rng, len(seq)), mode))
        check(cons, pieces)


def test_mixed_modes_and_mixed_case():
    rng = random.Random(7)
    cons = rand_seq(rng, 250, "ACGTacgtNU")
    pieces = [(mutate(rng, cons, 0.1), None, 0), (cons[:120], None, 1), (cons[140:], None, 2), (mutate(rng, cons, 0.2), None, 0)]
    pieces = [(s, rand_qual(rng, len(s)), m) for s, _q, m in pieces]
    check(cons, pieces)


def test_adversarial():
    rng = random.Random(11)
    cons = rand_seq(rng, 200)
    q = rand_qual(rng, 400)
    # identical sequences; all mismatches; piece longer than the consensus; slopes 0.8 / 1.25
    check(cons, [(cons, q[:200], 0), (cons, q[:200], 1), (cons, q[:200], 2)])
    mis = "".join("ACGT"[(CODE[c] + 1) % 4] for c in cons)
    check(cons, [(mis, q[:200], 0), (mis, q[:200], 1), (mis, q[:200], 2)])
    longer = mutate(rng, cons, 0.05) + rand_seq(rng, 120)
    check(cons, [(longer, rand_qual(rng, len(longer)), md) for md in (0, 1, 2)])
    for L in (160, 250):
        s = "".join(cons[int(i * 200 / L)] for i in range(L))
        check(cons, [(s, rand_qual(rng, L), md) for md in (0, 1, 2)])
    # an optimum that leaves the band: a 150-base insertion in the middle of a global pair
    ins = cons[:100] + rand_seq(rng, 150) + cons[100:]
    check(cons, [(ins, rand_qual(rng, len(ins)), 0), (ins, rand_qual(rng, len(ins)), 1)])
    # ties at the end cell: a periodic consensus and piece
    per = "AC" * 60
    check(per, [("AC" * 30, "I" * 60, 1), ("CA" * 30, "I" * 60, 2), ("A", "5", 1), ("G", "5", 2)])


def test_single_identical_piece_gives_min_q_60():
    rng = random.Random(3)
    cons = rand_seq(rng, 180)
    qual = "".join(chr(33 + x) for x in [0, 1, 59, 60, 61, 93] * 30)
    qual = qual[:180]
    out = _lib.consensus_qv_host(cons, [(cons, qual, 0)])
    want = "".join(chr(33 + min(60, min(93, max(0, ord(c) - 33)))) for c in qual)
    assert out == want


def test_clamp_and_uncovered_columns():
    rng = random.Random(5)
    cons = rand_seq(rng, 150)
    q = "~" * 150                                   # q = 93 each
    many = [(cons, q, 0)] * 5
    assert _lib.consensus_qv_host(cons, many) == chr(33 + 60) * 150
    assert _lib.consensus_qv_host("A" * 150, [("C" * 150, q, 0)]) == "!" * 150       # every column a mismatch: S < 0
    # a mode-1 piece covering the first 40 columns only: the rest get 0
    out = _lib.consensus_qv_host(cons, [(cons[:40], "5" * 40, 1)])
    assert out[:40] == "5" * 40 and out[40:] == "!" * 110
    out = _lib.consensus_qv_host(cons, [(cons[110:], "5" * 40, 2)])
    assert out[110:] == "5" * 40 and out[:110] == "!" * 110
    assert _lib.consensus_qv_host(cons, []) == "!" * 150


def test_mode2_is_mode1_reversed():
    rng = random.Random(9)
    for _ in range(5):
        cons = rand_seq(rng, rng.randrange(20, 260))
        seq = mutate(rng, cons[rng.randrange(0, len(cons) // 2):], 0.12)
        qual = rand_qual(rng, len(seq))
        fwd = _lib.consensus_qv_host(cons, [(seq, qual, 2)])
        rev = _lib.consensus_qv_host(cons[::-1], [(seq[::-1], qual[::-1], 1)])
        assert fwd == rev[::-1]


def test_refusals():
    ok = ("ACGT", "IIII", 0)
    for cons, pieces, rc in [("", [ok], -3), ("ACGT", [("", "", 0)], -3), ("ACGT", [("ACGT", "IIII", 3)], -3),
                             ("ACGT", [ok] * 253, -6), ("ACGTACGTACGTACGTACGT", [("ACGT", "IIII", 0)], -6),
                             ("ACGT", [("A" * 17, "I" * 17, 0)], -6)]:
        with pytest.raises(_lib.C3Error) as e:
            _lib.consensus_qv_host(cons, pieces)
        assert ("error %d:" % rc) in str(e.value)
    # the skew limit is a mode-0 rule only, and exactly 4x is accepted
    _lib.consensus_qv_host("ACGTACGTACGTACGTACGT", [("ACGT", "IIII", 1), ("ACGTA", "IIIII", 0)])
    _lib.consensus_qv_host("ACGT", [ok] * 252)


# ---- c3_write_consensus_fastq against c3_write_group ----------------------------------------------------------------

def _batch(tmp_path, recs):
    p = tmp_path / "in.fastq"
    with open(p, "w") as fh:
        for name, seq, qual in recs:
            fh.write("@%s\n%s\n+\n%s\n" % (name, seq, qual))
    rd = _lib.Reader(str(p))
    hb = rd.next(1000)
    return rd, hb


def _read_fasta(path):
    lines = open(path).read().split("\n") if path.exists() else []
    return [(lines[k][1:], lines[k + 1]) for k in range(0, len(lines) - 1, 2)]


def _read_fastq(path):
    lines = open(path).read().split("\n") if path.exists() else []
    return [(lines[k][1:], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


@pytest.mark.parametrize("zero", [True, False])
def test_fastq_records_follow_the_fasta_writer(tmp_path, zero):
    rng = random.Random(21 if zero else 22)
    recs = []
    for i in range(12):
        L = rng.randrange(50, 120)
        recs.append(("read%d" % i, rand_seq(rng, L), rand_qual(rng, L)))
    rd, hb = _batch(tmp_path, recs)
    n = hb.n
    res = np.zeros(n, dtype=_lib.RESULT_DTYPE)
    sid = np.array([i % 2 for i in range(n)], dtype=np.int16)
    sid[3] = -1                                         # unassigned
    cons_parts, qv_parts = [], []
    for i in range(n):
        L = len(recs[i][1])
        r = res[i]
        kind = i % 6
        r["status"] = _lib.ST_OK
        r["n_sub"], r["has_front"], r["has_tail"], r["front_end"], r["tail_beg"] = 2, 1, 1, 5, L - 5
        r["sub_beg"][:2] = [5, L // 2]; r["sub_end"][:2] = [L // 2, L - 5]
        if kind == 1:                                   # zero-repeat rescue: emitted only with zero
            r["n_sub"] = 0
        elif kind == 2:                                 # ST_LIMIT: no records
            r["status"] = _lib.ST_LIMIT
        elif kind == 3:                                 # no consensus
            r["status"] = _lib.ST_NO_CONSENSUS
        elif kind == 4:                                 # OK but empty consensus
            pass
        clen = 0 if kind in (2, 3, 4) else rng.randrange(10, 60)
        r["cons_len"] = clen
        cons_parts.append(rand_seq(rng, clen)); qv_parts.append(rand_qual(rng, clen))
    coff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum([len(c) for c in cons_parts], out=coff[1:])
    cbuf = np.frombuffer("".join(cons_parts).encode() + b"\0", dtype=np.uint8)
    qbuf = np.frombuffer("".join(qv_parts).encode() + b"\0", dtype=np.uint8)
    fa = [tmp_path / ("s%d.fasta" % s) for s in range(2)]
    fq = [tmp_path / ("s%d.fastq" % s) for s in range(2)]
    sub = [tmp_path / ("s%d_sub.fastq" % s) for s in range(2)]
    for _rep in range(2):                               # appends, like c3_write_group
        _lib.write_group(hb, res, cbuf, coff, sid, [str(p) for p in fa], [str(p) for p in sub], zero)
        _lib.write_consensus_fastq(hb, res, cbuf, coff, qbuf, sid, [str(p) for p in fq], zero)
    total = 0
    for s in range(2):
        a, q = _read_fasta(fa[s]), _read_fastq(fq[s])
        assert [(h, c) for h, c, _ in q] == a
        for h, c, qq in q:
            assert len(qq) == len(c)
            i = int(h.split("_")[0][4:])
            assert c == cons_parts[i] and qq == qv_parts[i]
        total += len(q)
    want = sum(1 for i in range(n) if sid[i] >= 0 and i % 6 not in (2, 3, 4) and (zero or i % 6 != 1))
    assert total == 2 * want
    rd.close()

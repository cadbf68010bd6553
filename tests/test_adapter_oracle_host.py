"""Independent checker of the adapter finder's oracle (oracle.oracle_py.adapter_align, oracle/c3o_adapter.c), and the proof that
the designed cases of adapter_edge_cases.py reach what they are for.  No GPU.

The checker is written from DESIGN.md 4.9 and the textbook recurrence (Gotoh, local): three matrices H, E, F, match 2,
mismatch -4, a gap of k bases 4 + 2k, rows = read bases, columns = adapter bases (strand 1: the reverse complement of the
adapter).  It has no direction bytes and no traceback and returns the whole H matrix, so it can say what the best score is, which
cells hold it and which of them comes first in row-major order -- and nothing about the path, which is pinned through the
identities that any path's counts must satisfy (adapter_edge_cases.check_fields) and through the designed cases, whose paths
are known by construction (one gap of k bases, one mismatch, none).

Two forms of the checker: gotoh_loops is the recurrence cell by cell in plain Python; gotoh_H runs a row at a time in numpy
(the horizontal gap as a running maximum) and is proved equal to the loops on small pairs before anything relies on it."""
import numpy as np
import pytest

import adapter_edge_cases as AC
from oracle import oracle_py as O

NEG = -10 ** 9
_CODE = np.zeros(256, dtype=np.int64)                       # every byte that is no base counts as A (N included)
for _k, _cs in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _c in _cs:
        _CODE[ord(_c)] = _k


def _codes(read, adapter, rc):
    q = _CODE[np.frombuffer(read.encode(), dtype=np.uint8)]
    r = _CODE[np.frombuffer(adapter.encode(), dtype=np.uint8)]
    return q, (3 - r[::-1] if rc else r)


def gotoh_loops(read, adapter, rc):
    q, r = _codes(read, adapter, rc)
    n, m = len(q), len(r)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    E = [[NEG] * (m + 1) for _ in range(n + 1)]           # best score of a cell whose alignment ends in a gap that consumes a read base
    F = [[NEG] * (m + 1) for _ in range(n + 1)]           # ... an adapter base
    for i in range(1, n + 1):
        for j in range(1, m + 1):
            E[i][j] = max(E[i - 1][j] - AC.GAP_EXT, H[i - 1][j] - AC.GAP_OPEN - AC.GAP_EXT)
            F[i][j] = max(F[i][j - 1] - AC.GAP_EXT, H[i][j - 1] - AC.GAP_OPEN - AC.GAP_EXT)
            s = AC.MATCH if q[i - 1] == r[j - 1] else AC.MISMATCH
            H[i][j] = max(0, H[i - 1][j - 1] + s, E[i][j], F[i][j])
    return np.array(H, dtype=np.int64).reshape(n + 1, m + 1)


def gotoh_H(read, adapter, rc):
    """the same H, one row at a time.  F[i][j] = max over k < j of H[i][k] - 4 - 2 (j - k); a cell that got its value from F adds
    nothing to that maximum (its own source reaches j more cheaply), so the maximum runs over T = max(0, diagonal, E)."""
    q, r = _codes(read, adapter, rc)
    n, m = len(q), len(r)
    H = np.zeros((n + 1, m + 1), dtype=np.int64)
    E = np.full(m + 1, NEG, dtype=np.int64)
    jj = np.arange(m + 1, dtype=np.int64)
    T = np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        E = np.maximum(E - AC.GAP_EXT, H[i - 1] - AC.GAP_OPEN - AC.GAP_EXT)
        T[1:] = np.maximum(np.maximum(H[i - 1, :-1] + np.where(r == q[i - 1], AC.MATCH, AC.MISMATCH), E[1:]), 0)
        run = np.maximum.accumulate(T + AC.GAP_EXT * jj)
        H[i, 1:] = np.maximum(T[1:], run[:-1] - AC.GAP_OPEN - AC.GAP_EXT * jj[1:])
    return H


def first_max(H):
    """(best, row, column) of the first maximum in row-major order"""
    k = int(np.argmax(H))                                    # numpy: the first occurrence in C order
    return int(H.max()), k // H.shape[1], k % H.shape[1]


def assert_row_is_optimum(row, H, m, rc, where):
    best, i, j = first_max(H)
    assert int(row[0]) == best, (where, int(row[0]), best)
    if best == 0:
        return
    assert int(row[2]) == i, (where, "qEnd", int(row[2]), i)
    got = m - int(row[3]) if rc else int(row[4])             # strand 1: columns are mirrored back to the forward strand
    assert got == j, (where, "end column", got, j)


GROUPS = AC.groups()
QUEUE_HOST = AC.queue(128)                                   # the queue batch at a size the checker can walk through
BATCHES = [b for g in ("seams", "hgaps", "vgaps", "ties") for b in GROUPS[g]] + [QUEUE_HOST]
PAIRS = AC.random_pairs(400)


def test_row_checker_equals_cell_by_cell_recurrence():
    n = 0
    for rd, ad in PAIRS:
        if len(rd) * len(ad) <= 2500:
            for rc in (0, 1):
                assert np.array_equal(gotoh_H(rd, ad, rc), gotoh_loops(rd, ad, rc)), (rd, ad, rc)
            n += 1
    b = GROUPS["ties"][0]
    for i, a, s, kind, _d in b.claims:                       # plateaus of equal cells, where the running maximum is all ties
        if kind in ("tie", "zero") and len(b.reads[i]) * len(b.adapters[a]) <= 5000:
            assert np.array_equal(gotoh_H(b.reads[i], b.adapters[a], s), gotoh_loops(b.reads[i], b.adapters[a], s))
            n += 1
    assert n >= 100


@pytest.mark.parametrize("b", BATCHES, ids=lambda b: b.name)
def test_oracle_is_the_first_optimum(b):
    """every (read, adapter, strand) of every batch: score, end cell and field identities"""
    tab = AC.oracle_table(b)
    for i, rd in enumerate(b.reads):
        for a, ad in enumerate(b.adapters):
            for s in (0, 1):
                assert_row_is_optimum(tab[i, a, s], gotoh_H(rd, ad, s), len(ad), s, (b.name, i, a, s))
    AC.check_table(b, tab)


def test_oracle_is_the_first_optimum_random_pairs():
    assert len(PAIRS) >= 300 and max(max(len(r), len(a)) for r, a in PAIRS) <= 150 and min(min(len(r), len(a)) for r, a in PAIRS) == 1
    scored = gapped = 0
    for rd, ad in PAIRS:
        for s in (0, 1):
            row = O.adapter_align(rd, ad, bool(s))
            assert_row_is_optimum(row, gotoh_H(rd, ad, s), len(ad), s, (rd, ad, s))
            AC.check_fields(row, len(rd), len(ad), (rd, ad, s))
            scored += row[0] > 0
            gapped += row[7] > 0 or row[8] > 0
    assert scored >= 400 and gapped >= 100                   # the pairs are no empty exercise


def _mirrored(row, m):
    out = row.copy()
    if row[0] > 0:
        out[3], out[4] = m - row[4], m - row[3]
    return out


@pytest.mark.parametrize("b", BATCHES, ids=lambda b: b.name)
def test_strand_1_is_strand_0_of_the_reverse_complement(b):
    tab = AC.oracle_table(b)
    for a, ad in enumerate(b.adapters):
        assert set(ad) <= set("ACGT")                        # (N is coded as A, whose complement is not N's)
        for i, rd in enumerate(b.reads):
            fwd = O.adapter_align(rd, AC.revcomp(ad), False)
            assert np.array_equal(tab[i, a, 1], _mirrored(fwd, len(ad))), (b.name, i, a)


def test_strand_1_is_strand_0_of_the_reverse_complement_random_pairs():
    for rd, ad in PAIRS:
        assert np.array_equal(O.adapter_align(rd, ad, True), _mirrored(O.adapter_align(rd, AC.revcomp(ad), False), len(ad))), (rd, ad)


# ---- the designed cases reach what they are for ----------------------------------------------------------------------------
def _claims(group, kind):
    return [(b, c) for b in GROUPS[group] for c in b.claims if c[3] == kind]


def _row(b, c):
    i, a, s = c[:3]
    d = dict(zip(AC.FIELDS, (int(v) for v in AC.oracle_table(b)[i, a, s])))
    return d, len(b.reads[i]), len(b.adapters[a])


def test_seam_cases():
    lens = {len(ad) for b in GROUPS["seams"] for ad in b.adapters}
    assert set(AC.SEAM_LENGTHS) <= lens
    exact = _claims("seams", "exact")
    assert {(len(b.adapters[c[1]]), c[2]) for b, c in exact} >= {(m, s) for m in AC.SEAM_LENGTHS for s in (0, 1)}
    for b, c in exact:
        d, L, m = _row(b, c)
        assert (d["score"], d["matches"], d["tStart"], d["tEnd"], d["qStart"], d["qEnd"]) == (2 * m, m, 0, m, 0, m), (b.name, c, d)
    subs = _claims("seams", "sub")
    # every seam column is substituted on both strands in an adapter where it is the last column of a full chunk / the first of
    # a partial one (127 .. 129, 191 .. 193) and deep inside a long adapter (511, 512)
    assert {(c[4], c[2]) for b, c in subs} == {(col, s) for col in AC.SEAM_COLUMNS for s in (0, 1)}
    assert {(len(b.adapters[c[1]]), c[4]) for b, c in subs} >= {(127, 64), (127, 65), (128, 65), (129, 65), (191, 128), (192, 129), (193, 129),
                                                               (512, 64), (512, 65), (512, 128), (512, 129), (511, 129)}
    for b, c in subs:
        d, L, m = _row(b, c)
        assert (d["misMatches"], d["tStart"], d["tEnd"], d["matches"], d["score"]) == (1, 0, m, m - 1, 2 * (m - 1) - 4), (b.name, c, d)
        assert d["qBaseInsert"] == d["tBaseInsert"] == 0
    for b, c in _claims("seams", "substring"):
        d, L, m = _row(b, c)
        assert L < m and (d["score"], d["matches"], d["qStart"], d["qEnd"]) == (2 * L, L, 0, L), (b.name, c, d)
    assert any(hi - lo >= 64 and lo < 64 < hi for b, c in _claims("seams", "substring") for lo, hi in [c[4]])
    empties = _claims("seams", "empty")
    assert len(empties) == 2 * len(GROUPS["seams"])
    for b, c in empties:
        assert b.reads[c[0]] == "" and not AC.oracle_table(b)[c[0]].any()          # all zero, the length included
    for b in GROUPS["seams"]:
        assert {len(r) for r in b.reads} >= set(AC.SHORT_READS)


def test_hgap_cases():
    cl = _claims("hgaps", "hgap")
    for m in (512, 200):
        for s in (0, 1):
            ks = sorted(c[4] for b, c in cl if len(b.adapters[c[1]]) == m and c[2] == s)
            assert ks == sorted(2 * 2 * list(AC.HGAP_KS) + ([80, 80] if m == 512 else [])), (m, s, ks)
    for seam in (64, 128):
        for k in AC.HGAP_KS:                                 # the removed columns contain a column on either side of the seam (k = 1: the last of the chunk)
            first = AC._straddle(seam, k)
            assert first <= seam <= first + k - 1 and (k == 1 or first + k - 1 >= seam + 1)
    assert (121, 80) in AC.hgap_placements(512) and 121 <= 129 and 121 + 80 - 1 >= 192          # chunk 129 .. 192 lies inside the gap
    for b, c in cl:
        d, L, m = _row(b, c)
        k = c[4]
        assert (d["tNumInsert"], d["tBaseInsert"], d["qNumInsert"], d["qBaseInsert"], d["misMatches"]) == (1, k, 0, 0, 0), (b.name, c, d)
        assert (d["tStart"], d["tEnd"], d["qStart"], d["qEnd"], d["score"]) == (0, m, 0, L, 2 * L - 4 - 2 * k) and L == m - k, (b.name, c, d)


def test_vgap_cases():
    cl = _claims("vgaps", "vgap")
    assert sorted({c[4] for b, c in cl}) == sorted(AC.VGAP_KS) and len(cl) == 2 * 2 * 2 * len(AC.VGAP_AFTER) * len(AC.VGAP_KS)
    for b, c in cl:
        d, L, m = _row(b, c)
        k = c[4]
        assert (d["qNumInsert"], d["qBaseInsert"], d["tNumInsert"], d["tBaseInsert"], d["misMatches"]) == (1, k, 0, 0, 0), (b.name, c, d)
        assert (d["tStart"], d["tEnd"], d["qStart"], d["qEnd"], d["score"]) == (0, m, 0, L, 2 * m - 4 - 2 * k) and L == m + k, (b.name, c, d)


def test_tie_cases():
    tb = GROUPS["ties"][0]
    cl = _claims("ties", "tie")
    assert len(cl) >= 12 and {c[2] for b, c in cl} == {0, 1}
    for b, c in cl:
        i, a, s = c[:3]
        H = gotoh_H(b.reads[i], b.adapters[a], s)
        assert H.max() > 0 and int((H == H.max()).sum()) >= 2, (b.name, c)
    xx = _claims("ties", "tie_xx")
    assert sorted(c[2] for b, c in xx) == [0, 1]
    for b, c in xx:
        i, a, s, _k, row = c
        H = gotoh_H(b.reads[i], b.adapters[a], s)
        assert H.max() == 140 and np.argwhere(H == 140).tolist() == [[row, 70], [row, 140]], (c, np.argwhere(H == H.max()).tolist())
        d, L, m = _row(b, c)
        assert (d["score"], d["qEnd"], d["tStart"], d["tEnd"]) == ((140, row, 0, 70) if s == 0 else (140, row, 70, 140)), (c, d)   # the smaller column
    qe = _claims("ties", "qEnd")
    assert len(qe) >= 3
    for b, c in qe:
        d, L, m = _row(b, c)
        assert (d["score"], d["qEnd"], d["matches"]) == (2 * m, c[4], m), (c, d)                 # the earlier row
    zero = _claims("ties", "zero")
    assert len(zero) >= 8
    for b, c in zero:
        i, a, s = c[:3]
        assert gotoh_H(b.reads[i], b.adapters[a], s).max() == 0
        row = AC.oracle_table(b)[i, a, s]
        assert not row[:11].any() and row[11] == len(b.reads[i]) > 0
    assert any(set(r) & set("Nn") and set(r) & set("acgt") for r in tb.reads)
    assert {"AC" * 100, "A" * 64, "A" * 65, "A" * 129, "A" * 130} <= set(tb.reads)
    assert {"A" * 64, "A" * 65, "A" * 129, "A" * 130, "AC" * 40, "CA" * 33} <= set(tb.adapters)


def test_queue_batch():
    for exceed in (128, 1000, 16 * 256):
        b = AC.queue(exceed)
        assert b.n_items() >= 3 * exceed and [len(a) for a in b.adapters] == list(AC.QUEUE_ADAPTER_LENGTHS)
        lens = np.array([len(r) for r in b.reads])
        assert lens.min() >= 20 and lens.max() <= 200
        assert np.median(np.abs(np.diff(lens))) >= 40        # the length jumps from one read to the next
        assert b.reads == AC.queue(exceed).reads             # deterministic
    tab = AC.oracle_table(QUEUE_HOST)
    assert (tab[:, :, :, 0] >= 22).sum() >= 10 and (tab[:, :, :, 0] < 22).sum() >= 10            # planted and unrelated items
    assert (tab[:, :, :, 7] > 0).any() and (tab[:, :, :, 8] > 0).any()


def test_scratch_sizes():
    """the direction bytes of every GPU batch stay far below 1 GiB on a device of up to 304 compute units"""
    cap = 16 * 304
    for b in [b for g in GROUPS.values() for b in g] + [AC.queue(cap)]:
        assert b.scratch_bytes(cap) < (1 << 30), (b, b.scratch_bytes(cap))
        assert max(map(len, b.adapters)) <= AC.SPLINT_MAX
        if max(map(len, b.adapters)) > 200:
            assert max(map(len, b.reads)) <= 700 and b.n_items() <= 600, b

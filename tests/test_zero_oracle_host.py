"""Independent checker of the zero-repeat rescue's oracle (oracle.oracle_py.zero_local = zr_local of oracle/c3o_zero.c), and
the proof that the designed pairs of zero_edge_cases.py reach what they are for.  No GPU.

The checker is written from DESIGN.md 4.7 and the textbook recurrence (Gotoh, local): three matrices H, E, F, match 2,
mismatch -4, a gap of k bases 4 + 2k, rows = d1, columns = d0; the end cell is the first maximum of H in row-major order; the
traceback prefers stop > diagonal > vertical > horizontal and, inside a gap, opening over extending.  It keeps whole matrices
and no direction bytes, and it returns the path, so a claim such as "one horizontal run over columns 63 .. 66" is checked on
the path itself.

Two forms: gotoh_loops is the recurrence cell by cell in plain Python; gotoh_rows runs a row at a time in numpy (the
horizontal gap as a running maximum) and is proved equal to the loops, all three matrices, before anything relies on it."""
import numpy as np
import pytest

import zero_edge_cases as ZC
from oracle import oracle_py as O

NEG = -10 ** 9
GO, GE = ZC.GAP_OPEN, ZC.GAP_EXT
_CODE = np.zeros(256, dtype=np.int64)                       # every byte that is no base counts as A
for _k, _cs in enumerate(("Aa", "Cc", "Gg", "TtUu")):
    for _c in _cs:
        _CODE[ord(_c)] = _k


def _codes(s):
    return _CODE[np.frombuffer(s.encode(), dtype=np.uint8)]


def gotoh_loops(d0, d1):
    r, q = _codes(d0), _codes(d1)
    n0, n1 = len(r), len(q)
    H = [[0] * (n0 + 1) for _ in range(n1 + 1)]
    E = [[NEG] * (n0 + 1) for _ in range(n1 + 1)]          # best score of an alignment that ends in a gap consuming a d1 base (vertical)
    F = [[NEG] * (n0 + 1) for _ in range(n1 + 1)]          # ... a d0 base (horizontal)
    for i in range(1, n1 + 1):
        for j in range(1, n0 + 1):
            E[i][j] = max(E[i - 1][j] - GE, H[i - 1][j] - GO - GE)
            F[i][j] = max(F[i][j - 1] - GE, H[i][j - 1] - GO - GE)
            s = ZC.MATCH if q[i - 1] == r[j - 1] else ZC.MISMATCH
            H[i][j] = max(0, H[i - 1][j - 1] + s, E[i][j], F[i][j])
    return tuple(np.array(M, dtype=np.int64).reshape(n1 + 1, n0 + 1) for M in (H, E, F))


def gotoh_rows(d0, d1):
    """the same three matrices, one row at a time.  F[i][j] = max over k < j of H[i][k] - 4 - 2 (j - k); a cell that got its value
    from F adds nothing to that maximum (its own source reaches j more cheaply), so the maximum runs over T = max(0, diagonal, E)."""
    r, q = _codes(d0), _codes(d1)
    n0, n1 = len(r), len(q)
    H = np.zeros((n1 + 1, n0 + 1), dtype=np.int64)
    E = np.full((n1 + 1, n0 + 1), NEG, dtype=np.int64)
    F = np.full((n1 + 1, n0 + 1), NEG, dtype=np.int64)
    jj = np.arange(n0 + 1, dtype=np.int64)
    T = np.zeros(n0 + 1, dtype=np.int64)
    for i in range(1, n1 + 1):
        E[i, 1:] = np.maximum(E[i - 1, 1:] - GE, H[i - 1, 1:] - GO - GE)
        T[1:] = np.maximum(np.maximum(H[i - 1, :-1] + np.where(r == q[i - 1], ZC.MATCH, ZC.MISMATCH), E[i, 1:]), 0)
        run = np.maximum.accumulate(T + GE * jj)
        F[i, 1:] = run[:-1] - GO - GE * jj[1:]
        H[i, 1:] = np.maximum(T[1:], F[i, 1:])
    return H, E, F


class Aln:
    """score, end cell, start cell and path of the alignment of DESIGN.md 4.7 on the matrices of either form"""

    def __init__(self, d0, d1, mats):
        H, E, F = self.H, self.E, self.F = mats
        r, q = _codes(d0), _codes(d1)
        k = int(np.argmax(H))                                # numpy: the first occurrence in C order = first in row-major order
        self.score = int(H.max())
        i, j = k // H.shape[1], k % H.shape[1]
        self.q_en, self.r_en = (i, j) if self.score > 0 else (0, 0)
        ops, st = [], "H"
        while self.score > 0:
            if st == "H":
                if H[i, j] == 0:                             # stop first (the border cells are 0 as well)
                    break
                s = ZC.MATCH if q[i - 1] == r[j - 1] else ZC.MISMATCH
                if H[i, j] == H[i - 1, j - 1] + s:
                    ops.append(("M" if s > 0 else "X", i, j)); i -= 1; j -= 1
                elif H[i, j] == E[i, j]:
                    st = "E"
                else:
                    assert H[i, j] == F[i, j]
                    st = "F"
            elif st == "E":                                  # consumes row i, stays in column j; opening preferred
                ops.append(("V", i, j))
                st = "H" if E[i, j] == H[i - 1, j] - GO - GE else "E"
                assert st == "H" or E[i, j] == E[i - 1, j] - GE
                i -= 1
            else:                                            # consumes column j, stays in row i
                ops.append(("H", i, j))
                st = "H" if F[i, j] == H[i, j - 1] - GO - GE else "F"
                assert st == "H" or F[i, j] == F[i, j - 1] - GE
                j -= 1
        self.q_st, self.r_st = (i, j) if self.score > 0 else (0, 0)
        self.ops = ops[::-1]

    def result(self):
        return (self.score, self.r_st, self.r_en, self.q_st, self.q_en)


LOOP_CELLS = 160000         # pairs up to 400 x 400 cells also go through the cell-by-cell form


def reference(d0, d1):
    a = Aln(d0, d1, gotoh_rows(d0, d1))
    if len(d0) * len(d1) <= LOOP_CELLS:
        b = Aln(d0, d1, gotoh_loops(d0, d1))
        assert a.result() == b.result() and a.ops == b.ops
    return a


def check_claim(kind, detail, a, where):
    cols = lambda kinds: [j for op, i, j in a.ops if op in kinds]
    rows = lambda kinds: [i for op, i, j in a.ops if op in kinds]
    if kind == "coords":
        assert (a.r_st, a.r_en, a.q_st, a.q_en) == tuple(detail), (where, a.result())
    elif kind == "score":
        assert a.score == detail, (where, a.score)
    elif kind == "accepted":
        assert a.score >= ZC.MIN_SCORE and a.r_en > a.r_st and a.q_en > a.q_st, (where, a.result())
    elif kind == "refused":
        assert a.score < ZC.MIN_SCORE, (where, a.score)
    elif kind == "diag_cols":
        assert set(range(detail[0], detail[1] + 1)) <= set(cols("MX")), (where, a.result())
    elif kind == "diag_rows":
        assert set(range(detail[0], detail[1] + 1)) <= set(rows("MX")), (where, a.result())
    elif kind == "sub_col":
        assert [j for op, i, j in a.ops if op == "X"] == [detail] and not cols("VH"), (where, a.ops)
    elif kind == "hrun":
        assert cols("H") == list(range(detail[0], detail[1] + 1)) and len(set(rows("H"))) == 1 and not cols("VX"), (where, a.ops)
    elif kind == "vrun":
        c, lo, hi = detail
        assert rows("V") == list(range(lo, hi + 1)) and set(cols("V")) == {c} and not cols("HX"), (where, a.ops)
    elif kind == "maxima":
        assert [tuple(v) for v in np.argwhere(a.H == a.H.max()).tolist()] == sorted(detail), (where, np.argwhere(a.H == a.H.max()).tolist())
        assert (a.q_en, a.r_en) == tuple(sorted(detail)[0]), where
    elif kind == "rival":
        i, j, sc = detail
        assert a.H[i, j] == sc == a.score - 2 and i < a.q_en, (where, int(a.H[i, j]), a.result())
    else:
        raise AssertionError("unknown claim %r" % (kind,))


GROUPS = ZC.groups()
ALL = [c for g in GROUPS.values() for c in g]
_refs = {}


def ref_of(c):
    """the reference alignment of a case: computed once, shared by the tests below"""
    if (c.group, c.name) not in _refs:
        _refs[(c.group, c.name)] = reference(c.d0, c.d1)
    return _refs[(c.group, c.name)]


def test_row_form_equals_cell_by_cell_recurrence():
    n = 0
    for d0, d1 in ZC.random_pairs(120, seed=12):
        if len(d0) * len(d1) <= 6000:
            for A, B in zip(gotoh_rows(d0, d1), gotoh_loops(d0, d1)):
                assert np.array_equal(np.maximum(A, NEG // 2), np.maximum(B, NEG // 2)), (d0, d1)      # (never-reachable cells: any very negative value)
            n += 1
    for d0, d1 in (("A" * 70, "A" * 66), ("AC" * 40, "CA" * 33), ("G" * 30, "A" * 30)):              # plateaus: the running maximum is all ties
        for A, B in zip(gotoh_rows(d0, d1), gotoh_loops(d0, d1)):
            assert np.array_equal(np.maximum(A, NEG // 2), np.maximum(B, NEG // 2))
        n += 1
    assert n >= 40


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_oracle_equals_reference_on_designed_pairs(group):
    """score, end cell and start cell, on every designed pair and on its twin"""
    looped = 0
    for c in GROUPS[group]:
        a = ref_of(c)
        assert O.zero_local(c.d0, c.d1) == a.result(), (c, a.result())
        looped += len(c.d0) * len(c.d1) <= LOOP_CELLS
        t0, t1 = c.twin
        assert O.zero_local(t0, t1) == reference(t0, t1).result(), (c, "twin")
    if group in ("seams64", "threshold"):
        assert looped >= len(GROUPS[group]) // 2             # the small groups also went through the cell-by-cell form


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_claims_hold_on_the_reference_path(group):
    for c in GROUPS[group]:
        assert c.claims, c
        a = ref_of(c)
        for kind, detail in c.claims:
            check_claim(kind, detail, a, c)
        assert set(c.d0 + c.d1) <= set("ACGT")
        assert c.long_only == (group in ZC.LONG_GROUPS)


def test_oracle_equals_reference_on_random_pairs():
    pairs = ZC.random_pairs(300)
    assert min(min(len(a), len(b)) for a, b in pairs) <= 3 and max(max(len(a), len(b)) for a, b in pairs) >= 200
    accepted = gapped = tied = 0
    for d0, d1 in pairs:
        a = reference(d0, d1)
        assert O.zero_local(d0, d1) == a.result(), (d0, d1, a.result())
        accepted += a.score >= ZC.MIN_SCORE
        gapped += any(op in "VH" for op, i, j in a.ops)
        tied += int((a.H == a.H.max()).sum()) > 1 and a.score > 0
    assert accepted >= 60 and gapped >= 60 and tied >= 30    # the pairs are no empty exercise


def test_oracle_zero_repeats_uses_these_coordinates():
    """c3o_zero_repeats = left + overlap consensus + right around zero_local's coordinates: with an exact overlap the result is
    d1[:q_en] + d0[r_en:], and a refused pair gives nothing"""
    for c in GROUPS["seams64"][:12] + GROUPS["threshold"] + GROUPS["limits"]:
        if any(k == "sub_col" for k, _d in c.claims):
            continue
        a = ref_of(c)
        exp = c.d1[:a.q_en] + c.d0[a.r_en:] if a.score >= ZC.MIN_SCORE else ""
        if not any(op == "X" for op, i, j in a.ops):
            assert O.zero_repeats(*c.pair()) == exp, c


def test_seam_coverage():
    g = GROUPS["seams64"]
    assert {len(c.d0) for c in g} >= set(ZC.SEAM_N0)
    for n0 in ZC.SEAM_N0:                                     # every n0 has an overlap that ends in its last column
        assert any(len(c.d0) == n0 and ref_of(c).r_en == n0 for c in g), n0
    ends = {ref_of(c).r_en for c in g}
    assert {64, 128, 192} <= ends
    assert {ref_of(c).r_st for c in g} >= {64, 128}           # an overlap that starts in column 65 / 129
    subs = sorted(d for c in g for k, d in c.claims if k == "sub_col")
    assert subs == [64, 65, 128, 129]
    through = {d for c in g for k, d in c.claims if k == "diag_cols"}
    assert {(64, 65), (128, 129), (192, 193)} <= through


def test_gap_coverage():
    runs = {d for c in GROUPS["hgaps"] for k, d in c.claims if k == "hrun"}
    for seam in (64, 128):
        got = sorted(b - a + 1 for a, b in runs if a <= seam and b >= seam + 1 and b - a < 10)
        assert got == [2, 3, 4, 5, 6], (seam, got)
    assert (121, 200) in runs and (60, 99) in runs           # over all of chunk 129 .. 192; out of chunk 0 into chunk 1
    # no gap from chunk 0 to chunk 2 can lie on a path: what chunk 0 can have collected does not pay for 64 columns
    assert ZC.MATCH * 64 < ZC.gap_cost(64)
    runs = {d for c in GROUPS["hgaps_long"] for k, d in c.claims if k == "hrun"}
    for seam in (8, 72, 512, 2048):
        assert any(a <= seam and b >= seam + 1 for a, b in runs), seam
    assert any(a <= 1025 and b >= 1536 for a, b in runs)     # a whole stripe inside the gap
    for g in ("hgaps", "hgaps_long"):                         # ... once more with a rival 2 points behind
        assert sum(any(k == "rival" for k, _d in c.claims) for c in GROUPS[g]) == 1
    n0s = [len(c.d0) for c in GROUPS["hgaps_long"]]
    assert 2600 <= max(n0s) <= 2700 and sum(2048 < n < 2560 for n in n0s) >= 2          # a partial second sweep with one live wave
    vr = {d for g in ("vgaps", "vgaps_long") for c in GROUPS[g] for k, d in c.claims if k == "vrun"}
    assert {c for c, lo, hi in vr} >= {64, 65, 512, 513, 2048, 2049}
    assert all(2 <= hi - lo + 1 <= 6 for c, lo, hi in vr)
    assert sum(lo <= 256 and hi >= 257 for c, lo, hi in vr) >= 3
    assert {len(c.d1) for c in GROUPS["vgaps_long"]} >= {255, 256, 257, 512, 513, 175}
    assert sum(("diag_rows", (256, 257)) in c.claims for c in GROUPS["vgaps_long"]) >= 3


def test_tie_coverage():
    """every tie case has at least two cells with the best score, the planted ones and no others: no flank outscores or equals
    the copies (the maxima claim), and the runner-up outside the planted end cells stays below them"""
    names = {c.name for c in GROUPS["ties"]}
    assert {"earlier_row_later_column", "one_row_columns_j_j64", "one_row_other_stripe", "three_by_three"} <= names
    for c in GROUPS["ties"]:
        a = ref_of(c)
        mx = dict(c.claims)["maxima"]
        assert len(mx) >= 2 and a.score == 110
        H = a.H.copy()
        for i, j in mx:
            H[i, j] = 0
        assert H.max() == 108, (c, H.max())                   # the cell before a copy's end; nothing else comes close
    c = {c.name: c for c in GROUPS["ties"]}["earlier_row_later_column"]
    (i0, j0), (i1, j1) = sorted(dict(c.claims)["maxima"])
    assert i0 < i1 and j0 > j1 and (j0 - 1) % 64 != (j1 - 1) % 64
    c = {c.name: c for c in GROUPS["ties"]}["one_row_columns_j_j64"]
    (i0, j0), (i1, j1) = sorted(dict(c.claims)["maxima"])
    assert i0 == i1 and j1 == j0 + 64
    c = {c.name: c for c in GROUPS["ties"]}["one_row_other_stripe"]
    (i0, j0), (i1, j1) = sorted(dict(c.claims)["maxima"])
    assert i0 == i1 and (j0 - 1) // ZC.ZL_STRIPE != (j1 - 1) // ZC.ZL_STRIPE and (j1 - j0) % 64 == 0
    c = {c.name: c for c in GROUPS["ties"]}["one_row_other_sweep"]
    (i0, j0), (i1, j1) = sorted(dict(c.claims)["maxima"])
    wave = lambda j: (j - 1) % ZC.ZL_SWEEP // ZC.ZL_STRIPE
    assert i0 == i1 and j0 <= ZC.ZL_SWEEP < j1 and wave(j0) > wave(j1)
    c = {c.name: c for c in GROUPS["ties"]}["earlier_row_next_sweep_same_lane"]
    (i0, j0), (i1, j1) = sorted(dict(c.claims)["maxima"])
    assert i0 < i1 and j0 == j1 + ZC.ZL_SWEEP


def test_threshold_and_limit_coverage():
    sc = sorted(dict(c.claims)["score"] for c in GROUPS["threshold"])
    assert sc == [76, 76, 78, 78, 78, 80, 80, 80]
    lens = {(len(c.d0), len(c.d1)) for c in GROUPS["limits"]}
    assert lens == {(4096, 120), (4097, 120), (1, 100), (100, 1)}
    for c in GROUPS["limits"][:2]:
        assert ref_of(c).r_en == len(c.d0)


# Removing the designed edit changes the coordinates (r_st, r_en, q_st, q_en) in: seams64 37 of 41 (the four substitutions
# change the score alone), hgaps 13 of 13, vgaps 10 of 10, ties 7 of 7, threshold 8 of 8, limits 4 of 4, hgaps_long 11 of 11,
# vgaps_long 18 of 18.
EFFECT = {"seams64": (37, 41), "hgaps": (13, 13), "vgaps": (10, 10), "ties": (7, 7), "threshold": (8, 8), "limits": (4, 4),
          "hgaps_long": (11, 11), "vgaps_long": (18, 18)}


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_minimum_effect_of_the_designed_edit(group):
    """no case without a twin; in at least 9 of 10 cases of a group the twin has other coordinates (and in all another result)"""
    changed = 0
    for c in GROUPS[group]:
        assert c.twin is not None and c.twin != (c.d0, c.d1), c
        a, t = O.zero_local(c.d0, c.d1), O.zero_local(*c.twin)
        assert a != t, c
        changed += a[1:] != t[1:]
    print("%s: the coordinates change in %d of %d cases" % (group, changed, len(GROUPS[group])))
    assert 10 * changed >= 9 * len(GROUPS[group]), (group, changed, len(GROUPS[group]))
    assert (changed, len(GROUPS[group])) == EFFECT[group]


def _zl_total(n0, n1, K):
    """c3_zl_layout(n0, n1, K).total (c3_args.h)"""
    dirs = (n1 + K - 1) // K * (n0 + 1) * 8
    car = (dirs + min(n1, K) * (n0 + 1) + 15) & ~15
    return (car + n1 * 12 + 255) & ~255


def test_queue_builder():
    from c3poa_amd import synth
    reads, strands = ZC.queue(60)
    assert (reads, strands) == ZC.queue(60) and set(strands) == {"+", "-"}
    ores, ocons = O.process_batch(synth.SPLINT1, reads, strands, threads=4)
    cand = [o for o, r in zip(ores, reads) if o.n_sub == 0 and o.has_front and o.has_tail and o.front_end > 0 and o.tail_beg < len(r[0])]
    assert len(cand) >= 54, len(cand)                         # nearly every read is a zero-repeat candidate ...
    assert 30 <= sum(o.status == 0 for o in cand) <= 44       # ... about two thirds of them with an overlap that is found
    assert 14 <= sum(o.status == 3 for o in cand)
    pieces = [(o.front_end, len(r[0]) - o.tail_beg) for o, r in zip(ores, reads)]
    assert max(max(p) for p in pieces) <= 1000
    # forced to k_zero_long with K = 1, 640 such reads do not get a slot each on any device of up to 304 compute units
    smax = max(_zl_total(f, t, 1) for f, t in pieces if f > 0 and t > 0)
    assert min(2 * 304, ZC.ZL_BUDGET // smax) < 600

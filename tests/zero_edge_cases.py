"""Case builders shared by the zero-repeat rescue edge tests (CPU: test_zero_oracle_host.py, GPU: test_gpu_zero_edges.py).
A plain module, no fixtures: everything is a pure, seeded function of its arguments, so both files see the same inputs.

A case is one pair of dangling pieces (d0, q0, d1, q1) -- d0 = the columns, d1 = the rows of the overlap alignment of DESIGN.md
4.7 -- plus *claims*: (kind, detail) tuples that state, as a property of the alignment path, which mechanism of k_zero /
k_zero_long the pair was built for.  The host test asserts every claim on the path of an independent reference, so a builder
cannot silently stop reaching the code it is for; the GPU test compares consensus and coordinates with the oracle.

How a pair is made: d0 = flank + segment + flank, d1 = flank + segment' + flank, where segment' is the segment with one
designed edit.  The flanks of d0 are random over two letters and the flanks of d1 random over the other two, so no flank base
of d0 ever matches a flank base of d1: the alignment cannot grow past the segment, and its coordinates are known exactly.
Every case also carries its *twin*, the same pair without the designed edit (the gap closed, the substitution undone; for a
placement case -- "the overlap ends at column 64" -- the overlap taken out; for a tie the winning copy taken out).

Columns and rows are DP indices, 1-based: column j is d0[j - 1], row i is d1[i - 1].
  k_zero       64 columns per pass of the wave: seams 64 | 65, 128 | 129, ...
  k_zero_long  8 columns per lane (8 | 9, ...), 512 per wave (512 | 513, ...: LDS ring), 2048 per sweep (2048 | 2049: the per-row
               carry array); checkpoint rows every K (default 256), the traceback recomputes one block of K rows at a time

Claim kinds (checked by test_zero_oracle_host.check_claim):
  coords (r_st, r_en, q_st, q_en)   score s            accepted / refused (s against the threshold 80)
  diag_cols (a, b) / diag_rows (a, b)   every column / row a .. b is consumed by a diagonal step
  sub_col c                             the diagonal step that consumes column c is a mismatch
  hrun (a, b)                           the path's only horizontal run consumes exactly columns a .. b
  vrun (c, a, b)                        the path's only vertical run consumes exactly rows a .. b, in column c
  maxima [(i, j), ...]                  exactly these cells hold the best score; the first of them is the end cell
  rival (i, j, s)                       cell (i, j), in a row above the end cell, holds s = the best score - 2
"""
import numpy as np

MATCH, MISMATCH, GAP_OPEN, GAP_EXT, MIN_SCORE = 2, -4, 4, 2, 80    # DESIGN.md 4.7 (c3_host.h: fixed)
ZW = 4096                   # k_zero: columns of its LDS rows; wider pairs go to k_zero_long
CHUNK = 64                  # k_zero: columns per pass
ZL_C, ZL_STRIPE, ZL_SWEEP, ZL_K = 8, 512, 2048, 256
ZERO_GRID_CAP = 512         # c3_stages.hip run_zero: k_zero runs min(reads, 512) workgroups
ZL_BUDGET = 1 << 30         # c3_stages.hip: k_zero_long scratch of all slots together


def rand_seq(rng, n, letters="ACGT"):
    return "".join(letters[i] for i in rng.integers(0, len(letters), n))


def other_base(c, step=1):
    return "ACGT"[("ACGT".index(c) + step) % 4]


def rand_qual(rng, n):
    return "".join(chr(33 + int(v)) for v in rng.integers(3, 41, n))


def gap_cost(g):
    return GAP_OPEN + GAP_EXT * g


class Case:
    def __init__(self, group, name, d0, d1, claims, twin, long_only=False):
        self.group, self.name, self.d0, self.d1, self.claims, self.twin, self.long_only = group, name, d0, d1, list(claims), twin, long_only
        rng = np.random.default_rng([53, 9, len(d0), len(d1)])
        self.q0, self.q1 = rand_qual(rng, len(d0)), rand_qual(rng, len(d1))

    def pair(self):
        return self.d0, self.q0, self.d1, self.q1

    def __repr__(self):
        return "Case(%s/%s %d x %d)" % (self.group, self.name, len(self.d0), len(self.d1))


class _Lay:
    """lays segments into flanks: d0 over one pair of letters, d1 over the other pair"""

    def __init__(self, rng):
        self.rng = rng
        p = [int(v) for v in rng.permutation(4)]
        self.a0 = "ACGT"[p[0]] + "ACGT"[p[1]]
        self.a1 = "ACGT"[p[2]] + "ACGT"[p[3]]

    def f0(self, n):
        return rand_seq(self.rng, n, self.a0)

    def f1(self, n):
        return rand_seq(self.rng, n, self.a1)

    def d0(self, n0, *placed):
        """n0 bases; placed = (first column, segment), in column order; flank everywhere else"""
        return _fill(n0, placed, self.f0)

    def d1(self, n1, *placed):
        return _fill(n1, placed, self.f1)


def _fill(n, placed, flank):
    out, at = [], 1
    for first, seg in placed:
        assert first >= at, (first, at)
        out.append(flank(first - at)); out.append(seg)
        at = first + len(seg)
    assert n >= at - 1, (n, at)
    out.append(flank(n - (at - 1)))
    s = "".join(out)
    assert len(s) == n
    return s


def _exact(group, name, rng, n0, n1, col, row, m, extra=(), long_only=False):
    """an exact m-mer overlap at columns col .. col + m - 1 and rows row .. row + m - 1; twin: no overlap"""
    L = _Lay(rng)
    x = rand_seq(rng, m)
    d0, d1 = L.d0(n0, (col, x)), L.d1(n1, (row, x))
    claims = [("coords", (col - 1, col - 1 + m, row - 1, row - 1 + m)), ("score", MATCH * m), ("accepted", None)] + list(extra)
    return Case(group, name, d0, d1, claims, (d0, L.d1(n1)), long_only)


# ---- seams of k_zero's 64-column chunks --------------------------------------------------------------------------------------
SEAM_N0 = (63, 64, 65, 127, 128, 129, 191, 192, 193)
SEAMS = (64, 128, 192)


def seams64():
    out = []
    M = 45
    for k, n0 in enumerate(SEAM_N0):
        rng = np.random.default_rng([53, 1, k])

        def rows():
            row = int(rng.integers(2, 25))
            return row, row + M - 1 + int(rng.integers(0, 20))

        row, n1 = rows()
        out.append(_exact("seams64", "n0_%d_ends_in_last_column" % n0, rng, n0, n1, n0 - M + 1, row, M))
        for s in SEAMS:
            if s < n0:                                    # ends in the last column of a full chunk, more columns follow
                row, n1 = rows()
                out.append(_exact("seams64", "n0_%d_ends_at_%d" % (n0, s), rng, n0, n1, s - M + 1, row, M))
            if s + 1 <= n0:                               # runs through the seam
                row, n1 = rows()
                hi = min(n0, s + 22)
                lo = min(s - 22, hi - M + 1)
                out.append(_exact("seams64", "n0_%d_through_%d" % (n0, s), rng, n0, n1 + 5, lo, row, hi - lo + 1, [("diag_cols", (s, s + 1))]))
        if n0 in (127, 129, 193):                         # the overlap starts in the first column of a chunk
            row, n1 = rows()
            out.append(_exact("seams64", "n0_%d_starts_at_65" % n0, rng, n0, n1, 65, row, M, [("diag_cols", (65, 66))]))
        if n0 == 193:
            row, n1 = rows()
            out.append(_exact("seams64", "n0_193_starts_at_129", rng, n0, n1, 129, row, M))
    # one substitution in the last column of a chunk and one in the first column of the next
    for k, (n0, c) in enumerate(((129, 64), (129, 65), (193, 128), (193, 129))):
        rng = np.random.default_rng([53, 1, 100 + k])
        L = _Lay(rng)
        lo, hi = c - 34, min(n0, c + 35)
        assert min(c - lo, hi - c) >= 20
        x = rand_seq(rng, hi - lo + 1)
        y = x[:c - lo] + other_base(x[c - lo], 1 + k % 3) + x[c - lo + 1:]
        row = 7 + k
        n1 = row + len(x) + 3
        d0 = L.d0(n0, (lo, x))
        out.append(Case("seams64", "n0_%d_sub_at_%d" % (n0, c), d0, L.d1(n1, (row, y)),
                        [("sub_col", c), ("coords", (lo - 1, hi, row - 1, row - 1 + len(x))), ("score", MATCH * (len(x) - 1) + MISMATCH)],
                        (d0, L.d1(n1, (row, x)))))
    return out


# ---- horizontal gaps: d1 lacks g bases of d0 ---------------------------------------------------------------------------------
def _straddle(seam, g):
    """first of g columns placed around the seam between columns seam | seam + 1"""
    return seam + 1 - (g + 1) // 2


def _hgap(group, name, rng, first, g, la, lb, right, row, long_only=False, rival=False):
    """segment A (la bases) | G (g bases, columns first .. first + g - 1) | B (lb bases) in d0, A | B in d1.
    rival: an unrelated exact overlap that scores 2 less than A | gap | B and ends in an earlier row (right of B in d0, above A in
    d1).  A carry that loses the gap's true source still finds the same path a few points cheaper -- the rows above smear the
    source over the columns in between -- and only the rival, which then wins, shows it."""
    assert MATCH * min(la, lb) >= gap_cost(g) + 20 or (group, name) == ("hgaps_long", "lane_8_9_g2"), (name, la, lb, g)
    L = _Lay(rng)
    a, b = rand_seq(rng, la), rand_seq(rng, lb)
    G = list(rand_seq(rng, g))
    # the gap cannot slide: its first base differs from B's first (no shift to the right), its last from A's last (none to the left)
    if G[0] == b[0]:
        G[0] = other_base(G[0])
    if G[-1] == a[-1]:
        G[-1] = other_base(G[-1], 2 if g == 1 or other_base(G[-1]) == b[0] else 1)
    if g > 1 and G[0] == b[0]:
        G[0] = other_base(G[0])
    G = "".join(G)
    assert G[0] != b[0] and G[-1] != a[-1]
    col = first - la
    assert col >= 1
    score = MATCH * (la + lb) - gap_cost(g)
    n0 = first + g + lb - 1 + right
    p0, p1, claims = [(col, a + G + b)], [], []
    if rival:
        y = rand_seq(rng, (score - 2) // MATCH)
        assert right >= 5 and MATCH * len(y) == score - 2
        p0.append((n0 + 1, y)); p1.append((1, y))
        claims.append(("rival", (len(y), n0 + len(y), score - 2)))
        n0 += len(y) + int(rng.integers(0, 9))
        row += len(y) + 5
    n1 = row - 1 + la + lb + int(rng.integers(0, 12))
    d0 = L.d0(n0, *p0)
    claims += [("hrun", (first, first + g - 1)), ("coords", (col - 1, first + g + lb - 1, row - 1, row - 1 + la + lb)), ("score", score)]
    return Case(group, name, d0, L.d1(n1, *(p1 + [(row, a + b)])), claims, (d0, L.d1(n1 + g, *(p1 + [(row, a + G + b)]))), long_only)


def hgaps():
    out = []
    for k, (seam, g) in enumerate([(s, g) for s in (64, 128) for g in (2, 3, 4, 5, 6)]):
        rng = np.random.default_rng([53, 2, k])
        first = _straddle(seam, g)
        assert first <= seam and first + g - 1 >= seam + 1
        out.append(_hgap("hgaps", "astride_%d_g%d" % (seam, g), rng, first, g, 45, 45, int(rng.integers(0, 30)), 3 + k))
    # A gap that opens in chunk 0 (columns <= 64) cannot close in chunk 2 (>= 129): it would be at least 64 columns long and
    # cost 4 + 2 * 64 = 132, more than the 2 * 64 a path can have collected in chunk 0, so no path takes it.  The longest gaps that
    # can lie on a path: out of chunk 0 deep into chunk 1 (carry_f, one seam), and out of chunk 1 over all of chunk 2 into
    # chunk 3 (carry_f accumulated over a chunk that adds nothing to it)
    rng = np.random.default_rng([53, 2, 50])
    out.append(_hgap("hgaps", "chunk0_into_chunk1_g40", rng, 60, 40, 59, 60, 9, 1))
    out.append(_hgap("hgaps", "chunk1_over_chunk2_g80", rng, 121, 80, 110, 110, 14, 5))
    out.append(_hgap("hgaps", "chunk1_over_chunk2_g70_rival", rng, 125, 70, 100, 100, 8, 1, rival=True))
    return out


def hgaps_long():
    """the same for k_zero_long: lane seams, the stripe seam 512 | 513, the sweep seam 2048 | 2049 (n0 <= 2700: the second sweep
    is partial, only wave 0 is live in it), a gap over a whole stripe"""
    out = []
    rng = np.random.default_rng([53, 3, 0])
    # columns 8 and 9: only 7 columns lie left of the gap, the margin is 2 * 7 - 8 = 6 (the claim is checked on the path all the same)
    out.append(_hgap("hgaps_long", "lane_8_9_g2", rng, 8, 2, 7, 60, 20, 4, True))
    for k, (seam, g) in enumerate([(72, 2), (72, 5), (512, 2), (512, 4), (512, 6), (2048, 2), (2048, 4), (2048, 6)]):
        rng = np.random.default_rng([53, 3, 1 + k])
        right = (int(rng.integers(0, 30)) if seam < 2048 else (10, 300, 2700 - 2048 - 3 - 45)[k - 5])
        out.append(_hgap("hgaps_long", "astride_%d_g%d" % (seam, g), rng, _straddle(seam, g), g, 45, 45, right, 2 + 3 * k, True))
    # A gap over all of stripe 513 .. 1024 would cost more than the 2 * 512 collected left of it; the first stripe a gap can pass
    # over is 1025 .. 1536: columns 1020 .. 1540, through the ring from wave 1 to wave 3, and the path goes on over 2048 | 2049
    rng = np.random.default_rng([53, 3, 20])
    out.append(_hgap("hgaps_long", "over_stripe_1025_1536_g521", rng, 1020, 521, 540, 540, 25, 6, True))
    rng = np.random.default_rng([53, 3, 21])
    out.append(_hgap("hgaps_long", "over_stripe_1025_1536_g521_rival", rng, 1020, 521, 540, 540, 25, 1, True, rival=True))
    return out


# ---- vertical gaps: d1 has g bases more than d0 ------------------------------------------------------------------------------
def _vgap(group, name, rng, col_end, row, g, la, lb, right, long_only=False, n1=None):
    """segment A (la bases, its last in column col_end) | B in d0; A | X (g bases, rows row + la .. row + la + g - 1) | B in d1"""
    assert MATCH * min(la, lb) >= gap_cost(g) + 20
    L = _Lay(rng)
    a, b = rand_seq(rng, la), rand_seq(rng, lb)
    X = list(rand_seq(rng, g))
    if X[0] == b[0]:
        X[0] = other_base(X[0])
    if X[-1] == a[-1]:
        X[-1] = other_base(X[-1], 2 if g == 1 or other_base(X[-1]) == b[0] else 1)
    if g > 1 and X[0] == b[0]:
        X[0] = other_base(X[0])
    X = "".join(X)
    assert X[0] != b[0] and X[-1] != a[-1]
    col = col_end - la + 1
    assert col >= 1
    n0 = col_end + lb + right
    need = row - 1 + la + g + lb
    n1 = need + int(rng.integers(0, 12)) if n1 is None else n1
    assert n1 >= need
    d1 = L.d1(n1, (row, a + X + b))
    claims = [("vrun", (col_end, row + la, row + la + g - 1)), ("coords", (col - 1, col_end + lb, row - 1, need)),
              ("score", MATCH * (la + lb) - gap_cost(g))]
    return Case(group, name, L.d0(n0, (col, a + b)), d1, claims, (L.d0(n0 + g, (col, a + X + b)), d1), long_only)


def vgaps():
    out = []
    for k, (c, g) in enumerate([(c, g) for c in (64, 65) for g in (2, 3, 4, 5, 6)]):
        rng = np.random.default_rng([53, 4, k])
        out.append(_vgap("vgaps", "col_%d_g%d" % (c, g), rng, c, 2 + 2 * k, g, 45, 45, int(rng.integers(0, 30))))
    return out


def vgaps_long():
    """vertical runs next to the stripe and sweep seams; runs and diagonals across the checkpoint row 256; n1 at the block edges"""
    out = []
    for k, (c, g) in enumerate([(512, 2), (512, 5), (513, 3), (513, 6), (2048, 2), (2048, 6), (2049, 4), (2049, 5)]):
        rng = np.random.default_rng([53, 5, k])
        # n1 = 175 = 7 * 25: with a checkpoint interval of 7 the last row is a multiple of K (a checkpoint that must NOT be written)
        out.append(_vgap("vgaps_long", "col_%d_g%d" % (c, g), rng, c, 20 + k, g, 45, 45, int(rng.integers(5, 60)) if c < 2048 else int(rng.integers(0, 6)), True, n1=175))
    for k, (first, g) in enumerate(((256, 2), (255, 4), (252, 6), (256, 5))):        # the E run covers rows 256 and 257
        rng = np.random.default_rng([53, 5, 20 + k])
        assert first <= 256 and first + g - 1 >= 257
        out.append(_vgap("vgaps_long", "rows_%d_%d" % (first, first + g - 1), rng, 100 + 7 * k, first - 45, g, 45, 45, 12, True))
    for k, n1 in enumerate((255, 256, 257, 512, 513)):
        rng = np.random.default_rng([53, 5, 40 + k])
        m = 50 if n1 < 300 else 300                     # 512 / 513: the path ends in the last block and crosses row 256 | 257 above it
        extra = [("diag_rows", (256, 257))] if n1 >= 257 and m == 300 else []
        out.append(_exact("vgaps_long", "n1_%d_ends_in_last_row" % n1, rng, 330, n1, 9 + k, n1 - m + 1, m, extra, True))
    rng = np.random.default_rng([53, 5, 60])
    out.append(_exact("vgaps_long", "diagonal_across_row_256", rng, 150, 300, 40, 226, 61, [("diag_rows", (256, 257))], True))
    return out


# ---- equal maxima ------------------------------------------------------------------------------------------------------------
def _copies(group, name, rng, n0, cols, n1, rows, xs0, xs1, win, maxima, long_only=False):
    """d0 holds the 55-mers xs0 at cols, d1 holds xs1 at rows; win = index into rows of the copy whose removal is the twin"""
    L = _Lay(rng)
    d0 = L.d0(n0, *zip(cols, xs0))
    p1 = list(zip(rows, xs1))
    d1 = L.d1(n1, *p1)
    m = len(xs0[0])
    i, j = maxima[0]
    claims = [("maxima", maxima), ("score", MATCH * m), ("coords", (j - m, j, i - m, i))]
    twin1 = L.d1(n1, *[(r, x if k != win else L.f1(len(x))) for k, (r, x) in enumerate(p1)])
    return Case(group, name, d0, d1, claims, (d0, twin1), long_only)


def ties():
    out = []
    m = 55
    rng = np.random.default_rng([53, 6, 0])
    x, y = rand_seq(rng, m), rand_seq(rng, m)
    # X early in d1 and late in d0, Y late in d1 and early in d0: (earlier row, later column) against (later row, earlier column)
    out.append(_copies("ties", "earlier_row_later_column", rng, 190, (10, 120), 170, (8, 100), (y, x), (x, y), 0,
                       [(8 + m - 1, 120 + m - 1), (100 + m - 1, 10 + m - 1)]))
    rng = np.random.default_rng([53, 6, 1])
    x = rand_seq(rng, m)
    # one row, columns j and j + 64: the same lane of k_zero keeps the first
    out.append(_copies("ties", "one_row_columns_j_j64", rng, 150, (12, 76), 80, (15,), (x, x), (x,), 0,
                       [(15 + m - 1, 12 + m - 1), (15 + m - 1, 76 + m - 1)]))
    rng = np.random.default_rng([53, 6, 2])
    x = rand_seq(rng, m)
    # one row, columns j and j + 576: other stripes of k_zero_long (waves 0 and 1), the same lane of k_zero
    out.append(_copies("ties", "one_row_other_stripe", rng, 700, (40, 616), 90, (21,), (x, x), (x,), 0,
                       [(21 + m - 1, 40 + m - 1), (21 + m - 1, 616 + m - 1)]))
    rng = np.random.default_rng([53, 6, 3])
    x = rand_seq(rng, m)
    # three copies in either piece: nine equal maxima.  (The copies lie 40 .. 60 unmatched bases apart: joining two of them
    # through the spacers costs at least 40 mismatches, more than the 110 a second copy adds)
    cols, rows = (5, 110, 225), (11, 106, 206)
    out.append(_copies("ties", "three_by_three", rng, 290, cols, 270, rows, (x, x, x), (x, x, x), 0,
                       [(r + m - 1, c + m - 1) for r in rows for c in cols]))
    rng = np.random.default_rng([53, 6, 5])
    x = rand_seq(rng, m)
    # one row, columns 600 and 2100: wave 1 of the first sweep against wave 0 of the second -- the merge over the waves of
    # k_zero_long meets the later column first
    out.append(_copies("ties", "one_row_other_sweep", rng, 2130, (546, 2046), 85, (15,), (x, x), (x,), 0,
                       [(15 + m - 1, 600), (15 + m - 1, 2100)]))
    rng = np.random.default_rng([53, 6, 6])
    x, y = rand_seq(rng, m), rand_seq(rng, m)
    # columns j (later row) and j + 2048 (earlier row): one lane of k_zero_long meets the later row first, in its first sweep
    out.append(_copies("ties", "earlier_row_next_sweep_same_lane", rng, 2140, (10, 2058), 170, (8, 100), (x, y), (y, x), 0,
                       [(8 + m - 1, 2058 + m - 1), (100 + m - 1, 10 + m - 1)]))
    rng = np.random.default_rng([53, 6, 4])
    x = rand_seq(rng, m)
    # two copies in d0 in other chunks and other lanes, two in d1
    cols, rows = (30, 131), (3, 95)
    out.append(_copies("ties", "two_by_two_other_lanes", rng, 200, cols, 160, rows, (x, x), (x, x), 0,
                       [(r + m - 1, c + m - 1) for r in rows for c in cols]))
    return out


# ---- the acceptance threshold ------------------------------------------------------------------------------------------------
def threshold():
    out = []
    for k, (m, sub, col) in enumerate(((40, False, 30), (40, False, 45), (39, False, 30), (39, False, 45), (41, True, 30), (41, True, 44),
                                       (42, True, 30), (43, True, 40))):
        rng = np.random.default_rng([53, 7, k])
        L = _Lay(rng)
        x = rand_seq(rng, m)
        y = x[:m // 2] + other_base(x[m // 2]) + x[m // 2 + 1:] if sub else x
        sc = MATCH * (m - 1) + MISMATCH if sub else MATCH * m
        row = 5 + 3 * k
        d0 = L.d0(col + m + 20, (col, x))
        n1 = row + m + 9
        claims = [("score", sc), ("accepted" if sc >= MIN_SCORE else "refused", None), ("coords", (col - 1, col - 1 + m, row - 1, row - 1 + m))]
        out.append(Case("threshold", "%dmer%s_col%d_score%d" % (m, "_sub" if sub else "", col, sc), d0, L.d1(n1, (row, y)), claims, (d0, L.d1(n1))))
    return out


# ---- the limits of k_zero ----------------------------------------------------------------------------------------------------
def limits():
    out = []
    rng = np.random.default_rng([53, 8, 0])
    out.append(_exact("limits", "n0_4096_ends_in_last_column", rng, ZW, 120, ZW - 49, 40, 50))
    rng = np.random.default_rng([53, 8, 1])
    out.append(_exact("limits", "n0_4097_ends_in_last_column", rng, ZW + 1, 120, ZW + 1 - 49, 33, 50, [("diag_cols", (ZW, ZW + 1))]))
    for k, (n0, n1) in enumerate(((1, 100), (100, 1))):
        rng = np.random.default_rng([53, 8, 2 + k])
        x = rand_seq(rng, 100)
        d0, d1 = (x[:1], x) if n0 == 1 else (x, x[:1])
        out.append(Case("limits", "n0_%d_n1_%d" % (n0, n1), d0, d1, [("score", MATCH), ("refused", None)], (x, x)))
    return out


def groups():
    """{group name: [Case]} of the designed groups (queue(n) is built by its user)"""
    g = {"seams64": seams64(), "hgaps": hgaps(), "vgaps": vgaps(), "ties": ties(), "threshold": threshold(), "limits": limits(),
         "hgaps_long": hgaps_long(), "vgaps_long": vgaps_long()}
    for name, cases in g.items():
        assert len({c.name for c in cases}) == len(cases) and all(c.group == name for c in cases)
    return g


SHORT_GROUPS = ("seams64", "hgaps", "vgaps", "ties", "threshold", "limits")      # fit k_zero: run on both kernels
LONG_GROUPS = ("hgaps_long", "vgaps_long")                                       # built for 512 / 2048 / K = 256: k_zero_long only


# ---- queue -------------------------------------------------------------------------------------------------------------------
def queue(n):
    """n single-splint reads (synth.make_zero_read, inserts of 500 .. 900 bases, either strand, about a third without overlap)
    as ([(seq, qual)], strands)"""
    from c3poa_amd import synth
    rng = np.random.default_rng([53, 10])
    reads, strands = [], []
    for i in range(n):
        L = int(rng.integers(500, 901))
        ov = int(rng.integers(60, 260))
        front = int(rng.integers(L // 2 - 40, L // 2 + 120))                      # d0 = ins[a:], d1 = ins[:b], overlap ins[a:b]
        a = L - front
        b = a + ov if i % 3 else max(30, a - int(rng.integers(20, 200)))         # every third read: the pieces do not meet
        b = min(b, L)
        s, q, st, _t = synth.make_zero_read(rng, synth.SPLINT1, L, a, b)
        reads.append((s, q)); strands.append(st)
    return reads, strands


# ---- random noisy pairs (host test) ------------------------------------------------------------------------------------------
def noisy(rng, s, err):
    out = []
    for c in s:
        u = rng.random()
        if u < err * 0.35:
            continue
        if u < err * 0.75:
            c = other_base(c, int(rng.integers(1, 4)))
        out.append(c)
        if rng.random() < err * 0.25:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def random_pairs(n, seed=11):
    """[(d0, d1)], 1 .. 220 bases, four-letter flanks: unrelated, sharing a noisy stretch, or the same over two letters (many ties)"""
    rng = np.random.default_rng([53, seed])
    out = []
    for i in range(n):
        d0 = rand_seq(rng, int(rng.integers(1, 221)))
        kind = i % 4
        if kind == 0:
            d1 = rand_seq(rng, int(rng.integers(1, 221)))
        else:
            lo = int(rng.integers(0, len(d0)))
            core = noisy(rng, d0[lo:lo + int(rng.integers(30, 200))], float(rng.choice([0.0, 0.05, 0.15, 0.3])))
            d1 = (rand_seq(rng, int(rng.integers(0, 60))) + core + rand_seq(rng, int(rng.integers(0, 60))))[:220] or "A"
            if kind == 2:
                d0, d1 = (s.replace("G", "A").replace("T", "C") for s in (d0, d1))
        out.append((d0, d1))
    return out

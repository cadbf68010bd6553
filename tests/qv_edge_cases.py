"""Cases shared by the k_qv edge tests (CPU: test_qv_edges_host.py, GPU: test_gpu_qv_edges.py).  A plain module, no fixtures:
every case is a pure function of a fixed seed, so both files see the same inputs.

A case is (name, cons, pieces, small): pieces = [(seq, qual, mode)] as Handle.consensus_qv takes them, except that a quality
string may hold any character 0 .. 255 (one per byte: lib_pieces() encodes them for the binding); small marks the cases the
slow Python restatement of include/c3poa.h (test_qv_host.spec_qv) can judge.  CLAIMS[name] states which mechanism of k_qv the
case was built for, as properties of the restatement's alignment (test_qv_host.spec_align's info); the host test asserts every
claim, so that a later edit cannot quietly stop reaching the code a case is for:
  d        the set of band steps lo(i) - lo(i-1) of every piece (mode 0; d_set() restates the centre formula)
  over     every piece has m > n + 64: the kernel stops at row n + 64 < m
  end      per piece, the end cell (mode 2: in the reversed frame)
  maxima   per piece, None or the cells of largest H, first the winner (smallest i, then smallest j)
  edges    per piece, (path touched band offset 0 with j > 0, path touched offset 127 with j < n)
  rows7    rows & 7 of every piece, rows = min(m, n + 64): where the last direction word is flushed
  quals    quality bytes that must be present

What the kernel does with them (k_qv.hip): lane l holds band cells 2l, 2l + 1; a row's up / diagonal neighbours come from lanes
l + (d >> 1) and one beside it (the odd-d fetch from l + (d >> 1) + 1); the piece's codes are refilled every 64 rows; direction
words hold 8 rows; modes 1 / 2 take the best cell by a per-lane strict maximum and a three-step wave reduction (value, then
smallest i, then smallest j); S lives in LDS up to 8192 columns and in a global slot above."""
import random

from test_qv_host import mutate, rand_qual, rand_seq, spec_qv

CASES = []
CLAIMS = {}


def d_set(n, m):
    """band steps of a mode-0 pair: c(i) = floor((i n + floor(m / 2)) / m) (include/c3poa.h)"""
    c = [(i * n + m // 2) // m for i in range(m + 1)]
    return {c[i] - c[i - 1] for i in range(1, m + 1)}


def rows_of(n, m, mode):
    """rows k_qv computes for a piece (row 0 not counted)"""
    return m if mode == 0 else min(m, n + 64)


def lib_pieces(pieces):
    """the pieces as the binding takes them: quality characters 0 .. 255 as one byte each"""
    return [(s, q.encode("latin-1"), md) for s, q, md in pieces]


def _add(name, cons, pieces, small=True, **claims):
    assert name not in CLAIMS and all(len(s) == len(q) and s for s, q, _m in pieces)
    CASES.append((name, cons, pieces, small))
    CLAIMS[name] = claims


def _resize(rng, s, m):
    return s[:m] + rand_seq(rng, max(0, m - len(s)))


def _other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def _stretch(cons, m):
    return "".join(cons[i * len(cons) // m] for i in range(m))


def _with_insertions(cons, m, k):
    """the consensus stretched to m - k bases with k extra bases spread over it, each unlike the base after it: k up moves"""
    s = list(_stretch(cons, m - k))
    for t in range(k):
        at = (t + 1) * (m - k) // (k + 1) + t
        s.insert(at, _other(s[at]))
    return "".join(s)


# ---- 1. skew, mode 0: piece[i] = cons[i * n // m], exact and with 5 % errors (length kept) -------------------------------------
SKEW = (((256, 64), {4}), ((255, 64), {3, 4}), ((200, 67), {2, 3}), ((200, 100), {2}), ((130, 100), {1, 2}), ((100, 130), {0, 1}),
        ((67, 200), {0, 1}), ((64, 256), {0, 1}), ((4, 1), {4}), ((1, 4), {0, 1}), ((1, 1), {1}),
        ((1000, 250), {4}), ((250, 1000), {0, 1}))       # the last two: past one 64-row refill of the piece codes

for _k, ((_n, _m), _d) in enumerate(SKEW):
    _rng = random.Random(7100 + _k)
    _cons = rand_seq(_rng, _n)
    _exact = _stretch(_cons, _m)
    _add("skew_%d_%d_exact" % (_n, _m), _cons, [(_exact, rand_qual(_rng, _m), 0)], d=_d)
    _add("skew_%d_%d_err" % (_n, _m), _cons, [(_resize(_rng, mutate(_rng, _exact, 0.05), _m), rand_qual(_rng, _m), 0)], d=_d)
    if _m >= 60 and _n <= 256:
        # up moves in rows of every step: the odd steps take the up neighbour of a lane's second cell from lane + (d >> 1) + 1
        _add("skew_%d_%d_ins" % (_n, _m), _cons, [(_with_insertions(_cons, _m, 6), rand_qual(_rng, _m), 0)], d=_d)

# ---- 2. long pieces, modes 1 and 2: cons + tail, head + cons ------------------------------------------------------------------
for _n in (1, 70, 200):
    for _t in (63, 64, 65, 200):
        _rng = random.Random(7200 + 1000 * _n + _t)
        _cons = rand_seq(_rng, _n)
        _add("long_n%d_t%d" % (_n, _t), _cons,
             [(_cons + rand_seq(_rng, _t), rand_qual(_rng, _n + _t), 1), (rand_seq(_rng, _t) + _cons, rand_qual(_rng, _n + _t), 2)],
             over=_t > 64, rows7=min(_n + _t, _n + 64) & 7)

# the best cell in the last, partial group of direction words of a piece cut at n + 64: 63 unmatched bases ahead of the whole
# consensus put it in row n + 63 (offset 1 of the band); rows = n + 64 = 267, rows & 7 = 3, the last group is rows 265 .. 267
_rng = random.Random(7290)
_cons = rand_seq(_rng, 203)
_junk = "".join(_other(c, 2) for c in _cons[:63])
_add("long_end_in_last_group", _cons,
     [(_junk + _cons + rand_seq(_rng, 20), rand_qual(_rng, 286), 1), (rand_seq(_rng, 20) + _cons + _junk[::-1], rand_qual(_rng, 286), 2)],
     over=True, rows7=3, end=[(266, 203), (266, 203)])

# ---- 3. nothing matches: the best cell is (0, 0), nothing is covered ----------------------------------------------------------
_rng = random.Random(7300)
_add("nothing_matches", "A" * 50, [("C" * 50, rand_qual(_rng, 50), 1), ("C" * 50, rand_qual(_rng, 50), 2)], end=[(0, 0), (0, 0)])

# ---- 4. row-group seams: the best cell lies in the last computed row, rows & 7 = 7, 0, 1 ---------------------------------------
for _L in (7, 8, 9, 63, 64, 65, 127, 128, 129):
    _rng = random.Random(7400 + _L)
    _cons = rand_seq(_rng, _L + 30)
    _add("seam_%d" % _L, _cons, [(_cons[:_L], rand_qual(_rng, _L), 1), (_cons[-_L:], rand_qual(_rng, _L), 2)],
         end=[(_L, _L), (_L, _L)], rows7=_L & 7)

# ---- 5. ties ------------------------------------------------------------------------------------------------------------------
# the periodic pair of test_qv_host.test_adversarial: many equal PATHS to one best cell (the traceback's priority decides), no
# second best cell -- so no maxima claim
_add("periodic", "AC" * 60, [("AC" * 30, "I" * 60, 1), ("CA" * 30, "I" * 60, 2), ("A", "5", 1), ("G", "5", 2)])
# a whole period too many in the piece: row 60 and row 62 end in equal cells of one diagonal (one lane)
_add("periodic_two_rows", "AC" * 30 + "GG" + "AC" * 4, [("AC" * 30 + "TT" + "AC" * 2, "I" * 66, 1)],
     maxima=[[(60, 60), (66, 66)]], end=[(60, 60)])


def _two_rows_one_lane(rng):
    """H = 80 at (40, 40), 76 at (41, 41), 78, 80 at (43, 43): both on the main diagonal, so one lane meets them in row order"""
    cons = rand_seq(rng, 60)
    return cons, cons[:40] + _other(cons[40]) + cons[41:43], [(40, 40), (43, 43)]


def _one_row_two_lanes(rng):
    """two mismatches on the diagonal tie with three deletions: (m, m) and (m, m + 3), lanes 32 and 33"""
    a = rand_seq(rng, 24)
    r = "ACG" * 6                  # r against "ATT" + r on the diagonal: C / T and G / T mismatch, the rest matches (period 3)
    return a + "ATT" + r, a + r, [(42, 42), (42, 45)]


def _two_rows_two_lanes(rng):
    """a matches against a matches, three deletions and six more matches: (a, a) in lane 32 and (a + 6, a + 9) in lane 33.  The
    later row holds the larger j: a reduction that took the largest i, or the smallest j first, would pick the other cell"""
    a = rand_seq(rng, 30)
    return a + "TTT" + "ACACAC" + "TTTTTT", a + "ACACAC" + "GGGGGG", [(30, 30), (36, 39)]


def _first_with_maxima(build, seed):
    """the first seed from `seed` on whose pair has exactly the maxima it was built for (a random prefix can add a third)"""
    for s in range(seed, seed + 50):
        rng = random.Random(s)
        cons, piece, want = build(rng)
        infos = []
        spec_qv(cons, [(piece, "I" * len(piece), 1)], infos)
        if infos[0]["maxima"] == want:
            return cons, [(piece, rand_qual(rng, len(piece)), 1)], want
    raise AssertionError(build.__name__)


for _k, _b in enumerate((_two_rows_one_lane, _one_row_two_lanes, _two_rows_two_lanes)):
    _cons, _pieces, _want = _first_with_maxima(_b, 7500 + 100 * _k)
    _add("tie" + _b.__name__, _cons, _pieces, maxima=[_want], end=[_want[0]])
    # the same tie in mode 2: both sequences reversed
    _add("tie" + _b.__name__ + "_mode2", _cons[::-1], [(s[::-1], q[::-1], 2) for s, q, _md in _pieces], maxima=[_want], end=[_want[0]])

# ---- 6. leaving the band ------------------------------------------------------------------------------------------------------
# 150 extra bases in the piece at column a, n = 200, m = 350.  Mode 0 (c(i) = 4i / 7): the leading diagonal reaches the insertion
# at offset 64 + 3a / 7 and the trailing one leaves it at 3a / 7 - 22.  In the middle (a = 100: 107 and 21) the whole path fits
# the band and touches no edge; a = 20 puts the trailing diagonal below offset 0, so the path is pressed against that edge.
# Mode 1 (c(i) = i) cannot hold 150 extra rows in any band of 128: it ends at its
# best cell (a, a) before the insertion and touches nothing -- the two ride cases below are its edge cases
_rng = random.Random(7600)
_cons = rand_seq(_rng, 200)
for _name, _a, _e in (("middle", 100, (False, False)), ("early", 20, (True, False))):
    _ins = _cons[:_a] + rand_seq(_rng, 150) + _cons[_a:]
    _add("band_piece_insert_" + _name, _cons, [(_ins, rand_qual(_rng, 350), 0), (_ins, rand_qual(_rng, 350), 1)],
         edges=[_e, (False, False)], end=[(350, 200), (_a, _a)])
# 150 extra columns in the middle of the consensus, n = 200 = 4 m: more than a band of 128 can span in one row, so the mode-0
# path is pressed against offset 127; mode 1 ends before the extra columns
_x = rand_seq(_rng, 50)
_cons = _x[:25] + rand_seq(_rng, 150) + _x[25:]
_add("band_cons_insert_middle", _cons, [(_x, rand_qual(_rng, 50), 0), (_x, rand_qual(_rng, 50), 1)], d={4},
     edges=[(False, True), (False, False)])
# mode 1 along an edge: the piece lacks 63 columns (j = i + 63: offset 127 for 197 rows) / holds 64 extra bases (j = i - 64:
# offset 0 for 260 rows); the matches after the gap pay for it, so the path goes on to the end
_cons = rand_seq(_rng, 300)
_add("band_ride_127", _cons, [(_cons[:40] + _cons[103:], rand_qual(_rng, 237), 1)], edges=[(False, True)], end=[(237, 300)])
_add("band_ride_0", _cons, [(_cons[:40] + rand_seq(_rng, 64) + _cons[40:], rand_qual(_rng, 364), 1)], edges=[(True, False)], end=[(364, 300)])

# ---- 7. letters and qualities ---------------------------------------------------------------------------------------------------
_rng = random.Random(7700)
_cons = rand_seq(_rng, 250, "ACGTacgtNU")


def _qual_bytes(rng, n):
    """every byte value 0 .. 255 can occur; '!' (0), '~' (93) and the clamped ends are made sure of"""
    q = [rng.randrange(256) for _ in range(n)]
    for k, v in enumerate((33, 126, 0, 255, 32, 127)):
        q[(7 + 13 * k) % n] = v
    return "".join(map(chr, q))


_ps = [mutate(_rng, _cons, 0.1), _cons[:120] + rand_seq(_rng, 9, "nNuUx"),
       rand_seq(_rng, 5, "acgt") + _cons[140:], _cons.swapcase()]
_add("letters_and_quals", _cons, [(s, _qual_bytes(_rng, len(s)), md) for s, md in zip(_ps, (0, 1, 2, 0))],
     quals={0, 32, 33, 126, 127, 255})

# ---- 8. the LDS / global switch (not small: the host statement judges) --------------------------------------------------------
for _n in (8191, 8192, 8193, 8209):
    _rng = random.Random(7800 + _n)
    _cons = rand_seq(_rng, _n)
    _ps = [mutate(_rng, _cons, 0.08), mutate(_rng, _cons[:_n - 700], 0.08) + rand_seq(_rng, 40), rand_seq(_rng, 40) + mutate(_rng, _cons[900:], 0.08)]
    _add("switch_%d" % _n, _cons, [(s, rand_qual(_rng, len(s)), md) for md, s in enumerate(_ps)], small=False)

SMALL_CELLS = sum((len(s) + 1) * 128 for _name, _c, ps, small in CASES if small for s, _q, _md in ps)

"""The polish stage under polish scorings next to its guards.  win_rows_dispatch (k_polish.hip, `ok16`) chooses per layer, at run
time, between the 16-bit register-blocked rows (unbanded and banded) and the 32-bit linear rows; extend_align (k_prep) chooses
per piece between the mask-free and the masked rows (`kstep`); c3_create admits -8191 .. 8191 for every pol_* field and wants
the match above two gaps.  Every case runs a scoring that puts layers (pieces) where the guard decides -- both sides in one window, keys next to
the top and the bottom of the 16-bit range, the last admitted and the first refused byte value, the signs that switch a path off
-- and compares the GPU with the CPU oracle bit for bit: statuses, subread counts, consensus lengths and bytes, window counts
and the counted cells of both alignment stages.  Every moved key goes to both sides.  Every case first asserts, on the oracle's
window capture (piece lengths), the shape it exists for, with thresholds of about half of what the generator gives today, so a
change of the generator fails loudly instead of hollowing the case out.  All GPU runs poison fresh device memory
(C3_DEBUG_POISON).  That the oracle itself is the unbanded optimum under these scorings: tests/test_independent_checkers.py."""
import os

import numpy as np
import pytest

from c3poa_amd import synth

import test_gpu_prep_rows as PR
import test_gpu_win_chain as WC

pytestmark = pytest.mark.gpu

# twelve reads of test_gpu_win_chain's batch: nine of the insert sweep, two insertion-first reads and the error-free read
SUBSET = (0, 3, 6, 9, 12, 15, 18, 19, 28, 29, 30, 31)
BIG = 400                       # a "big" layer: Q >= BIG
POL_MAX = 8191                  # c3_create: every pol_* field is -POL_MAX .. POL_MAX
_HOOKS = ("C3_DEBUG_WIN_CHAIN", "C3_DEBUG_POISON", "C3_DEBUG_BAND", "C3_DEBUG_HCAP_DIV", "C3_DEBUG_PREP_ROWS")
_cache = {}


def ok16(match, mismatch, gap, Q, R):
    """copy of win_rows_dispatch's `ok16` (k_polish.hip): the layer may take the 16-bit rows.  Keep the two in step."""
    pm = max(abs(match), abs(mismatch), abs(gap))
    return not (4 * pm * (max(R, Q) + 4) >= 31000 or 4 * (max(abs(match), mismatch) + abs(gap)) * (Q + 4) >= 31000 or pm > 30 or gap >= 0)


def _cfg(s):
    return dict(pol_match=s[0], pol_mismatch=s[1], pol_gap=s[2])


def _batch():
    if "batch" not in _cache:
        reads, strands = WC._batch()
        _cache["batch"] = ([reads[i] for i in SUBSET], [strands[i] for i in SUBSET])
    return _cache["batch"]


def _oracle(s):
    """oracle records, consensi and window capture of the subset under scoring s, computed once; every layer gets its row count R
    and the side of the guard it falls on"""
    from oracle import oracle_py as O
    if ("oracle", s) not in _cache:
        reads, strands = _batch()
        O.win_capture(True)
        try:
            ores, ocons = O.process_batch(synth.SPLINT1, reads, strands, params=O.default_params(**_cfg(s)), threads=1)
            als = O.win_captured()
        finally:
            O.win_capture(False)
        for a in als:
            a["R"] = int(np.count_nonzero(a["mask"]))
            a["ok16"] = ok16(s[0], s[1], s[2], a["Q"], a["R"])
        assert all(o.status == 0 for o in ores), [o.status for o in ores]
        _cache[("oracle", s)] = (ores, ocons, als)
    return _cache[("oracle", s)]


def _sides(als, big=False):
    """(layers on the 16-bit side, layers on the 32-bit side)"""
    sel = [a for a in als if not big or a["Q"] >= BIG]
    return sum(a["ok16"] for a in sel), sum(not a["ok16"] for a in sel)


def _gpu_run(s, env):
    from c3poa_amd import _lib
    reads, strands = _batch()
    keep = {k: os.environ.get(k) for k in _HOOKS}
    for k in _HOOKS:
        os.environ.pop(k, None)
    os.environ["C3_DEBUG_POISON"] = "1"
    os.environ.update(env)
    try:
        h = _lib.Handle(**_cfg(s))
        h.set_splints([synth.SPLINT1])
        h.upload([r[0] for r in reads], [r[1] for r in reads], strands)
        h.run()
        res, cons = h.results()
        t = h.timing()
        h.close()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, cons, t


def _check(s, env=None, oracle_cells=True):
    """GPU == oracle under scoring s, as test_gpu_win_chain._check compares.  returns (results, consensi, timing counters)"""
    ores, ocons, _ = _oracle(s)
    res, cons, t = _gpu_run(s, env or {})
    for i, o in enumerate(ores):
        assert int(res[i]["status"]) == o.status, (s, i, int(res[i]["status"]), o.status)
        for f in ("n_sub", "cons_len"):
            assert int(res[i][f]) == getattr(o, f), (s, i, f, int(res[i][f]), getattr(o, f))
        assert cons[i] == ocons[i], (s, i)
    for k in ("cells_poa", "cells_polish") if oracle_cells else ("cells_poa",):
        want = sum(int(getattr(o, k)) for o in ores)
        assert t[k] == want, (s, k, t[k], want)
    return res, cons, t


def _same(a, b, s):
    """two GPU runs of one scoring agree: records, consensi, counted and computed cells, band counters"""
    for i in range(len(a[0])):
        for f in ("status", "n_sub", "cons_len", "n_win"):
            assert int(a[0][i][f]) == int(b[0][i][f]), (s, i, f, int(a[0][i][f]), int(b[0][i][f]))
        assert a[1][i] == b[1][i], (s, i)
    for k in WC._TIMING:
        assert a[2][k] == b[2][k], (s, k, a[2][k], b[2][k])


@pytest.mark.parametrize("s,least,least_first", [((3, -15, -4), 10, 0), ((8, -8, -8), 5, 8)])
def test_both_sides_of_the_guard_in_one_run(s, least, least_first):
    """(3,-15,-4): the first condition decides, by R; (8,-8,-8): the second, by Q.  Big layers fall on both sides, and windows hold
    layers of both sides, so the 16-bit rows read what the linear rows left in the graph and the other way round; under (8,-8,-8)
    first layers (the chain phases) fall on both sides too.  The chain and the general first-layer phases must agree where a
    window's layers straddle the guard."""
    _, _, als = _oracle(s)
    n16, n32 = _sides(als, big=True)
    assert n16 >= least and n32 >= least, (s, n16, n32)
    mixed = {a["win"] for a in als if a["ok16"]} & {a["win"] for a in als if not a["ok16"]}
    assert len(mixed) >= 3, (s, len(mixed))
    first = [a for a in als if a["layer"] == 0]
    assert sum(a["ok16"] for a in first) >= 8 and sum(not a["ok16"] for a in first) >= least_first
    new = _check(s)
    old = _check(s, env={"C3_DEBUG_WIN_CHAIN": "0"})
    _same(new, old, s)


def test_neighbouring_scorings_move_layers_across_the_guard():
    """mismatch -14 and -15: one step of one score moves layers from the 16-bit to the 32-bit side; the GPU equals the oracle on
    both sides of the step"""
    a14, a15 = _oracle((3, -14, -4))[2], _oracle((3, -15, -4))[2]
    s14 = {(a["win"], a["layer"]) for a in a14 if a["ok16"]}
    s15 = {(a["win"], a["layer"]) for a in a15 if a["ok16"]}
    assert len(s14) >= 60 and len(s15) >= 50 and _sides(a14, big=True)[0] >= _sides(a15, big=True)[0] + 15
    _check((3, -14, -4))
    _check((3, -15, -4))


def test_keys_next_to_the_top_of_the_16_bit_range():
    """(14,-14,-1): the error-free read's layers score 14 per base, 4 * score reaches 28 000 and the horizontal scan's
    4 * (score - g * j) 30 000 of the 32 767 a key may hold"""
    s = (14, -14, -1)
    _, _, als = _oracle(s)
    top = [a for a in als if a["ok16"] and 4 * a["score"] >= 27000 and 4 * (a["score"] + abs(s[2]) * a["Q"]) >= 29000]
    assert len(top) >= 2, len(top)
    assert _sides(als, big=True)[0] >= 35
    t = _check(s)[2]
    assert t["n_band_layers"] > 0
    t = _check(s, env={"C3_DEBUG_BAND": "off"})[2]       # the unbanded rows: a band's keys count from the band start, these from column 0
    assert t["n_band_layers"] == 0


def test_keys_beyond_the_top_of_the_16_bit_range():
    """(17,-17,-1): the error-free read's 500-base layers end at 4 * score = 34 000, which no 16-bit key holds: they must be on
    the 32-bit side (real reads stay far below the guard's worst case pm * max(R, Q); this read attains it)"""
    s = (17, -17, -1)
    _, _, als = _oracle(s)
    over = [a for a in als if 4 * a["score"] > 32767]
    assert len(over) >= 3 and not any(a["ok16"] for a in over), (len(over), sum(a["ok16"] for a in over))
    assert _sides(als)[0] >= 20
    _check(s)


@pytest.mark.parametrize("s", [(1, -14, -14), (2, -3, -13)])
def test_keys_next_to_the_sentinel(s):
    """column 0 of row R holds 4 * g * R: within about 1 300 of W_NEG16 = -32 000, to which lane 0 adds g41"""
    _, _, als = _oracle(s)
    low = [a for a in als if a["ok16"] and 4 * abs(s[2]) * a["R"] >= 29000]
    assert len(low) >= 5, (s, len(low))
    assert _sides(als, big=True)[0] >= 35
    _check(s)
    _check(s, env={"C3_DEBUG_BAND": "off"})


def test_the_last_byte_value_the_guard_admits():
    """pm = 30: only short layers stay on the 16-bit side, with substitution bytes 4 * 30 + 3 = 123 and 4 * -30 + 3 = -117"""
    s = (30, -30, -30)
    _, _, als = _oracle(s)
    n16, n32 = _sides(als)
    assert n16 >= 10 and n32 >= 60, (n16, n32)
    _check(s)
    _check(s, env={"C3_DEBUG_BAND": "off"})


@pytest.mark.parametrize("s", [(31, -5, -4), (3, -31, -4), (3, -5, -31)])
def test_the_first_byte_value_the_guard_refuses(s):
    """pm = 31 in either field: every layer is linear"""
    _, _, als = _oracle(s)
    assert _sides(als)[0] == 0 and len(als) >= 60
    t = _check(s)[2]
    assert t["n_band_layers"] == 0


@pytest.mark.parametrize("s", [(3, -5, 0), (3, -5, 1)])
def test_gap_not_negative(s):
    """gap >= 0: the 16-bit rows' horizontal scan needs gap < 0; every layer is linear"""
    _, _, als = _oracle(s)
    assert _sides(als)[0] == 0 and len(als) >= 60
    t = _check(s)[2]
    assert t["n_band_layers"] == 0


@pytest.mark.parametrize("s,least,least32", [((-1, -14, -1), 30, 8), ((0, 0, -1), 60, 0)])
def test_no_positive_substitution_score(s, least, least32):
    """max(match, mismatch) <= 0: the band's certificate has no gain to bound, the band is off; the unbanded 16-bit rows still run.
    ((-14,-14,-1) is refused by c3_create: its match does not beat two gaps, DESIGN.md 4.6a, tests/test_cabi.py.  On the GPU its
    windows outgrow the graph's capacity: 12 of 12 reads end as C3_ST_LIMIT where the oracle, which has no capacity, polishes.)"""
    _, _, als = _oracle(s)
    assert _sides(als)[0] >= least and _sides(als)[1] >= least32, (s, _sides(als))
    t = _check(s)[2]
    assert t["n_band_layers"] == 0


@pytest.mark.parametrize("s", [(3, 4, -4), (1, -1, -1)])
def test_mismatch_above_match_and_a_small_scoring(s):
    """(3,4,-4): the larger substitution score is the mismatch (the band certificate's `ups`); (1,-1,-1): an ordinary small one.
    Every layer is on the 16-bit side."""
    _, _, als = _oracle(s)
    assert _sides(als)[1] == 0 and _sides(als, big=True)[0] >= 40
    t = _check(s)[2]
    assert t["n_band_layers"] > 0


@pytest.mark.parametrize("s", [(1, 14, -14), (1, 12, -12)])
def test_mismatch_far_above_match(s):
    """the horizontal scan carries 4 * (score - g * j), and the score grows by max(match, mismatch) per column, not by |match|.
    Layers whose end cell alone has 4 * (score + |g| * Q) beyond 32 767 must not be on the 16-bit side; a guard that bounds the
    scan by |match| + |g| (the same scoring with the mismatch's sign turned) admits a third of them"""
    _, _, als = _oracle(s)
    far = [a for a in als if 4 * (a["score"] + abs(s[2]) * a["Q"]) > 32767]
    assert len(far) >= 40, (s, len(far))
    assert not any(a["ok16"] for a in far), (s, sum(a["ok16"] for a in far))
    assert sum(ok16(s[0], -s[1], s[2], a["Q"], a["R"]) for a in far) >= 10
    assert _sides(als)[0] >= 20, (s, _sides(als))
    _check(s)
    _check(s, env={"C3_DEBUG_BAND": "off"})


@pytest.mark.parametrize("s", [(3, 4, -4), (14, -14, -1), (2, -3, -13)])
def test_band_certificate_under_other_scorings(s):
    """C3_DEBUG_BAND=verify compares band and full matrix of every accepted layer on the device (it counts their cells twice: the
    polish cells are compared between the two GPU runs only, as test_gpu_win_chain.test_band_modes does)"""
    new = _check(s, env={"C3_DEBUG_BAND": "verify"}, oracle_cells=False)
    old = _check(s, env={"C3_DEBUG_BAND": "verify", "C3_DEBUG_WIN_CHAIN": "0"}, oracle_cells=False)
    _same(new, old, s)
    assert new[2]["n_band_layers"] > 0 and new[2]["n_band_mismatch"] == 0


def test_second_launch_sees_both_sides_of_the_guard():
    """a first launch without DP scratch: the k_window<true> instance redoes windows whose layers are 16-bit and linear"""
    t = _check((3, -15, -4), env={"C3_DEBUG_HCAP_DIV": "100000"})[2]
    assert t["n_win_redo"] > 0


@pytest.mark.parametrize("s", [(POL_MAX, -5, -4), (-7, -5, -4), (3, POL_MAX, -4), (3, -POL_MAX, -4), (3, -5, -POL_MAX), (3, -5, 1),
                               (POL_MAX, -POL_MAX, 4095)])
def test_last_admitted_value_of_each_field(s):
    """the ends of c3_create's ranges, one field moved and the other two at their defaults: -8191 and 8191, and
    where the match has to stay above two gaps, match -7 and gap 1; the largest gap of all, 4095 under match 8191"""
    _, _, als = _oracle(s)
    assert len(als) >= 60 and (_sides(als)[0] == 0 or s == (-7, -5, -4))
    _check(s)


# ---- k_prep's extension rows: the switch between mask-free and masked rows reached through the scoring

def _kstep(s):
    return 4 * max(abs(s[0]), abs(s[1]), abs(s[2])) + 3


def _prep_reads(seeds, n_short):
    if ("prep", seeds, n_short) not in _cache:
        reads, strands = [], []
        for seed in seeds:
            r, st = PR._lost_splint_read(seed)
            reads.append(r); strands.append(st)
        for k in range(n_short):
            s, q, st, _ = synth.make_read(np.random.default_rng([19, k]), synth.SPLINT1, 1216, 3, 170 + 30 * k, 170 + 30 * k)
            reads.append((s, q)); strands.append(st)
        _cache[("prep", seeds, n_short)] = (reads, strands)
    return _cache[("prep", seeds, n_short)]


def _prep_check(s, reads, strands):
    """PR._check: default rows == masked rows (C3_DEBUG_PREP_ROWS=old) == oracle.  returns the pieces' row counts"""
    ores, _ = PR._check(reads, strands, **_cfg(s))
    assert all(o.status == 0 for o in ores)
    return [n for o, r in zip(ores, reads) for n in PR._pieces(o, len(r[0]))]


def test_prep_rows_switch_inside_one_batch():
    """700 x the default scoring (the same alignments): kstep = 14 003, pieces of 942 rows and more take the masked rows, shorter
    ones the mask-free rows"""
    s = (2100, -3500, -2800)
    reads, strands = _prep_reads((0, 1, 2, 3), 4)
    lens = _prep_check(s, reads, strands)
    bw = 2 * PR.W + 1
    masked = [n for n in lens if _kstep(s) * (n + bw) >= 1 << 24]
    assert len(masked) >= 3 and len(lens) - len(masked) >= 4, (sorted(lens), len(masked))


def test_prep_rows_all_masked_at_the_largest_admitted_scoring():
    """kstep = 32 767 (20 000 is outside the admitted range): every piece of 255 rows and more is beyond the switch, which leaves
    the mask-free rows the two shortest pieces"""
    s = (POL_MAX, -POL_MAX, -POL_MAX)
    reads, strands = _prep_reads((0, 1), 4)
    lens = _prep_check(s, reads, strands)
    bw = 2 * PR.W + 1
    masked = [n for n in lens if _kstep(s) * (n + bw) >= 1 << 24]
    assert masked == [n for n in lens if n >= 255] and len(masked) >= 8 and len(lens) - len(masked) <= 2, sorted(lens)


def test_batch_beyond_the_32_bit_keys_is_an_error():
    """subreads of about 4 580 bases: at kstep 32 767 the keys of the polish rows could come within reach of the rows' sentinels
    ((4 * 8191 + 3) * (2 * length + 4 * 257) >= 2^28 from 3 583 bases on), and the run is refused, not computed inexactly; at
    kstep 14 003 the same read is admitted and equals the oracle"""
    from c3poa_amd import _lib
    s, q, st, _ = synth.make_read(np.random.default_rng([15, 0]), synth.SPLINT1, 4300, 2, 108, 108)
    ores, _ = PR._check([(s, q)], [st], **_cfg((2100, -3500, -2800)))
    assert ores[0].status == 0 and ores[0].n_sub >= 2
    h = _lib.Handle(**_cfg((POL_MAX, -POL_MAX, -POL_MAX)))
    try:
        h.set_splints([synth.SPLINT1])
        h.upload([s], [q], [st])
        with pytest.raises(_lib.C3Error) as e:
            h.run()
        assert e.value.code == _lib.E_LIMIT and "polish scoring" in str(e.value), str(e.value)
    finally:
        h.close()


@pytest.mark.parametrize("s", [(-1, -1, -4), (3, 5, -4)])
def test_prep_rows_match_not_above_mismatch(s):
    """4 * (match - mismatch) <= 0: no match-flag form (sub_shift = -1), and a mismatch scores no less than a match"""
    reads, strands = _prep_reads((0, 1), 4)
    lens = _prep_check(s, reads, strands)
    assert len(lens) >= 8 and max(lens) > 1200 and min(lens) < 400, sorted(lens)

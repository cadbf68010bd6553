"""The low-complexity case set (tests/low_complexity_cases.py) is not hollow: what tests/test_gpu_low_complexity.py compares on
the device must hold the ties it exists for, and a later edit of a generator must fail here instead of quietly losing them.
CPU only: everything is asserted on the oracle.

The two shares come from the oracle's row statistics (oracle/c3o_poa.c): rows whose maximum sits in more than one column
([55] / [0]) and cells whose winning value has more than one source ([62] / [63]), summed over the POA alignments of every
family of a group.  Each floor is about half of what the generators give at the committed seeds (the convention of
tests/test_gpu_pol_window.py); the measured values stand beside them.

The control (one random insert) must stay below half of the smallest floor of the tied-row share: 0.56 % against floors of
1.7 % and more.  The multi-source share cannot show that contrast and is not asked to: a random insert already has 22 % of such
cells (a match after a match ties nothing, but M = E1 or ht = F1 next to every indel does), the low-complexity groups 22 - 36 %,
so only its floors are asserted."""
import ctypes as C
import collections

import pytest

import low_complexity_cases as LC
import test_gpu_poa_pair as PP
from oracle import oracle_py as O

#          group       tied rows: floor, measured     multi-source cells: floor, measured
FLOORS = {"tracts":   ((0.017, 0.0349), (0.108, 0.2159)),
          "noflank":  ((0.042, 0.0843), (0.118, 0.2351)),
          "runlen":   ((0.027, 0.0544), (0.182, 0.3648)),
          "drift":    ((0.021, 0.0418), (0.118, 0.2366)),
          "seam":     ((0.024, 0.0478), (0.109, 0.2171)),
          "equalq":   ((0.022, 0.0443), (0.126, 0.2524)),
          "dangling": ((0.020, 0.0404), (0.127, 0.2547))}
CONTROL = (0.0056, 0.2214)      # measured: tied rows, multi-source cells of the control
_cache = {}


def _rowstats(subs):
    """the oracle's row statistics of the POA of one family"""
    lib = O.lib()
    S = (C.c_int64 * 64).in_dll(lib, "c3o_poa_rowstats")
    on = C.c_int.in_dll(lib, "c3o_poa_rowstats_on")
    for i in range(64):
        S[i] = 0
    on.value = 1
    try:
        out = O.poa_msa(list(subs), out_cons=False, out_msa=True)
    finally:
        on.value = 0
    return [int(x) for x in S], out


def _shares():
    """group -> (tied-row share, multi-source share)"""
    if "shares" not in _cache:
        agg = collections.defaultdict(lambda: [0, 0, 0, 0])
        for c in LC.CASES:
            s, _ = _rowstats(c.subs)
            assert s[0] > 0 and s[63] == s[1] and 0 <= s[55] <= s[0] and 0 <= s[62] <= s[63], c.name
            a = agg[c.group]
            a[0] += s[0]; a[1] += s[55]; a[2] += s[62]; a[3] += s[63]
        _cache["shares"] = {g: (a[1] / a[0], a[2] / a[3]) for g, a in agg.items()}
    return _cache["shares"]


def _captured(c):
    """the oracle's window alignments of a case"""
    O.win_capture(True)
    try:
        O.determine_consensus(c.subs, c.quals, c.front, c.tail, params=O.default_params(**c.cfg))
        return O.win_captured()
    finally:
        O.win_capture(False)


def test_the_set_is_what_the_issue_lists():
    names = [c.name for c in LC.CASES]
    assert len(set(names)) == len(names) and 55 <= len(names) <= 80
    assert set(LC.GROUPS) == set(FLOORS) | {"control"}
    per = collections.Counter(c.group for c in LC.CASES)
    assert per == {"tracts": 30, "noflank": 12, "runlen": 4, "drift": 6, "seam": 15, "equalq": 3, "dangling": 2, "control": 1}
    for c in LC.CASES:
        assert all(len(s) <= LC.QMAX for s in c.subs), c.name
        if c.group in ("tracts", "noflank") and not c.cfg:
            assert len(c.subs) in LC.COUNTS
        if c.group == "equalq":
            assert all(len(set(q)) == 1 for q in c.quals) and len({q[0] for q in c.quals}) == 1
        if c.group == "runlen":                         # nothing but run lengths differs: the runs' bases are one sequence
            assert len({"".join(b for b, _ in LC._runs(s)) for s in c.subs}) == 1 and len(set(c.subs)) == len(c.subs)
        if c.group == "dangling":
            assert c.front and c.tail


def test_every_case_has_a_draft_and_a_consensus():
    for c, (cons, draft, cells) in zip(LC.CASES, LC.reference()):
        assert draft and cons, c.name                   # a case without a consensus compares nothing
        assert cells[0] > 0 and cells[1] > 0, c.name


def test_the_counters_are_diagnostics_only():
    """with the row statistics on, the oracle returns what it returns with them off"""
    c = LC.CASES[1]
    plain = O.poa_msa(list(c.subs), out_cons=False, out_msa=True)
    s, counted = _rowstats(c.subs)
    assert counted == plain and s[62] > 0 and s[63] == s[1]
    # all A against all A: every row but the last few has its maximum on a plateau or a single diagonal cell; M, E and F tie
    s, _ = _rowstats(["A" * 50, "A" * 50])
    assert s[0] == 50 and s[63] == s[1] and s[62] > 0


@pytest.mark.parametrize("group", sorted(FLOORS))
def test_tie_shares_have_a_floor(group):
    tied, multi = _shares()[group]
    (tied_floor, tied_then), (multi_floor, multi_then) = FLOORS[group]
    assert tied >= tied_floor, (group, tied, tied_then)
    assert multi >= multi_floor, (group, multi, multi_then)
    assert tied_floor <= 0.55 * tied_then and multi_floor <= 0.55 * multi_then      # the floors are about half of the measurement


def test_the_control_shows_the_contrast():
    tied, multi = _shares()["control"]
    assert tied < 0.5 * min(f[0][0] for f in FLOORS.values()), (tied, CONTROL)
    assert 0.1 < multi < 0.3, (multi, CONTROL)           # see the module docstring: no contrast in this share


def test_copy_number_drift_gives_the_pair_kernel_two_column_rows():
    drift = [c for c in LC.CASES if c.group == "drift"]
    assert len(drift) == 6
    for c in drift:
        f = PP._rows(c.subs[0], c.subs[1])
        assert f["can"] and f["wide"] >= 90, (c.name, f)                            # measured: 189 .. 482 rows of 65 - 128 columns
        a, b = len(c.subs[0]), len(c.subs[1])
        assert abs(a - b) >= 25, (c.name, a, b)


def test_window_seams_fall_inside_the_tract():
    seam = [c for c in LC.CASES if c.group == "seam"]
    assert len(seam) == 15
    for c in seam:
        als = _captured(c)
        assert len({a["win"] for a in als}) == 3, c.name                           # three windows at pol_window 500
        lo, hi = c.tract[0] + 30, c.tract[1] - 30                                   # inside the tract whatever the copies' indels did
        assert lo < 500 < 1000 < hi
        cut = [a for a in als if lo < a["win"] * 500 + a["begin"] < hi or lo < a["win"] * 500 + a["end"] < hi]
        assert len(cut) >= len(c.subs), (c.name, len(cut))                         # every subread is cut at a seam at least once


def test_window_equals_period():
    per = [c for c in LC.CASES if c.cfg.get("pol_window") == 64]
    assert [c.name for c in per] == ["window64_p64x10", "window64_p65x10"]
    for c in per:
        als = _captured(c)
        assert len({a["win"] for a in als}) > 15, c.name
        assert max(a["blen"] for a in als) == 64


def test_dangling_pieces_are_cut_inside_the_tract():
    for c in (c for c in LC.CASES if c.group == "dangling"):
        if "polyA" in c.name:                            # the front begins and the tail ends in the run of A
            assert c.front[0].count("A", 0, 30) >= 24 and c.tail[0].count("A", len(c.tail[0]) - 30) >= 24, c.name
        als = _captured(c)
        assert max(a["layer"] for a in als) >= len(c.subs), c.name                 # a dangling piece made it into a window


def test_every_read_of_the_batch_has_a_consensus():
    reads, strands = LC.BATCH
    assert len(reads) == 24 and sum(s == "-" for s in strands) == 8
    res, cons = LC.batch_reference()
    assert [r.status for r in res] == [0] * 24
    assert all(3 <= r.n_sub <= 6 for r in res) and {r.n_sub for r in res} == {3, 4, 5, 6}
    assert all(cons)

"""k_poa_pair's rows ("rows without their bookkeeping"): the query of subread 1 as a byte table in LDS with a
pad in front and behind, the row's substitution addends as a 4-byte table, the active lanes as a mask made on the scalar unit,
row records written lane by lane, direction bytes through a vector offset, the band arithmetic wholly on the scalar unit.  None
of it may change a result.  Every case goes through the helpers of tests/test_gpu_poa_pair.py, so it asserts, under
C3_DEBUG_POISON: default == C3_DEBUG_POA_PAIR=0 == the CPU oracle bit for bit, equal counted cells, and n_pair as predicted on
the oracle side.  The shapes are the smallest at which the changed code can go wrong; the oracle-side facts each case relies on
(taken or not, rows of 65-128 columns or none) are asserted, so a changed generator cannot hollow a case out."""
import numpy as np
import pytest

import test_gpu_poa_pair as P
from c3poa_amd import synth

pytestmark = pytest.mark.gpu

RBSPAN = {"C3_DEBUG_POA_RBSPAN": "3300"}
NARROW = {"C3_DEBUG_POA_WIDE": "0"}
TABLE_EDGES = ((1, 1), (2, 1), (1, 2), (3, 3), (5, 4), (16, 17), (17, 16), (33, 31), (64, 64), (65, 63))


def _slot_rule(subs, quals):
    """the other half of the prediction for jobs of a few bases: the kernel declines a read whose cells so far + 128 exceed the
    cells of a k_poa slot of the first pass (such a read must reach the second pass as before), and a slot of a
    probe job is sized for that job alone (c3_stages.hip: (2 maxq + 2)(2w + 1 + maxq / 5) at most, rounded up to 64).
    Returns True: taken (even all POA cells the oracle counts for the job + 128 fit), False: declined at row 1 (the source row
    + 128 does not)"""
    p = P.O.default_params()
    q0, q1, maxq, ns = len(subs[0]), len(subs[1]), max(len(s) for s in subs), len(subs)
    w = p.poa_band_b + int(p.poa_band_f * maxq)
    typ = int(1.5 * maxq * (1.0 + 0.15 * (ns - 1)) * (2 * w + 12)) + 4096
    cap = (min((2 * maxq + 2) * (2 * w + 1 + maxq // 5), typ) + 63) // 64 * 64
    w1 = p.poa_band_b + int(p.poa_band_f * q1)
    row0 = min(q1, max(q1 - q0, 0) + w1) + 1
    if row0 + 128 > cap:
        return False
    cells = P.O.determine_consensus(subs, quals, params=p, return_draft=True)[2][0]
    assert cells + 128 <= cap, (q0, q1, cells, cap)           # neither bound decides: not a shape for this test
    return True


@pytest.mark.parametrize("third", [False, True])
def test_edges_of_the_query_table(third):
    """the band touches column 0 and column Q1 in every row: the pad in front of the table and the bytes behind it are read;
    16 / 17 and 64 / 65 bases end on and just past a packed word and a lane block.  Every shape is one the oracle-side row facts
    allow; the jobs of one and two bases are declined all the same, by the slot rule (the build before this file declines them
    too), and for those the kernel is asserted to have run and declined"""
    rng = np.random.default_rng(11 + third)
    shapes = [P._family(rng, max(q0, q1), (q0, q1, q0) if third else (q0, q1)) for q0, q1 in TABLE_EDGES]
    fits = [_slot_rule(s, q) for s, q in shapes]
    assert fits == [False, False, False] + [True] * 7
    taken = [x for x, f in zip(shapes, fits) if f]
    facts = P._probe_runs(taken)
    assert all(f["can"] for f in facts), facts            # so n_pair == 1 was asserted for every one of them
    small = [x for x, f in zip(shapes, fits) if not f]
    facts = P._probe_runs(small, pair_runs=False)          # default == kernel off == oracle, n_pair == 0
    assert all(f["can"] for f in facts), facts
    with P._env(P.POISON):
        h = P._lib.Handle()
        for s, q in small:
            h.determine_consensus(s, q)
            t = h.timing()
            assert (int(t["n_pair"]), int(t["n_pair_declined"])) == (0, 1), (s, dict(t))
        h.close()


@pytest.mark.parametrize("rows", [63, 64, 65, 127, 128, 129, 192, 193])
def test_record_seams(rows):
    """Q0 + 1 rows: lane 63 of a record block, a last block of one row, a last block that is full"""
    rng = np.random.default_rng(2000 + rows)
    q0 = rows - 1
    shapes = [P._family(rng, q0, (q0, q1)) for q1 in (q0, q0 - 1, q0 + 1)]
    facts = P._probe_runs(shapes)
    assert all(f["can"] for f in facts), facts


@pytest.mark.parametrize("d", [-50, -40, 40, 50])
def test_band_shifts_through_two_column_rows(d):
    """an indel of 40-50 bases: fast -> two-column -> fast rows, the ring written on demand"""
    facts = P._probe_runs([P._ragged_pair(np.random.default_rng(909), 600, d, ns=2)])
    assert facts[0]["can"] and facts[0]["wide"] > 0, facts


@pytest.mark.parametrize("d", [1, 2, 3, 4, 8, 16, 30])
def test_band_shifts_in_fast_rows(d):
    """an indel of at most 30 bases: the band jumps while every row stays a fast row; the register path gives way to the ring
    path and back"""
    shapes = [P._ragged_pair(np.random.default_rng(7), 300, s * d, ns=2) for s in (-1, 1)]
    facts = P._probe_runs(shapes)
    assert all(f["can"] and f["wide"] == 0 and f["over"] == 0 for f in facts), facts


def test_a_moving_base():
    """C3_DEBUG_POA_RBSPAN=3300: the saturating rebase every few rows, in both row kinds, through the row masks"""
    shapes = [P._ragged_pair(np.random.default_rng(909), 600, d, ns=2) for d in (-40, 40)]
    shapes += [P._ragged_pair(np.random.default_rng(7), 300, d, ns=2) for d in (-8, 8)]
    shapes.append(P._family(np.random.default_rng(31), 1500, (1500, 1490, 1510)))
    facts = P._probe_runs(shapes, env=RBSPAN)
    assert all(f["can"] for f in facts), facts
    assert facts[0]["wide"] > 0 and facts[1]["wide"] > 0 and facts[2]["wide"] == 0 and facts[3]["wide"] == 0, facts


def test_one_wave_many_reads(monkeypatch):
    """one slot: every read of both batches goes through the same wave, so the query table, its pads, the ring and the row
    records a longer read left are met by a shorter one"""
    handle = P._lib.Handle
    monkeypatch.setattr(P._lib, "Handle", lambda **kw: handle(slots_poa=1, **kw))
    a = list(synth.generate("cfg2", n_reads=24))
    b = list(synth.generate("cfg3", n_reads=24, seed=77))
    P._check_batches([a, b], synth.CONFIGS["cfg2"]["mdist"])


def test_decline_unchanged():
    """Q1 = 1793 is declined, Q1 = 1792 taken (the NARROW instance forced, as tests/test_gpu_poa_pair.py does)"""
    rng = np.random.default_rng(41)
    shapes = [P._family(rng, 1790, (1785, P.QMAX + 1, 1780)), P._family(rng, 1790, (1785, P.QMAX, 1780))]
    facts = P._probe_runs(shapes, env=NARROW)
    assert not facts[0]["can"] and facts[1]["can"], facts  # so n_pair 0 and 1 were asserted

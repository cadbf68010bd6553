"""k_zero and k_zero_long at their edges: the column seams (64 of k_zero; 8 / 512 / 2048 of k_zero_long), gaps across them, the
checkpoint rows of the blockwise traceback, equal maxima, the acceptance threshold, the limits that route a pair, and
workgroups that take several reads one after the other.  Every designed pair of zero_edge_cases.py goes through
Handle.zero_repeats; the consensus must equal oracle_py.zero_repeats and the four coordinates the kernel found -- read back
from the record of the one resident read -- must equal oracle_py.zero_local.  test_zero_oracle_host.py shows that the oracle
is the alignment of DESIGN.md 4.7 on the same pairs and that every pair reaches the code it is for.

Where the coordinates come from: k_zero / k_zero_long leave (r_st, r_en) and (tail_beg + q_st, tail_beg + q_en) in
sub_beg[0..1] / sub_end[0..1] of a rescued read; k_poa and k_polish only read them, k_zero_finish clears n_sub but not the
arrays, and c3_batch_results copies them (whole records under C3_FULL_RESULTS=1).  All handles poison fresh device memory
(C3_DEBUG_POISON): a direction byte, checkpoint or row carry nobody wrote does not read as zero."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import zero_edge_cases as ZC
from c3poa_amd import synth

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1
GROUPS = ZC.groups()
MODES = {"k_zero": {}, "long": {"C3_DEBUG_ZERO_LONG": "1"}, "long_k1": {"C3_DEBUG_ZERO_LONG": "1", "C3_DEBUG_ZERO_K": "1"},
         "long_k7": {"C3_DEBUG_ZERO_LONG": "1", "C3_DEBUG_ZERO_K": "7"}}


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@contextlib.contextmanager
def _handle(poison=True, **cfg):
    """a Handle whose whole lifetime runs under C3_DEBUG_POISON=1 (poison=False: without); the variable is restored afterwards"""
    from c3poa_amd import _lib
    keep = os.environ.get("C3_DEBUG_POISON")
    os.environ.pop("C3_DEBUG_POISON", None)
    if poison:
        os.environ["C3_DEBUG_POISON"] = "1"
    h = None
    try:
        h = _lib.Handle(**cfg)
        yield h
    finally:
        if h is not None:
            h.close()
        os.environ.pop("C3_DEBUG_POISON", None)
        if keep is not None:
            os.environ["C3_DEBUG_POISON"] = keep


def _record(h, n0, n1):
    """the record of the one read (d0 + d1) that c3_zero_repeats left resident"""
    h.n, h.off = 1, np.array([0, n0 + n1], dtype=np.int64)
    res, _c = h.results(with_consensus=False)
    return res[0]


_expected = {}


def _oracle(O, c):
    """(consensus, (score, r_st, r_en, q_st, q_en)) of a case: computed once, shared by the modes"""
    if (c.group, c.name) not in _expected:
        _expected[(c.group, c.name)] = (O.zero_repeats(*c.pair()), O.zero_local(c.d0, c.d1))
    return _expected[(c.group, c.name)]


def _check_group(O, monkeypatch, group, mode):
    from c3poa_amd import _lib
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("C3_FULL_RESULTS", "1")
    compared = refused = 0
    with _handle() as h:
        for c in GROUPS[group]:
            cons, (score, r_st, r_en, q_st, q_en) = _oracle(O, c)
            n0, n1 = len(c.d0), len(c.d1)
            got = h.zero_repeats(c.d0, c.q0, c.d1, c.q1, 0)
            rec = _record(h, n0, n1)
            assert got == cons, (c, mode, len(got), len(cons))
            if score >= ZC.MIN_SCORE and r_en > r_st and q_en > q_st:
                coords = (int(rec["sub_beg"][0]), int(rec["sub_end"][0]), int(rec["sub_beg"][1]) - n0, int(rec["sub_end"][1]) - n0)
                assert coords == (r_st, r_en, q_st, q_en), (c, mode, coords, (r_st, r_en, q_st, q_en))
                assert (int(rec["status"]), int(rec["n_sub"]), int(rec["cons_len"])) == (_lib.ST_OK, 0, len(cons)) and cons, (c, mode)
                compared += 1
            else:
                assert (int(rec["status"]), int(rec["n_sub"]), int(rec["cons_len"]), got) == (_lib.ST_NO_CONSENSUS, 0, 0, ""), (c, mode)
                refused += 1
    # a coordinate was compared for every pair the oracle rescues: all but the pairs built to be refused
    want_refused = sum(any(k == "refused" for k, _d in c.claims) for c in GROUPS[group])
    assert (compared, refused) == (len(GROUPS[group]) - want_refused, want_refused), (group, mode, compared, refused)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("group", ZC.SHORT_GROUPS)
def test_designed_pairs(O, monkeypatch, group, mode):
    """the groups that fit k_zero, on k_zero and forced to k_zero_long with checkpoints every 256 rows, every row, every 7 rows
    (limits: the pair of 4097 columns runs on k_zero_long in every mode -- k_zero would refuse it)"""
    _check_group(O, monkeypatch, group, mode)


@pytest.mark.parametrize("mode", ["long", "long_k1", "long_k7"])
@pytest.mark.parametrize("group", ZC.LONG_GROUPS)
def test_designed_pairs_long(O, monkeypatch, group, mode):
    """the groups built for the stripe seam 512 | 513, the sweep seam 2048 | 2049 and the checkpoint row 256"""
    _check_group(O, monkeypatch, group, mode)


# ---- more reads than workgroups ----------------------------------------------------------------------------------------------
QUEUE_N = 640
_queue = {}


def _queue_batch(O):
    """the queue batch and the oracle's answer to it: computed once"""
    if not _queue:
        reads, strands = ZC.queue(QUEUE_N)
        ores, ocons = O.process_batch(SP, reads, strands, threads=8)
        pieces = [(o.front_end, len(r[0]) - o.tail_beg) for o, r in zip(ores, reads)
                  if o.n_sub == 0 and o.has_front and o.has_tail and o.front_end > 0 and o.tail_beg < len(r[0])]
        _queue[0] = (reads, strands, ores, ocons, pieces)
    return _queue[0]


def _run_batch(h, reads, strands):
    h.set_splints([SP])
    h.upload([r[0] for r in reads], [r[1] for r in reads], strands)
    h.run()
    res, cons = h.results()
    return [int(x) for x in res["status"]], [int(x) for x in res["n_sub"]], cons, h.timing()["cells_poa"]


def _assert_queue(got, ores, ocons):
    st, ns, cons, cells = got
    for i, o in enumerate(ores):
        assert (st[i], ns[i]) == (o.status, o.n_sub), i
        assert cons[i] == ocons[i], i
    assert cells == sum(o.cells_poa for o in ores)


def test_queue_reuses_k_zero_blocks(O):
    """more zero-repeat reads than run_zero launches workgroups (min(reads, 512)): a workgroup takes a second read over the LDS
    rows and direction bytes of its first, under another row stride.  Twice on one handle, then on poisoned memory."""
    reads, strands, ores, ocons, pieces = _queue_batch(O)
    assert all(f <= ZC.ZW and f * t <= (16 << 20) for f, t in pieces)              # all of them are k_zero's
    assert len(pieces) > ZC.ZERO_GRID_CAP, len(pieces)
    assert sum(o.status == 0 and o.n_sub == 0 for o in ores) >= 300 and sum(o.status == 3 for o in ores) >= 150
    with _handle(poison=False) as h:
        first = _run_batch(h, reads, strands)
        again = _run_batch(h, reads, strands)
    with _handle() as h:
        poisoned = _run_batch(h, reads, strands)
    _assert_queue(first, ores, ocons)
    assert again == first and poisoned == first


def _cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch brings a HIP runtime of its
    own, which finds no device in a process where the library's runtime is already at work"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         stdout=subprocess.PIPE, timeout=120, check=True).stdout
    cus = int(out.split()[-1])
    assert 1 <= cus <= 4096, cus
    return cus


def _zl_total(n0, n1, K):
    """c3_zl_layout(n0, n1, K).total (c3_args.h)"""
    dirs = (n1 + K - 1) // K * (n0 + 1) * 8
    car = (dirs + min(n1, K) * (n0 + 1) + 15) & ~15
    return (car + n1 * 12 + 255) & ~255


def test_queue_reuses_k_zero_long_slots(O, monkeypatch):
    """the same queue forced to k_zero_long with a checkpoint on every row: run_zero gives it min(reads, 2 * CUs, budget / largest
    slot) workgroups, fewer than reads, so a workgroup reuses its checkpoints, direction block and row carries"""
    reads, strands, ores, ocons, pieces = _queue_batch(O)
    cus = _cu_count()
    smax = max(_zl_total(f, t, 1) for f, t in pieces)
    slots = min(len(pieces), 2 * cus, max(1, ZC.ZL_BUDGET // smax))
    print("queue forced long: %d reads, %d CUs, largest slot %d bytes, %d slots" % (len(pieces), cus, smax, slots))
    assert len(pieces) > slots
    monkeypatch.setenv("C3_DEBUG_ZERO_LONG", "1")
    monkeypatch.setenv("C3_DEBUG_ZERO_K", "1")
    with _handle(poison=False) as h:
        first = _run_batch(h, reads, strands)
        again = _run_batch(h, reads, strands)
    with _handle() as h:
        poisoned = _run_batch(h, reads, strands)
    _assert_queue(first, ores, ocons)
    assert again == first and poisoned == first

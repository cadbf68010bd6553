"""k_qv at its guards (qv_edge_cases.py): band steps 0 .. 4 with the odd-step fetch, rows cut at n + 64 and the last direction
word's flush, a best cell of (0, 0), equal best cells across rows and lanes, paths along the band edges, letters outside
ACGT and every quality byte, the LDS / global switch of the support array at 8192 columns -- stand-alone on a reused handle and
in a batch whose workgroups mix both homes -- and the exact values of the counters.  The stand-alone results must equal
the host statement c3_consensus_qv_host and, on the small cases, the Python restatement of include/c3poa.h directly;
test_qv_edges_host.py shows that every case reaches the code it names.  The handles poison fresh device memory
(C3_DEBUG_POISON): a direction word or support slot nobody wrote does not read as zero."""
import os

import numpy as np
import pytest

import qv_edge_cases as QC
import test_qv_edges_host as EH
from c3poa_amd import _lib, synth
from test_gpu_qv import _pieces_of

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1
# long inserts: the consensus (insert + splint) is above the 8192 columns k_qv holds in LDS; the other fields are cfgL's
LONG_INSERT = 8400
LONG_SHAPE = dict(reads=6, seed=61, insert=LONG_INSERT, n_lo=2, n_hi=3, k0=108, k1=108, mdist=500)


@pytest.fixture(scope="module")
def poison():
    keep = os.environ.get("C3_DEBUG_POISON")
    os.environ["C3_DEBUG_POISON"] = "1"
    yield
    os.environ.pop("C3_DEBUG_POISON", None)
    if keep is not None:
        os.environ["C3_DEBUG_POISON"] = keep


@pytest.fixture(scope="module")
def h(poison):
    hd = _lib.Handle()
    hd.set_splints([SP])
    yield hd
    hd.close()


_host = {}


def _host_qv(case):
    """the host statement's answer to a whole case: computed once"""
    name, cons, pieces, _small = case
    if name not in _host:
        _host[name] = _lib.consensus_qv_host(cons, QC.lib_pieces(pieces))
    return _host[name]


@pytest.mark.parametrize("case", QC.CASES, ids=[c[0] for c in QC.CASES])
def test_device_equals_host_and_restatement(h, case):
    name, cons, pieces, small = case
    lp = QC.lib_pieces(pieces)
    got = h.consensus_qv(cons, lp)
    assert got == _host_qv(case)
    if small:
        assert got == EH._restated(case)[0]
    modes = sorted({p[2] for p in lp})
    if len(modes) > 1:                                           # one mode at a time: no sum hides a piece behind the clamp
        for md in modes:
            sub = [p for p in lp if p[2] == md]
            assert h.consensus_qv(cons, sub) == _lib.consensus_qv_host(cons, sub), md
    if name == "nothing_matches":
        assert got == "!" * len(cons)


def test_reused_handle(poison):
    """the whole list on one handle forwards, then backwards (every case after a larger one: the direction slot, the LDS and the
    global slot hold what the case before left), then tiny cases straight after the 8209-column one"""
    by_name = {c[0]: c for c in QC.CASES}
    hd = _lib.Handle()
    try:
        fwd = [hd.consensus_qv(c[1], QC.lib_pieces(c[2])) for c in QC.CASES]
        bwd = [hd.consensus_qv(c[1], QC.lib_pieces(c[2])) for c in reversed(QC.CASES)][::-1]
        assert fwd == [_host_qv(c) for c in QC.CASES]
        assert bwd == fwd
        for name in ("skew_1_1_exact", "nothing_matches", "seam_7", "seam_9", "tie_two_rows_two_lanes", "band_ride_0"):
            big, c = by_name["switch_8209"], by_name[name]
            assert hd.consensus_qv(big[1], QC.lib_pieces(big[2])) == _host_qv(big)
            assert hd.consensus_qv(c[1], QC.lib_pieces(c[2])) == _host_qv(c), name
    finally:
        hd.close()


# ---- the batch path ----------------------------------------------------------------------------------------------------------
def _mixed_recs():
    """ten cfg1 reads with six long-insert reads in between, none of them first"""
    short = list(synth.generate("cfg1", n_reads=10))
    long_ = list(synth.generate(LONG_SHAPE))
    recs = []
    for k, r in enumerate(short):
        recs.append(r)
        if k % 2 == 0 and long_:
            recs.append(long_.pop(0))
    return recs + long_


def _run_qv(h, recs):
    h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    h.run(qv=True)
    res, cons, qv = h.results(qv=True)
    return res, cons, qv, h.qv_timing()


def _expected_counters(recs, res, cons):
    """(n_reads, n_pieces, n_skipped, band_cells) of k_qv as they follow from the records: a piece is a non-empty subread, tail
    or front piece of a read with a consensus; a mode-0 piece beyond the skew limit is skipped, every other one is aligned over
    rows + 1 band rows (row 0 included), rows = m in mode 0 and min(m, n + 64) in modes 1 / 2"""
    n_reads = n_pieces = n_skipped = cells = 0
    for i, r in enumerate(recs):
        if res[i]["status"] != _lib.ST_OK or not cons[i]:
            continue
        n_reads += 1
        n = len(cons[i])
        ps = _pieces_of(res[i], r[1], r[2], cons[i])
        subs = sum(1 for b, e in zip(res[i]["sub_beg"][:res[i]["n_sub"]], res[i]["sub_end"][:res[i]["n_sub"]]) if e > b)
        n_skipped += subs - sum(1 for p in ps if p[2] == 0)
        n_pieces += len(ps)
        cells += sum((QC.rows_of(n, len(s), md) + 1) * 128 for s, _q, md in ps)
    return n_reads, n_pieces, n_skipped, cells


def _check_batch(recs, res, cons, qv, t):
    for i, r in enumerate(recs):
        if res[i]["status"] != _lib.ST_OK or not cons[i]:
            assert qv[i] == ""
            continue
        assert qv[i] == _lib.consensus_qv_host(cons[i], _pieces_of(res[i], r[1], r[2], cons[i])), i
    n_reads, n_pieces, n_skipped, cells = _expected_counters(recs, res, cons)
    print("qv counters: %s; expected reads %d pieces %d skipped %d cells %d" % (t, n_reads, n_pieces, n_skipped, cells))
    assert (t["n_reads"], t["n_pieces"], t["n_skipped"], t["band_cells"]) == (n_reads, n_pieces, n_skipped, cells)
    assert 0 <= t["edge_hits"] <= t["n_pieces"]
    return n_reads


def test_batch_mixes_lds_and_global_support(h):
    """consensuses above and below 8192 columns in one launch: workgroups past the first use their own global slot (S and the
    codes behind all the S slots), their neighbours LDS"""
    recs = _mixed_recs()
    assert len(recs) == 16 and len(recs[0][1]) < 6000 and max(len(r[1]) for r in recs) > 2 * LONG_INSERT
    res, cons, qv, t = _run_qv(h, recs)
    ok = [i for i in range(len(recs)) if res[i]["status"] == _lib.ST_OK and cons[i]]
    print("statuses %s cons_len %s" % ([int(s) for s in res["status"]], [int(c) for c in res["cons_len"]]))
    _check_batch(recs, res, cons, qv, t)
    assert sum(1 for i in ok if res[i]["cons_len"] > 8192) >= 2           # the global slots really ran, in more than one workgroup
    assert sum(1 for i in ok if res[i]["cons_len"] <= 8192) >= 2
    again = _run_qv(h, recs)                                              # the same slots a second time
    assert again[2] == qv


def test_batch_counters_cfg2(h):
    recs = list(synth.generate("cfg2", n_reads=64))
    res, cons, qv, t = _run_qv(h, recs)
    assert _check_batch(recs, res, cons, qv, t) > 32

"""The edge cases of k_qv (qv_edge_cases.py) on the CPU: the host statement c3_consensus_qv_host against the Python restatement
of include/c3poa.h on every small case, and every claim of a case -- band steps, rows past n + 64, end cells, equal maxima,
band-edge touches, flush positions, quality bytes -- asserted on the restatement's own alignment, so that
test_gpu_qv_edges.py can rely on each case reaching the code it names.  CPU only."""
import pytest

import qv_edge_cases as QC
from c3poa_amd import _lib
from test_qv_host import spec_qv

SMALL = [c for c in QC.CASES if c[3]]
_spec = {}


def _restated(case):
    """(QV string, [info per piece]) of the restatement: computed once per case"""
    name, cons, pieces, _small = case
    if name not in _spec:
        infos = []
        _spec[name] = (spec_qv(cons, pieces, infos), infos)
    return _spec[name]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_host_equals_restatement_and_claims_hold(case):
    name, cons, pieces, _small = case
    want, infos = _restated(case)
    assert _lib.consensus_qv_host(cons, QC.lib_pieces(pieces)) == want
    claims = QC.CLAIMS[name]
    n = len(cons)
    if "d" in claims:
        for (seq, _q, mode), info in zip(pieces, infos):
            if mode == 0:
                assert QC.d_set(n, len(seq)) == claims["d"] and info["d"] == claims["d"]
    if "over" in claims:
        assert all((len(seq) > n + 64) == claims["over"] for seq, _q, _m in pieces)
    if "rows7" in claims:
        assert all(QC.rows_of(n, len(seq), mode) & 7 == claims["rows7"] for seq, _q, mode in pieces)
    if "end" in claims:
        assert [info["end"] for info in infos] == claims["end"]
    if "maxima" in claims:
        for info, cells in zip(infos, claims["maxima"]):
            assert len(cells) >= 2 and info["maxima"] == cells and info["end"] == min(cells)
    if "edges" in claims:
        assert [(info["edge0"], info["edge127"]) for info in infos] == claims["edges"]
    if "quals" in claims:
        assert all(claims["quals"] <= set(map(ord, q)) for _s, q, _m in pieces)


def test_case_list_covers_what_it_names():
    """the list as a whole: every band step 0 .. 4, both edges, flushes at rows & 7 of 0, 1 and 7, rows cut at n + 64, a piece
    that matches nothing, three kinds of tie, and the four lengths around the LDS limit"""
    names = [c[0] for c in QC.CASES]
    assert len(set(names)) == len(names)
    cl = QC.CLAIMS
    assert set().union(*(c["d"] for c in cl.values() if "d" in c)) == {0, 1, 2, 3, 4}
    assert {frozenset(d) for _nm, d in QC.SKEW} >= {frozenset(s) for s in ({4}, {3, 4}, {2, 3}, {2}, {1, 2}, {0, 1}, {1})}
    assert any(c.get("over") for c in cl.values()) and {c["rows7"] for c in cl.values() if "rows7" in c} >= {0, 1, 7}
    edges = [e for c in cl.values() for e in c.get("edges", [])]
    assert (True, False) in edges and (False, True) in edges
    assert (0, 0) in cl["nothing_matches"]["end"]
    ties = [c["maxima"][0] for c in cl.values() if "maxima" in c]
    assert any(a[0] != b[0] and a[1] - a[0] == b[1] - b[0] for a, b in ties)          # two rows, one diagonal (one lane)
    assert any(a[0] == b[0] for a, b in ties)                                         # one row, two lanes
    assert any(a[0] < b[0] and (a[1] - a[0] + 64) // 2 != (b[1] - b[0] + 64) // 2 for a, b in ties)   # two rows, two lanes
    assert sorted(len(c[1]) for c in QC.CASES if not c[3]) == [8191, 8192, 8193, 8209]
    for _name, cons, pieces, small in QC.CASES:
        if not small:
            assert sorted(md for _s, _q, md in pieces) == [0, 1, 2]
    # the restatement's budget: about 3 M band cells over the small cases
    assert QC.SMALL_CELLS < 3_500_000


def test_nothing_matches_is_all_zero():
    _name, cons, pieces, _small = next(c for c in QC.CASES if c[0] == "nothing_matches")
    assert _lib.consensus_qv_host(cons, QC.lib_pieces(pieces)) == "!" * len(cons)


def test_two_row_tie_covers_40_columns():
    """row 40 wins over row 43: 40 columns are covered, the rest get 0"""
    _name, cons, pieces, _small = next(c for c in QC.CASES if c[0] == "tie_two_rows_one_lane")
    out = _lib.consensus_qv_host(cons, QC.lib_pieces(pieces))
    assert out[40:] == "!" * (len(cons) - 40)
    assert out[:40] == "".join(chr(33 + min(60, ord(c) - 33)) for c in pieces[0][1][:40])

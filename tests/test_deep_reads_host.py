"""The deep-read cases of tests/deep_read_cases.py on the CPU oracle: every case has the shape it exists for.  A change of the
generator, of a seed or of the oracle that hollows a case out -- a subread lost, a graph without many-predecessor rows, a
ladder whose node stays below its degree, a cap verdict that moved -- fails here instead of leaving
tests/test_gpu_deep_reads.py to compare something easier.  No GPU."""
import collections

import pytest

import deep_read_cases as D


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.mark.parametrize("read", D.sweep_reads(), ids=lambda r: r.name)
def test_depth_sweep_keeps_every_subread_and_has_many_predecessor_rows(read):
    rec, cons, stats, _ = D.oracle(read, rowstats=True)
    assert len(read.seq) <= 65000                                      # 120 x (284 + 250) is the longest
    assert rec["status"] == D.ST_OK and cons
    assert rec["n_sub"] == read.built and rec["n_peaks"] == read.built + 1, (rec["n_sub"], rec["n_peaks"])
    assert rec["has_front"] and rec["has_tail"]
    rows, general, many, far = stats[0], stats[4], stats[24], stats[25]
    assert rows > 400 * read.built and general > 0.2 * rows, (rows, general)
    assert many >= 100, many                                            # rows with more than four predecessors
    if read.built == 250:
        assert many >= 10000 and far >= 50000, (many, far)


def test_the_250_subread_read_has_one_window_of_252_layers():
    read = D.depth_read(250)
    rec, _, _, wins = D.oracle(read, capture=True)
    per = collections.Counter(w["win"] for w in wins)
    assert max(per.values()) == rec["n_sub"] + 2 == D.MAX_SUB + 2, per
    assert max(w["n"] for w in wins) >= 900                             # nodes of the window graph: four per backbone base


# the oracle's verdicts on the cap reads: (status, n_peaks, n_sub).  It has neither cap: its LIMIT is the status the product
# documents (include/c3poa.h), kept in step with it, and n_peaks = 0 beyond 255 peaks is c3_call_peaks' documented answer.
CAP_VERDICTS = {
    "sub250": (D.ST_OK, 251, 250),
    "sub251": (D.ST_LIMIT, 252, 251),
    "sub254": (D.ST_LIMIT, 255, 254),
    "peaks255": (D.ST_OK, 255, 248),
    "peaks256": (D.ST_LIMIT, 0, 0),
    "clean250": (D.ST_OK, 251, 250),
}


@pytest.mark.parametrize("name", list(D.CAP_SHAPES))
def test_cap_reads_get_the_pinned_verdicts(name):
    read = D.cap_read(name)
    units, odd, _err, _seed = D.CAP_SHAPES[name]
    rec, cons, _, _ = D.oracle(read)
    assert (rec["status"], rec["n_peaks"], rec["n_sub"]) == CAP_VERDICTS[name]
    assert bool(cons) == (rec["status"] == D.ST_OK)
    if name != "peaks256":
        assert rec["n_peaks"] == units + 1 and rec["n_sub"] == units - odd == read.built
    assert (rec["n_sub"] > D.MAX_SUB or units + 1 > D.MAX_KEPT_PEAKS) == (rec["status"] == D.ST_LIMIT)
    assert len(read.seq) <= 62500


def test_neighbours_are_ordinary_reads_under_the_deep_reads_cutoff():
    for read, strand in D.neighbours(8):
        rec, cons, _, _ = D.oracle(read, strand)
        assert (rec["status"], rec["n_sub"], rec["n_peaks"]) == (D.ST_OK, 3, 4) and len(cons) > 1400


@pytest.mark.parametrize("kind,N", list(D.LADDERS))
def test_ladders_reach_their_degree(O, kind, N):
    subs, quals = D.ladder(kind, N)
    assert len(subs) == N + 3 <= D.MAX_SUB
    _, msa, _ = O.poa_msa(list(subs))
    deg = D.msa_degrees(msa)
    assert deg == D.LADDERS[(kind, N)], deg
    assert deg[0] >= 30 if kind == "in" else deg[1] >= 16
    for q in ("mixed", "equal"):
        s2, q2 = D.ladder(kind, N, q)
        assert s2 == subs and len(O.determine_consensus(list(s2), list(q2))) > 250
    assert len(set(D.ladder(kind, N, "equal")[1][0])) == 1 and len(set(quals[0])) > 20


def test_quality_variants_and_the_filter_verdict():
    """all '!' leaves the -q 5 filter of the polish nothing: NO_CONSENSUS with all 128 subreads kept"""
    got = {r.name: D.oracle(r) for r in D.quality_variants()}
    assert {k: (v[0]["status"], v[0]["n_sub"]) for k, v in got.items()} == {
        "depth128_q93": (D.ST_OK, 128), "depth128_q0": (D.ST_NO_CONSENSUS, 128), "depth128_q0_q93": (D.ST_OK, 128),
        "depth250_q93": (D.ST_OK, 250)}
    assert all(bool(v[1]) == (k != "depth128_q0") for k, v in got.items())

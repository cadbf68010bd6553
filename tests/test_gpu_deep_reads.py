"""The consensus path on deep reads (tests/deep_read_cases.py): 31 to 250 kept subreads, both caps through the batch path, POA
nodes of 30 and more predecessors and of 16 and more successors, extreme qualities at depth, a deep read among shallow ones, the
forced second passes at depth, k_qv on 252 pieces and three-digit subread indices through the CLI's two emit paths.  Every
comparison with the CPU oracle is exact: status, consensus bytes, n_peaks, n_sub, the used prefix of peaks / sub_beg / sub_end,
the dangling-piece fields and the counted cells of both alignment stages.  tests/test_deep_reads_host.py asserts on the oracle
that every case has the shape it claims.  All GPU runs poison fresh device memory (C3_DEBUG_POISON).

Seconds per test on an MI355X (one wave per read: the 250-subread read is 2.1e5 serial POA rows and one 252-layer window) are
recorded in DESIGN.md 3."""
import os

import numpy as np
import pytest

from c3poa_amd import _lib, synth

import deep_read_cases as D

pytestmark = pytest.mark.gpu

_HOOKS = ("C3_DEBUG_WIN_CHAIN", "C3_DEBUG_POISON", "C3_DEBUG_BAND", "C3_DEBUG_HCAP_DIV", "C3_DEBUG_WIN_LDS", "C3_DEBUG_WIN_LCAP",
          "C3_DEBUG_POA_SMALL", "C3_DEBUG_POA_NO2COL", "C3_DEBUG_POA32", "C3_DEBUG_POA_WIDE", "C3_DEBUG_POA_PAIR", "C3_DEBUG_POA_RBSPAN")
_FIELDS = ("status", "n_peaks", "n_sub", "has_front", "has_tail", "front_end", "tail_beg", "cons_len", "draft_len", "n_win")
_alone = {}


def _gpu(items, mdist, env=None, qv=False, **cfg):
    """one batch on a fresh handle.  items: (read, strand) pairs; the splint table is the splints of the batch in order of first
    use.  returns (records as dicts of the specified fields, consensi, counters[, QV strings])"""
    splints = []
    for r, _ in items:
        if r.splint not in splints:
            splints.append(r.splint)
    keep = {k: os.environ.get(k) for k in _HOOKS}
    for k in _HOOKS:
        os.environ.pop(k, None)
    os.environ["C3_DEBUG_POISON"] = "1"
    os.environ.update(env or {})
    try:
        h = _lib.Handle(mdistcutoff=mdist, **cfg)
        try:
            h.set_splints(splints)
            h.upload([r.seq for r, _ in items], [r.qual for r, _ in items], [st for _, st in items],
                     np.array([splints.index(r.splint) for r, _ in items], dtype=np.int16))
            h.run(qv=qv)
            out = h.results(qv=True) if qv else h.results()
            t = h.timing()
        finally:
            h.close()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    recs = []
    for r in out[0]:
        d = {f: int(r[f]) for f in _FIELDS}
        # the arrays are defined up to n_peaks / n_sub only (include/c3poa.h)
        d["peaks"] = tuple(int(x) for x in r["peaks"][:max(0, min(d["n_peaks"], 256))])
        d["sub_beg"] = tuple(int(x) for x in r["sub_beg"][:max(0, min(d["n_sub"], 256))])
        d["sub_end"] = tuple(int(x) for x in r["sub_end"][:max(0, min(d["n_sub"], 256))])
        recs.append(d)
    return (recs, list(out[1]), t) + ((list(out[2]),) if qv else ())


def _equals_oracle(rec, cons, read, strand="+"):
    """one device record against the oracle's.  A read the product refuses for its size (C3_ST_LIMIT) has no consensus; of its
    other fields include/c3poa.h specifies n_peaks = 0 beyond 255 peaks (c3_call_peaks) and nothing else: n_sub of such a read,
    and n_peaks / n_sub / the slices of a read with more than 250 kept subreads, are left unspecified and are not compared
    (only that they index inside the record's arrays)."""
    o, ocons, _, _ = D.oracle(read, strand)
    assert rec["status"] == o["status"], (read.name, rec["status"], o["status"])
    assert cons == ocons, read.name
    if o["status"] == D.ST_LIMIT:
        assert cons == "" and rec["cons_len"] == 0
        assert 0 <= rec["n_peaks"] <= 256 and 0 <= rec["n_sub"] <= 256, (read.name, rec["n_peaks"], rec["n_sub"])
        if o["n_peaks"] == 0:
            assert rec["n_peaks"] == 0, (read.name, rec["n_peaks"])
        return o
    for f in ("n_peaks", "n_sub", "peaks", "sub_beg", "sub_end", "has_front", "has_tail", "front_end", "tail_beg"):
        assert rec[f] == o[f], (read.name, f, rec[f], o[f])
    assert rec["cons_len"] == len(ocons)
    return o


def _check(items, mdist, env=None, cells=True, **cfg):
    """a batch on the device, read by read against the oracle; the counted cells of both alignment stages against the oracle's
    sums.  returns (records, consensi, counters)"""
    recs, cons, t = _gpu(items, mdist, env, **cfg)
    os_ = [_equals_oracle(recs[i], cons[i], r, st) for i, (r, st) in enumerate(items)]
    if cells:
        for k in ("cells_poa", "cells_polish"):
            want = sum(o[k] for o in os_)
            assert t[k] == want, (k, t[k], want)
    return recs, cons, t


def _run_alone(read, strand="+"):
    """the read as a batch of its own, checked against the oracle, once per process"""
    if read.name not in _alone:
        recs, cons, t = _check([(read, strand)], read.mdist)
        _alone[read.name] = (recs[0], cons[0], t)
    return _alone[read.name]


def _no_redo_lost_a_read(recs, t):
    """the redo counters are consistent with every read having a result: a read redone by a later pass is counted once per
    pass at the most, and no read was left with C3_ST_LIMIT by a pass that ran out of room"""
    assert all(r["status"] != D.ST_LIMIT for r in recs), [r["status"] for r in recs]
    assert 0 <= t["n_poa_redo16"] <= t["n_poa_redo"] <= 2 * len(recs), (t["n_poa_redo"], t["n_poa_redo16"])
    assert 0 <= t["n_win_redo"] <= t["n_windows"] == sum(r["n_win"] for r in recs), (t["n_win_redo"], t["n_windows"])


# ---- 1: the depth sweep
@pytest.mark.parametrize("read", D.sweep_reads(), ids=lambda r: r.name)
def test_depth_sweep(read):
    rec, cons, t = _run_alone(read)
    assert rec["status"] == D.ST_OK and rec["n_sub"] == read.built and cons
    _no_redo_lost_a_read([rec], t)


# ---- 2: both caps, decided by k_peaks in a batch
def test_caps_in_one_batch_leave_the_neighbours_alone():
    """250 / 251 / 254 kept subreads, 255 / 256 peaks and the error-free 250 in one batch with two cfg1 reads, a neighbour first
    and one between the refused reads.  The refused reads carry C3_ST_LIMIT and no consensus, the admitted ones and the
    neighbours equal the oracle, and the neighbours equal themselves in a batch of their own."""
    nb = D.neighbours(2)
    caps = [(r, "+") for r in D.cap_reads()]
    items = [nb[0]] + caps[:3] + [nb[1]] + caps[3:]
    recs, cons, t = _check(items, 150)
    by_name = dict(zip(D.CAP_SHAPES, recs[1:4] + recs[5:]))
    assert [by_name[k]["status"] for k in D.CAP_SHAPES] == [D.ST_OK, D.ST_LIMIT, D.ST_LIMIT, D.ST_OK, D.ST_LIMIT, D.ST_OK]
    assert by_name["sub250"]["n_sub"] == D.MAX_SUB and by_name["peaks255"]["n_peaks"] == D.MAX_KEPT_PEAKS
    arecs, acons, _ = _check(list(nb), 150)
    assert [recs[0], recs[4]] == arecs and [cons[0], cons[4]] == acons
    a250 = _run_alone(D.depth_read(250))
    assert (by_name["sub250"], cons[1]) == a250[:2]
    assert t["n_poa_redo"] <= 2 * 5 and t["n_win_redo"] <= t["n_windows"]


# ---- 3: high-degree nodes by construction
@pytest.mark.parametrize("quals", ["mixed", "equal"])
@pytest.mark.parametrize("kind,N", list(D.LADDERS))
def test_ladders(kind, N, quals):
    """a node with 30 and more predecessors (in) or 16 and more successors (out) through determine_consensus: draft and
    polished consensus against the oracle's, and the MSA's degrees against the ones the oracle's MSA has"""
    from oracle import oracle_py as O
    subs, qs = D.ladder(kind, N, quals)
    want, wdraft, _cells = O.determine_consensus(list(subs), list(qs), return_draft=True)
    h = _lib.Handle()
    try:
        got, gdraft = h.determine_consensus(list(subs), list(qs), return_draft=True)
        _c, msa = h.poa_msa(list(subs), out_cons=True, out_msa=True) if quals == "mixed" else (None, None)
    finally:
        h.close()
    assert gdraft == wdraft and got == want and len(got) > 250
    if msa is not None:
        assert msa == O.poa_msa(list(subs))[1]
        assert D.msa_degrees(msa) == D.LADDERS[(kind, N)]


# ---- 4: extreme qualities at depth
@pytest.mark.parametrize("read", D.quality_variants(), ids=lambda r: r.name)
def test_quality_extremes_at_depth(read):
    """window edge weights of up to 2 * 93 * 130 at '~' on the 128-subread read and of 2 * 93 * 252, beyond 16 bits, on the
    250-subread read; at '!' the -q 5 filter leaves nothing and the verdict is the oracle's (NO_CONSENSUS, every subread kept)"""
    rec, cons, _ = _run_alone(read)
    assert rec["n_sub"] == read.built and bool(cons) == (read.name != "depth128_q0")


# ---- 5: a deep read among shallow ones
def test_deep_read_among_shallow_reads():
    """the 250-subread read first and last in a batch with eight cfg1 reads: every read equals the oracle and its result alone
    (the shallow ones as a batch of their own); the deep read once more with one POA slot and one window slot"""
    deep = (D.depth_read(250), "+")
    nb = list(D.neighbours(8))
    alone = _run_alone(deep[0])
    nrecs, ncons, _ = _check(nb, 150)
    for items, at in (([deep] + nb, 0), (nb + [deep], 8)):
        recs, cons, t = _check(items, 150)
        assert (recs[at], cons[at]) == alone[:2], at
        assert recs[:at] + recs[at + 1:] == nrecs and cons[:at] + cons[at + 1:] == ncons, at
        _no_redo_lost_a_read(recs, t)
    recs, cons, t = _check([deep], 150, slots_poa=1, slots_win=1)
    assert (recs[0], cons[0]) == alone[:2]
    _no_redo_lost_a_read(recs, t)


# ---- 6: the forced paths on the 128-subread read
@pytest.mark.parametrize("env,counter", [({"C3_DEBUG_POA_SMALL": "64"}, "n_poa_redo"), ({"C3_DEBUG_POA_NO2COL": "1"}, None),
                                         ({"C3_DEBUG_HCAP_DIV": "100000"}, "n_win_redo"), ({"C3_DEBUG_WIN_CHAIN": "0"}, None),
                                         ({"C3_DEBUG_BAND": "off"}, None), ({"C3_DEBUG_BAND": "verify"}, None)],
                         ids=["poa_small", "poa_no2col", "hcap_div", "win_chain_off", "band_off", "band_verify"])
def test_forced_paths_at_depth(env, counter):
    read = D.depth_read(128)
    alone = _run_alone(read)
    recs, cons, t = _check([(read, "+")], read.mdist, env)
    assert (recs[0], cons[0]) == alone[:2]
    assert t["n_band_mismatch"] == 0
    if counter == "n_poa_redo":
        assert t["n_poa_redo"] - t["n_poa_redo16"] == 1              # the one read, redone by the full-size pass
    elif counter == "n_win_redo":
        assert t["n_win_redo"] == t["n_windows"] > 0                 # every window through the second launch
    else:
        assert t["n_poa_redo"] == alone[2]["n_poa_redo"]
    if env.get("C3_DEBUG_BAND") == "off":
        assert t["n_band_layers"] == 0 and t["n_band_fallback"] == 0


# ---- 7: k_qv on 252 pieces; three-digit subread indices through both emit paths
def test_consensus_qv_of_252_pieces():
    import test_gpu_qv as QV
    read = D.depth_read(250)
    recs, cons, _t, qv = _gpu([(read, "+")], read.mdist, qv=True)
    alone = _run_alone(read)
    assert (recs[0], cons[0]) == alone[:2]
    pieces = QV._pieces_of(dict(recs[0], sub_beg=recs[0]["sub_beg"], sub_end=recs[0]["sub_end"]), read.seq, read.qual, cons[0])
    assert len(pieces) == D.MAX_SUB + 2 == 252                       # C3_QV_MAX_PIECES
    assert len(qv[0]) == len(cons[0]) and qv[0] == _lib.consensus_qv_host(cons[0], pieces)


def test_cli_emit_paths_agree_on_three_digit_subread_indices(tmp_path):
    import C3POa
    from c3poa_amd.seqio import fastx_read
    rng = np.random.default_rng(20275)
    deep = D.depth_read(250)
    recs = [("shallow0",) + D.concatemer(rng, D.SPLINT, 600, 3, 110, 110), ("deep250", deep.seq, deep.qual),
            ("shallow1",) + D.concatemer(rng, D.SPLINT, 600, 4, 110, 110)]
    trees = {}
    for emit in ("host", "gpu"):
        out = str(tmp_path / emit / "out")
        os.makedirs(out + "/tmp")
        fq, fa = str(tmp_path / emit / "reads.fastq"), str(tmp_path / emit / "splint.fasta")
        with open(fq, "w") as fh:
            for r in recs:
                fh.write("@%s\n%s\n+\n%s\n" % r)
        open(fa, "w").write(">Deep\n%s\n" % D.SPLINT)
        synth.write_psl(out + "/tmp/splint_to_read_alignments.psl", [r + ("+", "") for r in recs], splint_name="Deep")
        C3POa.main(C3POa.parse_args(["-r", fq, "-s", fa, "-o", out, "-g", "16", "-d", "150"] + (["--emit", "gpu"] if emit == "gpu" else [])))
        trees[emit] = {f: open(os.path.join(out, "Deep", f), "rb").read() for f in sorted(os.listdir(os.path.join(out, "Deep")))}
    assert sorted(trees["host"]) == ["R2C2_Consensus.fasta", "R2C2_Subreads.fastq"]
    assert trees["gpu"] == trees["host"]
    cons = list(fastx_read(str(tmp_path / "host" / "out" / "Deep" / "R2C2_Consensus.fasta")))
    subs = list(fastx_read(str(tmp_path / "host" / "out" / "Deep" / "R2C2_Subreads.fastq")))
    assert len(cons) == 3 and dict((r[0].split("_")[0], r[1]) for r in cons)["deep250"] == _run_alone(deep)[1]
    deep_subs = [r[0] for r in subs if r[0].startswith("deep250_")]
    # kept subreads _1 .. _250, the front piece _0 and the tail piece _251
    assert sorted(int(n.split("_")[-1]) for n in deep_subs) == list(range(D.MAX_SUB + 2))

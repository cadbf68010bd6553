"""Per-base consensus QVs on the GPU (k_qv): the stand-alone entry point and the batch path against the host statement
c3_consensus_qv_host byte for byte, the QV fetch rules, the overlap of fetch_qv with the next batch, the CLI's
--consensus-fastq output and a calibration sanity check on synthetic reads with known truth."""
import gzip
import os
import random

import numpy as np
import pytest

from c3poa_amd import _lib, synth
from c3poa_amd.seqio import fastx_read

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1


@pytest.fixture(scope="module")
def h():
    hd = _lib.Handle()
    hd.set_splints([SP])
    yield hd
    hd.close()


def _mutate(rng, s, rate):
    out = []
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(rng.choice("ACGT"))
        elif r < rate:
            out.append(c); out.append(rng.choice("ACGT"))
        else:
            out.append(c)
    return "".join(out) or "A"


def _seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _qual(rng, n):
    return "".join(chr(33 + rng.randrange(0, 94)) for _ in range(n))


@pytest.mark.parametrize("L", [1, 63, 64, 65, 127, 128, 129, 4096, 20000])
def test_standalone_equals_host(h, L):
    rng = random.Random(L)
    cons = _seq(rng, L)
    pieces = []
    for mode in (0, 1, 2):
        for _k in range(2):
            if mode == 0:
                s = _mutate(rng, cons, 0.12)
                while max(len(s), L) > 4 * min(len(s), L):
                    s = _mutate(rng, cons, 0.02)
            elif mode == 1:
                s = _mutate(rng, cons[:max(1, L - rng.randrange(0, L // 3 + 1))], 0.12)
            else:
                s = _mutate(rng, cons[rng.randrange(0, L // 3 + 1):], 0.12)
            pieces.append((s, _qual(rng, len(s)), mode))
    # a piece of exactly the length, identical, in every mode
    pieces += [(cons, _qual(rng, L), m) for m in (0, 1, 2)]
    assert h.consensus_qv(cons, pieces) == _lib.consensus_qv_host(cons, pieces)
    for m in (0, 1, 2):                                          # one mode at a time as well
        sub = [p for p in pieces if p[2] == m]
        assert h.consensus_qv(cons, sub) == _lib.consensus_qv_host(cons, sub)


def test_standalone_250_pieces_and_refusals(h):
    rng = random.Random(250)
    cons = _seq(rng, 700)
    pieces = [(_mutate(rng, cons, 0.1), None, 0) for _ in range(248)] + [(cons[:300], None, 1), (cons[400:], None, 2)]
    pieces = [(s, _qual(rng, len(s)), m) for s, _q, m in pieces]
    assert h.consensus_qv(cons, pieces) == _lib.consensus_qv_host(cons, pieces)
    ins = cons[:300] + _seq(rng, 200) + cons[300:]                 # an optimum that leaves the band
    p2 = [(ins, _qual(rng, len(ins)), 0), (ins, _qual(rng, len(ins)), 1)]
    assert h.consensus_qv(cons, p2) == _lib.consensus_qv_host(cons, p2)
    for cons_, pcs in [("", [("A", "I", 0)]), ("ACGT", [("", "", 0)]), ("ACGT", [("ACGT", "IIII", 5)]),
                       ("ACGT", [("ACGT", "IIII", 0)] * 253), ("A" * 40, [("ACG", "III", 0)])]:
        with pytest.raises(_lib.C3Error):
            h.consensus_qv(cons_, pcs)
        with pytest.raises(_lib.C3Error):
            _lib.consensus_qv_host(cons_, pcs)


def _zero_recs(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(900, 1600))
        a, b = int(rng.integers(100, L // 3)), int(rng.integers(2 * L // 3, L - 50))
        s, q, st, t = synth.make_zero_read(rng, SP, L, a, b)
        out.append(("zero%d" % k, s, q, st, t))
    return out


def _pieces_of(r, seq, qual, cons):
    """the support pieces of one record (include/c3poa.h), minus mode-0 pieces beyond the skew limit (the batch skips them)"""
    L, n = len(seq), len(cons)
    ps = [(seq[b:e], qual[b:e], 0) for b, e in zip(r["sub_beg"][:r["n_sub"]], r["sub_end"][:r["n_sub"]])
          if e > b and max(e - b, n) <= 4 * min(e - b, n)]
    if r["has_tail"] and r["tail_beg"] < L:
        ps.append((seq[r["tail_beg"]:], qual[r["tail_beg"]:], 1))
    if r["has_front"] and r["front_end"] > 0:
        ps.append((seq[:r["front_end"]], qual[:r["front_end"]], 2))
    return ps


@pytest.mark.parametrize("kind", ["cfg2", "zero", "cfgL"])
def test_batch_equals_host(h, kind):
    if kind == "zero":
        recs = _zero_recs(5, 48) + list(synth.generate("cfg1", n_reads=16))
    else:
        recs = list(synth.generate(kind, n_reads=64 if kind == "cfgL" else 512))
    h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    h.run()
    res0, cons0 = h.results()
    h.run(qv=True)
    res, cons, qv = h.results(qv=True)
    assert cons == cons0
    assert (res["status"] == res0["status"]).all() and (res["cons_len"] == res0["cons_len"]).all()
    t = h.qv_timing()
    n_ok = 0
    for i, r in enumerate(recs):
        if res[i]["status"] != _lib.ST_OK or not cons[i]:
            assert qv[i] == ""
            continue
        n_ok += 1
        assert len(qv[i]) == len(cons[i])
        assert qv[i] == _lib.consensus_qv_host(cons[i], _pieces_of(res[i], r[1], r[2], cons[i])), i
    assert n_ok > len(recs) // 2 and t["n_reads"] == n_ok and t["n_pieces"] > 0 and t["band_cells"] > 0
    if kind == "zero":
        assert any(res[i]["n_sub"] == 0 and res[i]["status"] == _lib.ST_OK for i in range(len(recs)))


def test_qv_fetch_refused_without_stage(h):
    recs = list(synth.generate("cfg1", n_reads=8))
    h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    with pytest.raises(_lib.C3Error):
        h.run(_lib.STAGE_QV)                                     # no polish in this call or before
    h.run()
    with pytest.raises(_lib.C3Error):
        h.results(qv=True)
    shape = h.results_snapshot()
    rb = _lib.ResultBuffers()
    with pytest.raises(_lib.C3Error):
        h.results_fetch_qv(rb, shape)
    rb2 = _lib.ResultBuffers()
    h.results_fetch(rb2, shape)                                  # the snapshot is still there for the plain fetch
    assert rb2.qv is None                                        # the QV buffer is only allocated when used
    h.run(_lib.STAGE_QV)                                         # polish ran earlier on this batch
    res2, cons2, qv2 = h.results(qv=True)
    assert all(len(a) == len(b) for a, b in zip(cons2, qv2))
    h.run(_lib.STAGE_POLISH)                                     # a rerun without QV: the QVs are stale
    with pytest.raises(_lib.C3Error):
        h.results(qv=True)


def test_fetch_qv_overlaps_next_batch(h):
    from concurrent.futures import ThreadPoolExecutor
    a = list(synth.generate("cfg2", n_reads=300))
    b = list(synth.generate("cfg2", n_reads=300, start=300))
    want = {}
    for k, recs in enumerate((a, b)):
        h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
        h.run(qv=True)
        want[k] = h.results(qv=True)
    pb = _lib.PinnedBatch("".join(r[1] for r in b).encode(), "".join(r[2] for r in b).encode(),
                          np.concatenate([[0], np.cumsum([len(r[1]) for r in b])]), "".join(r[3] for r in b))
    h.upload([r[1] for r in a], [r[2] for r in a], [r[3] for r in a])
    h.run(qv=True)
    shape = h.results_snapshot()
    h.stage_pinned(pb)
    rb = _lib.ResultBuffers(pinned=True)
    with ThreadPoolExecutor(1) as ex:
        fut = ex.submit(h.results_fetch_qv, rb, shape)           # copies batch a's snapshot ...
        h.commit()                                               # ... while batch b becomes resident and runs
        h.run(qv=True)
        got = fut.result()
    res, buf, coff, qv = got
    raw, qraw = buf.tobytes(), qv.tobytes()
    assert [raw[coff[i]:coff[i + 1]].decode() for i in range(len(a))] == want[0][1]
    assert [qraw[coff[i]:coff[i + 1]].decode() for i in range(len(a))] == want[0][2]
    assert h.results(qv=True)[2] == want[1][2]
    rb.close(); pb.close()


def _run_cli(tmp_path, recs, extra=()):
    import C3POa
    out = str(tmp_path / "out")
    os.makedirs(out + "/tmp")
    fq = str(tmp_path / "reads.fastq")
    with open(fq, "w") as fh:
        for r in recs:
            fh.write("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]))
    fa = str(tmp_path / "splint.fasta")
    open(fa, "w").write(">Splint1\n%s\n" % SP)
    synth.write_psl(out + "/tmp/splint_to_read_alignments.psl", recs)
    C3POa.main(C3POa.parse_args(["-r", fq, "-s", fa, "-o", out, "-g", "16"] + list(extra)))
    return out + "/Splint1/"


def test_cli_consensus_fastq(tmp_path):
    recs = list(synth.generate("cfg1", n_reads=40)) + _zero_recs(9, 6)
    plain = _run_cli(tmp_path / "a", recs)
    assert sorted(os.listdir(plain)) == ["R2C2_Consensus.fasta", "R2C2_Subreads.fastq"]
    withq = _run_cli(tmp_path / "b", recs, ["--consensus-fastq"])
    assert sorted(os.listdir(withq)) == ["R2C2_Consensus.fasta", "R2C2_Consensus.fastq", "R2C2_Subreads.fastq"]
    for f in ("R2C2_Consensus.fasta", "R2C2_Subreads.fastq"):
        assert open(plain + f, "rb").read() == open(withq + f, "rb").read()
    fa = list(fastx_read(withq + "R2C2_Consensus.fasta"))
    fq = list(fastx_read(withq + "R2C2_Consensus.fastq"))
    assert [(n, s) for n, s, _q in fq] == [(n, s) for n, s, _q in fa] and len(fq) > 30
    assert all(q is not None and len(q) == len(s) for _n, s, q in fq)
    gz = _run_cli(tmp_path / "c", recs, ["--consensus-fastq", "-co"])
    assert sorted(os.listdir(gz)) == ["R2C2_Consensus.fasta.gz", "R2C2_Consensus.fastq.gz", "R2C2_Subreads.fastq.gz"]
    assert gzip.open(gz + "R2C2_Consensus.fastq.gz").read() == open(withq + "R2C2_Consensus.fastq", "rb").read()


def _cigar_errors(cons, truth):
    """per consensus base: 1 when it is not a match in a unit-cost global alignment to the truth (substitution or
    insertion), from a plain edit-distance DP (small inputs)"""
    n, m = len(cons), len(truth)
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    D[:, 0] = np.arange(n + 1); D[0, :] = np.arange(m + 1)
    t = np.frombuffer(truth.encode(), dtype=np.uint8)
    for i in range(1, n + 1):
        sub = D[i - 1, :-1] + (t != ord(cons[i - 1]))
        row = np.minimum(sub, D[i - 1, 1:] + 1)
        x = np.concatenate(([i], row)) - np.arange(m + 1)
        D[i] = np.minimum.accumulate(x) + np.arange(m + 1)
    err = np.zeros(n, dtype=np.int8)
    i, j = n, m
    while i > 0:
        if j > 0 and D[i, j] == D[i - 1, j - 1] + (cons[i - 1] != truth[j - 1]):
            err[i - 1] = cons[i - 1] != truth[j - 1]; i -= 1; j -= 1
        elif D[i, j] == D[i - 1, j] + 1:
            err[i - 1] = 1; i -= 1
        else:
            j -= 1
    return err


def test_calibration_sanity(h):
    from c3poa_amd.seqio import revcomp
    recs = list(synth.generate("cfg1", n_reads=60, seed=77))
    h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    h.run(qv=True)
    res, cons, qv = h.results(qv=True)
    hi, lo = [0, 0], [0, 0]
    for i, r in enumerate(recs):
        if not cons[i]:
            continue
        truth = r[4]
        c = cons[i]
        # the consensus is in read orientation or reverse-complemented: take the better one
        best = min((_cigar_errors(c, t) for t in (truth, revcomp(truth))), key=lambda e: e.sum())
        q = np.frombuffer(qv[i].encode(), dtype=np.uint8) - 33
        hi[0] += int(best[q >= 40].sum()); hi[1] += int((q >= 40).sum())
        lo[0] += int(best[q < 20].sum()); lo[1] += int((q < 20).sum())
    assert hi[1] > 0 and lo[1] > 0
    assert hi[0] / hi[1] < lo[0] / lo[1]

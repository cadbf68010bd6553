"""Zero-repeat rescue of long dangling pieces (k_zero_long): parity with the oracle's zr_local at any piece length up
to the configured cap, routing between k_zero and k_zero_long, the zero_max_cells setting, the entry points and the CLI."""
import os
import types

import numpy as np
import pytest

from c3poa_amd import synth
from c3poa_amd.seqio import fastx_read, revcomp

pytestmark = pytest.mark.gpu

SP = synth.SPLINT1
MI = 1 << 20


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _zero_reads(seed, shapes, strand=None, err=True):
    """shapes: (insert_len, a, b) -> reads ins[a:] + splint + ins[:b]; returns [(seq, qual)], strands, truths"""
    rng = np.random.default_rng(seed)
    reads, strands, truths = [], [], []
    for L, a, b in shapes:
        s, q, st, t = synth.make_zero_read(rng, SP, L, a, b, err=err, strand=strand)
        reads.append((s, q)); strands.append(st); truths.append(t)
    return reads, strands, truths


def _gpu(reads, strands, **cfg):
    from c3poa_amd import _lib
    h = _lib.Handle(**cfg)
    h.set_splints([SP])
    h.upload([r[0] for r in reads], [r[1] for r in reads], strands)
    h.run()
    res, cons = h.results()
    cells = h.timing()["cells_poa"]
    h.close()
    return res, cons, cells


def _check(O, reads, strands, cap=16 * MI, **cfg):
    """GPU == oracle (status, n_sub, n_peaks, consensus bytes; counted cells); returns (gpu res, cons, oracle res)"""
    res, cons, cells = _gpu(reads, strands, zero_max_cells=cap, **cfg)
    P = O.default_params(zr_max_cells=cap, **({"zero": cfg["zero"]} if "zero" in cfg else {}))
    ores, ocons = O.process_batch(SP, reads, strands, params=P, threads=8)
    for i, o in enumerate(ores):
        assert (int(res[i]["status"]), int(res[i]["n_sub"]), int(res[i]["n_peaks"])) == (o.status, o.n_sub, o.n_peaks), i
        assert cons[i] == ocons[i], i
    if any(o.status == 0 for o in ores):
        assert cells == sum(o.cells_poa for o in ores)
    return res, cons, ores


def _pieces(o, read):
    return o.front_end, len(read[0]) - o.tail_beg


def test_default_cap_wide_front_matches_oracle(O):
    """d0 > 4096 columns within the default 16 Mi cells: k_zero cannot hold the row, k_zero_long rescues the read"""
    reads, strands, _t = _zero_reads(31, [(6000, 917, 3104), (6000, 1500, 2900), (5500, 900, 2600), (7000, 2400, 3300)],
                                     strand="+")
    res, cons, ores = _check(O, reads, strands)
    fronts = [_pieces(o, r) for o, r in zip(ores, reads)]
    assert all(f > 4096 and f * t <= 16 * MI for f, t in fronts), fronts
    assert [o.status for o in ores] == [0, 0, 0, 0]
    assert all(len(c) > 5000 for c in cons)


def test_raised_cap_long_pieces(O):
    """Handle(zero_max_cells=64 Mi / 128 Mi): 4-8 kb pieces on both strands, an error-free pair, 30 000 x 300 and
    300 x 30 000, a pair without overlap"""
    rng = np.random.default_rng(32)
    shapes = []
    for _ in range(18):
        L = int(rng.integers(6000, 11000))
        a = int(rng.integers(L - 8000, L - 4000))
        b = int(rng.integers(max(a + 800, 4000), min(L, 8000) + 1))
        shapes.append((L, a, b))
    reads, strands, truths = _zero_reads(33, shapes)
    r2, s2, t2 = _zero_reads(34, [(9000, 2000, 7000)], strand="+", err=False)            # error-free pair
    r3, s3, t3 = _zero_reads(35, [(30100, 100, 300), (30100, 29800, 30000)], strand="-")  # 30 000 x 300, 300 x 30 000
    r4, s4, t4 = _zero_reads(36, [(9000, 5000, 4000)], strand="+")                       # no overlap
    reads += r2 + r3 + r4; strands += s2 + s3 + s4; truths += t2 + t3 + t4
    assert "+" in strands and "-" in strands
    res, cons, ores = _check(O, reads, strands, cap=64 * MI)
    pieces = [_pieces(o, r) for o, r in zip(ores, reads)]
    assert sum(f * t > 16 * MI for f, t in pieces) >= 8
    assert pieces[19][0] < 600 and pieces[19][1] > 29000 and pieces[20][0] > 29000 and pieces[20][1] < 600   # (- strand)
    st = [o.status for o in ores]
    assert st[-1] == 3 and st[18] == 0 and st[19] == 0 and st[20] == 0
    assert sum(s == 0 for s in st[:18]) >= 15
    assert synth.identity(cons[18], truths[18]) > 0.99
    for i in [k for k in range(18) if st[k] == 0][:5]:
        assert synth.identity(cons[i], truths[i]) >= 0.85, i
    # the same reads under 128 Mi: nothing changes
    res2, cons2, _c = _gpu(reads, strands, zero_max_cells=128 * MI)
    assert cons2 == cons and list(res2["status"]) == list(res["status"])


def _rescue_shapes():
    return [(1300, a, b) for a, b in ((686, 1040), (212, 1230), (376, 1006), (260, 424), (300, 983), (700, 600), (100, 1299))]


@pytest.mark.parametrize("zk", [None, "7"])
def test_forced_long_path_parity(O, monkeypatch, zk):
    """C3_DEBUG_ZERO_LONG=1 sends every eligible read to k_zero_long (shapes of test_zero_repeat_rescue plus 200 seeded
    reads); C3_DEBUG_ZERO_K=7 makes every traceback cross row blocks, and the longer pieces span two column sweeps"""
    monkeypatch.setenv("C3_DEBUG_ZERO_LONG", "1")
    if zk:
        monkeypatch.setenv("C3_DEBUG_ZERO_K", zk)
    reads, strands, _t = _zero_reads(21, _rescue_shapes(), strand="+")
    r2, s2, _t2 = _zero_reads(22, [(1300, 500, 900)], strand="+", err=False)
    reads += r2 + [(revcomp(r2[0][0]), r2[0][1][::-1])]; strands += s2 + ["-"]
    rng = np.random.default_rng(23)
    shapes = []
    for _ in range(200):
        L = int(rng.integers(300, 3500))
        a, b = sorted(int(x) for x in rng.integers(1, L, 2))
        if rng.random() < 0.2:
            a, b = b, a                                                    # mostly no overlap
        shapes.append((L, a, b))
    r3, s3, _t3 = _zero_reads(24, shapes)
    res, cons, ores = _check(O, reads + r3, strands + s3)
    assert sum(o.status == 0 for o in ores) >= 120


def test_cap_edges(O):
    from c3poa_amd import _lib
    reads, strands, _t = _zero_reads(41, [(7000, 1500, 5200)], strand="+")
    P = O.default_params(zr_max_cells=64 * MI)
    ores, _c = O.process_batch(SP, reads, strands, params=P, threads=1)
    f, t = _pieces(ores[0], reads[0])
    assert ores[0].status == 0 and f * t > 16 * MI
    res, cons, o2 = _check(O, reads, strands, cap=f * t)                 # exactly at the cap: rescued
    assert int(res[0]["status"]) == 0
    res, cons, o2 = _check(O, reads, strands, cap=f * t - 1)             # one cell above it: not tried
    assert int(res[0]["status"]) == 3 and o2[0].status == 3
    res, cons, o2 = _check(O, reads, strands, cap=64 * MI, zero=0)       # -z
    assert int(res[0]["status"]) == 3 and cons == [""]
    for bad in (0, -1, 1 << 31, 1 << 40):
        with pytest.raises(_lib.C3Error):
            _lib.Handle(zero_max_cells=bad)
    _lib.Handle(zero_max_cells=(1 << 31) - 1).close()


def test_entry_point_and_shim_long_pair(O):
    from c3poa_amd import _lib, shims
    reads, strands, _t = _zero_reads(51, [(8000, 1800, 6200)], strand="+")
    cap = 64 * MI
    P = O.default_params(zr_max_cells=cap)
    ores, _c = O.process_batch(SP, reads, strands, params=P, threads=1)
    s, q = reads[0]
    p, tb = ores[0].front_end, ores[0].tail_beg
    d0, q0, d1, q1 = s[:p], q[:p], s[tb:], q[tb:]
    assert len(d0) * len(d1) > 16 * MI
    ref = O.zero_repeats(d0, q0, d1, q1, P)
    assert len(ref) > 7000
    h = _lib.Handle(zero_max_cells=cap)
    assert h.zero_repeats(d0, q0, d1, q1, 500) == ref
    h.close()
    h = _lib.Handle()
    assert h.zero_repeats(d0, q0, d1, q1, 500) == "" == O.zero_repeats(d0, q0, d1, q1)     # default cap: not tried
    h.close()
    args = types.SimpleNamespace(mdistcutoff=500, zero=True, zero_max_cells=cap)
    assert shims.determine_consensus(args, ("rd", s, q), [], [], [d0, d1], [q0, q1]) == (ref, 0)


def test_batch_hygiene_long_short_normal():
    from c3poa_amd import _lib
    long_r, long_s, _t = _zero_reads(61, [(7000, 1200, 5600), (6500, 2000, 5000)])
    short_r, short_s, _t2 = _zero_reads(62, [(1300, 400, 900), (1300, 650, 1100)])
    recs = list(synth.generate("cfg1", n_reads=12))
    mixed_r = long_r[:1] + [(r[1], r[2]) for r in recs[:6]] + short_r + long_r[1:] + [(r[1], r[2]) for r in recs[6:]]
    mixed_s = long_s[:1] + [r[3] for r in recs[:6]] + short_s + long_s[1:] + [r[3] for r in recs[6:]]
    plain_r = [(r[1], r[2]) for r in recs]
    plain_s = [r[3] for r in recs]
    cap = 64 * MI

    def fresh(rd, st):
        res, cons, cells = _gpu(rd, st, zero_max_cells=cap)
        return [int(x) for x in res["status"]], [int(x) for x in res["n_sub"]], cons, cells

    h = _lib.Handle(zero_max_cells=cap)
    h.set_splints([SP])
    for rd, st in ((mixed_r, mixed_s), (mixed_r, mixed_s), (plain_r, plain_s)):
        h.upload([r[0] for r in rd], [r[1] for r in rd], st)
        h.run()
        res, cons = h.results()
        got = ([int(x) for x in res["status"]], [int(x) for x in res["n_sub"]], cons, h.timing()["cells_poa"])
        assert got == fresh(rd, st)
    h.close()
    assert fresh(mixed_r, mixed_s)[0][0] == 0


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
    return {n: s for n, s, _q in fastx_read(out + "/Splint1/R2C2_Consensus.fasta")}


def test_cli_zero_max_cells(O, tmp_path):
    from c3poa_amd import records
    recs = list(synth.generate("cfg1", n_reads=10))
    zr, zs, zt = _zero_reads(71, [(6400, 1500, 6100), (6300, 1600, 6000), (6500, 1500, 6200)])
    for k, (r, s, t) in enumerate(zip(zr, zs, zt)):
        recs.insert(3 * k + 1, ("zero%d" % k, r[0], r[1], s, t))
    P = O.default_params(zr_max_cells=64 * MI)
    zidx = [i for i, r in enumerate(recs) if r[0].startswith("zero")]
    ores, ocons = O.process_batch(SP, [(recs[i][1], recs[i][2]) for i in zidx], [recs[i][3] for i in zidx], params=P, threads=3)
    exp = {}
    for i, o, c in zip(zidx, ores, ocons):
        f, t = _pieces(o, (recs[i][1],))
        assert o.status == 0 and c and f * t > 16 * MI
        exp[records.consensus_header(recs[i][0], recs[i][2], len(recs[i][1]), o.n_sub, len(c))[1:]] = c
    got = _run_cli(tmp_path / "a", recs, ["--zero-max-cells", "67108864"])
    assert {k: v for k, v in got.items() if k.startswith("zero")} == exp
    got = _run_cli(tmp_path / "b", recs)
    assert not any(k.startswith("zero") for k in got)
    assert len(got) >= 8

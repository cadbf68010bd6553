"""k_prep's extension rows: the mask-free rows (rows 1 .. C - W of a dangling piece), the masked rows (every row under the
test hook C3_DEBUG_PREP_ROWS=old) and the packed direction stream (one dword per lane and three rows) must give the same
pipeline results as each other and as the CPU oracle, bit for bit.  Every case states the shape it exists for as an assertion
on the oracle's records (piece lengths: front_end and L - tail_beg), so a change of the read generator cannot hollow it out.
Both GPU runs poison fresh device memory (C3_DEBUG_POISON): a direction word nobody wrote does not read as zero."""
import os

import numpy as np
import pytest

from c3poa_amd import synth
from c3poa_amd.seqio import revcomp

pytestmark = pytest.mark.gpu

W = 128                         # default dang_band
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


def _rnd(rng, n):
    return _ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _noisy(rng, clean, rc):
    """clean concatemer -> (seq, qual, strand) with the generator's error model, reverse-complemented when rc"""
    if rc:
        clean = revcomp(clean)
    s, q = synth._mutate(rng, np.frombuffer(clean.encode(), dtype=np.uint8))
    return s.decode(), q.decode(), "-" if rc else "+"


def _gpu_run(reads, strands, rows_old, cfg):
    from c3poa_amd import _lib
    keep = {k: os.environ.get(k) for k in ("C3_DEBUG_PREP_ROWS", "C3_DEBUG_POISON")}
    os.environ["C3_DEBUG_POISON"] = "1"
    if rows_old:
        os.environ["C3_DEBUG_PREP_ROWS"] = "old"
    else:
        os.environ.pop("C3_DEBUG_PREP_ROWS", None)
    try:
        h = _lib.Handle(**cfg)
        h.set_splints([synth.SPLINT1])
        h.upload([r[0] for r in reads], [r[1] for r in reads], strands)
        h.run()
        res, cons = h.results()
        cells = h.timing()["cells_polish"]
        h.close()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, cons, cells


def _pieces(o, L):
    """lengths of the dangling pieces of one oracle record (the rows of their extension alignments)"""
    out = []
    if o.status == 0 and o.has_front:
        out.append(o.front_end)
    if o.status == 0 and o.has_tail:
        out.append(L - o.tail_beg)
    return out


def _check(reads, strands, **cfg):
    """default rows == masked rows == oracle.  returns (oracle records, results of the default run)"""
    from oracle import oracle_py as O
    P = O.default_params(**cfg)
    ores, ocons = O.process_batch(synth.SPLINT1, reads, strands, params=P, threads=8)
    new, new_cons, new_cells = _gpu_run(reads, strands, False, cfg)
    old, old_cons, old_cells = _gpu_run(reads, strands, True, cfg)
    for i in range(len(reads)):
        for f in ("status", "n_sub", "front_end", "tail_beg", "n_win", "cons_len"):
            assert int(new[i][f]) == int(old[i][f]), (i, f, int(new[i][f]), int(old[i][f]))
        assert new_cons[i] == old_cons[i], i
        o = ores[i]
        assert int(new[i]["status"]) == o.status, (i, int(new[i]["status"]), o.status)
        if o.status == 0:
            for f in ("n_sub", "front_end", "tail_beg", "cons_len"):
                assert int(new[i][f]) == getattr(o, f), (i, f, int(new[i][f]), getattr(o, f))
        assert new_cons[i] == ocons[i], i
    ocells = sum(r.cells_polish for r in ores)
    assert new_cells == ocells and old_cells == ocells, (new_cells, old_cells, ocells)
    return ores, new


def test_piece_length_sweep():
    """pieces of every length residue mod 3 (the partial last direction word), across the 64-row blocks, across the 100-base
    threshold of a dangling piece, shorter and longer than the band half-width"""
    reads, strands = [], []
    for k in range(0, 201, 3):
        s, q, st, _ = synth.make_read(np.random.default_rng([11, k]), synth.SPLINT1, 1216, 3, k, k)
        reads.append((s, q)); strands.append(st)
    # A piece ends at a splint's peak, half a splint (142 bases) inside it: the reads above have no piece under 141 rows.  Reads
    # that END inside the last splint, c bases short of its end, have tails of about 142 - c rows, down to the 100-base threshold
    # and below it (no tail piece).
    n_sweep = len(reads)
    for c in range(0, 64, 4):
        rng = np.random.default_rng([11, 1000 + c])
        ins = _rnd(rng, 1216)
        s, q, st = _noisy(rng, ins[-108:] + (synth.SPLINT1 + ins) * 3 + synth.SPLINT1[:len(synth.SPLINT1) - c], rc=bool(c & 4))
        reads.append((s, q)); strands.append(st)
    ores, _ = _check(reads, strands)
    lens = [n for o, r in zip(ores, reads) for n in _pieces(o, len(r[0]))]
    assert {n % 3 for n in lens} == {0, 1, 2}
    assert min(lens) < W < max(lens)
    assert any(n <= 128 for n in lens) and any(128 < n <= 192 for n in lens) and any(192 < n <= 256 for n in lens) and any(n > 256 for n in lens)
    short = ores[n_sweep:]
    assert all(o.status == 0 for o in short) and any(o.has_tail for o in short) and any(not o.has_tail for o in short)


def test_long_pieces_both_strands():
    reads, strands, want = [], [], []
    for ins, n, k0, k1 in ((1216, 3, 20, 1100), (1216, 3, 1100, 20), (2000, 2, 1700, 1900)):
        for strand in "+-":
            seed = 0
            while True:                  # the generator draws the strand: first seed that gives the wanted one
                s, q, st, _ = synth.make_read(np.random.default_rng([12, ins, k0, seed]), synth.SPLINT1, ins, n, k0, k1)
                if st == strand:
                    break
                seed += 1
            reads.append((s, q)); strands.append(st); want.append(1000 if ins == 1216 else 1700)
    ores, _ = _check(reads, strands)
    for o, r, w in zip(ores, reads, want):
        assert max(_pieces(o, len(r[0])), default=0) > w, (_pieces(o, len(r[0])), w)
    assert set(strands) == {"+", "-"}


def _lost_splint_read(seed):
    """three good units and one splint replaced by random bases: its peak is missed, so the piece on that side spans two units.
    Even seeds lose the first splint (long front piece), odd seeds the last one (long tail piece)."""
    rng = np.random.default_rng([13, seed])
    ins = _rnd(rng, 1216)
    good = (synth.SPLINT1 + ins) * 3 + synth.SPLINT1
    junk = _rnd(rng, len(synth.SPLINT1))
    clean = ins[-108:] + junk + ins + good + ins[:108] if seed % 2 == 0 else ins[-108:] + good + ins + junk + ins[:108]
    s, q, st = _noisy(rng, clean, rc=bool((seed >> 1) & 1))
    return (s, q), st


LOST_SPLINT_SEEDS = (0, 1, 2, 3, 4, 5)


def test_rows_beyond_the_draft():
    """pieces longer than draft + W: rows i > C - W take the masked body inside a mask-free piece, rows i > C + W have no
    valid cell at all"""
    reads, strands = zip(*[_lost_splint_read(s) for s in LOST_SPLINT_SEEDS])
    ores, res = _check(list(reads), list(strands))
    n_front = n_tail = 0
    for o, g, r in zip(ores, res, reads):
        C = int(g["draft_len"])                # (the oracle's record has no draft length; the draft itself is compared through the consensus)
        assert o.status == 0 and C > 1000
        f = o.has_front and o.front_end > C + W
        t = o.has_tail and len(r[0]) - o.tail_beg > C + W
        assert f or t, (o.front_end, len(r[0]) - o.tail_beg, C)
        n_front += bool(f); n_tail += bool(t)
    assert n_front >= 2 and n_tail >= 2


@pytest.mark.parametrize("band", [0, 20, 159, 160, 255])
def test_other_bands(band):
    """0: the smallest band c3_create admits, the diagonal alone (bw = 1: one valid offset, in lane 0); 20: static invalid cells from lane 8 on; 159: bw = 319, the widest band with 5 offsets per lane; 160: bw = 321, the first band
    that takes the wide rows (8 offsets per lane, two rows per direction word); 255: bw = 511, the widest band the lanes hold"""
    recs = list(synth.generate("cfg1", n_reads=8))
    ores, _ = _check([(r[1], r[2]) for r in recs], [r[3] for r in recs], dang_band=band)
    assert sum(len(_pieces(o, len(r[1]))) for o, r in zip(ores, recs)) >= 8


def test_draft_beyond_lds():
    """a draft of more than 4 096 bases: the extension reads the draft from global memory (its own rows, same direction layout)"""
    s, q, st, _ = synth.make_read(np.random.default_rng([15, 0]), synth.SPLINT1, 4300, 2, 108, 108)
    ores, res = _check([(s, q)], [st])
    assert ores[0].status == 0 and int(res[0]["draft_len"]) > 4096 and len(_pieces(ores[0], len(s))) == 2


def test_extreme_scores():
    """a tail without any similarity to the draft (every row's scores fall: the lowest keys, no positive maximum) and an
    error-free read with top qualities whose tail is a prefix of the insert (the highest keys)"""
    rng = np.random.default_rng([16, 0])
    ins = _rnd(rng, 1216)
    s, q, st = _noisy(rng, ins[-108:] + (synth.SPLINT1 + ins) * 3 + synth.SPLINT1 + _rnd(rng, 400), rc=False)
    clean = ins[-108:] + (synth.SPLINT1 + ins) * 3 + synth.SPLINT1 + ins[:400]
    reads = [(s, q), (clean, "I" * len(clean))]
    ores, _ = _check(reads, [st, "+"])
    for o, r in zip(ores, reads):
        assert o.status == 0 and o.has_tail and len(r[0]) - o.tail_beg >= 400


@pytest.mark.parametrize("match,mismatch", [(2, -5), (3, -1), (7, -9)])
def test_other_polish_scoring(match, mismatch):
    """4 * (match - mismatch) = 28: not a power of two, the rows compare the draft nibble; 16 and 64: other shifts of the
    match-flag form than the default's 32"""
    recs = list(synth.generate("cfg1", n_reads=8))
    ores, _ = _check([(r[1], r[2]) for r in recs], [r[3] for r in recs], pol_match=match, pol_mismatch=mismatch)
    assert sum(len(_pieces(o, len(r[1]))) for o, r in zip(ores, recs)) >= 8


def test_wide_band_shapes():
    """dang_band 200 (bw = 401: the wide rows, 8 offsets per lane, two rows per direction word): pieces of both residues mod 2,
    pieces beyond draft + W, and a draft beyond the LDS copy"""
    reads, strands = [], []
    for k in range(100, 112):
        s, q, st, _ = synth.make_read(np.random.default_rng([17, k]), synth.SPLINT1, 1216, 3, k, k)
        reads.append((s, q)); strands.append(st)
    for seed in (0, 1):
        r, st = _lost_splint_read(seed)
        reads.append(r); strands.append(st)
    s, q, st, _ = synth.make_read(np.random.default_rng([15, 0]), synth.SPLINT1, 4300, 2, 108, 108)
    reads.append((s, q)); strands.append(st)
    ores, res = _check(reads, strands, dang_band=200)
    lens = [n for o, r in zip(ores, reads) for n in _pieces(o, len(r[0]))]
    assert {n % 2 for n in lens} == {0, 1}
    assert any(n > int(g["draft_len"]) + 200 for o, g, r in zip(ores, res, reads) for n in _pieces(o, len(r[0])))
    assert int(res[-1]["draft_len"]) > 4096 and len(_pieces(ores[-1], len(reads[-1][0]))) == 2


def test_band_beyond_the_lanes_is_an_error():
    """dang_band 256 (bw = 513 > 64 x 8 offsets): refused when the handle is created, not skipped silently in the run"""
    from c3poa_amd import _lib
    with pytest.raises(_lib.C3Error):
        _lib.Handle(dang_band=256)
    _lib.Handle(dang_band=255).close()

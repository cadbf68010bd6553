"""k_conk at the read lengths, splint lengths and scorings that default runs never reach: reads shorter than one 16-step
block and around every multiple of 16 up to 80 (last_word, the out-of-read kill, the slow block for the whole read), reads
shorter than the splint, a 40-base splint in a batch whose rows-per-lane come from a 512-base one (472 padding rows),
non-ACGT and lower-case letters in the first and last column, other scorings up to the edge of the 16-bit score cells, the
guard in c3_set_splints on both sides, and the scan mode (c3_scan_splints) at the same lengths.  Everything is compared with
the CPU oracle, exactly."""
import numpy as np
import pytest

from c3poa_amd import synth
from c3poa_amd.seqio import revcomp

pytestmark = pytest.mark.gpu

LENGTHS = list(range(1, 81)) + [95, 96, 97, 127, 128, 129, 255, 256, 257, 511, 512, 513]


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


def _rand(rng, L):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, L))


def _splint(S):
    return synth.SPLINT1 if S == len(synth.SPLINT1) else _rand(np.random.default_rng(7000 + S), S)


def _n_first_lower_last(s):
    """a non-ACGT letter in column 0, a lower-case one in column L-1 (L = 1: the 'N')"""
    z = list(s)
    z[-1] = z[-1].lower()
    z[0] = "N"
    return "".join(z)


def _lower_first_n_last(s):
    z = list(s)
    z[-1] = "N"
    z[0] = z[0].lower()
    return "".join(z)


def _reads(seed, splints):
    """[(seq, strand)]: every length four times -- both strands plain, then 'N' first / lower-case last on '+' and
    lower-case first / 'N' last on '-' -- and reads that hold each splint verbatim on either strand"""
    rng = np.random.default_rng(seed)
    out = []
    for L in LENGTHS:
        out.append((_rand(rng, L), "+"))
        out.append((_rand(rng, L), "-"))
        out.append((_n_first_lower_last(_rand(rng, L)), "+"))
        out.append((_lower_first_n_last(_rand(rng, L)), "-"))
    for sp in splints:
        out.append((_rand(rng, 30) + sp + _rand(rng, 50), "+"))
        out.append((_rand(rng, 17) + revcomp(sp) + _rand(rng, 3), "-"))
        out.append((sp, "+"))
        out.append((sp[:len(sp) // 2], "-"))
    return out


def _check_tracks(h, O, reads, splints, sids, **score):
    from c3poa_amd import _lib
    h.upload([r for r, _s in reads], ["I" * len(r) for r, _s in reads], [s for _r, s in reads], splint_ids=sids)
    h.run(_lib.STAGE_CONK)
    for i, (r, st) in enumerate(reads):
        sp = splints[sids[i]]
        want = O.conk(sp if st == "+" else revcomp(sp), r, **score)
        got = h.track(i)
        assert np.array_equal(want, got), (i, len(r), st, len(sp), np.flatnonzero(want != got)[:10].tolist())


@pytest.mark.parametrize("S", [40, 284, 512])
def test_read_lengths(O, S):
    from c3poa_amd import _lib
    sp = _splint(S)
    reads = _reads(S, [sp])
    assert min(len(r) for r, _s in reads) == 1 and any(len(r) < S for r, _s in reads)
    h = _lib.Handle()
    h.set_splints([sp])
    _check_tracks(h, O, reads, [sp], [0] * len(reads))
    h.close()


def test_mixed_splint_lengths(O):
    """rows per lane come from the longest splint of the table: the 40-base splint runs with 472 padding rows"""
    from c3poa_amd import _lib
    splints = [_splint(40), _splint(284), _splint(512)]
    reads = _reads(99, splints)
    # four reads per length: shift the splint by one per group so that every splint meets every length on both strands
    sids = [(i + i // 4) % 3 for i in range(len(reads))]
    for L in (1, 15, 16, 17, 33, 64, 513):
        assert {sids[i] for i, (r, _s) in enumerate(reads) if len(r) == L} == {0, 1, 2}
    h = _lib.Handle()
    h.set_splints(splints)
    _check_tracks(h, O, reads, splints, sids)
    h.close()


# (match, mismatch, penalty): the last two sit on the guard (62 * 512 = 31744 <= 32000), once through match, once through a
# mismatch score that is larger than match -- a cell grows by the larger of the two per splint row
@pytest.mark.parametrize("score", [(1, -1, 2), (2, -3, 5), (5, -5, 20), (62, -62, 20), (5, 62, 20)], ids=str)
def test_scoring(O, score):
    from c3poa_amd import _lib
    match, mismatch, penalty = score
    sp = _splint(512)
    rng = np.random.default_rng(match * 1000 + penalty)
    reads = [(_rand(rng, L), "+-"[k & 1]) for k, L in enumerate((1, 7, 16, 33, 100, 511, 512, 513, 600, 1100))]
    reads.append((_rand(rng, 40) + sp + _rand(rng, 70), "+"))
    reads.append((_rand(rng, 9) + revcomp(sp) + _rand(rng, 1), "-"))
    reads.append((sp, "+"))
    if match >= mismatch:
        # the largest cell a read with the splint inside can reach is match * 512, on the splint's last row
        top = O.conk(sp, reads[-1][0], penalty=penalty, match=match, mismatch=mismatch)
        assert top[0] >= match * 512
    h = _lib.Handle(conk_match=match, conk_mismatch=mismatch, conk_penalty=penalty)
    h.set_splints([sp])
    _check_tracks(h, O, reads, [sp], [0] * len(reads), penalty=penalty, match=match, mismatch=mismatch)
    h.close()


@pytest.mark.parametrize("cfg,S,ok", [
    (dict(conk_match=62), 512, True), (dict(conk_match=63), 512, False),
    (dict(conk_match=127), 251, True), (dict(conk_match=127), 252, False),
    (dict(conk_penalty=0), 512, True), (dict(conk_penalty=-1), 40, False),
    (dict(conk_penalty=32000), 512, True), (dict(conk_penalty=32001), 40, False),
    (dict(conk_mismatch=62), 512, True), (dict(conk_mismatch=63), 512, False),
    (dict(conk_match=-5, conk_mismatch=-127), 512, True)], ids=str)
def test_set_splints_guard(cfg, S, ok):
    """16-bit score cells: max(match, mismatch) * S <= 32000 and 0 <= penalty <= 32000, refused with C3_E_LIMIT otherwise"""
    from c3poa_amd import _lib
    h = _lib.Handle(**cfg)
    if ok:
        h.set_splints([_splint(S)])
    else:
        with pytest.raises(_lib.C3Error) as e:
            h.set_splints([_splint(40), _splint(S)])
        assert e.value.code == _lib.E_LIMIT and "32000" in str(e.value)
    h.close()


def test_scan_splints(O):
    from c3poa_amd import _lib
    splints = [_splint(40), _splint(512)]
    rng = np.random.default_rng(5)
    seqs = [_rand(rng, L) for L in LENGTHS]
    seqs += [_n_first_lower_last(_rand(rng, L)) for L in (1, 2, 16, 17, 64, 65)]
    for sp in splints:
        seqs += [_rand(rng, 30) + sp + _rand(rng, 50), _rand(rng, 5) + revcomp(sp) + _rand(rng, 200), sp]
    h = _lib.Handle()
    h.set_splints(splints)
    h.upload(seqs, ["I" * len(s) for s in seqs], ["?"] * len(seqs))
    tab, sid, st = h.scan_splints()
    otab, osid, ost = O.scan_splints(seqs, splints)
    bad = np.argwhere(tab != otab)
    assert bad.size == 0, (bad[:6].tolist(), [len(seqs[i]) for i in bad[:6, 0]])
    assert sid.tolist() == osid.tolist() and st == ost
    assert set(st) >= {ord("+"), ord("-"), ord("?")}                 # the assignment rule was reached from both sides
    h.close()

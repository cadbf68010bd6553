"""GPU tests of C3POa_demux.py --parse gpu: c3_demux_emit_text (k_fasta / k_fastx, k_demux, k_dsplit, k_inflate, k_bgzf) against
its host statement c3_demux_emit_text_host field for field and byte for byte, stream_off included, at the smallest shapes that
can break the placement and the copies, and the CLI's device tree against the host path's.

Index sets: two indexes per set (S = 9), the golden files (S = 21 * 9 = 189), 63 x 63 (S = 4096 exactly: pairs of letters
repeated four times, 16 + 15 letters, inside the limit of 31 distinct bytes), 64 x 64 (above the cap).  Reads carry exact copies
of the indexes in a head of 'N', so every winner is known without the search and the search is the host statement's."""
import gzip
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

from c3poa_amd import _lib, demux
from demux_emit_cases import GOLD, ROOT, sets_of
from demux_text_cases import IN_BGZF, KEEP_QUALS, OUT_BGZF, SPLIT, compressed, golden_texts, qual_of, records_of, small_text, to_fastq
from test_inflate_host import bgzf_members

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "C3POa_demux.py")
NX, TSO = os.path.join(GOLD, "demux_nextera.fasta"), os.path.join(GOLD, "demux_tso.fasta")


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


class Sets:
    """index sets with their names and sequences at hand: .sets (a DemuxSets), .a / .b = [(name, sequence bytes)]"""

    def __init__(self, a, b):
        self.a, self.b = a, b
        self.sets = _lib.DemuxSets([n for n, _s in a], [s for _n, s in a], [n for n, _s in b], [s for _n, s in b])
        self.S = (len(a) + 1) * (len(b) + 1)

    def head(self, s, filler=b"N"):
        """300 head bytes that send a read to stream s: exact copies of the two indexes (none for the empty field)"""
        ia, ib = divmod(s, len(self.b) + 1)
        h = bytearray(filler * 300)
        if ia < len(self.a):
            h[10:10 + len(self.a[ia][1])] = self.a[ia][1]
        if ib < len(self.b):
            h[150:150 + len(self.b[ib][1])] = self.b[ib][1]
        return bytes(h)


def letter_pairs(letters, n):
    out = [bytes([x, y]) * 4 for i, x in enumerate(letters) for y in letters[i + 1:]]
    assert len(out) >= n
    return out[:n]


@pytest.fixture(scope="module")
def S9():
    return Sets([("a0", b"ACGTACGTAC"), ("a_1", b"TTGGCCAATT")], [("b0", b"GGGGCCCCAAAA"), ("", b"CATCATCATCAT")])


@pytest.fixture(scope="module")
def S189():
    an, asq = demux.load_indexes(NX)
    bn, bsq = demux.load_indexes(TSO)
    s = Sets(list(zip(an, [x.encode() for x in asq])), list(zip(bn, [x.encode() for x in bsq])))
    assert s.S == 189
    return s


@pytest.fixture(scope="module")
def S4096():
    la, lb = b"ABCDEFGHIJKLMOPQ", b"RSTUVWXYZabcdef"                # 16 + 15 letters, no 'N' (the filler of the heads)
    s = Sets([("a%d" % i, x) for i, x in enumerate(letter_pairs(la, 63))], [("b%d" % i, x) for i, x in enumerate(letter_pairs(lb, 63))])
    assert s.S == 4096 == _lib.DEMUX_MAX_STREAMS
    return s


def bases(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), n))


def fasta(name, seq, wrap=None, eol=b"\n"):
    lines = [seq] if not wrap else [seq[i:i + wrap] for i in range(0, len(seq), wrap)]
    return b">" + name + eol + b"".join(x + eol for x in lines)


def fastq(name, seq, i=0):
    return b"@" + name + b"\n" + seq + b"\n+\n" + qual_of(i, len(seq)) + b"\n"


def same(d, h, what=""):
    """device result against the host statement's, field for field"""
    assert d.guards_intact and d.untouched_beyond_results, what
    assert d.info == h.info, (what, d.info, h.info)
    assert np.array_equal(d.stream_off, h.stream_off), what
    assert np.array_equal(d.hashes, h.hashes), what
    da, ha = d.arena.tobytes(), h.arena.tobytes()
    if da != ha:
        bad = next((i for i, (x, y) in enumerate(zip(da, ha)) if x != y), min(len(da), len(ha)))
        raise AssertionError("%s: arena differs from byte %d of %d: %r / %r" % (what, bad, len(ha), da[max(0, bad - 20):bad + 20], ha[max(0, bad - 20):bad + 20]))
    return h


def both(handle, sets, text, flags=0, at_eof=True, what=""):
    """one whole text on a fresh file of the handle, against the host statement"""
    handle.demux_text_reset()
    d = handle.demux_emit_text(sets, text, at_eof=at_eof, flags=flags)
    h = _lib.demux_emit_text_host(sets, text, at_eof=at_eof, kind=_lib.fastx_kind(text), flags=flags)
    return same(d, h, what)


def text_of(kind, S_, streams, lens, rng, names=None):
    """records for the given streams (None: a read of 300 bases, which is dropped) with sequence lengths lens"""
    recs = []
    for i, (s, ln) in enumerate(zip(streams, lens)):
        seq = (S_.head(s) if s is not None else b"N" * 300)[:ln] + bases(rng, max(0, ln - 300))
        name = b"r%d" % i if names is None else names[i]
        recs.append(fasta(name, seq) if kind == 2 else fastq(name, seq, i))
    return b"".join(recs)


@pytest.mark.parametrize("kind", (2, 4))
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 511, 513, 1003])
def test_record_counts_at_the_tile_edges(handle, S189, n, kind):
    rng = np.random.default_rng(n)
    streams = [int(x) for x in rng.integers(0, 189, n)]
    text = text_of(kind, S189, streams, [301 + i % 7 for i in range(n)], rng)
    for flags in (SPLIT, SPLIT | KEEP_QUALS if kind == 4 else 0):
        if n == 0:
            handle.demux_text_reset()
            d = handle.demux_emit_text(S189.sets, b"", at_eof=True, flags=flags)
            assert d.info["n_records"] == 0 and d.info["kind"] == 0 and not d.stream_off.any() and d.guards_intact
            continue
        h = both(handle, S189.sets, text, flags)
        assert h.info["n_kept"] == n and h.info["n_streams"] == (189 if flags & SPLIT else 1)
        if flags & SPLIT:                                              # the winners are the planted ones: every stream holds its reads in order
            got = h.streams()
            for s in set(streams):
                names = [r.split(b"|", 1)[0][1:] for r in records_of(got[s], flags & KEEP_QUALS)]
                assert names == [b"r%d" % i for i, x in enumerate(streams) if x == s], s


PATTERNS = ("one_stream", "round_robin", "change_at_255_256_257", "unkept_at_tile_edges", "only_unkept")


def pattern(name, S, n=600):
    if name == "one_stream":
        return [S // 2] * n
    if name == "round_robin":
        return [i % S for i in range(n)]
    if name == "change_at_255_256_257":
        return [0] * 255 + [1, S - 1, 2] + [0] * (n - 258)
    if name == "unkept_at_tile_edges":                                 # dropped reads around kept records 255 .. 257 and 511 .. 513
        return [None if i in (254, 255, 256, 258, 259, 517, 518, 519, 521) else (i * 7) % S for i in range(n)]
    return [None] * n


@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("which", ("S9", "S189"))
def test_key_patterns(handle, request, which, name):
    S_ = request.getfixturevalue(which)
    rng = np.random.default_rng(len(name))
    streams = pattern(name, S_.S)
    lens = [300 if s is None else 301 + i % 5 for i, s in enumerate(streams)]
    for kind in (2, 4):
        text = text_of(kind, S_, streams, lens, rng)
        h = both(handle, S_.sets, text, SPLIT | (KEEP_QUALS if kind == 4 else 0), what=name)
        assert h.info["n_records"] == 600 and h.info["n_kept"] == sum(s is not None for s in streams)
        sizes = np.diff(h.stream_off)
        assert set(np.flatnonzero(sizes).tolist()) == {s for s in streams if s is not None}
        whole = both(handle, S_.sets, text, KEEP_QUALS if kind == 4 else 0)
        assert sum(len(s) for s in h.streams()) == len(whole.arena)


def test_4096_streams_and_the_cap(handle, S4096):
    rng = np.random.default_rng(4096)
    streams = [0, 4095, 63, 64, 4032, 2048] + [int(x) for x in rng.integers(0, 4096, 594)]
    text = text_of(2, S4096, streams, [301 + i % 3 for i in range(600)], rng)
    h = both(handle, S4096.sets, text, SPLIT)
    assert h.info["n_streams"] == 4096 and h.info["n_kept"] == 600
    assert set(np.flatnonzero(np.diff(h.stream_off)).tolist()) == set(streams)
    z = both(handle, S4096.sets, text[:len(text) // 8], SPLIT | OUT_BGZF)
    assert z.info["n_kept"] > 50
    la, lb = b"ABCDEFGHIJKLMOPQ", b"RSTUVWXYZabcdef"
    over = Sets([("a%d" % i, x) for i, x in enumerate(letter_pairs(la, 64))], [("b%d" % i, x) for i, x in enumerate(letter_pairs(lb, 64))])
    handle.demux_text_reset()
    with pytest.raises(_lib.C3Error) as e:
        handle.demux_emit_text(over.sets, text, at_eof=True, flags=SPLIT)
    assert e.value.code == _lib.E_LIMIT and "C3_DEMUX_MAX_STREAMS" in str(e.value) and e.value.guards_intact and e.value.untouched
    assert both(handle, over.sets, text[:20000], 0).info["n_streams"] == 1


def test_sequence_and_name_lengths(handle, S9):
    """the sequence lengths round 300 and round 32 768, and 70 000; names of 0-256 bytes SAMPLED at 0, 1, 3, 4, 5, 17, 255 and 256
    bytes (with the 1-16 of test_every_alignment_and_copy_tail: the head, dword and tail cases of the copy, not a sweep)"""
    rng = np.random.default_rng(70000)
    lens = [300, 301, 302, 32767, 32768, 32769, 70000, 301]
    name_lens = [0, 1, 3, 4, 5, 255, 256, 17]
    streams = [1, 2, 3, 4, 5, 6, 7, 8]
    for kind in (2, 4):
        names = [b"n" * k for k in name_lens]
        text = text_of(kind, S9, streams, lens, rng, names)
        for flags in ((0, SPLIT) if kind == 2 else (0, KEEP_QUALS, SPLIT | KEEP_QUALS)):
            h = both(handle, S9.sets, text, flags)
            assert h.info["n_kept"] == 7
    # kind 2 wrapped at 60 columns with CRLF, long records included
    text = b"".join(fasta(b"w%d" % i, S9.head(i)[:ln] + bases(rng, max(0, ln - 300)), wrap=60, eol=b"\r\n") for i, ln in enumerate(lens))
    assert both(handle, S9.sets, text, SPLIT).info["n_kept"] == 7
    with pytest.raises(_lib.C3Error) as e:
        handle.demux_text_reset()
        handle.demux_emit_text(S9.sets, text, at_eof=True, flags=KEEP_QUALS)
    assert e.value.code == _lib.E_ARG and "C3_DEMUX_KEEP_QUALS on a FASTA text" in str(e.value) and e.value.untouched


@pytest.mark.parametrize("keep", (0, KEEP_QUALS))
def test_every_alignment_and_copy_tail(handle, S9, keep):
    """copy tails of 0 .. 260 bytes behind 301 at every (source, destination) alignment mod 16 of the copy k_dsplit_emit makes:
    of the sequence (keep = 0) and of the quality (KEEP_QUALS).  No index is planted, so a record is '>' name '|_' and the name
    length steers the destination."""
    rng = np.random.default_rng(16 + keep)
    recs, src, dst, seen = [], 0, 0, set()
    for rep in range(3):
        for tail in rng.permutation(261):
            sl = 301 + int(tail)
            body = lambda nl: dst + 4 + nl + (sl + 3 if keep else 0)      # noqa: E731
            nl = next((k for k in range(1, 17) if (src % 16, body(k) % 16) not in seen), 1)
            seen.add((src % 16, body(nl) % 16))
            seq = b"N" * 300 + bases(rng, sl - 300)
            name = b"%d." % len(recs)
            name = name + b"x" * (nl - len(name)) if nl >= len(name) else name[:nl]
            recs.append((name, seq))
            src += sl
            dst += 5 + len(name) + sl + (3 + sl if keep else 0)
    assert len(seen) == 256
    text = b"".join(fastq(n, s, i) for i, (n, s) in enumerate(recs))
    h = both(handle, S9.sets, text, keep)
    assert h.info["n_kept"] == len(recs) == 783
    if not keep:
        fa = b"".join(fasta(n, s) for n, s in recs)
        assert both(handle, S9.sets, fa, 0).arena.tobytes() == h.arena.tobytes()


@pytest.mark.parametrize("kind", (2, 4))
def test_pieces_cut_at_every_byte(handle, tmp_path, kind):
    text, nx, tso = small_text(kind, tmp_path)
    sets = sets_of(nx, tso)
    flags = SPLIT | (KEEP_QUALS if kind == 4 else 0)
    whole = both(handle, sets, text, flags)
    assert whole.info["n_records"] == 3 and whole.info["n_kept"] == 2
    for c in range(1, len(text)):
        handle.demux_text_reset()
        d1 = handle.demux_emit_text(sets, text[:c], at_eof=False, flags=flags)
        same(d1, _lib.demux_emit_text_host(sets, text[:c], at_eof=False, kind=kind, flags=flags), c)
        d2 = handle.demux_emit_text(sets, text[c:], at_eof=True, flags=flags)      # the handle puts the tail in front
        same(d2, _lib.demux_emit_text_host(sets, text[d1.info["consumed"]:], at_eof=True, kind=kind, flags=flags), c)
        assert [a + b for a, b in zip(d1.streams(), d2.streams())] == whole.streams(), c


@pytest.mark.parametrize("fresh", (65535, 65536, 65537))
def test_128k_text_in_pieces(handle, S189, fresh):
    rng = np.random.default_rng(fresh)
    recs, size = [], 0
    while size <= 128 * 1024:
        recs.append(fastq(b"r%d" % len(recs), S189.head(len(recs) % 189) + bases(rng, 40 + len(recs) % 50), len(recs)))
        size += len(recs[-1])
    text = b"".join(recs)
    whole = _lib.demux_emit_text_host(S189.sets, text, at_eof=True, kind=4, flags=SPLIT | KEEP_QUALS)
    handle.demux_text_reset()
    # pieces as the CLI feeds them: only the fresh bytes go up, the tail stays on the device
    got, hs, pos, calls = None, [], 0, 0
    while pos < len(text):
        piece = text[pos:pos + fresh]
        pos += len(piece)
        r = handle.demux_emit_text(S189.sets, piece, at_eof=pos >= len(text), flags=SPLIT | KEEP_QUALS)
        assert r.info["departed"] == 0 and r.guards_intact
        got = r.streams() if got is None else [a + b for a, b in zip(got, r.streams())]
        hs.append(r.hashes)
        calls += 1
    assert calls == 3 and got == whole.streams() and np.array_equal(np.concatenate(hs), whole.hashes)


def test_reset_between_files_and_reuse_after_a_refusal(handle, S9):
    rng = np.random.default_rng(3)
    fa = text_of(2, S9, [1, 2, 3, 4], [310, 320, 330, 340], rng)
    fq = text_of(4, S9, [5, 6, 7, 8], [310, 320, 330, 340], rng)
    handle.demux_text_reset()
    first = handle.demux_emit_text(S9.sets, fa, at_eof=False, flags=SPLIT)          # the last record stays behind as the tail
    assert first.info["n_records"] == 3 and first.info["kind"] == 2 and first.info["consumed"] < len(fa)
    handle.demux_text_reset()                                                       # another file, of the other kind
    d = handle.demux_emit_text(S9.sets, fq, at_eof=True, flags=SPLIT | KEEP_QUALS)
    same(d, _lib.demux_emit_text_host(S9.sets, fq, kind=4, flags=SPLIT | KEEP_QUALS), "after reset")
    # a refusal keeps the tail: the same piece again gives what one text gives
    cut = len(fq) // 2
    handle.demux_text_reset()
    p1 = handle.demux_emit_text(S9.sets, fq[:cut], at_eof=False, flags=SPLIT | KEEP_QUALS)
    for kw in ({"cap": 10, "max_records": 100}, {"cap": 1 << 20, "max_records": 1}):
        with pytest.raises(_lib.C3Error) as e:
            handle.demux_emit_text(S9.sets, fq[cut:], at_eof=True, flags=SPLIT | KEEP_QUALS, **kw)
        assert e.value.code == _lib.E_LIMIT and e.value.untouched and e.value.guards_intact
    p2 = handle.demux_emit_text(S9.sets, fq[cut:], at_eof=True, flags=SPLIT | KEEP_QUALS)
    h2 = _lib.demux_emit_text_host(S9.sets, fq[p1.info["consumed"]:], kind=4, flags=SPLIT | KEEP_QUALS)
    same(p2, h2, "after refusals")
    with pytest.raises(_lib.C3Error) as e:
        _lib.demux_emit_text_host(S9.sets, fq[p1.info["consumed"]:], kind=4, flags=SPLIT | KEEP_QUALS, cap=10, max_records=100)
    assert e.value.stream_off[-1] == h2.stream_off[-1]
    t = handle.demux_text_timing()
    assert t["n_kept"] == p2.info["n_kept"] and t["n_streams"] == 9 and t["n_waits"] >= 4 and t["ms_call"] > 0 and t["ms_demux"] > 0 and t["ms_split"] > 0


def test_departures(handle, S9):
    rng = np.random.default_rng(9)
    n = 300
    for kind in (2, 4):
        recs = [text_of(kind, S9, [i % 9], [301 + i % 4], rng, [b"r%d" % i]) for i in range(n)]
        for at in (0, n // 2, n - 1):
            t = bytearray(b"".join(recs))
            t[sum(len(r) for r in recs[:at]) + 120] = 0xC3
            for at_eof in (False, True):
                h = both(handle, S9.sets, bytes(t), SPLIT, at_eof=at_eof, what=(kind, at))
                assert (h.info["departed"], h.info["n_records"]) == (1, at)
        if kind == 4:                                                  # a record that is not strict: its '+' line is missing
            for at in (0, n // 2, n - 1):
                t = b"".join(recs[:at]) + recs[at].replace(b"\n+\n", b"\n", 1) + b"".join(recs[at + 1:])
                h = both(handle, S9.sets, t, SPLIT | KEEP_QUALS, what=("strict", at))
                assert (h.info["departed"], h.info["n_records"]) == (1, at)
    t = b"ACGT\n" + fasta(b"r", S9.head(3) + b"ACGT")                  # a FASTA text cannot begin with a sequence line: not '>' nor '@'
    handle.demux_text_reset()
    d = handle.demux_emit_text(S9.sets, t, at_eof=True)
    assert (d.info["departed"], d.info["kind"], d.info["n_records"], d.info["consumed"]) == (1, 0, 0, 0)
    # departure 2 of c3_fasta (a sequence line in front of the first header) cannot reach the device call: a file of kind 2 begins
    # with '>', which opens a record, and the kept tail always starts at a header line.  The host statement, which takes the kind
    # as stated, shows the rule
    h2 = _lib.demux_emit_text_host(S9.sets, b"ACGT\n" + t[5:], kind=2)
    assert (h2.info["departed"], h2.info["n_records"], h2.info["consumed"]) == (2, 0, 0)


def test_bgzf_in_and_out(handle, S189):
    rng = np.random.default_rng(21)
    recs = [fastq(b"r%d" % i, S189.head((i * 5) % 189) + bases(rng, 100 + i % 300), i) for i in range(240)]
    text = b"".join(recs)
    plain = _lib.demux_emit_text_host(S189.sets, text, kind=4, flags=SPLIT | KEEP_QUALS)
    for members in (_lib.bgzf_compress_host(text), b"".join(bgzf_members(text, block=40000))):
        handle.demux_text_reset()
        d = handle.demux_emit_text(S189.sets, members, at_eof=True, flags=SPLIT | KEEP_QUALS | IN_BGZF)
        same(d, plain, "bgzf in")
        assert handle.demux_text_timing()["text_bytes"] == len(text)
    # members in two pieces, the cut inside a record
    ms = bgzf_members(text, block=30000)
    handle.demux_text_reset()
    d1 = handle.demux_emit_text(S189.sets, b"".join(ms[:3]), at_eof=False, flags=SPLIT | KEEP_QUALS | IN_BGZF)
    d2 = handle.demux_emit_text(S189.sets, b"".join(ms[3:]), at_eof=True, flags=SPLIT | KEEP_QUALS | IN_BGZF)
    assert [a + b for a, b in zip(d1.streams(), d2.streams())] == plain.streams() and d1.info["consumed"] < d1.info["text_bytes"] == 90000
    # a truncated member
    bad = _lib.bgzf_compress_host(text)[:-9]
    handle.demux_text_reset()
    with pytest.raises(_lib.C3Error) as e:
        handle.demux_emit_text(S189.sets, bad, at_eof=True, flags=IN_BGZF)
    assert e.value.code == _lib.E_DATA and e.value.untouched and e.value.guards_intact
    damaged = bytearray(_lib.bgzf_compress_host(text))
    damaged[len(damaged) // 2] ^= 0x55
    with pytest.raises(_lib.C3Error) as e:
        handle.demux_emit_text(S189.sets, bytes(damaged), at_eof=True, flags=IN_BGZF)
    assert e.value.code == _lib.E_DATA and e.value.untouched
    # out: every non-empty stream is c3_bgzf_compress_host of the plain stream
    for flags in (OUT_BGZF, SPLIT | OUT_BGZF, SPLIT | OUT_BGZF | KEEP_QUALS):
        z = both(handle, S189.sets, text, flags)
        p = _lib.demux_emit_text_host(S189.sets, text, kind=4, flags=flags & ~OUT_BGZF)
        assert z.streams() == compressed(p.streams())
    handle.demux_text_reset()
    with pytest.raises(_lib.C3Error) as e:
        handle.demux_emit_text(S189.sets, text, at_eof=True, flags=SPLIT | OUT_BGZF, cap=1000, max_records=1000)
    assert e.value.code == _lib.E_LIMIT and e.value.untouched
    assert e.value.stream_off[-1] == sum(int(_lib.load().c3_bgzf_bound(len(s))) for s in _lib.demux_emit_text_host(S189.sets, text, kind=4, flags=SPLIT).streams() if s)


def test_unsplit_fasta_equals_demux_emit(handle, tmp_path):
    for tag, kind, text, nx, tso in golden_texts(tmp_path):
        if kind == 2:
            sets = sets_of(nx, tso)
            old = handle.demux_emit(text, sets)
            h = both(handle, sets, text, 0, what=tag)
            assert h.streams() == [old.out] and np.array_equal(h.hashes, old.hashes)
            both(handle, sets, text, SPLIT, what=tag)
        else:
            both(handle, sets_of(nx, tso), text, SPLIT | KEEP_QUALS, what=tag)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------
def run_cli(args, timeout=300):
    p = subprocess.run([sys.executable, CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    stats = [json.loads(line) for line in p.stderr.splitlines() if line.startswith("{")]
    return p, (stats[-1] if stats else None)


def tree(d):
    out = {}
    for base, _dirs, files in os.walk(str(d)):
        for f in files:
            p = os.path.join(base, f)
            assert not f.endswith(".part")
            raw = open(p, "rb").read()
            if f.endswith(".gz"):
                assert raw.endswith(_lib.BGZF_EOF) and raw.count(_lib.BGZF_EOF) == 1
            out[os.path.relpath(p, str(d))] = gzip.decompress(raw) if f.endswith(".gz") else raw
    return out


@pytest.fixture(scope="module")
def cli_inputs(tmp_path_factory):
    """~40 golden paper reads as FASTA, FASTQ and BGZF FASTQ, and the host path's trees for them (made once, in this process)"""
    d = tmp_path_factory.mktemp("demux_cli")
    text = [t for t in golden_texts(d) if t[0] == "paper"][0][2]
    fa = b"".join(b">" + r for r in text.split(b">")[1:41])
    fq = to_fastq(fa)
    files = {"fasta": d / "in.fasta", "fastq": d / "in.fastq", "bgzf": d / "in.fastq.gz"}
    files["fasta"].write_bytes(fa)
    files["fastq"].write_bytes(fq)
    files["bgzf"].write_bytes(b"".join(bgzf_members(fq, block=7000)) + _lib.BGZF_EOF)
    host = {}
    for key in ("fasta", "fastq"):
        for split in (False, True):
            for keep in ((False, True) if key == "fastq" else (False,)):
                out = d / ("host_%s_%d_%d" % (key, split, keep))
                demux.run_text_host(str(files[key]), str(out), NX, TSO, split=split, keep_quals=keep, host_search=True)
                host[(key, split, keep)] = tree(out)
    return files, host


MATRIX = [(k, s, z, q) for k in ("fasta", "fastq", "bgzf") for s in (False, True) for z in (False, True) for q in ((False, True) if k != "fasta" else (False,))]


@pytest.mark.parametrize("key,split,bgzf,keep", MATRIX)
def test_cli_device_tree_equals_host_tree(cli_inputs, tmp_path, key, split, bgzf, keep):
    files, host = cli_inputs
    flags = (["--split"] if split else []) + (["--bgzf"] if bgzf else []) + (["--keep-quals"] if keep else []) + (["--inflate", "gpu"] if key == "bgzf" else [])
    p, stats = run_cli(["-i", files[key], "-o", tmp_path / "o", "-n", NX, "-t", TSO, "--emit", "gpu", "--parse", "gpu", "--emit-stats"] + flags)
    assert p.returncode == 0, p.stderr
    want = host[("fastq" if key == "bgzf" else key, split, keep)]
    assert tree(tmp_path / "o") == {k + (".gz" if bgzf else ""): v for k, v in want.items()} and len(want) == (1 if not split else len(want)) > 0
    assert stats["fallback"] is None and stats["records_device"] == 40 and stats["files"] == len(want) and stats["streams"] == (189 if split else 1)
    assert stats["inflated_bytes"] == os.path.getsize(files["fastq" if key != "fasta" else "fasta"])
    assert "falls back" not in p.stderr


def test_cli_chunk_growth_and_zlib_input(cli_inputs, tmp_path):
    files, host = cli_inputs
    p, stats = run_cli(["-i", files["fastq"], "-o", tmp_path / "g", "-n", NX, "-t", TSO, "--emit", "gpu", "--parse", "gpu", "--emit-stats", "--split", "--keep-quals",
                        "--demux-chunk", 512])
    assert p.returncode == 0 and stats["fallback"] is None and stats["chunks"] > 100 and stats["records_device"] == 40
    assert tree(tmp_path / "g") == host[("fastq", True, True)]
    # BGZF without --inflate gpu, and plain gzip: through zlib on the host, the same files
    plain_gz = tmp_path / "plain.fastq.gz"
    plain_gz.write_bytes(gzip.compress(files["fastq"].read_bytes()))
    for inp in (files["bgzf"], plain_gz):
        p, stats = run_cli(["-i", inp, "-o", tmp_path / ("z" + inp.name), "-n", NX, "-t", TSO, "--emit", "gpu", "--parse", "gpu", "--emit-stats", "--split", "--keep-quals"])
        assert p.returncode == 0 and stats["fallback"] is None, p.stderr
        assert tree(tmp_path / ("z" + inp.name)) == host[("fastq", True, True)]
    # --keep-quals on a FASTA input: the message of C3POa_postprocessing.py, nothing left behind
    p, _ = run_cli(["-i", files["fasta"], "-o", tmp_path / "kq", "-n", NX, "-t", TSO, "--emit", "gpu", "--parse", "gpu", "--keep-quals"])
    assert p.returncode == 1 and "--keep-quals: the records of %s have no quality line" % files["fasta"] in p.stderr and not (tmp_path / "kq").exists()
    # no read long enough
    short = tmp_path / "short.fasta"
    short.write_bytes(b">a\nACGT\n>b\n" + b"A" * 300 + b"\n")
    p, _ = run_cli(["-i", short, "-o", tmp_path / "e1", "-n", NX, "-t", TSO, "--emit", "gpu", "--parse", "gpu", "--bgzf"])
    assert p.returncode == 0 and (tmp_path / "e1" / "Indexed_reads.fasta.gz").read_bytes() == _lib.BGZF_EOF
    p, _ = run_cli(["-i", short, "-o", tmp_path / "e2", "-n", NX, "-t", TSO, "--emit", "gpu", "--parse", "gpu", "--bgzf", "--split"])
    assert p.returncode == 0 and os.listdir(tmp_path / "e2") == ["samples"] and os.listdir(tmp_path / "e2" / "samples") == []


def host_tree(inp, out, nx, tso, **kw):
    demux.run_text_host(str(inp), str(out), str(nx), str(tso), host_search=True, **kw)
    return tree(out)


def test_cli_fallbacks_give_the_host_tree(cli_inputs, tmp_path):
    files, host = cli_inputs
    fq = files["fastq"].read_bytes()
    recs = records_of(fq, True)
    base = ["--emit", "gpu", "--parse", "gpu", "--emit-stats", "--split", "--keep-quals", "--bgzf"]

    def check(tag, inp, nx, tso, reason):
        p, stats = run_cli(["-i", inp, "-o", tmp_path / tag, "-n", nx, "-t", tso] + base)
        assert p.returncode == 0, p.stderr
        assert reason in stats["fallback"] and "falls back to the host path" in p.stderr, stats
        want = host_tree(inp, tmp_path / (tag + "_h"), nx, tso, split=True, keep_quals=True)
        assert tree(tmp_path / tag) == {k + ".gz": v for k, v in want.items()} and want

    # a piece departs: a blank line between two records is not strict four-line FASTQ
    dep = tmp_path / "dep.fastq"
    dep.write_bytes(b"".join(recs[:20]) + b"\n" + b"".join(recs[20:]))
    check("dep", dep, NX, TSO, "departs from the strict FASTQ rule")
    # a name turns up twice
    twice = tmp_path / "twice.fastq"
    twice.write_bytes(fq + recs[3])
    check("twice", twice, NX, TSO, "repeated names")
    # an index name holds '|'
    piped = tmp_path / "piped.fasta"
    piped.write_text(open(NX).read().replace(">", ">lib|", 1))
    check("piped", files["fastq"], piped, TSO, "holds '|'")
    # more sample streams than the device takes
    la, lb = b"ABCDEFGHIJKLMOPQ", b"RSTUVWXYZabcdef"
    wide = [tmp_path / "wide_a.fasta", tmp_path / "wide_b.fasta"]
    for path, letters, c in zip(wide, (la, lb), "ab"):
        path.write_bytes(b"".join(b">%s%d\n%s\n" % (c.encode(), i, x) for i, x in enumerate(letter_pairs(letters, 64))))
    check("wide", files["fastq"], wide[0], wide[1], "sample streams")
    # the call is refused: a member with a damaged body (a flipped byte: the CRC fails; an invalid block type: zlib.error before
    # any CRC); the host path cannot read the file either: its one-line message is the last thing on stderr, nothing is left behind
    for tag, at, mask in (("crc", os.path.getsize(files["bgzf"]) // 2, 0x55), ("block_type", 18, 0x06)):
        raw = bytearray(files["bgzf"].read_bytes())
        raw[at] = raw[at] ^ mask if tag == "crc" else raw[at] | mask
        bad = tmp_path / ("bad_%s.fastq.gz" % tag)
        bad.write_bytes(bytes(raw))
        with pytest.raises(zlib.error if tag == "block_type" else gzip.BadGzipFile):
            gzip.decompress(bytes(raw))
        p, stats = run_cli(["-i", bad, "-o", tmp_path / ("bad_" + tag), "-n", NX, "-t", TSO, "--inflate", "gpu"] + base)
        assert p.returncode == 1 and stats["fallback"].startswith("c3_demux_emit_text:"), (tag, p.stderr)
        assert p.stderr.splitlines()[-1].startswith("C3POa_demux: ") and "Traceback" not in p.stderr, (tag, p.stderr)
        assert not (tmp_path / ("bad_" + tag)).exists()


def test_more_samples_than_open_files(handle, cli_inputs, tmp_path, monkeypatch):
    """--split keeps at most demux.MAX_OPEN_PARTS .part files open and appends to the others by opening them per write: with the
    bound at 3 and at 0 the tree is the one of the unbounded run (a run that reaches thousands of samples must not run out of
    file descriptors), and nothing stays open"""
    files, host = cli_inputs
    want = host[("fastq", True, True)]
    assert len(want) > 6
    for bound in (3, 0):
        monkeypatch.setattr(demux, "MAX_OPEN_PARTS", bound)
        stats = {}
        done = demux.run_text_gpu(str(files["fastq"]), str(tmp_path / str(bound)), NX, TSO, split=True, keep_quals=True, bgzf=True, chunk=2048, handle=handle,
                                  stats=stats)
        assert done == (40, 40) and stats["fallback"] is None and stats["files"] == len(want) and stats["chunks"] > 10
        assert tree(tmp_path / str(bound)) == {k + ".gz": v for k, v in want.items()}
        links = [os.path.realpath(os.path.join("/proc/self/fd", fd)) for fd in os.listdir("/proc/self/fd")]
        assert not [x for x in links if x.startswith(os.path.realpath(str(tmp_path)))]

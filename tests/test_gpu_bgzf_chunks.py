"""The BGZF chunk loop (c3h::bgzf_chunks) run more than once.  One chunk is 2048 blocks of 65280 bytes, which no other test
fills, so every path that compresses through the loop runs here twice: with the default chunk, and with C3_BGZF_CHUNK=2 on
streams longer than 2 * 65280 bytes.  Members are cut every 65280 input bytes whatever the chunk, so the two outputs are equal
byte for byte, and they inflate to the plain stream."""
import gzip

import numpy as np
import pytest

import test_gpu_demux_text as DT
import test_gpu_emit as GE
import test_gpu_post_emit as E
import test_gpu_post_text as PT
from c3poa_amd import _lib
from demux_text_cases import KEEP_QUALS, OUT_BGZF

pytestmark = pytest.mark.gpu

BLOCK = 65280


def both_chunks(monkeypatch, run):
    """run() with the default chunk and with chunks of two blocks"""
    monkeypatch.delenv("C3_BGZF_CHUNK", raising=False)
    whole = run()
    monkeypatch.setenv("C3_BGZF_CHUNK", "2")
    small = run()
    monkeypatch.delenv("C3_BGZF_CHUNK")
    return whole, small


def inflates_to(comp, plain):
    return gzip.decompress(comp) == plain and _lib.bgzf_decompress_host(comp) == plain


@pytest.mark.parametrize("n", [2 * BLOCK, 2 * BLOCK + 1, 5 * BLOCK - 7], ids=["one_chunk", "one_byte_more", "three_chunks_short_last"])
def test_compress(monkeypatch, n):
    rng = np.random.default_rng(n)
    data = bytes(rng.choice(np.frombuffer(b"ACGTN\n@+IIIHH", dtype=np.uint8), n))
    z = _lib.Bgzf(0)
    whole, small = both_chunks(monkeypatch, lambda: z.compress(data))
    z.close()
    assert small == whole and len(PT.members(whole)) == (n + BLOCK - 1) // BLOCK
    assert inflates_to(whole, data)
    assert whole == _lib.bgzf_compress_host(data)


def test_post_emit_text(monkeypatch):
    recs, adapters = E._dataset(45, 300, "dir")
    plan = PT.plan_of(adapters, "")
    text = PT.text_of(recs, 4)
    assert len(text) < 1 << 20
    h = _lib.Handle()
    h.set_splints([a[1] for a in adapters])

    def run(out_bgzf=True):
        h.post_text_reset()
        res = h.post_emit_text(plan, text, at_eof=True, out_bgzf=out_bgzf, keep_quals=True)
        assert res.guards_intact and res.untouched_beyond_results and res.info["n_records"] == len(recs)
        return res.streams()

    whole, small = both_chunks(monkeypatch, run)
    plain = run(out_bgzf=False)
    h.close()
    assert len(plain[0]) > 2 * BLOCK                              # the main read stream takes a second chunk of two blocks
    assert small == whole
    n_z = len(plain) - 2                                          # the read streams and the 10x stream are compressed; the last two stay plain
    for s, (comp, want) in enumerate(zip(whole, plain)):
        assert (inflates_to(comp, want) if s < n_z and want else comp == want), s


def test_demux_emit_text(monkeypatch):
    sets = DT.Sets([("a0", b"ACGTACGTAC"), ("a_1", b"TTGGCCAATT")], [("b0", b"GGGGCCCCAAAA"), ("", b"CATCATCATCAT")])
    rng = np.random.default_rng(46)
    text = DT.text_of(4, sets, [int(x) for x in rng.integers(0, sets.S, 300)], [1000] * 300, rng)
    assert len(text) < 1 << 20
    h = _lib.Handle()

    def run(flags=OUT_BGZF | KEEP_QUALS):
        h.demux_text_reset()
        res = h.demux_emit_text(sets.sets, text, at_eof=True, flags=flags)
        assert res.guards_intact and res.untouched_beyond_results and res.info["n_kept"] == 300
        return res.streams(), h.demux_text_timing()["n_waits"]

    (whole, waits), (small, waits_small) = both_chunks(monkeypatch, run)
    (plain,), waits_plain = run(flags=KEEP_QUALS)
    h.close()
    assert len(plain) > 2 * BLOCK
    assert small == whole and inflates_to(whole[0], plain)
    chunks = (len(plain) + 2 * BLOCK - 1) // (2 * BLOCK)
    assert waits == waits_plain + 2 and waits_small == waits_plain + 2 * chunks          # two waits per compressed chunk


def test_emit_fetch(monkeypatch):
    h = _lib.Handle()
    h.set_splints([GE.SP, GE.SPLINT2])
    hb, sid, st = GE._batch(90, 7000)
    h.upload_host(hb, st, np.maximum(sid, 0))
    h.run(qv=True)
    eb = _lib.EmitBuffers()

    def run(bgzf=True):
        ns = h.emit_snapshot(hb, True, bgzf, True)
        buf, so = h.emit_fetch(eb, ns)
        return [buf.arr[int(so[x]):int(so[x + 1])].tobytes() for x in range(ns)]

    whole, small = both_chunks(monkeypatch, run)
    plain = run(bgzf=False)
    eb.close()
    h.close()
    assert len(plain) == 6 and max(len(x) for x in plain) > 2 * BLOCK and all(plain)
    assert small == whole
    for comp, want in zip(whole, plain):
        assert inflates_to(comp, want)

"""c3_emit_group_host, the host statement of k_emit (--emit gpu of the main CLI), against the writer that exists:
its streams are the files c3_write_group / c3_write_consensus_fastq make of the same group.  No GPU needed."""
import ctypes as C
import os

import numpy as np
import pytest

import emit_cases as EC
from c3poa_amd import _lib


@pytest.fixture(scope="module")
def groups():
    return {k: f().arrays() for k, f in EC.GROUPS.items()}


@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("with_qv", [False, True])
@pytest.mark.parametrize("which", sorted(EC.GROUPS))
def test_streams_equal_written_files(groups, tmp_path, which, with_qv, zero):
    hb, res, cons, coff, qv, sid = groups[which]
    want = EC.written_files(tmp_path, hb, res, cons, coff, qv if with_qv else None, sid, zero)
    got = _lib.emit_group_host(hb, res, cons, coff, qv if with_qv else None, sid, EC.N_SPLINTS, zero)
    assert got.K == (3 if with_qv else 2) and len(got.stream_off) == EC.N_SPLINTS * got.K + 1
    for x, (a, b) in enumerate(zip(got.streams(), want)):
        assert a == b, "stream %d of %s differs (first at %d)" % (x, which, next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), min(len(a), len(b))))
    if which == "main":
        assert all(len(w) > 0 for w in want) and got.n_records > 600
    else:
        assert got.n_records == 0 and int(got.stream_off[-1]) == 0


def test_without_consensus_bytes(groups, tmp_path):
    hb, res, cons, coff, qv, sid = groups["main"]
    want = EC.written_files(tmp_path, hb, res, None, coff, None, sid, True)
    got = _lib.emit_group_host(hb, res, None, None, None, sid, EC.N_SPLINTS, True)
    assert got.streams() == want and want[0] == b"" and want[1] != b""


def test_cases_cover_every_alignment_pair(groups):
    """the subread records of 0..9 bases of the main group meet every (source, destination) alignment pair on both copies"""
    hb, res, cons, coff, qv, sid = groups["main"]
    got = _lib.emit_group_host(hb, res, cons, coff, None, sid, EC.N_SPLINTS, True)
    at = {s: int(got.stream_off[s * 2 + 1]) for s in range(EC.N_SPLINTS)}
    seen = set()
    for i in range(hb.n):
        r = res[i]
        if not (0 <= sid[i] < EC.N_SPLINTS) or r["status"] in (1, 2, 4) or (r["n_sub"] == 0 and not (r["has_front"] and r["has_tail"])) or (r["n_sub"] and r["status"] == 5):
            continue
        nl, L, ns = int(hb.name_off[i + 1] - hb.name_off[i]), int(hb.off[i + 1] - hb.off[i]), int(r["n_sub"])
        pieces = [(k + 1, int(r["sub_beg"][k]), int(r["sub_end"][k])) for k in range(ns)] if ns else [(0, 0, int(r["front_end"])), (1, int(r["tail_beg"]), L)]
        if ns and r["has_front"]:
            pieces.append((0, 0, int(r["front_end"])))
        if ns and r["has_tail"]:
            pieces.append((ns + 1 if r["has_front"] else 0, int(r["tail_beg"]), L))
        for idx, b, e in pieces:
            body = at[int(sid[i])] + 1 + nl + 1 + len(str(idx)) + 1
            if e - b <= 9:
                seen.add((e - b, (int(hb.off[i]) + b) % 4, body % 4)); seen.add((e - b, (int(hb.off[i]) + b) % 4, (body + e - b + 3) % 4))
            at[int(sid[i])] = body + 2 * (e - b) + 4
    assert at == {s: int(got.stream_off[s * 2 + 2]) for s in range(EC.N_SPLINTS)}         # the walk above is the layout
    for ln in range(10):
        assert {(a, d) for l, a, d in seen if l == ln} == {(a, d) for a in range(4) for d in range(4)}, ln


def _avgq_header(tot, L):
    """the average-quality field of the consensus header for a read of L bases with quality sum tot + 33 * L"""
    g = EC.Group()
    g.add("q", L, 0, subs=[(0, L)], clen=1, name=b"n", qual=EC.qual_with(tot, L))
    hb, res, cons, coff, qv, sid = g.arrays()
    out = _lib.emit_group_host(hb, res, cons, coff, None, sid, 1, True).stream(0)
    return out.split(b"\n")[0].split(b"_")[1].decode()


def test_avgq_pins():
    for tot, L, txt in EC.AVGQ_PINS:
        assert str(round(tot / L, 2)) == txt
        assert _avgq_header(tot, L) == txt, (tot, L)


def test_avgq_text_exhaustive():
    """every 1 <= L <= 64 and -33 L <= tot <= 93 L, one group per L (a read per tot): the header field is str(round(tot / L, 2))"""
    for L in range(1, 65):
        tots = list(range(-33 * L, 93 * L + 1))
        n = len(tots)
        hb = _lib.HostBatch.from_lists([b"n"] * n, [b"A" * L] * n, [EC.qual_with(tot, L) for tot in tots])
        res = np.zeros(n, dtype=_lib.RESULT_DTYPE)
        res["n_sub"] = 1; res["sub_end"][:, 0] = L; res["cons_len"] = 1
        cons, coff, sid = np.full(n + 16, ord("C"), dtype=np.uint8), np.arange(n + 1, dtype=np.int64), np.zeros(n, dtype=np.int16)
        lines = _lib.emit_group_host(hb, res, cons, coff, None, sid, 1, True).stream(0).split(b"\n")[0::2]
        got = [ln.split(b"_")[1].decode() for ln in lines[:n]]
        want = [str(round(tot / L, 2)) for tot in tots]
        assert got == want, (L, next((t, a, b) for t, a, b in zip(tots, got, want) if a != b))


def test_limit_fills_stream_off_and_leaves_the_arena(groups):
    hb, res, cons, coff, qv, sid = groups["main"]
    full = _lib.emit_group_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    need = int(full.stream_off[-1])
    arena = np.full(need + 64, 0xA5, dtype=np.uint8)
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=need - 1, arena=arena)
    assert ei.value.code == _lib.E_LIMIT and "arena too small" in str(ei.value)
    assert list(ei.value.stream_off) == list(full.stream_off) and (arena == 0xA5).all()
    ok = _lib.emit_group_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=need, arena=arena)      # exactly enough: nothing behind it is touched
    assert ok.streams() == full.streams() and (arena[need:] == 0xA5).all()


REFUSALS = [
    ("n_sub above 250", lambda res, coff, hb: res["n_sub"].__setitem__(0, 251), "read 0: n_sub outside 0 .. 250"),
    ("n_sub negative", lambda res, coff, hb: res["n_sub"].__setitem__(0, -1), "read 0: n_sub outside 0 .. 250"),
    ("beg negative", lambda res, coff, hb: res["sub_beg"].__setitem__((0, 1), -1), "read 0: subread outside 0 <= beg <= end <= L"),
    ("end before beg", lambda res, coff, hb: res["sub_end"].__setitem__((0, 1), 99), "read 0: subread outside 0 <= beg <= end <= L"),
    ("end beyond L", lambda res, coff, hb: res["sub_end"].__setitem__((0, 2), 301), "read 0: subread outside 0 <= beg <= end <= L"),
    ("front_end beyond L", lambda res, coff, hb: res["front_end"].__setitem__(0, 301), "read 0: front_end outside the read"),
    ("front_end negative", lambda res, coff, hb: res["front_end"].__setitem__(0, -1), "read 0: front_end outside the read"),
    ("tail_beg beyond L", lambda res, coff, hb: res["tail_beg"].__setitem__(0, 301), "read 0: tail_beg outside the read"),
    ("tail_beg negative", lambda res, coff, hb: res["tail_beg"].__setitem__(0, -5), "read 0: tail_beg outside the read"),
    ("zero-repeat tail", lambda res, coff, hb: res["tail_beg"].__setitem__(1, 1000), "read 1: tail_beg outside the read"),
    ("cons_off falls", lambda res, coff, hb: coff.__setitem__(1, 10 ** 6), "read 1: cons_off not ascending"),
    ("cons_off start", lambda res, coff, hb: coff.__setitem__(0, -1), "offsets must start at 0"),
]


@pytest.mark.parametrize("what,spoil,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_validation_refusals(what, spoil, text):
    hb, res, cons, coff, qv, sid = EC.main_group().arrays()
    spoil(res, coff, hb)
    arena = np.full(1 << 20, 0xA5, dtype=np.uint8)
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True, cap=len(arena), arena=arena)
    assert ei.value.code == _lib.E_ARG and text in str(ei.value), str(ei.value)
    assert (arena == 0xA5).all()                                  # refused before anything is formatted


def test_more_refusals(groups):
    hb, res, cons, coff, qv, sid = groups["main"]
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_host(hb, res, cons, coff, None, sid, 65, True)
    assert ei.value.code == _lib.E_LIMIT and "more than 64 splints" in str(ei.value)
    with pytest.raises(_lib.C3Error) as ei:
        _lib.emit_group_host(hb, res, None, None, qv, sid, EC.N_SPLINTS, True)
    assert ei.value.code == _lib.E_ARG and "qv without cons" in str(ei.value)
    # a record that writes nothing is not looked at: rubbish in an unassigned read is no refusal
    hb, res, cons, coff, qv, sid = EC.nothing_kept_group().arrays()
    res["n_sub"][0] = 9999; res["front_end"][1] = -7
    assert _lib.emit_group_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True).n_records == 0


def test_append_streams_appends_at_the_end(groups, tmp_path):
    hb, res, cons, coff, qv, sid = groups["main"]
    got = _lib.emit_group_host(hb, res, cons, coff, qv, sid, EC.N_SPLINTS, True)
    paths = [str(tmp_path / ("f%d" % x)) for x in range(6)]
    for x, p in enumerate(paths[:4]):                             # four files exist with bytes in them, two do not exist yet
        open(p, "wb").write(b"OLD%d\n" % x)
    _lib.load().c3_writer_reset()
    _lib.append_streams(paths, got.arena.ctypes.data, got.stream_off)
    _lib.append_streams(paths[:3] + [None] * 3, got.arena.ctypes.data, got.stream_off)         # a second group; NULL paths are skipped
    for x, p in enumerate(paths):
        old = b"OLD%d\n" % x if x < 4 else b""
        assert open(p, "rb").read() == old + got.stream(x) * (2 if x < 3 else 1), x
    # the same bytes as the writer appends for the same group
    want = EC.written_files(tmp_path, hb, res, cons, coff, qv, sid, True)
    assert [open(p, "rb").read()[len(b"OLD0\n") if x < 4 else 0:][:len(want[x])] for x, p in enumerate(paths)] == want


def test_append_streams_reports_io_failure(tmp_path):
    arena = np.frombuffer(b"hello", dtype=np.uint8)
    with pytest.raises(OSError) as ei:
        _lib.append_streams([str(tmp_path / "no_such_dir" / "f")], arena.ctypes.data, np.array([0, 5]))
    assert "no_such_dir" in str(ei.value) and "No such file or directory" in str(ei.value)

"""CPU tests of the sample demultiplexer's host side (c3poa_amd/demux.py, c3_demux_host) against golden outputs made by
running the reference's own paper/Demultiplex_R2C2_reads.py (tests/golden/make_golden_demux.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from c3poa_amd import _lib, demux

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def demux_golden():
    return json.load(open(os.path.join(GOLD, "demux_cases.json")))["cases"]


def case_files(case, d):
    """input / Nextera / TSO paths of one golden case (texts written byte for byte, CR and CRLF kept)"""
    paths = []
    for key in ("input", "nextera", "tso"):
        v = case[key]
        if key != "input" and v.endswith(".fasta") and "\n" not in v:
            paths.append(os.path.join(GOLD, v))
            continue
        p = os.path.join(str(d), "%s_%s.fasta" % (case["name"], key))
        with open(p, "w", newline="") as f:
            f.write(v)
        paths.append(p)
    return paths


def write_text(path, text):
    with open(path, "w", newline="") as f:
        f.write(text)
    return str(path)


def lev_windows(head, idx):
    """textbook Levenshtein of idx against every window head[i : i+m], i < 300 - m (vectorised over the windows)"""
    m = len(idx)
    W = len(head) - m
    if m == 0:
        return np.zeros(W, dtype=np.int64)
    h = np.frombuffer(head, dtype=np.uint8).astype(np.int64)
    prev = np.repeat(np.arange(m + 1)[:, None], W, axis=1)         # prev[j]: row 0 (no index byte) over window prefix j
    for i in range(1, m + 1):
        cur = np.empty_like(prev)
        cur[0] = i
        for j in range(1, m + 1):
            sub = prev[j - 1] + (h[j - 1:j - 1 + W] != idx[i - 1])
            cur[j] = np.minimum(np.minimum(sub, prev[j] + 1), cur[j - 1] + 1)
        prev = cur
    return prev[m]


def test_read_fasta_semantics(tmp_path):
    text = (">r 1  \r\nACGT\r\n\r\nTT \n>r\t2\nGG\n  \n>r 1  \nCCC\rAA\n>x\n> \n A\n>empty\n")
    d = demux.read_fasta(write_text(tmp_path / "a.fa", text))
    # trailing whitespace of headers goes, inner spaces / tabs stay; a repeated header keeps its position and takes the
    # last record; a lone CR ends a line; blank and whitespace-only lines are skipped; leading spaces of sequence kept
    assert list(d.items()) == [("r 1", "CCCAA"), ("r\t2", "GG"), ("x", ""), ("", " A"), ("empty", "")]
    with pytest.raises(demux.DemuxError):
        demux.read_fasta(write_text(tmp_path / "b.fa", "ACGT\n>r\nACGT\n"))
    assert demux.read_fasta(write_text(tmp_path / "c.fa", "\n\n>r\nAC\nGT\n")) == {"r": "ACGT"}


def test_golden_through_host_statement(demux_golden, tmp_path):
    seen = set()
    for case in demux_golden:
        inp, nx, tso = case_files(case, tmp_path)
        got = demux.demultiplex(demux.read_fasta(inp), nx, tso, host=True)
        want = demux.read_fasta(write_text(tmp_path / ("%s_want.fa" % case["name"]), case["output"]))
        assert list(got.items()) == list(want.items()), case["name"]
        for name in got:
            f = name.rsplit("|", 1)[1]
            seen.add((f.startswith("_"), f.endswith("_")))
    assert seen == {(False, False), (True, False), (False, True), (True, True)}   # calls and no-calls in both sets


def test_write_fasta_file_matches_golden(demux_golden, tmp_path):
    for case in demux_golden:
        inp, nx, tso = case_files(case, tmp_path)
        out = tmp_path / case["name"]
        out.mkdir()
        demux.write_fasta_file(str(out), demux.demultiplex(demux.read_fasta(inp), nx, tso, host=True))
        with open(out / "Indexed_reads.fasta", "rb") as f:
            assert f.read() == case["output"].encode(), case["name"]


def test_batch_size_does_not_change_host_result(demux_golden, tmp_path):
    case = demux_golden[0]
    inp, nx, tso = case_files(case, tmp_path)
    reads = demux.read_fasta(inp)
    full = demux.demultiplex(reads, nx, tso, host=True)
    assert list(demux.demultiplex(reads, nx, tso, host=True, batch=7).items()) == list(full.items())


def test_host_distances_match_python_levenshtein():
    rng = np.random.default_rng(11)
    alphabet = np.array([0, 1, 10, 13, 32, 65, 67, 71, 78, 84, 97, 99, 103, 116, 200, 255], dtype=np.uint8)
    for trial in range(4):
        heads = rng.choice(alphabet, size=(3, 300)).astype(np.uint8)
        sets = []
        for s in range(2):
            k = int(rng.integers(2, 5))
            sets.append([bytes(rng.choice(alphabet, size=int(rng.integers(1, 33))).astype(np.uint8)) for _ in range(k)])
        # plant mutated copies of the indexes so that small distances occur
        for r in range(3):
            for s in range(2):
                ix = sets[s][int(rng.integers(0, len(sets[s])))]
                p = int(rng.integers(0, 300 - len(ix)))
                heads[r, p:p + len(ix)] = np.frombuffer(ix, dtype=np.uint8)
                heads[r, p + int(rng.integers(0, len(ix)))] = 99
        win, dist = _lib.demux_host(heads, sets[0], sets[1], return_dist=True)
        for r in range(3):
            want = [int(lev_windows(heads[r].tobytes(), np.frombuffer(ix, dtype=np.uint8).astype(np.int64)).min())
                    for ix in sets[0] + sets[1]]
            assert dist[r].tolist() == want, (trial, r)
            for s, (k0, ns) in enumerate(((0, len(sets[0])), (len(sets[0]), len(sets[1])))):
                d = want[k0:k0 + ns]
                order = sorted(range(ns), key=lambda k: d[k])
                call = order[0] if d[order[0]] < 4 and d[order[0]] < d[order[1]] - 1 else -1
                assert win[r, s] == call


def test_text_beyond_latin1_stays_exact(tmp_path):
    idx_a, idx_b = ["CAT\u2713GG", "TT\u00e9AA"], ["GG\u03b1CC", "ACGTA"]
    nx = write_text(tmp_path / "nx.fa", "".join(">a%d\n%s\n" % (i, s) for i, s in enumerate(idx_a)))
    tso = write_text(tmp_path / "tso.fa", "".join(">b%d\n%s\n" % (i, s) for i, s in enumerate(idx_b)))
    rng = np.random.default_rng(4)
    reads = {}
    for r in range(6):
        s = list("".join(rng.choice(list("ACGT\u2713\u00e9\u03b1\u4e00"), 400)))
        s[50:56] = list(idx_a[r % 2][:5] + "\u4e00")
        s[200:205] = list(idx_b[r % 2])
        reads["r%d" % r] = "".join(s)
    got = demux.demultiplex(reads, nx, tso, host=True)

    def lev(a, b):
        prev = list(range(len(b) + 1))
        for i, ca in enumerate(a, 1):
            cur = [i]
            for j, cb in enumerate(b, 1):
                cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
            prev = cur
        return prev[-1]

    for (name, seq), key in zip(reads.items(), got):
        fields = []
        for names, idx in ((["a0", "a1"], idx_a), (["b0", "b1"], idx_b)):
            d = [min(lev(x, seq[i:i + len(x)]) for i in range(300 - len(x))) for x in idx]
            o = sorted(range(2), key=lambda k: d[k])
            fields.append(names[o[0]] if d[o[0]] < 4 and d[o[0]] < d[o[1]] - 1 else "")
        assert key == "%s|%s_%s" % (name, fields[0], fields[1])


def test_empty_index_has_distance_zero():
    heads = np.full((1, 300), ord("A"), dtype=np.uint8)
    win, dist = _lib.demux_host(heads, [b"", b"CCCCCC"], [b"GG", b"TTT"], return_dist=True)
    assert dist.tolist() == [[0, 6, 2, 3]] and win.tolist() == [[0, -1]]


def _raw_host(heads, set_a, set_b):
    args, keep, res = _lib._demux_args(heads, set_a, set_b, False)
    lib = _lib.load()
    return lib.c3_demux_host(*args), lib.c3_last_error(None).decode()


def test_host_refusals(tmp_path):
    heads = np.zeros((2, 300), dtype=np.uint8)
    ok = [b"ACGT", b"TTGA"]
    rc, msg = _raw_host(heads, [b"ACGT"], ok)
    assert rc == -3 and "at least 2" in msg                                       # C3_E_ARG
    rc, msg = _raw_host(heads, ok, [b"A%03d" % i for i in range(129)])
    assert rc == -6 and "128" in msg                                              # C3_E_LIMIT
    rc, msg = _raw_host(heads, ok, [b"A" * 33, b"C"])
    assert rc == -6 and "32" in msg
    rc, msg = _raw_host(heads, ok, [bytes(range(100, 132)), b"C"])
    assert rc == -6 and "distinct" in msg
    assert _raw_host(heads, ok, [b"A" * 32, bytes(range(100, 127))])[0] == 0      # 31 distinct bytes, 32 long: accepted
    with pytest.raises(_lib.C3Error):
        _lib.demux_host(heads, ok, [b"A"])
    lib = _lib.load()
    off = np.zeros(3, dtype=np.int64)
    assert lib.c3_demux_host(2, None, 2, b"", off.ctypes.data, 2, b"", off.ctypes.data, None, None) == -3


def test_index_file_refusals(tmp_path):
    one = write_text(tmp_path / "one.fa", ">A1\nACGTACGT\n")
    two = write_text(tmp_path / "two.fa", ">A1\nACGTACGT\n>A2\nTTGACCAA\n")
    long_ = write_text(tmp_path / "long.fa", ">A1\n%s\n>A2\nTTGACCAA\n" % ("ACGT" * 9))
    for bad in (one, long_):
        with pytest.raises(demux.DemuxError):
            demux.demultiplex({"r": "A" * 400}, bad, two, host=True)
        with pytest.raises(demux.DemuxError):
            demux.demultiplex({"r": "A" * 400}, two, bad, host=True)


def test_cli_refusals_exit_nonzero(tmp_path):
    reads = write_text(tmp_path / "r.fa", ">r\n%s\n" % ("ACGT" * 100))
    one = write_text(tmp_path / "one.fa", ">A1\nACGTACGT\n")
    two = write_text(tmp_path / "two.fa", ">A1\nACGTACGT\n>A2\nTTGACCAA\n")
    headless = write_text(tmp_path / "h.fa", "ACGT\n>r\nACGT\n")
    cli = os.path.join(ROOT, "C3POa_demux.py")
    for inp, nx, tso in ((reads, one, two), (reads, two, one), (headless, two, two)):
        p = subprocess.run([sys.executable, cli, "-i", inp, "-o", str(tmp_path / "out"), "-n", nx, "-t", tso],
                           capture_output=True, text=True, timeout=120)
        assert p.returncode != 0 and "C3POa_demux:" in p.stderr
        assert not os.path.exists(tmp_path / "out" / "Indexed_reads.fasta")

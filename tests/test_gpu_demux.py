"""GPU tests of the sample demultiplexer: k_demux (c3_demux_indexes) against its host statement c3_demux_host, the
golden outputs of the reference's paper/Demultiplex_R2C2_reads.py through the device, and the CLI C3POa_demux.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from c3poa_amd import _lib, demux

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def handle():
    h = _lib.Handle()
    yield h
    h.close()


@pytest.fixture(scope="module")
def demux_golden():
    return json.load(open(os.path.join(GOLD, "demux_cases.json")))["cases"]


@pytest.fixture(scope="module")
def paper_sets():
    _, a = demux.load_indexes(os.path.join(GOLD, "demux_nextera.fasta"))
    _, b = demux.load_indexes(os.path.join(GOLD, "demux_tso.fasta"))
    return [s.encode() for s in a], [s.encode() for s in b]


def case_files(case, d):
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


def mutate(rng, s, edits, alphabet=b"ACGT"):
    s = bytearray(s)
    for _ in range(edits):
        op, p = int(rng.integers(0, 3)), int(rng.integers(0, max(1, len(s))))
        c = alphabet[int(rng.integers(0, len(alphabet)))]
        if op == 0 and s:
            s[p] = c
        elif op == 1:
            s.insert(p, c)
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def adversarial_heads(rng, sets, n, alphabet=b"ACGT"):
    """random heads with mutated copies of the indexes planted anywhere (both window edges included), ties, uniform and
    lowercase / N heads"""
    al = np.frombuffer(alphabet, dtype=np.uint8)
    heads = rng.choice(al, size=(n, 300)).astype(np.uint8)
    allidx = sets[0] + sets[1]
    for r in range(n):
        kind = r % 10
        if kind == 0:
            heads[r] = ord("N") if r % 20 == 0 else ord(alphabet[:1])
        elif kind == 1:
            heads[r] = np.frombuffer(bytes(rng.choice(np.frombuffer(b"acgtnN", dtype=np.uint8), 300)), dtype=np.uint8)
        for _ in range(int(rng.integers(0, 4))):
            ix = allidx[int(rng.integers(0, len(allidx)))]
            x = mutate(rng, ix, int(rng.integers(0, 6)), alphabet)[:299]
            where = int(rng.integers(0, 3))
            p = (300 - len(x) - 1, 300 - len(x), int(rng.integers(0, 301 - len(x))))[where]
            heads[r, p:p + len(x)] = np.frombuffer(x, dtype=np.uint8)
    return heads


def check_equal(handle, heads, sa, sb):
    win_d, dist_d = handle.demux_indexes(heads, sa, sb, return_dist=True)
    win_h, dist_h = _lib.demux_host(heads, sa, sb, return_dist=True)
    bad = np.nonzero((dist_d != dist_h).any(axis=1) | (win_d != win_h).any(axis=1))[0]
    assert bad.size == 0, "reads %s differ (first: dev %s / %s, host %s / %s)" % (
        bad[:10].tolist(), win_d[bad[0]].tolist(), dist_d[bad[0]].tolist(), win_h[bad[0]].tolist(), dist_h[bad[0]].tolist())
    assert np.array_equal(handle.demux_indexes(heads, sa, sb), win_h)           # without the matrix: same winners
    return win_d, dist_d


def test_paper_sets_match_host(handle, paper_sets):
    rng = np.random.default_rng(1)
    heads = adversarial_heads(rng, paper_sets, 2000)
    win, dist = check_equal(handle, heads, *paper_sets)
    assert (win[:, 0] >= 0).sum() > 100 and (win[:, 1] >= 0).sum() > 100 and (win < 0).sum() > 100
    assert dist.min() == 0 and dist.max() >= 8


def test_random_sets_match_host(handle):
    rng = np.random.default_rng(2)
    alphabet = bytes([0, 9, 10, 13, 32, 65, 67, 71, 78, 84, 97, 99, 103, 116, 128, 200, 254, 255])
    for trial, (na, nb, n) in enumerate([(2, 2, 300), (128, 3, 40), (5, 128, 40), (128, 128, 24), (37, 64, 64)]):
        sets = [[bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), int(rng.integers(1, 33))))
                 for _ in range(k)] for k in (na, nb)]
        al = alphabet
        if trial == 0:                                         # 31 distinct index bytes (the limit), a 32-byte index
            sets = [[bytes(range(100, 131)), b"d" * 5], [b"ef", bytes(range(130, 99, -1)) + b"d"]]
            al = bytes(range(95, 136))
        heads = adversarial_heads(rng, sets, n, al)
        check_equal(handle, heads, *sets)


def test_read_counts_off_the_workgroup(handle, paper_sets):
    rng = np.random.default_rng(3)
    heads = adversarial_heads(rng, paper_sets, 1003)
    full_w, full_d = _lib.demux_host(heads, *paper_sets, return_dist=True)
    for n in (1, 2, 7, 9, 13, 255, 257, 1003):
        w, d = handle.demux_indexes(heads[:n], *paper_sets, return_dist=True)
        assert np.array_equal(w, full_w[:n]) and np.array_equal(d, full_d[:n]), n
    assert handle.demux_indexes(heads[:0], *paper_sets).shape == (0, 2)


def test_golden_through_device(handle, demux_golden, tmp_path):
    for case in demux_golden:
        inp, nx, tso = case_files(case, tmp_path)
        reads = demux.read_fasta(inp)
        out = tmp_path / case["name"]
        out.mkdir()
        demux.write_fasta_file(str(out), demux.demultiplex(reads, nx, tso, handle=handle))
        with open(out / "Indexed_reads.fasta", "rb") as f:
            assert f.read() == case["output"].encode(), case["name"]
        for batch in (1, 5, 64):                               # batches smaller than the input: same result
            small = demux.demultiplex(reads, nx, tso, handle=handle, batch=batch)
            assert list(small.items()) == list(demux.demultiplex(reads, nx, tso, handle=handle).items()), (case["name"], batch)


def test_cli_matches_golden_and_refuses(demux_golden, tmp_path):
    cli = os.path.join(ROOT, "C3POa_demux.py")
    for case in demux_golden:
        inp, nx, tso = case_files(case, tmp_path)
        out = tmp_path / ("cli_" + case["name"]) / "new_dir"
        p = subprocess.run([sys.executable, cli, "-i", inp, "-o", str(out), "-n", nx, "-t", tso],
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        with open(out / "Indexed_reads.fasta", "rb") as f:
            assert f.read() == case["output"].encode(), case["name"]
    one = tmp_path / "one.fasta"
    one.write_text(">A1\nACGTACGTAC\n")
    inp, nx, tso = case_files(demux_golden[0], tmp_path)
    p = subprocess.run([sys.executable, cli, "-i", inp, "-o", str(tmp_path / "bad"), "-n", nx, "-t", str(one)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "at least 2" in p.stderr


def test_device_abi_errors(handle):
    lib = _lib.load()
    heads = np.zeros((4, 300), dtype=np.uint8)
    ok = [b"ACGT", b"TTGA"]
    for sa, sb, code, text in (([b"ACGT"], ok, -3, "at least 2"), (ok, [b"A%03d" % i for i in range(129)], -6, "128"),
                               (ok, [b"A" * 33, b"C"], -6, "32"), (ok, [bytes(range(100, 132)), b"C"], -6, "distinct")):
        args, keep, res = _lib._demux_args(heads, sa, sb, False)
        assert lib.c3_demux_indexes(handle.h, *args) == code
        assert text in lib.c3_last_error(handle.h).decode()
        with pytest.raises(_lib.C3Error):
            handle.demux_indexes(heads, sa, sb)
    args, keep, res = _lib._demux_args(heads, ok, ok, False)
    assert lib.c3_demux_indexes(None, *args) == -3
    assert handle.demux_indexes(heads, ok, ok).shape == (4, 2)          # the handle still works after the refusals

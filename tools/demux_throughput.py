#!/usr/bin/env python3
"""Throughput of the sample demultiplexer on N synthetic consensus reads (1-2 kb) that carry noisy copies of the paper's
Nextera and TSO indexes (0-4 edits) in their first 300 bases:
  kernel alone: Handle.demux_indexes over all heads in batches of demux.BATCH (timed after a warm-up call)
  CLI end to end: C3POa_demux.py as a child process (FASTA in -> Indexed_reads.fasta out), with the host phases
  (read_fasta / demultiplex / write_fasta_file) timed in process to show which side is the bound.
After the timed regions a sample of reads is checked against the host statement c3_demux_host (winners, distances and
the names the CLI wrote).  Prints one JSON line per measurement.
Usage: python tools/demux_throughput.py N [sample]"""
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c3poa_amd import _lib, demux  # noqa: E402

NX = os.path.join(ROOT, "tests", "golden", "demux_nextera.fasta")
TSO = os.path.join(ROOT, "tests", "golden", "demux_tso.fasta")


def noisy(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        op, p = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
        c = b"ACGT"[int(rng.integers(0, 4))]
        if op == 0:
            s[p] = c
        elif op == 1:
            s.insert(p, c)
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def make_reads(rng, n, set_a, set_b):
    """heads (n, 300) uint8 and read lengths; the tail of read i is a window of one shared random pool"""
    heads = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (n, 300))]
    pools = [[noisy(rng, s, e) for e in (0, 0, 1, 1, 2, 3, 4) for _ in range(8)] for s in set_a + set_b]
    na = len(set_a)
    ka, kb = rng.integers(0, na, n), rng.integers(0, len(set_b), n) + na
    va, vb = rng.integers(0, len(pools[0]), n), rng.integers(0, len(pools[0]), n)
    pa, pb = rng.integers(0, 120, n), rng.integers(150, 265, n)
    for i in range(n):
        x, y = pools[ka[i]][va[i]], pools[kb[i]][vb[i]]
        heads[i, pa[i]:pa[i] + len(x)] = np.frombuffer(x, dtype=np.uint8)
        heads[i, pb[i]:pb[i] + len(y)] = np.frombuffer(y, dtype=np.uint8)
    return heads, rng.integers(1000, 2001, n)


def write_fasta(path, heads, lens, pool):
    with open(path, "wb") as f:
        for b0 in range(0, len(lens), 65536):
            f.write(b"".join(b">r%08d_%d\n%s%s\n" % (i, lens[i], heads[i].tobytes(), pool[i % 4096: i % 4096 + lens[i] - 300])
                             for i in range(b0, min(len(lens), b0 + 65536))))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    n_sample = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    rng = np.random.default_rng(7)
    a_names, a_seqs = demux.load_indexes(NX)
    b_names, b_seqs = demux.load_indexes(TSO)
    set_a, set_b = [s.encode() for s in a_seqs], [s.encode() for s in b_seqs]
    t = time.time()
    heads, lens = make_reads(rng, n, set_a, set_b)
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4096 + 2000)].tobytes()
    t_gen = time.time() - t

    h = _lib.Handle(device=0)
    h.demux_indexes(heads[:demux.BATCH], set_a, set_b)            # warm-up: code object load, buffers
    t = time.time()
    win = np.concatenate([h.demux_indexes(heads[b0:b0 + demux.BATCH], set_a, set_b) for b0 in range(0, n, demux.BATCH)])
    dt_k = time.time() - t
    print(json.dumps({"demux_kernel_reads_per_s": round(n / dt_k), "reads": n, "seconds": round(dt_k, 3),
                      "batch": demux.BATCH, "called_both": int(((win >= 0).all(axis=1)).sum())}), flush=True)

    d = tempfile.mkdtemp(prefix="c3demux_")
    try:
        inp, out = os.path.join(d, "cons.fasta"), os.path.join(d, "out")
        write_fasta(inp, heads, lens, pool)
        cli = [sys.executable, os.path.join(ROOT, "C3POa_demux.py"), "-i", inp, "-o", out, "-n", NX, "-t", TSO]
        t = time.time()
        p = subprocess.run(cli, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000)
        dt_cli = time.time() - t
        if p.returncode != 0:
            sys.exit("CLI failed (%d): %s" % (p.returncode, p.stderr))
        # the CLI's phases, in process on the same handle
        t0 = time.time(); reads = demux.read_fasta(inp)
        t1 = time.time(); indexed = demux.demultiplex(reads, NX, TSO, handle=h)
        os.makedirs(os.path.join(d, "again"))
        t2 = time.time(); demux.write_fasta_file(os.path.join(d, "again"), indexed)
        t3 = time.time()
        print(json.dumps({"demux_cli_reads_per_s": round(n / dt_cli), "reads": n, "seconds": round(dt_cli, 2),
                          "in_process_s": {"read_fasta": round(t1 - t0, 2), "demultiplex": round(t2 - t1, 2),
                                           "write_fasta_file": round(t3 - t2, 2)}, "generate_s": round(t_gen, 1)}), flush=True)

        # sample check against the host statement, after the timed regions
        idx = np.sort(rng.choice(n, min(n, n_sample), replace=False))
        w_h, d_h = _lib.demux_host(heads[idx], set_a, set_b, return_dist=True)
        w_d, d_d = h.demux_indexes(heads[idx], set_a, set_b, return_dist=True)
        bad = int(((w_h != win[idx]).any(axis=1) | (w_h != w_d).any(axis=1) | (d_h != d_d).any(axis=1)).sum())
        names = []
        with open(os.path.join(out, "Indexed_reads.fasta")) as f:
            for line in f:
                if line.startswith(">"):
                    names.append(line[1:].rstrip("\n"))
        want = ["r%08d_%d|%s_%s" % (i, lens[i], (a_names + [""])[w_h[k, 0]], (b_names + [""])[w_h[k, 1]]) for k, i in enumerate(idx)]
        bad_cli = sum(names[i] != w for i, w in zip(idx, want)) if len(names) == n else len(idx)
        print(json.dumps({"sample": len(idx), "mismatches": bad + bad_cli, "kernel_mismatches": bad, "cli_mismatches": bad_cli}))
    finally:
        h.close()
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

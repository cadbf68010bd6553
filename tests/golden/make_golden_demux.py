#!/usr/bin/env python3
"""Golden vectors for the sample demultiplexer, made by RUNNING THE REFERENCE'S OWN SCRIPT
(paper/Demultiplex_R2C2_reads.py of rvolden/C3POa) on generated inputs.

Run beside a reference checkout:  python tests/golden/make_golden_demux.py <C3POa checkout>  ->  tests/golden/demux_cases.json,
plus the paper's two index files copied as fixtures (demux_nextera.fasta, demux_tso.fasta).
The script parses sys.argv and calls main() at module level, so it is run with runpy under a patched sys.argv; the one
package it imports that is not installed here, editdistance, is stubbed with a textbook Levenshtein.  What is pinned is
the reference's FASTA parsing, window rule, decision rule and output format.  Nothing else from the reference is copied:
inputs are generated, outputs are what the reference computes from them.  The tests read only the JSON and fixtures.
"""
import contextlib
import io
import json
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("C3POA_REFERENCE", "")
SCRIPT = os.path.join(REF, "paper", "Demultiplex_R2C2_reads.py")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True


def _lev(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


ed = types.ModuleType("editdistance"); ed.eval = _lev
sys.modules["editdistance"] = ed

rng = np.random.default_rng(5)
rnd = lambda n, al="ACGT": "".join(al[i] for i in rng.integers(0, len(al), n))  # noqa: E731


def mutate(s, edits):
    """`edits` random substitutions / insertions / deletions"""
    s = list(s)
    for _ in range(edits):
        op, p = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
        if op == 0:
            s[p] = "ACGT".replace(s[p], "")[int(rng.integers(0, 3))] if s[p] in "ACGT" else "A"
        elif op == 1:
            s.insert(p, "ACGT"[int(rng.integers(0, 4))])
        elif len(s) > 1:
            del s[p]
    return "".join(s)


def read_idx(path):
    out, name = [], None
    for line in open(path):
        line = line.rstrip()
        if line.startswith(">"):
            out.append([line[1:], ""])
        elif line:
            out[-1][1] += line
    return out


def place(head_len, total, items):
    """random read of `total` bases with (position, text) items written into its first head_len bases"""
    s = list(rnd(total))
    for pos, txt in items:
        s[pos:pos + len(txt)] = list(txt)
    return "".join(s)[:total] if len(s) >= total else "".join(s)


def records(reads, width=None, eol="\n"):
    out = []
    for name, seq in reads:
        out.append(">" + name + eol)
        if width:
            out += [seq[i:i + width] + eol for i in range(0, len(seq), width)]
        else:
            out.append(seq + eol)
    return "".join(out)


def paper_case(nx, tso):
    reads = []
    k = 0

    def name(tag):
        nonlocal k
        k += 1
        return "r%03d_%s" % (k, tag)

    for e1 in range(6):                                  # Nextera at 0..5 edits, TSO at 0..5 edits, anywhere in the head
        for rep in range(8):
            a, t = nx[int(rng.integers(0, len(nx)))][1], tso[int(rng.integers(0, len(tso)))][1]
            e2 = int(rng.integers(0, 6))
            pa, pt = int(rng.integers(0, 120)), int(rng.integers(150, 270))
            reads.append((name("e%d_%d" % (e1, e2)), place(300, int(rng.integers(301, 1500)), [(pa, mutate(a, e1)), (pt, mutate(t, e2))])))
    for rep in range(6):                                 # two indexes equally close -> no call
        i, j = rng.choice(len(nx), 2, replace=False)
        reads.append((name("tie"), place(300, 800, [(20, nx[i][1]), (80, nx[j][1]), (200, tso[rep % 8][1])])))
    for rep in range(6):                                 # runner-up exactly 1 worse -> no call (one edit vs. two)
        i, j = rng.choice(len(tso), 2, replace=False)
        reads.append((name("near"), place(300, 700, [(10, mutate(nx[rep][1], 1)), (60, mutate(nx[rep + 7][1], 2)),
                                                     (150, mutate(tso[i][1], 1)), (220, mutate(tso[j][1], 2))])))
    for rep in range(4):                                 # window 300-m-1 (searched) and 300-m (not searched)
        a, t = nx[rep][1], tso[rep][1]
        reads.append((name("edge_in"), place(300, 900, [(10, t), (300 - len(a) - 1, a)])))
        reads.append((name("edge_out"), place(300, 900, [(10, t), (300 - len(a), a)])))
        reads.append((name("edge_out_t"), place(300, 900, [(10, a), (300 - len(t), t)])))
    reads.append((name("len300"), place(300, 300, [(5, nx[0][1]), (100, tso[0][1])])))        # dropped
    reads.append((name("len301"), place(300, 301, [(5, nx[1][1]), (100, tso[1][1])])))        # kept
    reads.append((name("len299"), place(300, 299, [(5, nx[1][1])])))                          # dropped
    for rep in range(4):                                 # lowercase and N bytes: case-sensitive, N matches only N
        a, t = nx[rep + 2][1], tso[rep + 2][1]
        reads.append((name("lower"), place(300, 600, [(30, a.lower()), (130, t)])))
        an = a[:5] + "N" + a[6:]
        reads.append((name("N"), place(300, 600, [(30, an), (130, t[:3] + "NN" + t[5:])])))
        reads.append((name("lowbody"), place(300, 600, [(0, rnd(300, "acgtnN")), (40, a), (200, t)])))
    reads.append(("dup name", place(300, 700, [(10, nx[3][1]), (100, tso[3][1])])))           # a repeated header:
    reads.append((name("between"), place(300, 700, [(10, nx[4][1])])))
    reads.append(("dup name", place(300, 650, [(10, nx[5][1]), (100, tso[5][1])])))           # first position, last seq
    reads.append((name("tab\tin header "), place(300, 500, [(10, nx[6][1]), (100, tso[6][1])])))
    reads.append((name("spaces in header"), place(300, 500, [(10, nx[7][1]), (100, tso[7][1])])))
    head = records(reads[:60], width=60) + "\n" + records(reads[60:100]) + records(reads[100:], width=77, eol="\r\n")
    return head


def custom_case():
    """index files of its own: headers with spaces, a repeated header, lowercase and N in an index, CRLF, a lone CR,
    two indexes one edit apart"""
    nx = ">n 1\nACGTACGTTTGCA\n\n>n\t2\r\nGGATCCAAGT\r\n>n3\nTTTTTTTTTT\n>n4\nacgtacgtac\n>n3\nCAGNNCAGTT\n>n5\nAC\rGTTGCATGCA\n"
    tso = ">t1\nGGGGCCCCAAAA\n>t2\nGGGGCCCCAAAT\n>t3 x\nTGATGATGATGA\n"
    reads = []
    for i, (a, t) in enumerate([("ACGTACGTTTGCA", "TGATGATGATGA"), ("GGATCCAAGT", "GGGGCCCCAAAA"), ("CAGNNCAGTT", "GGGGCCCCAAAT"),
                                ("CAGAACAGTT", "TGATGATGATGA"), ("TTTTTTTTTT", "TGATGATGATGA"), ("acgtacgtac", "TGATGATGATGA"),
                                ("ACGTACGTAC", "TGATGATGATGA"), ("ACGTTGCATGCA", "TGATGATcATGA"), ("GTTGCATGCA", "TGATGA"),
                                ("ACGTACGTTTGCA", "GGGGCCCCTTTT")]):
        for e in range(2):
            reads.append(("c%02d_%d" % (i, e), place(300, 400 + 10 * i, [(int(rng.integers(0, 100)), mutate(a, e) if e else a),
                                                                        (int(rng.integers(150, 280)), t)])))
    return records(reads[:10], width=50) + records(reads[10:], eol="\r\n"), nx, tso


def empty_index_case():
    """an index with no sequence lines: distance 0 to every window (editdistance of two empty strings)"""
    nx = ">e0\n>e1\nACGTTGCAAC\n>e2\nTTGGCCAATT\n"
    tso = ">t1\nGGGGCCCCAAAA\n>t2\n\n>t3\nTGATGATGATGA\n"
    reads = [("z%d" % i, place(300, 500, [(40, "ACGTTGCAAC" if i % 2 else "TTGGCCAATT"), (120, "GGGGCCCCAAAA")])) for i in range(4)]
    return records(reads), nx, tso


def run_reference(inp, nx, tso):
    d = tempfile.mkdtemp()
    try:
        paths = {}
        for key, text in (("i", inp), ("n", nx), ("t", tso)):
            paths[key] = os.path.join(d, key + ".fasta")
            with open(paths[key], "w", newline="") as f:
                f.write(text)
        out = os.path.join(d, "out")
        os.mkdir(out)
        argv = sys.argv
        sys.argv = [SCRIPT, "-i", paths["i"], "-o", out, "-n", paths["n"], "-t", paths["t"]]
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                runpy.run_path(SCRIPT, run_name="__main__")
        finally:
            sys.argv = argv
        with open(os.path.join(out, "Indexed_reads.fasta"), newline="") as f:
            return f.read()
    finally:
        shutil.rmtree(d)


def main():
    if not os.path.isfile(SCRIPT):
        sys.exit("usage: make_golden_demux.py <C3POa checkout> (paper/Demultiplex_R2C2_reads.py not found)")
    shutil.copyfile(os.path.join(REF, "paper", "Nextera_Indexes.fasta"), os.path.join(HERE, "demux_nextera.fasta"))
    shutil.copyfile(os.path.join(REF, "paper", "TSO_Indexes.fasta"), os.path.join(HERE, "demux_tso.fasta"))
    nx_text = open(os.path.join(HERE, "demux_nextera.fasta")).read()
    tso_text = open(os.path.join(HERE, "demux_tso.fasta")).read()
    nx, tso = read_idx(os.path.join(HERE, "demux_nextera.fasta")), read_idx(os.path.join(HERE, "demux_tso.fasta"))
    cases = [{"name": "paper", "input": paper_case(nx, tso), "nextera": "demux_nextera.fasta", "tso": "demux_tso.fasta"}]
    inp, a, b = custom_case()
    cases.append({"name": "custom_indexes", "input": inp, "nextera": a, "tso": b})
    inp, a, b = empty_index_case()
    cases.append({"name": "empty_index", "input": inp, "nextera": a, "tso": b})
    for c in cases:
        a = nx_text if c["nextera"] == "demux_nextera.fasta" else c["nextera"]
        b = tso_text if c["tso"] == "demux_tso.fasta" else c["tso"]
        c["output"] = run_reference(c["input"], a, b)
        print(c["name"], c["output"].count(">"), "records", file=sys.stderr)
    with open(os.path.join(HERE, "demux_cases.json"), "w") as f:
        json.dump({"source": "paper/Demultiplex_R2C2_reads.py run on generated inputs (make_golden_demux.py)",
                   "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()

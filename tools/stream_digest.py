#!/usr/bin/env python3
"""sha256 of every file C3POa.py writes, over the modes that go through c3poa_amd/stream.py: run it on two builds of the
pipeline with the same native library and compare the listings (profiles/stream_refactor_digest.txt keeps one pair).

    python tools/stream_digest.py [--dir /dev/shm] [--timeout 300]

Input: 256 cfg1 reads and two splints (nobody uses Splint2), C3_GPU_BATCH_READS=64 -- four batches, so stage / commit and the
fetch beside the next run all happen.  Every mode is a child process of its own under `timeout`; the first non-zero status
ends the tool with that status.  One worker each, so the bytes do not depend on thread timing; the last mode (-n 2 on one
GPU, four byte ranges) appends in an order that does, and its files are hashed as sorted records.  The .gz files of -co are
hashed inflated: Python's gzip puts the time of day into their headers.  Needs one GPU."""
import argparse
import gzip
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np                          # noqa: E402

import bam_cases as B                       # noqa: E402
import test_inflate_host as H               # noqa: E402
from c3poa_amd import synth                 # noqa: E402

SPLINT2 = "".join("ACGT"[x] for x in np.random.default_rng(11).integers(0, 4, len(synth.SPLINT1)))     # nobody's splint
TWO = {"C3_DEVICE_MAP": "0,0", "C3_MIN_RANGE_BYTES": "1"}
# (name, output directory, input, whether the PSL is written beforehand, arguments, environment, what is hashed: raw | gunzip | sorted)
MODES = [("fused", "fused", "reads.fastq", False, [], {}, "raw"),
         ("fused_rerun", "fused", "reads.fastq", False, [], {}, "raw"),            # finds the PSL of the run before
         ("co", "co", "reads.fastq", True, ["-co"], {}, "gunzip"),
         ("bgzf", "bgzf", "reads.fastq", True, ["--bgzf"], {}, "raw"),
         ("consensus_fastq", "qv", "reads.fastq", True, ["--consensus-fastq"], {}, "raw"),
         ("emit_gpu", "emit", "reads.fastq", True, ["--emit", "gpu"], {}, "raw"),
         ("emit_gpu_bgzf_qv", "emit_all", "reads.fastq", True, ["--emit", "gpu", "--bgzf", "--consensus-fastq"], {}, "raw"),
         ("bgzf_in_inflate_parse_gpu", "bgzf_in", "reads.fastq.gz", True, ["--inflate", "gpu", "--parse", "gpu"], {}, "raw"),
         ("bam_in", "bam", "reads.bam", True, [], {}, "raw"),
         ("two_workers_sorted_records", "two", "reads.fastq", True, ["-n", "2"], TWO, "sorted")]


def digest(path, how):
    data = open(path, "rb").read()
    if how == "gunzip" and path.endswith(".gz"):
        data = gzip.decompress(data)
    if how == "sorted":                     # FASTA records are two lines here, FASTQ records four; anything else line by line
        lines = data.split(b"\n")
        k = 2 if path.endswith(".fasta") else 4 if path.endswith(".fastq") else 1
        data = b"\n".join(sorted(b"\n".join(lines[i:i + k]) for i in range(0, len(lines), k)))
    return hashlib.sha256(data).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--timeout", type=int, default=300, help="seconds each child may take")
    a = ap.parse_args()
    d = tempfile.mkdtemp(prefix="c3digest_", dir=a.dir)
    try:
        recs = list(synth.generate("cfg1", n_reads=256))
        text = "".join("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]) for r in recs).encode()
        bam = B.header(b"@HD\tVN:1.6\tSO:unsorted\n") + b"".join(B.record(r[0].encode(), r[1], bytes(ord(c) - 33 for c in r[2])) for r in recs)
        for name, data in (("reads.fastq", text), ("reads.fastq.gz", H.bgzf_file(text)), ("reads.bam", H.bgzf_file(bam)),
                           ("splint.fasta", (">Splint1\n%s\n>Splint2\n%s\n" % (synth.SPLINT1, SPLINT2)).encode())):
            with open(os.path.join(d, name), "wb") as fh:
                fh.write(data)
        for name, sub, reads, psl, extra, env, how in MODES:
            out = os.path.join(d, sub)
            os.makedirs(out + "/tmp", exist_ok=True)
            if psl:
                synth.write_psl(out + "/tmp/splint_to_read_alignments.psl", recs)
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", os.path.join(d, reads),
                   "-s", os.path.join(d, "splint.fasta"), "-o", out] + extra
            rc = subprocess.run(cmd, env=dict(os.environ, C3_GPU_BATCH_READS="64", **env), stdout=subprocess.DEVNULL).returncode
            if rc != 0:
                print("%s: exit status %d" % (name, rc), flush=True)
                return rc
            for dp, _dn, fns in sorted(os.walk(out)):
                for fn in sorted(fns):
                    p = os.path.join(dp, fn)
                    print("%s  %s/%s" % (digest(p, how), name, os.path.relpath(p, out)), flush=True)
        return 0
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())

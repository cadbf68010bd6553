#!/usr/bin/env python3
"""-r reads.bam with --inflate gpu --parse gpu (k_bam) against BGZF FASTQ of the same reads (k_fastq):
    python tools/bam_parse_throughput.py [--reads N] [--dir DIR] [--part P[,P]] [--parent TREE]

part "kernel" (N cfg2 reads, default 100 000): the native reader with the device parser under `rocprofv3 --kernel-trace
--stats`, a process of its own per file: on the .bam the k_bam kernels beside k_inflate of the same run, on the BGZF FASTQ of
the same reads the eight k_fastq kernels beside k_inflate; the chain kernels (header, guess, resolve, fill) are summed apart,
with the reads per tile that explain their time.
part "reader": the reader alone (every record delivered) with the device inflater and parser, BGZF FASTQ (the path that was
there before) against BAM, alternated twice, FASTQ first, each run a process of its own.
part "bench" (needs --parent TREE, a built checkout of the parent commit): bench.py --gpus 1 --steps 3 --warmup 1 in TREE and
here, alternated twice, parent first.
Both files are zlib level 6 BGZF with full members.  Every GPU step runs under a time limit; the first one that fails ends the
job.  Results are merged into profiles/bam_parse_throughput.json.  DIR should be a tmpfs (default /dev/shm)."""
import argparse
import csv
import glob
import json
import os
import shutil
import struct
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CODE = np.zeros(256, dtype=np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE[_c] = _i


def fastq_to_bam(fq, bam):
    """the 4-line FASTQ `fq` as the inflated bytes of an unaligned BAM without tags (flag 4, what a basecaller writes less its
    tags); returns (records, bytes)"""
    n = size = 0
    with open(fq, "rb") as src, open(bam, "wb") as dst:
        dst.write(b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 0))
        size = 12
        while True:
            h = src.readline()
            if not h:
                break
            s, _p, q = src.readline().rstrip(b"\n"), src.readline(), src.readline().rstrip(b"\n")
            name = h[1:].split()[0] + b"\0"
            c = CODE[np.frombuffer(s, dtype=np.uint8)]
            if len(c) & 1:
                c = np.append(c, np.uint8(0))
            packed = ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()
            qual = (np.frombuffer(q, dtype=np.uint8) - 33).astype(np.uint8).tobytes()
            body = struct.pack("<iiBBHHHIiii", -1, -1, len(name), 0, 4680, 0, 4, len(s), -1, -1, 0) + name + packed + qual
            dst.write(struct.pack("<I", len(body)) + body)
            size += 4 + len(body)
            n += 1
    return n, size


def child_reader(path):
    from c3poa_amd import _lib
    t0 = time.perf_counter()
    rd = _lib.Reader(path, n_sets=2, inflate_device=0, parse_device=True)
    n = bases = 0
    while True:
        hb = rd.next(65536, 0, 1 << 31)
        if hb.n == 0:
            break
        n += hb.n
        bases += int(hb.off[-1])
    wall = time.perf_counter() - t0
    print(json.dumps({"reads": n, "bases": bases, "wall_s": wall, "inflate_wait_s": rd.inflate_wait(), "parse_stats": rd.parse_stats()}), flush=True)
    rd.close()


def me(*a):
    return [sys.executable, os.path.abspath(__file__)] + list(a)


CHAIN = ("k_bam_header", "k_bam_guess", "k_bam_resolve", "k_bam_fill")


def kernel_rows(step, d, path, tag, want):
    pdir = d + "/prof_" + tag
    step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", tag, "--"] + me("--reader", path), 600, capture=False)
    rows = {}
    for f in glob.glob(pdir + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if want in r["Name"] or "k_inflate" in r["Name"]:
                rows[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6}
    if not any(want + "_gather" in k for k in rows):
        raise SystemExit("no %s_gather row in the kernel statistics" % want)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--part", default="all", help="kernel, reader, bench, a comma-separated list of them, or all")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (part bench)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_parse_throughput.json"))
    ap.add_argument("--reader", default=None)
    a = ap.parse_args()
    if a.reader:
        return child_reader(a.reader)
    parts = {"kernel", "reader", "bench"} if a.part == "all" else set(a.part.split(","))
    if not parts <= {"kernel", "reader", "bench"}:
        raise SystemExit("--part: kernel, reader, bench or all")
    if "bench" in parts and not a.parent:
        raise SystemExit("part bench needs --parent TREE")
    from bgzf_throughput import make_input
    from inflate_throughput import bgzip, step
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    d = tempfile.mkdtemp(prefix="c3bam_", dir=a.dir)
    try:
        if parts & {"kernel", "reader"}:
            fq = make_input(d, a.reads)
            fq_bytes = os.path.getsize(fq)
            n, bam_bytes = fastq_to_bam(fq, d + "/reads.unc")
            assert n == a.reads
            gz, bam = d + "/zlib6.fastq.gz", d + "/zlib6.bam"
            bgzip(fq, gz, 6)
            bgzip(d + "/reads.unc", bam, 6)
            os.remove(d + "/reads.unc")
            sizes = {"reads": a.reads, "fastq_bytes": fq_bytes, "bam_bytes": bam_bytes, "bam_over_fastq": bam_bytes / fq_bytes,
                     "fastq_gz_bytes": os.path.getsize(gz), "bam_file_bytes": os.path.getsize(bam), "reads_per_tile": a.reads / (bam_bytes / 65536)}
            if "kernel" in parts:
                kb, kf = kernel_rows(step, d, bam, "bam", "k_bam"), kernel_rows(step, d, gz, "fastq", "k_fastq")
                tot = lambda rows, sel: sum(v["total_ms"] for k, v in rows.items() if sel(k))      # noqa: E731
                res["kernel"] = dict(sizes, bam_kernels=kb, fastq_kernels=kf,
                                     k_bam_total_ms=tot(kb, lambda k: "k_bam" in k), k_bam_chain_ms=tot(kb, lambda k: any(c in k for c in CHAIN)),
                                     k_bam_gather_ms=tot(kb, lambda k: "k_bam_gather" in k), k_inflate_ms_bam_run=tot(kb, lambda k: "k_inflate" in k),
                                     k_fastq_total_ms=tot(kf, lambda k: "k_fastq" in k), k_inflate_ms_fastq_run=tot(kf, lambda k: "k_inflate" in k))
                res["kernel"]["chain_longer_than_inflate"] = res["kernel"]["k_bam_chain_ms"] > res["kernel"]["k_inflate_ms_bam_run"]
                print(json.dumps(res["kernel"]), flush=True)
                save()
            if "reader" in parts:
                runs = []
                for rep in range(2):
                    for name, path in (("fastq_bgzf", gz), ("bam", bam)):
                        r = step(me("--reader", path), 300)
                        assert r["reads"] == a.reads and r["parse_stats"][1] == 0
                        runs.append({"run": name, "rep": rep, "wall_s": r["wall_s"], "reads_per_s": a.reads / r["wall_s"],
                                     "inflate_wait_s": r["inflate_wait_s"], "parse_stats": r["parse_stats"]})
                        print(json.dumps(runs[-1]), flush=True)
                rate = {t: [r["reads_per_s"] for r in runs if r["run"] == t] for t in ("fastq_bgzf", "bam")}
                spread = max(max(v) / min(v) - 1 for v in rate.values())
                res["reader"] = dict(sizes, runs=runs, best_reads_per_s={t: max(v) for t, v in rate.items()}, spread_of_the_alternation=spread,
                                     bam_not_slower_beyond_the_spread=max(rate["bam"]) >= max(rate["fastq_bgzf"]) * (1 - spread))
                print(json.dumps(res["reader"]), flush=True)
                save()
        if "bench" in parts:
            runs = []
            for rep in range(2):
                for name, tree in (("parent", os.path.abspath(a.parent)), ("change", ROOT)):
                    r = step([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"], 900)
                    runs.append({"run": name, "rep": rep, "result": r})
                    print(json.dumps(runs[-1]), flush=True)
            res["bench"] = {"command": "bench.py --gpus 1 --steps 3 --warmup 1", "runs": runs}
            save()
    finally:
        shutil.rmtree(d, ignore_errors=True)
    save()


if __name__ == "__main__":
    main()

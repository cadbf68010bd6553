#!/usr/bin/env python3
"""--parse gpu against the reader's host parser:  python tools/fastq_parse_throughput.py [--reads N] [--cli-reads M] [--dir DIR] [--part P[,P]]

part "kernel" (N cfg2 reads, default 100 000, ~1 GB of FASTQ as a zlib level 6 BGZF file): the native reader with the device
parser under `rocprofv3 --kernel-trace --stats` in a process of its own: the k_fastq kernels and k_inflate, per pass over the
file, with the bytes the gather moves per second.
part "reader": the reader alone (every record delivered), host parser against device parser, both with the device inflater,
alternated twice, each run a process of its own.
part "cli" (M cfg2 reads, default 1 000 000): the command line, exec to exit, on the plain file, with --inflate gpu and with
--inflate gpu --parse gpu, alternated twice.
Every GPU step runs under a time limit; the first one that fails ends the job.  Results are merged into
profiles/fastq_parse_throughput.json.  DIR should be a tmpfs (default /dev/shm)."""
import argparse
import csv
import glob
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child_reader(path, parse):
    from c3poa_amd import _lib
    t0 = time.perf_counter()
    rd = _lib.Reader(path, n_sets=2, inflate_device=0, parse_device=parse)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--cli-reads", type=int, default=1000000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--part", default="all", help="kernel, reader, cli, a comma-separated list of them, or all")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fastq_parse_throughput.json"))
    ap.add_argument("--reader", default=None)
    ap.add_argument("--parse", action="store_true")
    a = ap.parse_args()
    if a.reader:
        return child_reader(a.reader, a.parse)
    parts = {"kernel", "reader", "cli"} if a.part == "all" else set(a.part.split(","))
    if not parts <= {"kernel", "reader", "cli"}:
        raise SystemExit("--part: kernel, reader, cli or all")
    from bgzf_throughput import make_input
    from inflate_throughput import bgzip, step
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    d = tempfile.mkdtemp(prefix="c3fq_", dir=a.dir)
    try:
        if parts & {"kernel", "reader"}:
            fq = make_input(d, a.reads)
            text_bytes = os.path.getsize(fq)
            gz = d + "/zlib6.fastq.gz"
            bgzip(fq, gz, 6)
            if "kernel" in parts:
                pdir = d + "/prof"
                step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "fastq", "--"] + me("--reader", gz, "--parse"),
                     600, capture=False)
                rows = {}
                for f in glob.glob(pdir + "/**/*kernel_stats.csv", recursive=True):
                    for r in csv.DictReader(open(f)):
                        if "k_fastq" in r["Name"] or "k_inflate" in r["Name"]:
                            rows[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6}
                if not any("k_fastq_gather" in k for k in rows):
                    raise SystemExit("no k_fastq_gather row in the kernel statistics")
                gather_ms = sum(v["total_ms"] for k, v in rows.items() if "k_fastq_gather" in k)
                res["kernel"] = {"reads": a.reads, "text_bytes": text_bytes, "kernels": rows,
                                 "k_fastq_total_ms": sum(v["total_ms"] for k, v in rows.items() if "k_fastq" in k),
                                 "gather_gb_per_s_read_plus_written": 2 * text_bytes / (gather_ms * 1e-3) / 1e9}
                print(json.dumps(res["kernel"]), flush=True)
            if "reader" in parts:
                runs = []
                for rep in range(2):
                    for name, parse in (("host_parse", False), ("device_parse", True)):
                        r = step(me("--reader", gz) + (["--parse"] if parse else []), 300)
                        assert r["reads"] == a.reads
                        runs.append({"run": name, "rep": rep, "wall_s": r["wall_s"], "reads_per_s": a.reads / r["wall_s"],
                                     "gb_per_s": text_bytes / r["wall_s"] / 1e9, "inflate_wait_s": r["inflate_wait_s"], "parse_stats": r["parse_stats"]})
                        print(json.dumps(runs[-1]), flush=True)
                best = {t: max(r["reads_per_s"] for r in runs if r["run"] == t) for t in ("host_parse", "device_parse")}
                res["reader"] = {"reads": a.reads, "text_bytes": text_bytes, "runs": runs, "best_reads_per_s": best}
            json.dump(res, open(a.out, "w"), indent=1)
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d, exist_ok=True)
        if "cli" in parts:
            fq = make_input(d, a.cli_reads)
            bgzip(fq, d + "/reads.fastq.gz", 6)
            runs = []
            for rep in range(2):
                for tag, reads, extra in (("plain", "reads.fastq", []), ("inflate_gpu", "reads.fastq.gz", ["--inflate", "gpu"]),
                                          ("inflate_parse_gpu", "reads.fastq.gz", ["--inflate", "gpu", "--parse", "gpu"])):
                    out = d + "/out_" + tag
                    shutil.rmtree(out, ignore_errors=True)
                    os.makedirs(out + "/tmp")
                    shutil.copy(d + "/reads.psl", out + "/tmp/splint_to_read_alignments.psl")
                    t0 = time.perf_counter()
                    step([sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", d + "/" + reads, "-s", d + "/splint.fasta", "-o", out] + extra, 600, capture=False)
                    wall = time.perf_counter() - t0
                    runs.append({"run": tag, "rep": rep, "wall_s": wall, "reads_per_s": a.cli_reads / wall})
                    print(json.dumps(runs[-1]), flush=True)
                    shutil.rmtree(out, ignore_errors=True)
            res["cli"] = {"reads": a.cli_reads, "runs": runs,
                          "best_wall_s": {t: min(r["wall_s"] for r in runs if r["run"] == t) for t in ("plain", "inflate_gpu", "inflate_parse_gpu")}}
            print(json.dumps(res["cli"]), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

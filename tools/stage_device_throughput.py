#!/usr/bin/env python3
"""The reader's device sets against its page-locked host sets:  python tools/stage_device_throughput.py [--reads N] [--dir DIR]

N cfg2 reads (default 100 000, ~1 GB of FASTQ as a zlib level 6 BGZF file): the reader alone with the device
parser, host sets (the parent path) against device sets, alternated twice, each run a process of its own; with the page-locked
bytes each holds at the end.
Every GPU step runs under a time limit; the first one that fails ends the job.  Results are merged into
profiles/stage_device_throughput.json.  DIR should be a tmpfs (default /dev/shm)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def child_reader(path, stage):
    from c3poa_amd import _lib
    t0 = time.perf_counter()
    rd = _lib.Reader(path, n_sets=4, inflate_device=0, parse_device=True, stage_device=stage)
    n = bases = 0
    while True:
        hb = rd.next(65536, 0, 1 << 31)
        if hb.n == 0:
            break
        assert (hb.dev is not None) == stage
        n += hb.n
        bases += int(hb.off[-1])
    wall = time.perf_counter() - t0
    print(json.dumps({"reads": n, "bases": bases, "wall_s": wall, "inflate_wait_s": rd.inflate_wait(), "parse_stats": rd.parse_stats(),
                      "stage_stats": rd.stage_stats(), "page_locked_bytes": rd.reserved_bytes()}), flush=True)
    rd.close()


def me(*a):
    return [sys.executable, os.path.abspath(__file__)] + list(a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stage_device_throughput.json"))
    ap.add_argument("--reader", default=None)
    ap.add_argument("--stage", action="store_true")
    a = ap.parse_args()
    if a.reader:
        return child_reader(a.reader, a.stage)
    from bgzf_throughput import make_input
    from inflate_throughput import bgzip, step
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    d = tempfile.mkdtemp(prefix="c3st_", dir=a.dir)
    try:
        fq = make_input(d, a.reads)
        text_bytes = os.path.getsize(fq)
        gz = d + "/zlib6.fastq.gz"
        bgzip(fq, gz, 6)
        os.remove(fq)
        runs = []
        for rep in range(2):
            for name, stage in (("host_sets", False), ("device_sets", True)):
                r = step(me("--reader", gz) + (["--stage"] if stage else []), 300)
                assert r["reads"] == a.reads
                runs.append(dict(r, run=name, rep=rep, reads_per_s=a.reads / r["wall_s"], gb_per_s=text_bytes / r["wall_s"] / 1e9))
                print(json.dumps(runs[-1]), flush=True)
        res["reader"] = {"reads": a.reads, "text_bytes": text_bytes, "runs": runs,
                         "best_reads_per_s": {t: max(r["reads_per_s"] for r in runs if r["run"] == t) for t in ("host_sets", "device_sets")},
                         "page_locked_bytes": {t: max(r["page_locked_bytes"] for r in runs if r["run"] == t) for t in ("host_sets", "device_sets")}}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""c3_gunzip against zlib on plain gzip:  python tools/gunzip_throughput.py [--reads N] [--dir DIR] [--reps R]

N cfg2 reads (default 100 000, ~1 GB of FASTQ) as one `gzip -6` stream (zlib level 6, one member).  Measured, every GPU step a
process of its own under a time limit, the first failure ending the job:
  kernels   the four k_gunzip kernels under `rocprofv3 --kernel-trace --stats` (kernel time per pass over the file, GB/s of
            inflated text), and k_inflate the same way on the same text as a BGZF file (bgzip layout, level 6)
  call      c3_gunzip with the profiler off (host wall time, copies included, pageable buffers), at the default piece size
            and at C3_GUNZIP_PIECE 1024 .. 16384, alternated with one zlib stream inflating the same file on one CPU thread
  reader    the native reader alone on that file, every record delivered: gzread (the parent's path) against
            c3_reader_gunzip_on_device, alone and with the device parser, alternated twice (--part reader runs this alone and merges into the JSON)
Results go to profiles/gunzip_throughput.json.  Not measured here: the command line, disk instead of tmpfs, files above 4 GiB.  DIR should be a tmpfs (default /dev/shm)."""
import argparse
import csv
import glob
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from inflate_throughput import bgzip, me as _me, step      # noqa: E402

KERNELS = ("k_gunzip_find", "k_gunzip_decode", "k_gunzip_window", "k_gunzip_resolve")


def me(*a):
    return [sys.executable, os.path.abspath(__file__)] + list(a)


def child_call(path, reps, text_bytes):
    """c3_gunzip of the file's bytes (pageable buffers, as a caller of the C ABI holds them): warm-up + reps"""
    import ctypes as C
    import numpy as np
    from c3poa_amd import _lib
    lib = _lib.load()
    data = np.fromfile(path, dtype=np.uint8)
    dst = np.empty(text_bytes, dtype=np.uint8)
    dst[::4096] = 0
    z = _lib.Bgzf(0)
    olen = C.c_int64(0)
    walls = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        rc = lib.c3_gunzip(z.z, data.ctypes.data, len(data), dst.ctypes.data, text_bytes, C.byref(olen))
        assert rc == 0 and olen.value == text_bytes, (rc, olen.value)
        if k:
            walls.append(time.perf_counter() - t0)
    st = _lib.gunzip_stats()
    z.close()
    print(json.dumps({"bytes_in": len(data), "bytes_out": text_bytes, "crc32": zlib.crc32(dst.tobytes()), "wall_s": walls, "stats": st}), flush=True)


def child_reader(path, gunzip, parse=False):
    """the native reader alone, every record delivered: gzread (the parent's path) or c3_reader_gunzip_on_device"""
    from c3poa_amd import _lib
    t0 = time.perf_counter()
    rd = _lib.Reader(path, n_sets=2, inflate_device=0 if gunzip else None, gunzip_device=gunzip, parse_device=parse)
    n = 0
    while True:
        hb = rd.next(65536, 0, 1 << 31)
        if hb.n == 0:
            break
        n += hb.n
    wall = time.perf_counter() - t0
    print(json.dumps({"reads": n, "wall_s": wall, "inflate_wait_s": rd.inflate_wait(), "stats": rd.gunzip_stats()}), flush=True)
    rd.close()


def child_zlib(path, reps):
    data = open(path, "rb").read()
    walls = []
    for _k in range(reps):
        t0 = time.perf_counter()
        out = zlib.decompress(data, 31)
        walls.append(time.perf_counter() - t0)
    print(json.dumps({"bytes_out": len(out), "crc32": zlib.crc32(out), "wall_s": walls}), flush=True)


def kernel_stats(d, args, names):
    pdir = d + "/prof"
    shutil.rmtree(pdir, ignore_errors=True)
    step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "gunzip", "--"] + args, 600, capture=False)
    rows = {}
    for f in glob.glob(pdir + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            for n in names:
                if r["Name"].startswith(n + "("):
                    rows[n] = {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"])}
    if set(rows) != set(names):
        raise SystemExit("kernel statistics lack %s" % sorted(set(names) - set(rows)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gunzip_throughput.json"))
    ap.add_argument("--call", default=None)
    ap.add_argument("--zlib", default=None)
    ap.add_argument("--reader", default=None)
    ap.add_argument("--gunzip", action="store_true")
    ap.add_argument("--parse", action="store_true")
    ap.add_argument("--part", choices=["call", "reader", "all"], default="all")
    ap.add_argument("--text-bytes", type=int, default=0)
    a = ap.parse_args()
    if a.call:
        return child_call(a.call, a.reps, a.text_bytes)
    if a.zlib:
        return child_zlib(a.zlib, a.reps)
    if a.reader:
        return child_reader(a.reader, a.gunzip, a.parse)
    from bgzf_throughput import make_input
    d = tempfile.mkdtemp(prefix="c3gz_", dir=a.dir)
    try:
        fq = make_input(d, a.reads)
        text_bytes = os.path.getsize(fq)
        gzp, bgz = d + "/reads.fastq.gz", d + "/reads.bgzf.gz"
        co = zlib.compressobj(6, zlib.DEFLATED, 31)
        with open(fq, "rb") as f, open(gzp, "wb") as g:
            for blk in iter(lambda: f.read(1 << 24), b""):
                g.write(co.compress(blk))
            g.write(co.flush())
        bgzip(fq, bgz, 6)
        res = json.load(open(a.out)) if os.path.exists(a.out) else {}
        res.update({"reads": a.reads, "text_bytes": text_bytes, "gzip_bytes": os.path.getsize(gzp)})
        if a.part in ("reader", "all"):
            res["reader"] = []
            for rep in range(2):
                for tag, extra in (("gunzip host (gzread)", []), ("gunzip gpu", ["--gunzip"]), ("gunzip gpu, parse gpu", ["--gunzip", "--parse"])):
                    r = step(me("--reader", gzp) + extra, 600)
                    assert r["reads"] == a.reads
                    res["reader"].append({"run": tag, "rep": rep, "wall_s": r["wall_s"], "reads_per_s": a.reads / r["wall_s"],
                                          "inflate_wait_s": r["inflate_wait_s"], "stats": r["stats"]})
                    print(json.dumps(res["reader"][-1]), flush=True)
            if a.part == "reader":
                json.dump(res, open(a.out, "w"), indent=1)
                return
        passes = a.reps + 1
        ks = kernel_stats(d, me("--call", gzp, "--reps", str(a.reps), "--text-bytes", str(text_bytes)), KERNELS)
        res["kernels"] = {n: {"ms_per_pass": r["total_ns"] / 1e6 / passes, "launches_per_pass": r["calls"] / passes} for n, r in ks.items()}
        tot = sum(r["ms_per_pass"] for r in res["kernels"].values())
        res["kernels_ms_per_pass"] = tot
        res["kernels_gb_per_s"] = text_bytes / (tot * 1e-3) / 1e9
        ki = kernel_stats(d, _me("--device-call", bgz, "--reps", str(a.reps)), ("k_inflate",))["k_inflate"]
        res["k_inflate_same_text_bgzf"] = {"ms_per_pass": ki["total_ns"] / 1e6 / passes, "gb_per_s": text_bytes / (ki["total_ns"] / 1e9 / passes) / 1e9}
        res["call"] = []
        for rep in range(2):
            for piece in ("default", "1024", "2048", "4096", "8192", "16384"):
                r = step(me("--call", gzp, "--reps", str(a.reps), "--text-bytes", str(text_bytes)), 600, env={} if piece == "default" else {"C3_GUNZIP_PIECE": piece})
                res["call"].append({"piece": piece, "rep": rep, "wall_s": r["wall_s"], "gb_per_s_best": text_bytes / min(r["wall_s"]) / 1e9, "stats": r["stats"]})
                print(json.dumps(res["call"][-1]), flush=True)
            r = step(me("--zlib", gzp, "--reps", str(a.reps)), 600)
            res["call"].append({"piece": "zlib, one stream", "rep": rep, "wall_s": r["wall_s"], "gb_per_s_best": text_bytes / min(r["wall_s"]) / 1e9})
            print(json.dumps(res["call"][-1]), flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
        print(json.dumps({k: res[k] for k in ("kernels", "kernels_gb_per_s", "k_inflate_same_text_bgzf")}), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""--inflate gpu against the zlib threads:  python tools/inflate_throughput.py [--reads N] [--cli-reads M] [--dir DIR] [--part P]

part "kernel" (N cfg2 reads, default 100 000, ~1 GB of FASTQ): the text as a BGZF file made by zlib level 6 (bgzip layout)
and as one made by k_bgzf.  For each file: k_inflate under `rocprofv3 --kernel-trace --stats` in a process of its own (kernel
time, GB/s of inflated bytes), c3_bgzf_decompress with the profiler off (host wall time of the call, copies included), and
the native reader alone (every record parsed) with the zlib threads at C3_GZ_THREADS 8 and 16 and with the device inflater,
alternated twice.
part "cli" (M cfg2 reads, default 1 000 000): the command line, exec to exit, on the BGZF file with --inflate host, with
--inflate gpu, and on the plain file, alternated twice.
Every GPU step is a process of its own under a time limit; the first one that fails ends the job.  Results are merged into
profiles/inflate_throughput.json.  DIR should be a tmpfs (default /dev/shm)."""
import argparse
import csv
import glob
import json
import multiprocessing as mp
import os
import shutil
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _bgzip_chunk(job):
    path, beg, end, level = job
    with open(path, "rb") as f:
        f.seek(beg)
        data = f.read(end - beg)
    out = []
    for i in range(0, len(data), 0xff00):
        chunk = data[i:i + 0xff00]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = co.compress(chunk) + co.flush()
        out.append(struct.pack("<BBBBIBBH", 0x1f, 0x8b, 8, 4, 0, 0, 0xff, 6) + b"BC" + struct.pack("<HH", 2, len(comp) + 25) + comp
                   + struct.pack("<II", zlib.crc32(chunk), len(chunk)))
    return b"".join(out)


def bgzip(src, dst, level=6, procs=16):
    size = os.path.getsize(src)
    step = 0xff00 * 256
    with mp.Pool(procs) as pool, open(dst, "wb") as f:
        for part in pool.imap(_bgzip_chunk, [(src, b, min(b + step, size), level) for b in range(0, size, step)]):
            f.write(part)
        f.write(EOF_MEMBER)


# ---- child processes (each one GPU step) -------------------------------------------------------------------------------
def child_make_kbgzf(src, dst):
    import numpy as np
    from c3poa_amd import _lib
    z = _lib.Bgzf(0)
    with open(dst, "wb") as f:
        f.write(z.compress(np.fromfile(src, dtype=np.uint8).tobytes()))
        f.write(EOF_MEMBER)
    z.close()


def child_device_call(path, reps):
    """c3_bgzf_decompress of the file's bytes (pageable buffers, as a caller of the C ABI holds them): warm-up + reps"""
    import ctypes as C
    import numpy as np
    from c3poa_amd import _lib
    lib = _lib.load()
    data = np.fromfile(path, dtype=np.uint8)
    nm, ob = _lib.bgzf_scan(data.tobytes())
    dst = np.empty(ob, dtype=np.uint8)
    dst[::4096] = 0
    z = _lib.Bgzf(0)
    olen = C.c_int64(0)
    walls = []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        assert lib.c3_bgzf_decompress(z.z, data.ctypes.data, len(data), dst.ctypes.data, ob, C.byref(olen)) == 0 and olen.value == ob
        if k:
            walls.append(time.perf_counter() - t0)
    z.close()
    print(json.dumps({"bytes_in": len(data), "bytes_out": ob, "members": nm, "crc32": zlib.crc32(dst.tobytes()), "wall_s": walls}), flush=True)


def child_reader(path, device):
    from c3poa_amd import _lib
    t0 = time.perf_counter()
    rd = _lib.Reader(path, n_sets=2, inflate_device=0 if device else None)
    n = 0
    while True:
        hb = rd.next(65536, 0, 1 << 31)
        if hb.n == 0:
            break
        n += hb.n
    wall = time.perf_counter() - t0
    print(json.dumps({"reads": n, "wall_s": wall, "inflate_wait_s": rd.inflate_wait()}), flush=True)
    rd.close()


def step(args, limit, env=None, capture=True):
    """one child process under a time limit; a failure ends the job (nothing more is started on the GPU)"""
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + args, env=e, capture_output=capture, text=True)
    if r.returncode != 0:
        sys.stderr.write((r.stderr or "")[-2000:])
        raise SystemExit("step failed (%d): %s" % (r.returncode, " ".join(args)))
    return json.loads(r.stdout.strip().splitlines()[-1]) if capture and r.stdout.strip() else None


def me(*a):
    return [sys.executable, os.path.abspath(__file__)] + list(a)


def kernel_stats(d, path, reps):
    pdir = d + "/prof"
    shutil.rmtree(pdir, ignore_errors=True)
    step(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "inflate", "--"] + me("--device-call", path, "--reps", str(reps)),
         600, capture=False)
    for f in glob.glob(pdir + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_inflate" in r["Name"]:
                return {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "avg_ns": float(r["AverageNs"])}
    raise SystemExit("no k_inflate row in the kernel statistics")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--cli-reads", type=int, default=1000000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--part", choices=["kernel", "cli", "all"], default="all")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate_throughput.json"))
    ap.add_argument("--make-kbgzf", nargs=2, default=None)
    ap.add_argument("--device-call", default=None)
    ap.add_argument("--reader", default=None)
    ap.add_argument("--device", action="store_true")
    a = ap.parse_args()
    if a.make_kbgzf:
        return child_make_kbgzf(*a.make_kbgzf)
    if a.device_call:
        return child_device_call(a.device_call, a.reps)
    if a.reader:
        return child_reader(a.reader, a.device)
    from bgzf_throughput import make_input
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    d = tempfile.mkdtemp(prefix="c3inf_", dir=a.dir)
    try:
        if a.part in ("kernel", "all"):
            fq = make_input(d, a.reads)
            text_bytes = os.path.getsize(fq)
            bgzip(fq, d + "/zlib6.fastq.gz", 6)
            step(me("--make-kbgzf", fq, d + "/kbgzf.fastq.gz"), 300, capture=False)
            row = {"reads": a.reads, "text_bytes": text_bytes, "files": {}}
            for tag in ("zlib6", "kbgzf"):
                p = "%s/%s.fastq.gz" % (d, tag)
                ks = kernel_stats(d, p, a.reps)
                ms = ks["avg_ns"] / 1e6 * ks["calls"] / (a.reps + 1)          # kernel time of one pass over the file (its chunks summed)
                call = step(me("--device-call", p, "--reps", str(a.reps)), 300)
                f = {"file_bytes": os.path.getsize(p), "members": call["members"], "k_inflate_ms_per_pass": ms,
                     "k_inflate_gb_per_s": text_bytes / (ms * 1e-3) / 1e9, "device_call_wall_s": call["wall_s"],
                     "device_call_gb_per_s_best": text_bytes / min(call["wall_s"]) / 1e9, "reader": []}
                for rep in range(2):
                    for name, env, dev in (("host_8", {"C3_GZ_THREADS": "8"}, False), ("host_16", {"C3_GZ_THREADS": "16"}, False), ("gpu", {}, True)):
                        r = step(me("--reader", p) + (["--device"] if dev else []), 300, env=env)
                        assert r["reads"] == a.reads
                        f["reader"].append({"run": name, "rep": rep, "wall_s": r["wall_s"], "reads_per_s": a.reads / r["wall_s"],
                                            "gb_per_s": text_bytes / r["wall_s"] / 1e9, "inflate_wait_s": r["inflate_wait_s"]})
                if tag == "zlib6":                                                 # members per launch (what was chosen)
                    f["chunk_sweep"] = {str(c): step(me("--device-call", p, "--reps", str(a.reps)), 300, env={"C3_INFLATE_CHUNK": str(c)})["wall_s"]
                                        for c in (1024, 2048, 4096, 8192, 16384)}
                row["files"][tag] = f
                print(json.dumps({tag: f}), flush=True)
            res["kernel"] = row
            json.dump(res, open(a.out, "w"), indent=1)
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d, exist_ok=True)
        if a.part in ("cli", "all"):
            fq = make_input(d, a.cli_reads)
            bgzip(fq, d + "/reads.fastq.gz", 6)
            runs = []
            for rep in range(2):
                for tag, reads, extra in (("bgzf_host", "reads.fastq.gz", ["--inflate", "host"]), ("bgzf_gpu", "reads.fastq.gz", ["--inflate", "gpu"]),
                                          ("plain", "reads.fastq", [])):
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
            best = {t: min(r["wall_s"] for r in runs if r["run"] == t) for t in ("bgzf_host", "bgzf_gpu", "plain")}
            res["cli"] = {"reads": a.cli_reads, "runs": runs, "best_wall_s": best, "gpu_rate_over_host": best["bgzf_host"] / best["bgzf_gpu"],
                          "gpu_rate_over_plain": best["plain"] / best["bgzf_gpu"]}
            print(json.dumps(res["cli"]), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""--bgzf cost and ratio:  python tools/bgzf_throughput.py [--reads N] [--co-reads M] [--dir DIR] [--part P]

part "small" (M cfg2 reads, default 100 000): the CLI plain, with -co and with -co --bgzf on the same input (wall times, the
ratio of every file type for both), then k_bgzf on the subread text of that run in a process of its own under
`rocprofv3 --kernel-trace --stats` (kernel time and GB/s of input) and once more without the profiler (host wall time of
Bgzf.compress, copies included).
part "large" (N cfg2 reads, default 1 000 000): the CLI with no compression and with -co --bgzf, alternated twice on one
input (reads/s from the wall time of each command line, a process of its own).
Results are merged into profiles/bgzf_throughput.json.  DIR should be a tmpfs (default /dev/shm)."""
import argparse
import csv
import glob
import json
import multiprocessing as mp
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILES = ["R2C2_Consensus.fasta", "R2C2_Subreads.fastq"]


def _gen(job):
    from c3poa_amd import synth
    s0, cnt, path = job
    st = []
    with open(path, "w") as fh:
        for r in synth.generate("cfg2", n_reads=cnt, start=s0):
            fh.write("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]))
            st.append(r[3])
    return "".join(st)


def make_input(d, n):
    fq = d + "/reads.fastq"
    chunk = 5000
    jobs = [(s0, min(chunk, n - s0), "%s/part%07d.fastq" % (d, s0)) for s0 in range(0, n, chunk)]
    with mp.Pool(16) as pool:
        strands = pool.map(_gen, jobs)
    with open(fq, "wb") as fh, open(d + "/reads.psl", "w") as psl:
        for (s0, cnt, path), st in zip(jobs, strands):
            with open(path, "rb") as src:
                shutil.copyfileobj(src, fh, 1 << 24)
            os.remove(path)
            for k in range(cnt):
                psl.write("\t".join(["280", "4", "0", "0", "0", "0", "0", "0", st[k], "r%08d" % (s0 + k), "5000", "0", "284",
                                     "Splint1", "284", "0", "284", "1", "284,", "0,", "0,"]) + "\n")
    from c3poa_amd import synth
    open(d + "/splint.fasta", "w").write(">Splint1\n%s\n" % synth.SPLINT1)
    return fq


def run_cli(d, tag, extra):
    out = d + "/out_" + tag
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out + "/tmp")
    shutil.copy(d + "/reads.psl", out + "/tmp/splint_to_read_alignments.psl")
    cmd = [sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", d + "/reads.fastq", "-s", d + "/splint.fasta", "-o", out] + extra
    t0 = time.perf_counter()
    subprocess.run(cmd, check=True, timeout=900, stdout=subprocess.DEVNULL)
    wall = time.perf_counter() - t0
    sizes = {f: os.path.getsize(out + "/Splint1/" + f) for f in os.listdir(out + "/Splint1")}
    print(json.dumps({"run": tag, "wall_s": wall, "sizes": sizes}), flush=True)
    return out, wall, sizes


def kernel_only(path, reps):
    """child process: c3_bgzf_compress of the file's bytes (pageable buffers, as a caller of the C ABI holds them), warm-up +
    reps; prints the host wall times of the calls (copies in and out included)"""
    import ctypes as C
    import numpy as np
    from c3poa_amd import _lib
    lib = _lib.load()
    data = np.fromfile(path, dtype=np.uint8)
    cap = int(lib.c3_bgzf_bound(len(data)))
    dst = np.empty(cap, dtype=np.uint8)
    dst[::4096] = 0                                       # touch the pages once
    z = _lib.Bgzf(0)
    olen = C.c_int64(0)
    walls, n_out = [], 0
    for k in range(reps + 1):                             # the first call allocates the device buffers (not timed)
        n = len(data)
        t0 = time.perf_counter()
        assert lib.c3_bgzf_compress(z.z, data.ctypes.data, n, dst.ctypes.data, cap, C.byref(olen)) == 0
        if k:
            walls.append(time.perf_counter() - t0)
            n_out = olen.value
    z.close()
    print(json.dumps({"bytes_in": len(data), "bytes_out": n_out, "wall_s": walls}), flush=True)


def kernel_stats(d, path, reps):
    pdir = d + "/prof"
    shutil.rmtree(pdir, ignore_errors=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pdir, "-o", "bgzf", "--", sys.executable, os.path.abspath(__file__),
           "--kernel-only", path, "--reps", str(reps)]
    subprocess.run(cmd, check=True, timeout=600, stdout=subprocess.DEVNULL)
    rows = {}
    for f in glob.glob(pdir + "/**/*kernel_stats.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "bgzf" in r["Name"]:
                rows[r["Name"]] = {"calls": int(r["Calls"]), "total_ns": float(r["TotalDurationNs"]), "avg_ns": float(r["AverageNs"])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--co-reads", type=int, default=100000)
    ap.add_argument("--dir", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--part", choices=["small", "large", "all"], default="all")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgzf_throughput.json"))
    ap.add_argument("--kernel-only", default=None)
    a = ap.parse_args()
    if a.kernel_only:
        return kernel_only(a.kernel_only, a.reps)
    res = json.load(open(a.out)) if os.path.exists(a.out) else {}
    d = tempfile.mkdtemp(prefix="c3bgzf_", dir=a.dir)
    try:
        if a.part in ("small", "all"):
            t0 = time.time()
            make_input(d, a.co_reads)
            print("generated %d reads in %.1f s" % (a.co_reads, time.time() - t0), file=sys.stderr)
            row = {"reads": a.co_reads, "input_bytes": os.path.getsize(d + "/reads.fastq")}
            p_out, p_wall, p_sizes = run_cli(d, "plain", [])
            _o, c_wall, c_sizes = run_cli(d, "co", ["-co"])
            b_out, b_wall, b_sizes = run_cli(d, "bgzf", ["-co", "--bgzf"])
            row["wall_s"] = {"plain": p_wall, "co": c_wall, "co_bgzf": b_wall}
            row["ratio"] = {f: {"co": p_sizes[f] / c_sizes[f + ".gz"], "bgzf": p_sizes[f] / b_sizes[f + ".gz"],
                                "bgzf_over_co": c_sizes[f + ".gz"] / b_sizes[f + ".gz"]} for f in FILES}
            sub = p_out + "/Splint1/R2C2_Subreads.fastq"
            n_in = os.path.getsize(sub)
            shutil.rmtree(b_out, ignore_errors=True)
            ks = kernel_stats(d, sub, a.reps)
            done = (a.reps + 1) * n_in                      # bytes the profiled process compressed (reps + the warm-up call)
            row["kernel"] = {"input_bytes": n_in, "stats": ks}
            for name, v in ks.items():
                key = "k_bgzf_pack" if "pack" in name else "k_bgzf"
                ms = v["total_ns"] / 1e6 * n_in / done
                row["kernel"]["ms_%s_per_pass" % key] = ms
                row["kernel"]["gb_per_s_%s" % key] = n_in / (ms * 1e-3) / 1e9
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernel-only", sub, "--reps", str(a.reps)],
                                 check=True, timeout=600, capture_output=True, text=True).stdout
            w = json.loads(out.strip().splitlines()[-1])
            row["host_call"] = {"wall_s": w["wall_s"], "gb_per_s_best": w["bytes_in"] / min(w["wall_s"]) / 1e9,
                                "ratio": w["bytes_in"] / w["bytes_out"]}
            res["small"] = row
            print(json.dumps(row), flush=True)
            shutil.rmtree(d, ignore_errors=True)
            os.makedirs(d, exist_ok=True)
        if a.part in ("large", "all"):
            t0 = time.time()
            make_input(d, a.reads)
            print("generated %d reads in %.1f s" % (a.reads, time.time() - t0), file=sys.stderr)
            runs = []
            for rep in range(2):
                for tag, extra in (("plain", []), ("co_bgzf", ["-co", "--bgzf"])):
                    o, wall, sizes = run_cli(d, tag, extra)
                    runs.append({"run": tag, "rep": rep, "wall_s": wall, "reads_per_s": a.reads / wall, "sizes": sizes})
                    shutil.rmtree(o, ignore_errors=True)
            best = {t: min(r["wall_s"] for r in runs if r["run"] == t) for t in ("plain", "co_bgzf")}
            res["large"] = {"reads": a.reads, "runs": runs, "best_wall_s": best,
                            "bgzf_rate_over_plain": best["plain"] / best["co_bgzf"]}
            print(json.dumps(res["large"]), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

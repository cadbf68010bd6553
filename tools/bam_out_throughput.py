#!/usr/bin/env python3
"""Throughput of the BAM form of the main CLI's record writer (k_bamout, --emit gpu --bam) beside the text form it sits next to
(k_emit), on N synthetic cfg2 reads:
  kernels: for one resident batch of up to 100 000 reads the event times of the length pass, the scans and the write pass of
      both forms, with the bytes each stores; k_bgzf's time and the compressed size of the BAM subread stream against the
      FASTQ subread stream
  CLI end to end: C3POa.py on a PSL as a child process with --emit gpu --bgzf (the path that exists) and --emit gpu --bam,
      alternated `reps` times with the existing path first, input and output on tmpfs when the machine has one
  bench.py --gpus 1 --steps 3 --warmup 1 in a built checkout of the parent commit (C3_BAM_OUT_PARENT names its directory; skipped
      when unset) and in this one, alternated `reps` times: it does not reach this code
Prints one JSON line per measurement and writes profiles/bam_out_throughput.json.
Usage: python tools/bam_out_throughput.py [N] [reps]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from c3poa_amd import _lib, synth  # noqa: E402
from emit_throughput import BATCH, tree, write_inputs  # noqa: E402

NOT_MEASURED = ["output on a disk (tmpfs only)", "more than one GPU", "more than one splint", "reads above TX_LONG bases in the workload"]


def device_part(fq, strands, result):
    rd = _lib.Reader(fq, n_sets=2)
    h = _lib.Handle(device=0)
    h.set_splints([synth.SPLINT1])
    warm = rd.next(2000, min_len=0)
    h.upload_host(warm, strands[:warm.n], np.zeros(warm.n, dtype=np.int16))
    h.run(qv=True)
    eb = _lib.EmitBuffers()
    for bam in (False, True):                                         # warm-up: buffers grown, kernels loaded
        for bg in (False, True):
            h.emit_fetch(eb, h.emit_snapshot(warm, True, bg, True, bam=bam))
    hb = rd.next(BATCH, min_len=0)
    h.upload_host(hb, strands[warm.n:warm.n + hb.n], np.zeros(hb.n, dtype=np.int16))
    h.run(qv=True)
    n = hb.n
    k = {"batch_reads": n}
    for bam in (False, True):
        form = {}
        for bg in (False, True):
            best = None
            for _rep in range(3):                                     # the fastest write pass of three: the arenas have their size
                eb, so = h.emit_fetch(eb, h.emit_snapshot(hb, True, bg, True, bam=bam))
                tm = h.emit_timing()
                if best is None or tm["ms_write"] < best[0]["ms_write"]:
                    best = (tm, so.copy())
            tm, so = best
            sub = int(so[2] - so[1])                                  # stream 1 is the subread stream in both forms
            if not bg:
                form.update({x: round(float(tm[x]), 3) for x in ("ms_len", "ms_scan", "ms_write")})
                # stored: the length pass one EmitHead and three lengths per read, the scans three offsets per read and the
                # workgroup sums twice, the write pass the streams
                form.update(len_bytes_stored=48 * n, scan_bytes_stored=24 * n + 2 * 8 * (form_cols(bam) + 1) * ((n + 255) // 256),
                            write_bytes_stored=int(tm["out_bytes"]), records=int(tm["n_records"]), subread_stream_bytes=sub,
                            write_GBps=round(tm["out_bytes"] / max(tm["ms_write"], 1e-6) / 1e6, 1))
            else:
                form.update(ms_bgzf=round(float(tm["ms_bgzf"]), 3), bgzf_bytes=int(tm["out_bytes"]), subread_stream_bgzf_bytes=sub)
        k["bam" if bam else "text"] = form
    t, b = k["text"], k["bam"]
    k["write_bytes_bam_over_text"] = round(b["write_bytes_stored"] / t["write_bytes_stored"], 4)
    k["subread_bytes_bam_over_text"] = round(b["subread_stream_bytes"] / t["subread_stream_bytes"], 4)
    k["subread_bgzf_bytes_bam_over_text"] = round(b["subread_stream_bgzf_bytes"] / t["subread_stream_bgzf_bytes"], 4)
    k["ms_write_bam_over_text"] = round(b["ms_write"] / t["ms_write"], 3)
    k["ms_bgzf_bam_over_text"] = round(b["ms_bgzf"] / t["ms_bgzf"], 3)
    result["device"] = k
    print(json.dumps({"bam_out_device": k}), flush=True)
    eb.close(); rd.close(); h.close()


def form_cols(bam):
    return 2 if bam else 3                                            # streams of one splint (QVs computed)


def cli_part(d, fq, strands, n, reps, result):
    modes = (("bgzf", ["--bgzf"]), ("bam", ["--bam"]))               # the path that exists first
    runs, stats, sizes = {m: [] for m, _f in modes}, {}, {}
    for r in range(reps):
        for mode, flags in modes:
            out = os.path.join(d, "out_" + mode)
            shutil.rmtree(out, ignore_errors=True)
            os.makedirs(out + "/tmp")
            with open(out + "/tmp/splint_to_read_alignments.psl", "w") as fh:
                for i, st in enumerate(strands):
                    fh.write("\t".join(["280", "4", "0", "0", "0", "0", "0", "0", st, "r%08d" % i, "5000", "0", "284", "Splint1", "284", "0", "284", "1", "284,", "0,", "0,"]) + "\n")
            cli = [sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", fq, "-s", os.path.join(d, "splint.fasta"), "-o", out, "--emit", "gpu"] + flags
            t = time.time()
            p = subprocess.run(cli, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000, env=dict(os.environ, C3_STREAM_STATS="1"))
            dt = time.time() - t
            if p.returncode != 0:
                sys.exit("CLI --emit gpu %s failed (%d): %s" % (mode, p.returncode, p.stderr[-2000:]))
            runs[mode].append(round(dt, 2))
            stats[mode] = [ln for ln in p.stderr.splitlines() if ln.startswith("stream: ")][-1:]
            sizes[mode] = {os.path.basename(f): os.path.getsize(f) for f in tree(out).values()}
            print(json.dumps({"bam_out_cli": mode, "rep": r, "seconds": round(dt, 2), "reads_per_s": round(n / dt)}), flush=True)
    best = {m: min(v) for m, v in runs.items()}
    spread = max(max(v) - min(v) for v in runs.values())
    result["cli"] = {"seconds": runs, "reads_per_s": {m: round(n / best[m]) for m in best}, "ratio_bam_over_bgzf": round(best["bgzf"] / best["bam"], 3),
                     "spread_s": round(spread, 2), "differ_beyond_spread": bool(abs(best["bgzf"] - best["bam"]) > spread),
                     "file_bytes": sizes, "output_bytes": {m: sum(v.values()) for m, v in sizes.items()}, "stream_stats": stats}
    print(json.dumps({"bam_out_cli_summary": {k: v for k, v in result["cli"].items() if k != "stream_stats"}}), flush=True)


def bench_part(reps, result):
    parent = os.environ.get("C3_BAM_OUT_PARENT")
    if not parent or not os.path.exists(os.path.join(parent, "bench.py")):
        result["bench"] = "not measured: C3_BAM_OUT_PARENT does not name a built checkout of the parent commit"
        return
    trees = (("parent", os.path.abspath(parent)), ("this", ROOT))
    vals = {m: [] for m, _p in trees}
    env = {k: v for k, v in os.environ.items() if k not in ("C3POA_LIB", "PYTHONPATH")}
    for r in range(reps):
        for m, path in trees:
            p = subprocess.run([sys.executable, os.path.join(path, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"],
                               capture_output=True, text=True, timeout=1500, env=env, cwd=path)
            if p.returncode != 0:
                result["bench"] = "failed: bench.py in the %s tree (%d): %s" % (m, p.returncode, p.stderr[-600:])
                return
            vals[m].append(json.loads(p.stdout.strip().splitlines()[-1])["value"])
            print(json.dumps({"bam_out_bench": m, "rep": r, "reads_per_s": vals[m][-1]}), flush=True)
    spread = max(max(v) - min(v) for v in vals.values())
    result["bench"] = {"reads_per_s": vals, "spread": round(spread, 1),
                       "this_over_parent": round(float(np.mean(vals["this"]) / np.mean(vals["parent"])), 4),
                       "differ_beyond_spread": bool(abs(np.mean(vals["this"]) - np.mean(vals["parent"])) > spread)}


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    result = {"reads": n, "reps": reps, "not_measured": NOT_MEASURED}
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="c3bamout_", dir=tmp_root)
    result["tmpfs"] = tmp_root is not None
    try:
        t = time.time()
        fq, strands = write_inputs(n, d)
        result["generate_s"] = round(time.time() - t, 1)
        result["input_bytes"] = os.path.getsize(fq)
        device_part(fq, strands, result)
        cli_part(d, fq, strands, n, reps, result)
    finally:
        shutil.rmtree(d, ignore_errors=True)
    bench_part(reps, result)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    dst = os.environ.get("C3_BAM_OUT_THROUGHPUT_JSON", os.path.join(ROOT, "profiles", "bam_out_throughput.json"))
    with open(dst, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

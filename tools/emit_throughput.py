#!/usr/bin/env python3
"""Throughput of the main CLI's record formatter on the GPU (k_emit, --emit gpu) on N synthetic cfg2 reads:
  kernels: the event times of k_emit's three steps (lengths, scans, write) for one resident batch of up to 100 000 reads, plain
      and with the BGZF flag (k_bgzf inside the fetch), after a warm-up batch
  stand-alone call: c3_emit_group with its copies for the same batch (the fetched records, consensus and QV bytes go up again)
  CLI end to end: C3POa.py on a PSL as a child process, plain and with --bgzf, each with --emit host and --emit gpu alternated
      `reps` times in one session, input and output on tmpfs when the machine has one; the output trees of the last pair of
      each mode are compared byte for byte
Prints one JSON line per measurement and writes profiles/emit_throughput.json.
Usage: python tools/emit_throughput.py [N] [reps]"""
import json
import multiprocessing as mp
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c3poa_amd import _lib, synth  # noqa: E402

BATCH = 100000


def _gen(job):
    s0, cnt, path = job
    st = []
    with open(path, "w") as fh:
        for r in synth.generate("cfg2", n_reads=cnt, start=s0):
            fh.write("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]))
            st.append(r[3])
    return "".join(st)


def write_inputs(n, d):
    fq, chunk = os.path.join(d, "reads.fastq"), 5000
    jobs = [(s0, min(chunk, n - s0), "%s/part%06d.fastq" % (d, s0)) for s0 in range(0, n, chunk)]
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        strands = "".join(pool.map(_gen, jobs))
    with open(fq, "wb") as fh:
        for _s0, _cnt, path in jobs:
            with open(path, "rb") as src:
                shutil.copyfileobj(src, fh, 1 << 24)
            os.remove(path)
    open(os.path.join(d, "splint.fasta"), "w").write(">Splint1\n%s\n" % synth.SPLINT1)
    return fq, strands


def tree(root):
    return {os.path.relpath(os.path.join(b, f), root): os.path.join(b, f) for b, _d, fs in os.walk(root) for f in fs if f.startswith("R2C2_")}


def same_trees(a, b):
    ta, tb = tree(a), tree(b)
    if sorted(ta) != sorted(tb):
        return False
    for k in ta:
        if os.path.getsize(ta[k]) != os.path.getsize(tb[k]):
            return False
        with open(ta[k], "rb") as fa, open(tb[k], "rb") as fb:
            while True:
                x, y = fa.read(1 << 24), fb.read(1 << 24)
                if x != y:
                    return False
                if not x:
                    break
    return True


def device_part(fq, strands, result):
    rd = _lib.Reader(fq, n_sets=2)
    h = _lib.Handle(device=0)
    h.set_splints([synth.SPLINT1])
    warm = rd.next(2000, min_len=0)
    h.upload_host(warm, strands[:warm.n], np.zeros(warm.n, dtype=np.int16))
    h.run(qv=True)
    eb = _lib.EmitBuffers()
    for bg in (False, True):                                          # warm-up: buffers grown, kernels loaded
        h.emit_fetch(eb, h.emit_snapshot(warm, True, bg, True))
    hb = rd.next(BATCH, min_len=0)
    h.upload_host(hb, strands[warm.n:warm.n + hb.n], np.zeros(hb.n, dtype=np.int16))
    h.run(qv=True)
    k = {"batch_reads": hb.n}
    for bg in (False, True):
        for _rep in range(2):                                         # the second of two: the arenas have their size
            eb, so = h.emit_fetch(eb, h.emit_snapshot(hb, True, bg, True))
            tm = h.emit_timing()
        key = "bgzf" if bg else "plain"
        k[key] = {x: round(float(tm[x]), 3) for x in ("ms_len", "ms_scan", "ms_write", "ms_bgzf", "ms_call")}
        k[key]["out_bytes"] = int(tm["out_bytes"])
        if not bg:
            k["text_bytes"] = int(tm["out_bytes"]); k["records"] = int(tm["n_records"])
            k["write_GBps"] = round(tm["out_bytes"] / max(tm["ms_write"], 1e-6) / 1e6, 1)
        else:
            k["bgzf_text_GBps"] = round(k["text_bytes"] / max(tm["ms_bgzf"], 1e-6) / 1e6, 2)
    rb = _lib.ResultBuffers()
    res, buf, coff, qv = h.results_fetch_qv(rb, h.results_snapshot())
    sid = np.zeros(hb.n, dtype=np.int16)
    h.emit_group(hb, res, buf, coff, qv, sid, 1, True)
    t = time.time()
    got = h.emit_group(hb, res, buf, coff, qv, sid, 1, True)
    k["ms_python_standalone"] = round((time.time() - t) * 1e3, 1)
    tm = h.emit_timing()
    k["standalone"] = {x: round(float(tm[x]), 3) for x in ("ms_len", "ms_scan", "ms_write", "ms_call")}
    k["standalone_equals_resident"] = bool(int(got.stream_off[-1]) == k["text_bytes"])
    t = time.time()
    _lib.emit_group_host(hb, res, buf, coff, qv, sid, 1, True)
    k["ms_host_statement_two_calls"] = round((time.time() - t) * 1e3, 1)
    result["device"] = k
    print(json.dumps({"emit_device": k}), flush=True)
    eb.close(); rd.close(); h.close()


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    result = {"reads": n, "reps": reps}
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="c3emit_", dir=tmp_root)
    result["tmpfs"] = tmp_root is not None
    try:
        t = time.time()
        fq, strands = write_inputs(n, d)
        result["generate_s"] = round(time.time() - t, 1)
        result["input_bytes"] = os.path.getsize(fq)
        device_part(fq, strands, result)
        result["cli"] = {}
        for mode, flags in (("plain", []), ("bgzf", ["--bgzf"])):
            runs = {"host": [], "gpu": []}
            stats = {}
            for r in range(reps):
                for emit in ("host", "gpu"):
                    out = os.path.join(d, "out_" + emit)
                    shutil.rmtree(out, ignore_errors=True)
                    os.makedirs(out + "/tmp")
                    with open(out + "/tmp/splint_to_read_alignments.psl", "w") as fh:
                        for i, st in enumerate(strands):
                            fh.write("\t".join(["280", "4", "0", "0", "0", "0", "0", "0", st, "r%08d" % i, "5000", "0", "284", "Splint1", "284", "0", "284", "1", "284,", "0,", "0,"]) + "\n")
                    cli = [sys.executable, os.path.join(ROOT, "C3POa.py"), "-r", fq, "-s", os.path.join(d, "splint.fasta"), "-o", out, "--emit", emit] + flags
                    t = time.time()
                    p = subprocess.run(cli, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000, env=dict(os.environ, C3_STREAM_STATS="1"))
                    dt = time.time() - t
                    if p.returncode != 0:
                        sys.exit("CLI --emit %s %s failed (%d): %s" % (emit, mode, p.returncode, p.stderr[-2000:]))
                    runs[emit].append(round(dt, 2))
                    stats[emit] = [ln for ln in p.stderr.splitlines() if ln.startswith("stream: ")][-1:]
                    print(json.dumps({"emit_cli": mode, "emit": emit, "rep": r, "seconds": round(dt, 2), "reads_per_s": round(n / dt)}), flush=True)
            best = {m: min(v) for m, v in runs.items()}
            spread = max(runs["host"]) - min(runs["host"])
            c = {"seconds": runs, "reads_per_s_host": round(n / best["host"]), "reads_per_s_gpu": round(n / best["gpu"]),
                 "ratio_gpu_over_host": round(best["host"] / best["gpu"], 3), "host_spread_s": round(spread, 2),
                 "gpu_faster_beyond_spread": bool(best["host"] - max(runs["gpu"]) > spread),
                 "trees_equal": same_trees(os.path.join(d, "out_host"), os.path.join(d, "out_gpu")),
                 "output_bytes": sum(os.path.getsize(p) for p in tree(os.path.join(d, "out_gpu")).values()), "stream_stats": stats}
            result["cli"][mode] = c
            print(json.dumps({"emit_cli_summary": mode, **{k: v for k, v in c.items() if k != "stream_stats"}}), flush=True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        dst = os.environ.get("C3_EMIT_THROUGHPUT_JSON", os.path.join(ROOT, "profiles", "emit_throughput.json"))
        with open(dst, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

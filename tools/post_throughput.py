#!/usr/bin/env python3
"""Throughput of the post-processing step on N synthetic consensus-like reads (0.6-1.6 kb) with planted 5'/3' adapters
(a few edits each; every 16th read without adapters):
  kernels: the event times of k_post's three passes (classify, scans, emit) for one batch, after a warm-up call
  device call: c3_post_emit with its copies (upload of the batch and the table, download of the arena), and the
      scan_adapters call that feeds it, for the same batch
  CLI end to end: C3POa_postprocessing.py -t as a child process with --emit host and with --emit gpu, alternated `reps`
      times in one session, input and output on tmpfs when the machine has one
After the timed regions the two output trees of the last pair are compared byte for byte.  Prints one JSON line per
measurement and writes profiles/post_emit_throughput.json.
Usage: python tools/post_throughput.py [N] [reps]"""
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
from c3poa_amd import _lib  # noqa: E402
from c3poa_amd.seqio import revcomp  # noqa: E402

BATCH = 200000


def noisy(rng, s, edits):
    s = bytearray(s)
    for _ in range(edits):
        op, p = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
        c = b"ACGT"[int(rng.integers(0, 4))]
        if op == 0:
            s[p] = c
        elif op == 1:
            s.insert(p, c)
        elif len(s) > 1:
            del s[p]
    return bytes(s)


def write_inputs(rng, n, fasta, adapters):
    a5 = "".join("ACGT"[i] for i in rng.integers(0, 4, 33))
    a3 = "".join("ACGT"[i] for i in rng.integers(0, 4, 36))
    with open(adapters, "w") as f:
        f.write(">3Prime_adapter\n%s\n>5Prime_adapter\n%s\n" % (a3, a5))
    left = [[noisy(rng, x.encode(), e) for e in (0, 0, 1, 1, 2, 3) for _ in range(8)] for x in (a5, a3)]
    right = [[noisy(rng, revcomp(x).encode(), e) for e in (0, 0, 1, 1, 2, 3) for _ in range(8)] for x in (a3, a5)]
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 1 << 20)].tobytes()
    lens, at, pre, post = rng.integers(500, 1500, n), rng.integers(0, (1 << 20) - 1600, n), rng.integers(5, 45, n), rng.integers(5, 45, n)
    v = rng.integers(0, 48, (n, 2))
    with open(fasta, "wb") as f:
        for b0 in range(0, n, 65536):
            recs = []
            for i in range(b0, min(n, b0 + 65536)):
                body = pool[at[i]:at[i] + lens[i]]
                flip = i % 3 == 0
                s = body if i % 16 == 5 else pool[i % 4096:i % 4096 + pre[i]] + left[flip][v[i, 0]] + body + right[flip][v[i, 1]] + pool[i % 5000:i % 5000 + post[i]]
                recs.append(b">r%08d_11.9_5000_3_%d\n%s\n" % (i, len(s), s))
            f.write(b"".join(recs))


def tree(root):
    out = {}
    for base, _d, files in os.walk(root):
        for fn in files:
            out[os.path.relpath(os.path.join(base, fn), root)] = open(os.path.join(base, fn), "rb").read()
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rng = np.random.default_rng(7)
    result = {"reads": n, "reps": reps}
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="c3post_", dir=tmp_root)
    result["tmpfs"] = tmp_root is not None
    try:
        fa, ad = os.path.join(d, "cons.fasta"), os.path.join(d, "adapters.fasta")
        t = time.time()
        write_inputs(rng, n, fa, ad)
        result["generate_s"] = round(time.time() - t, 1)
        result["input_bytes"] = os.path.getsize(fa)

        # one batch in process: adapter scan, then the device call twice (warm-up, timed)
        from c3poa_amd.seqio import fastx_read
        adapters = [(r[0], r[1]) for r in fastx_read(ad)]
        plan = _lib.PostPlan(adapters, None, trim=True)
        rd = _lib.Reader(fa, n_sets=1)
        hb = rd.next(BATCH, min_len=0)
        h = _lib.Handle(device=0)
        h.set_splints([a[1] for a in adapters])
        t = time.time()
        h.upload_host(hb, b"?" * hb.n, np.zeros(hb.n, dtype=np.int16))
        tab = h.scan_adapters()
        dt_scan = time.time() - t
        batch = _lib.PostBatch.from_host(hb)
        h.post_emit(plan, batch, tab)
        t = time.time()
        arena, so, kept = h.post_emit(plan, batch, tab)
        dt_call = time.time() - t
        tm = h.post_emit_timing()
        k = {"batch_reads": hb.n, "kept": kept, "in_bytes": int(tm["in_bytes"]), "out_bytes": int(tm["out_bytes"]),
             "ms_classify": round(tm["ms_classify"], 3), "ms_scan": round(tm["ms_scan"], 3), "ms_emit": round(tm["ms_emit"], 3),
             "ms_call_with_copies": round(tm["ms_call"], 2), "ms_python_call": round(dt_call * 1e3, 2),
             "emit_GBps_out": round(tm["out_bytes"] / max(tm["ms_emit"], 1e-6) / 1e6, 1),
             "device_call_reads_per_s": round(hb.n / (tm["ms_call"] / 1e3)), "ms_scan_adapters_call": round(dt_scan * 1e3, 1)}
        t = time.time()
        _lib.post_emit_host(plan, batch, tab)
        k["ms_host_statement"] = round((time.time() - t) * 1e3, 1)
        result["device"] = k
        print(json.dumps({"post_emit_device": k}), flush=True)
        rd.close()
        h.close()

        runs = {"host": [], "gpu": []}
        for r in range(reps):
            for mode in ("host", "gpu"):
                out = os.path.join(d, "out_" + mode)
                shutil.rmtree(out, ignore_errors=True)
                cli = [sys.executable, os.path.join(ROOT, "C3POa_postprocessing.py"), "-i", fa, "-a", ad, "-o", out, "-t", "--emit", mode]
                t = time.time()
                p = subprocess.run(cli, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000)
                dt = time.time() - t
                if p.returncode != 0:
                    sys.exit("CLI --emit %s failed (%d): %s" % (mode, p.returncode, p.stderr[-2000:]))
                runs[mode].append(round(dt, 2))
                print(json.dumps({"post_cli": mode, "rep": r, "seconds": round(dt, 2), "reads_per_s": round(n / dt)}), flush=True)
        best = {m: min(v) for m, v in runs.items()}
        th, tg = tree(os.path.join(d, "out_host")), tree(os.path.join(d, "out_gpu"))
        result["cli"] = {"seconds": runs, "reads_per_s_host": round(n / best["host"]), "reads_per_s_gpu": round(n / best["gpu"]),
                         "ratio_gpu_over_host": round(best["host"] / best["gpu"], 2),
                         "trees_equal": th == tg, "files": len(th), "output_bytes": sum(len(v) for v in tg.values())}
        print(json.dumps({"post_cli_summary": result["cli"]}), flush=True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        dst = os.environ.get("C3_POST_THROUGHPUT_JSON", os.path.join(ROOT, "profiles", "post_emit_throughput.json"))
        with open(dst, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

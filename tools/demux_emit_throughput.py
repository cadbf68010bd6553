#!/usr/bin/env python3
"""Throughput of C3POa_demux.py --emit gpu on N synthetic consensus reads (1-2 kb, one sequence line each) that carry noisy
copies of the paper's Nextera and TSO indexes in their first 300 bases (the reads of tools/demux_throughput.py):
  kernels: the event times of c3_demux_emit_timing (parse kernels, k_demux, emit kernels) summed over the chunks of the file,
      after a warm-up pass
  device call: c3_demux_emit with its copies over the same chunks, against the host statement c3_demux_emit_host on one
      thread (on the first `sample` reads: its textbook index search is slow), bytes compared
  CLI end to end: C3POa_demux.py as a child process with --emit host and --emit gpu, alternated `reps` times in one session,
      input and output on tmpfs when the machine has one; the output files of every pair compared byte for byte
Prints one JSON line per measurement and writes profiles/demux_emit_throughput.json.
Usage: python tools/demux_emit_throughput.py [N] [reps] [sample]"""
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
from c3poa_amd import _lib, demux  # noqa: E402
import demux_throughput as DT  # noqa: E402


class TimedHandle:
    """a Handle whose demux_emit_raw adds up c3_demux_emit_timing"""

    def __init__(self, h):
        self.handle, self.lib, self.h = h, h.lib, h.h
        self.sums = {}

    def demux_emit_raw(self, *a):
        r = self.handle.demux_emit_raw(*a)
        for k, v in self.handle.demux_emit_timing().items():
            self.sums[k] = self.sums.get(k, 0) + v
        return r


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    n_sample = int(sys.argv[3]) if len(sys.argv) > 3 else 2000
    rng = np.random.default_rng(7)
    a_names, a_seqs = demux.load_indexes(DT.NX)
    b_names, b_seqs = demux.load_indexes(DT.TSO)
    heads, lens = DT.make_reads(rng, n, [s.encode() for s in a_seqs], [s.encode() for s in b_seqs])
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4096 + 2000)].tobytes()
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="c3demux_emit_", dir=tmp_root)
    result = {"reads": n, "tmpfs": tmp_root is not None, "chunk_bytes": demux.EMIT_CHUNK}
    h = _lib.Handle(device=0)
    try:
        inp = os.path.join(d, "cons.fasta")
        DT.write_fasta(inp, heads, lens, pool)
        result["input_bytes"] = os.path.getsize(inp)

        # the device call over the chunks of the file, in process (second pass: buffers and code objects are there)
        for rep in range(2):
            th, stats = TimedHandle(h), {}
            t = time.time()
            done = demux.run_emit_gpu(inp, os.path.join(d, "inproc"), DT.NX, DT.TSO, handle=th, stats=stats)
            dt = time.time() - t
        if done is None:
            sys.exit("device path fell back: %s" % stats["fallback"])
        s = th.sums
        result["kernels_ms"] = {"parse": round(s["ms_parse"], 2), "k_demux": round(s["ms_demux"], 2), "emit": round(s["ms_emit"], 2)}
        result["device_call"] = {"ms_with_copies": round(s["ms_call"], 1), "chunks": stats["chunks"], "reads_per_s": round(n / (s["ms_call"] / 1e3)),
                                 "run_emit_gpu_s": round(dt, 3), "out_bytes": int(s["out_bytes"])}
        print(json.dumps({"kernels_ms": result["kernels_ms"], "device_call": result["device_call"]}), flush=True)

        # the host statement on one thread, on a sample, and its bytes against the device's
        with open(inp, "rb") as f:
            text = f.read(int(lens[:n_sample].sum()) + 16 * n_sample + 64)
        text = text[:text.rfind(b">")]
        sets = _lib.DemuxSets(a_names, a_seqs, b_names, b_seqs)
        t = time.time()
        host = _lib.demux_emit_host(text, sets)
        dt_h = time.time() - t
        dev = h.demux_emit(text, sets)
        result["host_statement"] = {"sample_reads": host.info["n_records"], "seconds": round(dt_h, 3),
                                    "reads_per_s": round(host.info["n_records"] / dt_h), "equal_to_device": dev.out == host.out and dev.info == host.info}
        print(json.dumps({"host_statement": result["host_statement"]}), flush=True)

        # the CLI, host and gpu alternated
        cli = [sys.executable, os.path.join(ROOT, "C3POa_demux.py"), "-i", inp, "-n", DT.NX, "-t", DT.TSO]
        runs, equal = {"host": [], "gpu": []}, True
        for rep in range(reps):
            for emit in ("host", "gpu"):
                out = os.path.join(d, "cli_" + emit)
                shutil.rmtree(out, ignore_errors=True)
                t = time.time()
                p = subprocess.run(cli + ["-o", out, "--emit", emit, "--emit-stats"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000)
                runs[emit].append(round(time.time() - t, 3))
                if p.returncode != 0:
                    sys.exit("CLI --emit %s failed (%d): %s" % (emit, p.returncode, p.stderr))
                if emit == "gpu":
                    result["cli_stats"] = json.loads([line for line in p.stderr.splitlines() if line.startswith("{")][-1])
            with open(os.path.join(d, "cli_host", "Indexed_reads.fasta"), "rb") as fa, open(os.path.join(d, "cli_gpu", "Indexed_reads.fasta"), "rb") as fb:
                equal = equal and fa.read() == fb.read()
        result["cli_seconds"] = runs
        result["cli_reads_per_s"] = {k: round(n / min(v)) for k, v in runs.items()}
        result["cli_outputs_equal"] = equal
        print(json.dumps({"cli_seconds": runs, "cli_reads_per_s": result["cli_reads_per_s"], "cli_outputs_equal": equal,
                          "cli_stats": result.get("cli_stats")}), flush=True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        dst = os.environ.get("C3_DEMUX_EMIT_THROUGHPUT_JSON", os.path.join(ROOT, "profiles", "demux_emit_throughput.json"))
        with open(dst, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        if not equal or not result["host_statement"]["equal_to_device"]:
            sys.exit("outputs differ")
    finally:
        h.close()
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of C3POa_demux.py --emit gpu --parse gpu on the N synthetic consensus reads of tools/demux_throughput.py (1-2 kb,
noisy copies of the golden 20 + 8 indexes in the first 300 bases), as FASTA, as FASTQ and as BGZF FASTQ, on tmpfs when the
machine has one.
  yardstick: the unchanged parent path, C3POa_demux.py --emit gpu on the FASTA file, measured in the same session.  Every other
      command line is alternated with it `reps` times, the parent path first.
  command lines: --parse gpu (FASTA); + --split; FASTQ in with --keep-quals; BGZF in through zlib on the host and with
      --inflate gpu; --bgzf out, unsplit and split
  in process, after a warm-up pass: the times of c3_demux_text_timing_get summed over the pieces of the file for the plain, the
      split, the --keep-quals and the --split --bgzf run -- parse, k_demux, placement (k_dsplit_key / _tile / _cols / _offs),
      k_dsplit_emit, the per-stream compression loop -- the stream waits per call, and the host time spent appending to the
      .part files
Prints one JSON line per measurement and writes profiles/demux_text_throughput.json.
Usage: python tools/demux_text_throughput.py [N] [reps]"""
import gzip
import hashlib
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
    """a Handle whose demux_emit_text adds up c3_demux_text_timing_get"""

    def __init__(self, h):
        self.handle, self.sums, self.calls = h, {}, 0

    def demux_text_reset(self):
        self.handle.demux_text_reset()

    def demux_emit_text(self, *a, **kw):
        r = self.handle.demux_emit_text(*a, **kw)
        self.calls += 1
        for k, v in self.handle.demux_text_timing().items():
            self.sums[k] = self.sums.get(k, 0) + v
        return r


def write_fastq(path, heads, lens, pool):
    qual = bytes(33 + (j * 7) % 41 for j in range(2048))
    with open(path, "wb") as f:
        for b0 in range(0, len(lens), 65536):
            f.write(b"".join(b"@r%08d_%d\n%s%s\n+\n%s\n" % (i, lens[i], heads[i].tobytes(), pool[i % 4096: i % 4096 + lens[i] - 300], qual[:lens[i]])
                             for i in range(b0, min(len(lens), b0 + 65536))))


def tree(d):
    """{relative path: SHA-1 of the plain bytes} of an output directory (.gz files inflated, read in pieces)"""
    out = {}
    for base, _dirs, files in os.walk(d):
        for f in files:
            p = os.path.join(base, f)
            sha = hashlib.sha1()
            with (gzip.open(p, "rb") if f.endswith(".gz") else open(p, "rb")) as fh:
                for piece in iter(lambda: fh.read(16 << 20), b""):
                    sha.update(piece)
            name = os.path.relpath(p, d)
            out[name[:-3] if f.endswith(".gz") else name] = sha.hexdigest()
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rng = np.random.default_rng(7)
    _a, a_seqs = demux.load_indexes(DT.NX)
    _b, b_seqs = demux.load_indexes(DT.TSO)
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="c3demux_text_", dir=tmp_root)
    free = shutil.disk_usage(d).free
    asked = n
    while n > 1000 and n * 9000 > free:                       # ~1.5 kB FASTA + 3 kB FASTQ + 1 kB BGZF per read, and the largest output
        n //= 2
    result = {"reads": n, "reads_asked": asked, "tmpfs": tmp_root is not None, "chunk_bytes": demux.EMIT_CHUNK}
    heads, lens = DT.make_reads(rng, n, [s.encode() for s in a_seqs], [s.encode() for s in b_seqs])
    pool = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 4096 + 2000)].tobytes()
    h = _lib.Handle(device=0)
    try:
        fa, fq, fz = (os.path.join(d, x) for x in ("cons.fasta", "cons.fastq", "cons.fastq.gz"))
        DT.write_fasta(fa, heads, lens, pool)
        write_fastq(fq, heads, lens, pool)
        z = _lib.Bgzf()
        with open(fq, "rb") as src, open(fz, "wb") as dst:
            while True:
                piece = src.read(1024 * _lib.BGZF_BLOCK)
                if not piece:
                    break
                dst.write(z.compress(piece))
            dst.write(_lib.BGZF_EOF)
        z.close()
        result["input_bytes"] = {"fasta": os.path.getsize(fa), "fastq": os.path.getsize(fq), "fastq_bgzf": os.path.getsize(fz)}

        # in process: the stage times over the pieces of the file (second pass: buffers and code objects are there)
        stages = {}
        for tag, inp, kw in (("plain", fa, {}), ("split", fa, {"split": True}), ("keep_quals", fq, {"keep_quals": True}),
                             ("split_bgzf", fa, {"split": True, "bgzf": True}), ("inflate_gpu", fz, {"inflate_gpu": True})):
            for rep in range(2):
                th, stats = TimedHandle(h), {}
                shutil.rmtree(os.path.join(d, "inproc"), ignore_errors=True)
                t = time.time()
                done = demux.run_text_gpu(inp, os.path.join(d, "inproc"), DT.NX, DT.TSO, handle=th, stats=stats, **kw)
                dt = time.time() - t
            if done is None:
                sys.exit("device path fell back: %s" % stats["fallback"])
            s = th.sums
            stages[tag] = {k[3:]: round(s[k], 2) for k in ("ms_inflate", "ms_parse", "ms_demux", "ms_split", "ms_emit", "ms_bgzf", "ms_call")}
            stages[tag].update(calls=th.calls, waits_per_call=round(s["n_waits"] / th.calls, 1), run_text_gpu_s=round(dt, 3),
                               append_s=stats["append_seconds"], files=stats["files"], out_bytes=int(s["out_bytes"]))
            print(json.dumps({tag: stages[tag]}), flush=True)
        shutil.rmtree(os.path.join(d, "inproc"), ignore_errors=True)
        result["stages_ms"] = stages

        # the CLI: every command line alternated with the parent path, the parent path first
        cli = [sys.executable, os.path.join(ROOT, "C3POa_demux.py"), "-n", DT.NX, "-t", DT.TSO]
        new = ["--emit", "gpu", "--parse", "gpu", "--emit-stats"]
        lines = [("parse_gpu", fa, new), ("split", fa, new + ["--split"]), ("fastq_keep_quals", fq, new + ["--keep-quals"]),
                 ("bgzf_in_zlib_host", fz, new), ("bgzf_in_inflate_gpu", fz, new + ["--inflate", "gpu"]),
                 ("bgzf_out", fa, new + ["--bgzf"]), ("bgzf_out_split", fa, new + ["--bgzf", "--split"])]
        runs, trees = {"parent_emit_gpu": []}, {}

        def run(tag, inp, flags):
            out = os.path.join(d, "cli_out")
            shutil.rmtree(out, ignore_errors=True)
            t = time.time()
            p = subprocess.run(cli + ["-i", inp, "-o", out] + flags, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000)
            runs.setdefault(tag, []).append(round(time.time() - t, 3))
            if p.returncode != 0:
                sys.exit("%s failed (%d): %s" % (tag, p.returncode, p.stderr))
            st = [line for line in p.stderr.splitlines() if line.startswith("{")]
            if st and json.loads(st[-1])["fallback"] is not None:
                sys.exit("%s fell back: %s" % (tag, st[-1]))
            if tag not in trees:
                trees[tag] = tree(out)
            return json.loads(st[-1]) if st else None

        for tag, inp, flags in lines:
            for rep in range(reps):
                run("parent_emit_gpu", fa, ["--emit", "gpu", "--emit-stats"])
                st = run(tag, inp, flags)
            result.setdefault("cli_stats", {})[tag] = st
            print(json.dumps({tag: runs[tag], "parent_emit_gpu": runs["parent_emit_gpu"][-reps:]}), flush=True)
        shutil.rmtree(os.path.join(d, "cli_out"), ignore_errors=True)
        result["cli_seconds"] = runs
        result["cli_reads_per_s"] = {k: round(n / min(v)) for k, v in runs.items()}
        # the files: --parse gpu and --bgzf give the parent's file; the split trees hold its records; BGZF in gives what zlib gives
        same = {"parse_gpu": trees["parse_gpu"] == trees["parent_emit_gpu"], "bgzf_out": trees["bgzf_out"] == trees["parent_emit_gpu"],
                "bgzf_out_split": trees["bgzf_out_split"] == trees["split"], "inflate_gpu": trees["bgzf_in_inflate_gpu"] == trees["bgzf_in_zlib_host"],
                "fastq_in": trees["bgzf_in_zlib_host"] == trees["parent_emit_gpu"]}
        result["cli_outputs_equal"] = same
        print(json.dumps({"cli_reads_per_s": result["cli_reads_per_s"], "cli_outputs_equal": same}), flush=True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        dst = os.environ.get("C3_DEMUX_TEXT_THROUGHPUT_JSON", os.path.join(ROOT, "profiles", "demux_text_throughput.json"))
        with open(dst, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        if not all(same.values()):
            sys.exit("outputs differ")
    finally:
        h.close()
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the text path of the post-processing step on the data set of tools/post_throughput.py
(N synthetic consensus-like reads of 0.6-1.6 kb with planted adapters), input and output on tmpfs when the machine has one:
  device call: c3_post_emit_text on the first 64 MiB of the file, plain and as BGZF members, after a warm-up call, with the
      times of c3_post_text_timing_get
  CLI pairs, each alternated `reps` times in one session as child processes of C3POa_postprocessing.py -t:
      1  plain input     --emit gpu                      against  --emit gpu --parse gpu
      2  BGZF input      --emit gpu (zlib threads)       against  --emit gpu --parse gpu --inflate gpu
      3  compressed out  --emit gpu -n 2 -co             against  --emit gpu --parse gpu --bgzf
  and the size of the compressed trees of pair 3.
After the timed regions the decompressed output trees of the last runs are compared byte for byte.  Prints one JSON line per
measurement and writes profiles/post_text_throughput.json.
Usage: python tools/post_text_throughput.py [N] [reps]"""
import gzip
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
from c3poa_amd import _lib  # noqa: E402
from post_throughput import write_inputs  # noqa: E402

PIECE = 64 << 20


def tree(root):
    """{path without .gz: text} and the bytes on disk"""
    out, size = {}, 0
    for base, _d, files in os.walk(root):
        for fn in files:
            p = os.path.join(base, fn)
            size += os.path.getsize(p)
            rel = os.path.relpath(p, root)
            out[rel[:-3] if fn.endswith(".gz") else rel] = gzip.open(p, "rb").read() if fn.endswith(".gz") else open(p, "rb").read()
    return out, size


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    rng = np.random.default_rng(7)
    result = {"reads": n, "reps": reps}
    tmp_root = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None
    d = tempfile.mkdtemp(prefix="c3ptext_", dir=tmp_root)
    result["tmpfs"] = tmp_root is not None
    try:
        fa, fz, ad = os.path.join(d, "cons.fasta"), os.path.join(d, "cons.fasta.gz"), os.path.join(d, "adapters.fasta")
        write_inputs(rng, n, fa, ad)
        z = _lib.Bgzf()
        with open(fa, "rb") as src, open(fz, "wb") as dst:
            while True:
                piece = src.read(1024 * _lib.BGZF_BLOCK)
                if not piece:
                    break
                dst.write(z.compress(piece))
            dst.write(_lib.BGZF_EOF)
        z.close()
        result["input_bytes"], result["input_bgzf_bytes"] = os.path.getsize(fa), os.path.getsize(fz)

        # one piece in process: warm-up, then the timed call, plain and BGZF
        from c3poa_amd import postprocess as PP
        from c3poa_amd.seqio import fastx_read
        adapters = [(r[0], r[1]) for r in fastx_read(ad)]
        plan = _lib.PostPlan(adapters, None, trim=True)
        h = _lib.Handle(device=0)
        h.set_splints([a[1] for a in adapters])
        for label, path, in_bgzf in (("plain", fa, False), ("bgzf", fz, True)):
            piece = next(PP._text_pieces(path, PIECE, in_bgzf))[0]
            for out_bgzf in (False, True):
                for _rep in range(2):
                    h.post_text_reset()
                    t = time.time()
                    res = h.post_emit_text(plan, np.frombuffer(piece, dtype=np.uint8), at_eof=False, in_bgzf=in_bgzf, out_bgzf=out_bgzf)
                    dt = time.time() - t
                tm = h.post_text_timing()
                k = {"input": label, "out_bgzf": out_bgzf, "piece_bytes": len(piece), "ms_python_call": round(dt * 1e3, 1)}
                k.update({f: (round(v, 2) if isinstance(v, float) else int(v)) for f, v in tm.items()})
                k["records_per_s_call"] = round(res.info["n_records"] / (tm["ms_call"] / 1e3))
                result.setdefault("device", []).append(k)
                print(json.dumps({"post_text_device": k}), flush=True)
        h.close()

        base = [sys.executable, os.path.join(ROOT, "C3POa_postprocessing.py"), "-a", ad, "-t", "--emit", "gpu"]
        pairs = {"1_plain_input": [("emit_gpu", ["-i", fa]), ("parse_gpu", ["-i", fa, "--parse", "gpu", "--emit-stats"])],
                 "2_bgzf_input": [("emit_gpu_zlib", ["-i", fz]), ("parse_inflate_gpu", ["-i", fz, "--parse", "gpu", "--inflate", "gpu", "--emit-stats"])],
                 "3_compressed_output": [("n2_co", ["-i", fa, "-n", "2", "-co"]), ("parse_gpu_bgzf", ["-i", fa, "--parse", "gpu", "--bgzf", "--emit-stats"])]}
        trees, result["cli"] = {}, {}
        for pair, modes in pairs.items():
            runs = {m: [] for m, _f in modes}
            for r in range(reps):
                for mode, flags in modes:
                    out = os.path.join(d, "out_" + mode)
                    shutil.rmtree(out, ignore_errors=True)
                    t = time.time()
                    p = subprocess.run(base + flags + ["-o", out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, timeout=3000)
                    dt = time.time() - t
                    if p.returncode != 0:
                        sys.exit("CLI %s failed (%d): %s" % (mode, p.returncode, p.stderr[-2000:]))
                    if "--emit-stats" in flags and '"fallback": false' not in p.stderr:
                        sys.exit("CLI %s fell back: %s" % (mode, p.stderr[-2000:]))
                    runs[mode].append(round(dt, 2))
                    print(json.dumps({"post_text_cli": mode, "rep": r, "seconds": round(dt, 2), "reads_per_s": round(n / dt)}), flush=True)
            (ma, _a), (mb, _b) = modes
            spread = round(max(runs[ma]) - min(runs[ma]), 2)
            summary = {"seconds": runs, "parent_spread_s": spread, "ratio_parent_over_new": round(min(runs[ma]) / min(runs[mb]), 2)}
            for m in (ma, mb):
                trees[m], size = tree(os.path.join(d, "out_" + m))
                summary["tree_bytes_" + m] = size
                shutil.rmtree(os.path.join(d, "out_" + m), ignore_errors=True)
            summary["trees_equal"] = trees[ma] == trees[mb] == trees["emit_gpu"]
            trees = {"emit_gpu": trees["emit_gpu"]}
            result["cli"][pair] = summary
            print(json.dumps({"post_text_pair": pair, **summary}), flush=True)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        dst = os.environ.get("C3_POST_TEXT_THROUGHPUT_JSON", os.path.join(ROOT, "profiles", "post_text_throughput.json"))
        with open(dst, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()

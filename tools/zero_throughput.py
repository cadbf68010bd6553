"""Zero-repeat rescue throughput: batches of only zero-repeat reads (one splint, two overlapping dangling pieces).

    python tools/zero_throughput.py [--out profiles/zero_throughput.json] [--reps 3]

For each piece length (2, 4, 8, 16 kb per piece) one batch: reads/s and counted Gcell/s (the alignment cells
front * tail that the oracle counts, and the POA cells of the overlap) from the host clock around run(), which ends
in a device synchronise, after a warm-up run.  At 3 kb x 3 kb, k_zero against the forced k_zero_long path
(C3_DEBUG_ZERO_LONG=1), alternated in one process.  A 32-read parity sample against the oracle (8 kb batch).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from c3poa_amd import _lib, synth  # noqa: E402


def batch(piece, n, seed):
    """reads ins[a:] + splint + ins[:b] with both pieces ~`piece` long and an overlap of half a piece"""
    rng = np.random.default_rng(seed)
    L, a, b = piece * 3 // 2, piece // 2, piece
    return [synth.make_zero_read(rng, synth.SPLINT1, L, a, b) for _ in range(n)]


def timed_runs(h, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        h.run()
        ts.append(time.perf_counter() - t0)
    return ts


def measure(recs, cap, reps, force_long=False):
    if force_long:
        os.environ["C3_DEBUG_ZERO_LONG"] = "1"
    else:
        os.environ.pop("C3_DEBUG_ZERO_LONG", None)
    h = _lib.Handle(zero_max_cells=cap)
    h.set_splints([synth.SPLINT1])
    h.upload([r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs])
    h.run()                                                          # warm-up: code objects, scratch
    ts = timed_runs(h, reps)
    res, cons = h.results()
    tm = h.timing()
    h.close()
    os.environ.pop("C3_DEBUG_ZERO_LONG", None)
    lens = np.array([len(r[0]) for r in recs])
    zc = int(np.sum(res["front_end"].astype(np.int64) * (lens - res["tail_beg"])))
    return ts, res, cons, zc, tm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "zero_throughput.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parity", type=int, default=32)
    args = ap.parse_args()
    out = {"sizes": [], "ab_3kb": None, "parity": None}
    sizes = ((2000, 1024), (4000, 512), (8000, 256), (16000, 64))
    keep = None
    for piece, n in sizes:
        recs = batch(piece, n, 1000 + piece)
        cap = min((1 << 31) - 1, 2 * piece * piece)
        ts, res, cons, zc, tm = measure(recs, cap, args.reps)
        t = min(ts)
        ok = int(np.sum(res["status"] == 0))
        row = {"piece": piece, "reads": n, "rescued": ok, "s_best": t, "s_all": ts, "reads_per_s": n / t,
               "align_cells": zc, "align_gcells_per_s": zc / t / 1e9, "cells_poa": int(tm["cells_poa"]),
               "poa_gcells_per_s": tm["cells_poa"] / t / 1e9}
        out["sizes"].append(row)
        print(json.dumps(row), flush=True)
        if piece == 8000:
            keep = (recs, res, cons, cap)
    # k_zero vs forced k_zero_long on pieces both can hold (3 kb x 3 kb), alternated
    recs = batch(3000, 512, 3000)
    ab = {"piece": 3000, "reads": len(recs), "k_zero_s": [], "k_zero_long_s": []}
    same = True
    ref = None
    for _ in range(3):
        for key, force in (("k_zero_s", False), ("k_zero_long_s", True)):
            ts, res, cons, zc, tm = measure(recs, 16 << 20, 1, force_long=force)
            ab[key].append(ts[0])
            if ref is None:
                ref = cons
            same = same and cons == ref
    ab["align_cells"] = zc
    ab["long_over_short"] = min(ab["k_zero_long_s"]) / min(ab["k_zero_s"])
    ab["same_consensus"] = same
    out["ab_3kb"] = ab
    print(json.dumps(ab), flush=True)
    # parity sample against the oracle
    from oracle import oracle_py as O
    recs, res, cons, cap = keep
    k = min(args.parity, len(recs))
    ores, ocons = O.process_batch(synth.SPLINT1, [(r[0], r[1]) for r in recs[:k]], [r[2] for r in recs[:k]],
                                  params=O.default_params(zr_max_cells=cap), threads=16)
    mism = sum(1 for i in range(k) if cons[i] != ocons[i] or int(res[i]["status"]) != ores[i].status)
    out["parity"] = {"piece": 8000, "reads": k, "mismatches": mism}
    print(json.dumps(out["parity"]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

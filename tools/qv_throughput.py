"""Per-base consensus QV stage (k_qv) cost and calibration.

    python tools/qv_throughput.py [--out profiles/qv_throughput.json] [--reps 3]

For cfg2 (100 000 reads), cfg4, cfgL and a zero-repeat batch: one handle, the batch resident, runs of STAGES_ALL and
STAGES_ALL | STAGE_QV alternated `reps` times after a warm-up of each.  Reports k_qv time (hipEvents, ms_qv), band cells/s,
pieces, the edge-hit fraction, and the wall time of the two kinds of step (host clock around c3_batch_run, which ends in a
device synchronise).  Then a calibration table on cfg1 reads with known truth: every consensus is aligned to its truth
(unit-cost edit distance), each consensus base is an error when it is not a match, and the error rate per QV bin is given.
The QVs are support scores, not calibrated probabilities: the table shows how far apart the two are.
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
from c3poa_amd.seqio import revcomp  # noqa: E402


def zero_batch(n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        L = int(rng.integers(900, 1600))
        a, b = int(rng.integers(100, L // 3)), int(rng.integers(2 * L // 3, L - 50))
        s, q, st, t = synth.make_zero_read(rng, synth.SPLINT1, L, a, b)
        out.append(("z", s, q, st, t))
    return out


def measure(name, recs, reps):
    h = _lib.Handle()
    h.set_splints([synth.SPLINT1])
    h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    h.run()
    h.run(qv=True)                                                   # warm-up of both kinds (code objects, scratch)
    base, withq, qt = [], [], []
    for _ in range(reps):
        t0 = time.perf_counter(); h.run(); base.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); h.run(qv=True); withq.append(time.perf_counter() - t0)
        qt.append(h.qv_timing())
    h.close()
    ms_qv = min(t["ms_qv"] for t in qt)
    t = qt[-1]
    row = {"batch": name, "reads": len(recs), "reads_with_qv": t["n_reads"], "pieces": t["n_pieces"],
           "skipped": t["n_skipped"], "band_cells": t["band_cells"], "ms_qv_best": ms_qv, "ms_qv_all": [x["ms_qv"] for x in qt],
           "gcells_per_s": t["band_cells"] / (ms_qv * 1e-3) / 1e9, "edge_hit_fraction": t["edge_hits"] / max(1, t["n_pieces"]),
           "ms_step_all": [1e3 * x for x in base], "ms_step_all_qv": [1e3 * x for x in withq],
           "added_ms_per_step": 1e3 * (min(withq) - min(base)), "step_ratio": min(withq) / min(base),
           "ms_qv_per_100k_reads": ms_qv * 1e5 / len(recs)}
    print(json.dumps(row), flush=True)
    return row


def errors(cons, truth):
    """1 per consensus base that is not a match in a unit-cost global alignment to truth"""
    n, m = len(cons), len(truth)
    D = np.zeros((n + 1, m + 1), dtype=np.int32)
    D[:, 0] = np.arange(n + 1); D[0, :] = np.arange(m + 1)
    t = np.frombuffer(truth.encode(), dtype=np.uint8)
    ar = np.arange(m + 1)
    for i in range(1, n + 1):
        row = np.minimum(D[i - 1, :-1] + (t != ord(cons[i - 1])), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(np.concatenate(([i], row)) - ar) + ar
    err = np.zeros(n, dtype=np.int8)
    i, j = n, m
    while i > 0:
        if j > 0 and D[i, j] == D[i - 1, j - 1] + (cons[i - 1] != truth[j - 1]):
            err[i - 1] = cons[i - 1] != truth[j - 1]; i -= 1; j -= 1
        elif D[i, j] == D[i - 1, j] + 1:
            err[i - 1] = 1; i -= 1
        else:
            j -= 1
    return err


def calibration(n_reads):
    recs = list(synth.generate("cfg1", n_reads=n_reads, seed=4242))
    h = _lib.Handle()
    h.set_splints([synth.SPLINT1])
    h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
    h.run(qv=True)
    res, cons, qv = h.results(qv=True)
    h.close()
    edges = [0, 10, 20, 30, 40, 50, 60, 61]
    tot, bad = np.zeros(len(edges) - 1, dtype=np.int64), np.zeros(len(edges) - 1, dtype=np.int64)
    for i, r in enumerate(recs):
        if not cons[i]:
            continue
        e = min((errors(cons[i], t) for t in (r[4], revcomp(r[4]))), key=lambda x: int(x.sum()))
        q = np.frombuffer(qv[i].encode(), dtype=np.uint8).astype(np.int64) - 33
        b = np.digitize(q, edges) - 1
        tot += np.bincount(b, minlength=len(tot))[:len(tot)]
        bad += np.bincount(b, weights=e, minlength=len(tot)).astype(np.int64)[:len(tot)]
    rows = []
    for k in range(len(tot)):
        rate = bad[k] / tot[k] if tot[k] else None
        rows.append({"qv_bin": "%d-%d" % (edges[k], edges[k + 1] - 1), "bases": int(tot[k]), "errors": int(bad[k]),
                     "error_rate": rate, "empirical_phred": (-10 * np.log10(rate) if rate else None)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qv_throughput.json"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--calib-reads", type=int, default=120)
    args = ap.parse_args()
    out = {"batches": [], "calibration": None}
    for name, recs in (("cfg2", list(synth.generate("cfg2", n_reads=100000))),
                       ("cfg4", list(synth.generate("cfg4", n_reads=10000))),
                       ("cfgL", list(synth.generate("cfgL", n_reads=5000))),
                       ("zero", zero_batch(10000, 17))):
        out["batches"].append(measure(name, recs, args.reps))
        del recs
    out["calibration"] = calibration(args.calib_reads)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()

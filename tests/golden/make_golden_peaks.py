#!/usr/bin/env python3
"""Generate the peak-calling edge fixtures by RUNNING THE REFERENCE'S OWN PYTHON (read-only, /root/reference).

Run in the build container only (the reference does not travel to the GPU box):
    python tests/golden/make_golden_peaks.py
Outputs (committed): tests/golden/peaks_edges.json, tests/golden/peaks_edges.npz and its continuation files
peaks_edges_<k>.npz (the smoothed fp64 tracks do not compress; every file stays well below the size limit for a committed file).

What is pinned here: bin/call_peaks.py + bin/savitzky_golay.py + scipy.signal.find_peaks at the settings, lengths and
min_dist values of tests/peaks_edge_tracks.py (other windows, pass counts and orders than 3/41/2; lengths around the window,
the 256-key exit of the median select, the 1024-point smoothing tile and its halo).
  * peaks_edges.json: the reference's peaks of every case
  * peaks_edges*.npz: the input tracks (one per name, shared by the settings) and, for one min_dist per (setting, track),
    the reference's smoothed track
Every case is also run through the oracle; the generator stops at the first one where the oracle's peaks differ from the
reference's or its smoothed track leaves the tolerance of tests/test_oracle_golden.py.  The one kind of case that is not
pinned is an exact tie between two peaks closer than min_dist (see exact_tie): it is listed under `ties`, never dropped
silently, and anything else that differs stops the run.
Nothing from /root/reference is copied: only inputs we generate and the outputs it computes.
"""
import io
import json
import os
import sys
import zipfile

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

# numpy>=1.24 removed np.int / np.mat which bin/savitzky_golay.py:19-20,30 uses
np.int = int
np.mat = np.asmatrix

sys.path.insert(0, os.path.join(REF, "bin"))
from call_peaks import call_peaks            # noqa: E402
from savitzky_golay import savitzky_golay    # noqa: E402

import peaks_edge_tracks as T                # noqa: E402
from oracle import oracle_py as O            # noqa: E402

PART_BYTES = 900 * 1024
MAX_PEAKS = 255                              # a GPU read keeps at most C3_MAX_PEAKS - 1 peaks: the grid stays below


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that a rerun gives the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays:
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue())


def packed_size(name, a):
    buf = io.BytesIO()
    write_npz(buf, [(name, a)])
    return buf.tell()


def exact_tie(osm, cand, md):
    """two peaks closer than md whose heights are bit-equal in the oracle's track: the specification's answer there is
    'later index first', the reference's depends on the last bit of its BLAS sums (the step track smooths to a mirror-symmetric
    overshoot at either edge of a step).  Such a case cannot be pinned from the reference; it is listed under `ties` and the
    tests check it against the oracle alone."""
    return any(0 < b - a < md and osm[a] == osm[b] for a in cand for b in cand)


def main():
    peaks = {}
    tracks = {}
    smoothed = []
    ties = []
    worst = 0.0
    for s in T.SETTINGS:
        iters, window, order = s
        for name, t in T.grid_tracks(s):
            if name in tracks:
                assert np.array_equal(tracks[name], t)
            tracks[name] = t
            sm = t
            for _ in range(iters):
                sm = savitzky_golay(sm, window, order)
            sm = np.asarray(sm, dtype=np.float64)
            assert len(sm) == len(t), (s, name)
            for md in T.MIN_DISTS:
                pk = [int(p) for p in call_peaks(t, md, iters, window, order)]
                opk, osm = O.call_peaks(t, md, iters, window, order, return_smoothed=True)
                key = T.case_key(s, name, md)
                if opk.tolist() != pk and exact_tie(osm, O.call_peaks(t, 1, iters, window, order), md):
                    ties.append(key)
                    continue
                assert opk.tolist() == pk, "oracle and reference disagree on the peaks of %s: %s / %s" % (key, opk.tolist(), pk)
                np.testing.assert_allclose(osm, sm, rtol=1e-9, atol=1e-7, err_msg=key)
                assert len(pk) <= MAX_PEAKS, (key, len(pk))
                if iters == 0 and len(pk) > 1:
                    # scipy orders equal peaks by an unstable argsort: keep ties out of what is pinned
                    h = t[pk]
                    assert len(set(h.tolist())) == len(pk) or md <= np.diff(pk).min(), key
                peaks[key] = pk
            den = np.maximum(np.abs(sm), 1e-300)
            worst = max(worst, float(np.max(np.abs(osm - sm) / den)) if iters else 0.0)
            smoothed.append(("sm/%s/%s" % (T.setting_id(s), name), sm))
    json.dump(dict(settings=[list(s) for s in T.SETTINGS], min_dists=list(T.MIN_DISTS), smoothed_min_dist=T.SMOOTHED_MIN_DIST,
                   ties=ties, peaks=peaks), open(os.path.join(HERE, "peaks_edges.json"), "w"), indent=0, sort_keys=True)
    # tracks first, then the smoothed tracks, cut into files of at most PART_BYTES
    parts, cur, size = [], [], 0
    for name, a in [("track/" + k, v) for k, v in sorted(tracks.items())] + smoothed:
        b = packed_size(name, a)
        if cur and size + b > PART_BYTES:
            parts.append(cur)
            cur, size = [], 0
        cur.append((name, a))
        size += b
    parts.append(cur)
    for old in os.listdir(HERE):
        if old.startswith("peaks_edges") and old.endswith(".npz"):
            os.remove(os.path.join(HERE, old))
    for k, part in enumerate(parts):
        write_npz(os.path.join(HERE, "peaks_edges.npz" if k == 0 else "peaks_edges_%d.npz" % k), part)
    print("ties:", ties)
    print("wrote %d cases, %d tracks, %d smoothed tracks in %d npz files; oracle vs reference smoothed: max relative "
          "difference %.3g" % (len(peaks), len(tracks), len(smoothed), len(parts), worst))


if __name__ == "__main__":
    main()

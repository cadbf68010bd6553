"""Track builders and case lists shared by the peak-calling edge tests (CPU: test_peaks_edges_host.py, GPU:
test_gpu_peaks_edges.py) and by tests/golden/make_golden_peaks.py.  A plain module, no fixtures: everything here is a pure
function of its arguments, so the generator, the CPU tests and the GPU tests see the same inputs.

Two families:
  * the smoothed grid (SETTINGS x lengths(window) x MIN_DISTS): noise + Gaussian bumps, a step track, an all-equal track;
    expected values come from the reference (tests/golden/peaks_edges*.{json,npz}) and from the oracle;
  * exact-arithmetic tracks for sg_iters = 0 (small integers, no smoothing): expected values come from py_call_peaks below,
    a restatement of the specification in plain Python that shares no code with oracle/c3o_signal.c.
"""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# (sg_iters, sg_window, sg_order)
SETTINGS = [(3, 41, 2), (1, 41, 2), (2, 41, 2), (0, 41, 2), (3, 5, 2), (3, 21, 2), (3, 43, 2), (3, 45, 2), (1, 127, 2),
            (2, 127, 2), (3, 41, 3)]
MIN_DISTS = (1, 50, 500)
SMOOTHED_MIN_DIST = 50          # the one min_dist per (setting, length) whose smoothed track is stored
STEP_N, EQUAL_N = 3000, 700


def setting_id(s):
    return "i%d_w%d_o%d" % s


def lengths(window):
    """track lengths for a window: around the shortest legal track, the window itself, the radix select's 256-key exit,
    the 1024-point smoothing tile and its three-pass halo, and tile counts 2, 3 (+1) and 5"""
    half = (window - 1) // 2
    return sorted({half + 1, half + 2, window - 1, window, window + 1, 2 * window, 255, 256, 257, 1023, 1024, 1025,
                   1024 + 3 * half, 1024 + 3 * half + 1, 2047, 2048, 2049, 3073, 5000})


def all_lengths():
    return sorted({n for _i, w, _o in SETTINGS for n in lengths(w)})


def bump_track(n):
    """seeded noise plus Gaussian bumps of pairwise distinct heights, one track per length"""
    rng = np.random.default_rng(1000 + n)
    x = np.arange(n)
    y = np.abs(rng.normal(10, 3, n))
    period = max(60, min(300, n // 3))
    for k, c in enumerate(range(period // 2, n, period)):
        y += (400 + 37 * k) * np.exp(-0.5 * ((x - c) / 15.0) ** 2)
    return y.astype(np.int32)


def distinct_track(n):
    """bump_track(n) with every value made distinct (low bits = a seeded permutation): without smoothing (sg_iters = 0) an
    integer track is full of equal peaks, and scipy orders equal peaks by an unstable argsort"""
    assert n <= 8192
    rng = np.random.default_rng(2000 + n)
    return (bump_track(n).astype(np.int64) * 8192 + rng.permutation(n)).astype(np.int32)


def step_track():
    z = np.zeros(STEP_N, dtype=np.int32)
    z[1000:1400] = 5000
    z[2000:2400] = 5000
    return z


def equal_track():
    return np.full(EQUAL_N, 7, dtype=np.int32)


def grid_tracks(setting):
    """[(name, track)] of one setting; the name is the key in the fixture files"""
    iters, window, _order = setting
    out = []
    for n in lengths(window):
        out.append(("dist_%d" % n, distinct_track(n)) if iters == 0 else ("bump_%d" % n, bump_track(n)))
    out.append(("step", step_track()))
    out.append(("equal", equal_track()))
    return out


def load_fixtures():
    """(peaks_edges.json, {array name: array} over peaks_edges.npz and its continuation files)"""
    js = json.load(open(os.path.join(GOLDEN, "peaks_edges.json")))
    arrays = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "peaks_edges*.npz"))):
        with np.load(path) as z:
            for k in z.files:
                assert k not in arrays, k
                arrays[k] = z[k]
    return js, arrays


def case_key(setting, name, min_dist):
    return "%s/%s/d%d" % (setting_id(setting), name, min_dist)


# ---- the specification in plain Python (sg_iters = 0: the track is used as it is) -------------------------------------------
def py_call_peaks(x, min_dist):
    """bin/call_peaks.py:12-16 on an unsmoothed track, with scipy.signal.find_peaks(x, distance=, height=) spelled out:
    median gate -> strict local maxima (a plateau counts once, at its midpoint, rounded down) -> height >= 3 * median ->
    highest first, equal heights later index first, each kept peak removing the others closer than min_dist."""
    x = [float(v) for v in x]
    n = len(x)
    s = sorted(x)
    med = s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0
    if max(x) < 6 * med:
        return []
    cand = []
    i = 1
    while i < n - 1:
        if x[i - 1] < x[i]:
            j = i
            while j + 1 < n - 1 and x[j + 1] == x[i]:
                j += 1
            if x[j + 1] < x[i]:
                cand.append((i + j) // 2)
            i = j
        i += 1
    cand = [p for p in cand if x[p] >= 3 * med]
    dist = max(int(min_dist), 1)
    alive = set(cand)
    kept = []
    for p in sorted(cand, key=lambda q: (x[q], q), reverse=True):
        if p in alive:
            kept.append(p)
            alive -= {q for q in alive if abs(q - p) < dist}
    return sorted(kept)


def _flat(n, v=10):
    return [v] * n


def _with(base, **at):
    z = list(base)
    for k, v in at.items():
        z[int(k[1:])] = v
    return z


def _plateau(n, lo, hi, v=100, base=10):
    """x[lo:hi] = v on a flat baseline"""
    z = [base] * n
    z[lo:hi] = [v] * (hi - lo)
    return z


def exact_cases():
    """[(name, track, min_dist, expected or None)] for sg_iters = 0.  `expected` is stated by hand where the issue of a
    case is a specific answer; every case is also checked against py_call_peaks and the oracle."""
    C = []
    # median gate: max >= 6 * median passes, one less is gated
    C.append(("gate_pass", _with(_flat(101), i50=60), 1, [50]))
    C.append(("gate_fail", _with(_flat(101), i50=59), 1, []))
    # inclusive height: x == 3 * median is a peak, one less is not (x[50] keeps the gate open)
    C.append(("height_incl", _with(_flat(101), i50=60, i20=30), 1, [20, 50]))
    C.append(("height_excl", _with(_flat(101), i50=60, i20=29), 1, [50]))
    # equal heights closer than min_dist: the later index wins
    eq = _with(_flat(101), i10=100, i13=100, i16=100)
    C.append(("equal_d3", eq, 3, [10, 13, 16]))
    C.append(("equal_d4", eq, 4, [10, 16]))
    C.append(("equal_d7", eq, 7, [16]))
    # plateaus: midpoint rounded down
    C.append(("plateau_odd", _plateau(101, 40, 45), 1, [42]))
    C.append(("plateau_even", _plateau(101, 40, 44), 1, [41]))
    C.append(("plateau_two", _plateau(101, 40, 42), 1, [40]))
    # a plateau that touches either end is no peak; nor is a rise without a fall
    C.append(("plateau_at_start", _plateau(101, 0, 5), 1, []))
    C.append(("plateau_at_end", _plateau(101, 96, 101), 1, []))
    C.append(("plateau_both_ends_and_one", [90] * 5 + [10] * 45 + [100] + [10] * 45 + [90] * 5, 1, [50]))
    # a plateau across the boundary between two threads' chunks of ceil(n / 256) points, even and odd widths
    for n in (257, 512, 1000):
        chunk = -(-n // 256)
        for k in (1, 100, (n - 4) // chunk):
            b = k * chunk
            for lo, hi in ((b - 1, b + 1), (b - 2, b + 1), (b - 3, b + 4), (b, b + 3), (b - 3, b)):
                if lo >= 1 and hi <= n - 1:
                    C.append(("straddle_n%d_k%d_%d_%d" % (n, k, lo - b, hi - b), _plateau(n, lo, hi), 1, [(lo + hi - 1) // 2]))
        # one plateau over several whole chunks
        C.append(("straddle_wide_n%d" % n, _plateau(n, chunk * 3 - 1, chunk * 7 + 1), 1, [(chunk * 3 - 1 + chunk * 7) // 2]))
    # all zeros: median 0, the gate is open (0 < 0 is false), no strict maximum
    C.append(("zeros", [0] * 300, 1, []))
    # all equal: the radix select never narrows the keys down (n > 256) / exits at once (n <= 256)
    for n in (256, 257, 700):
        C.append(("all_equal_%d" % n, [7] * n, 1, []))
    # even n, two values: the two middle order statistics equal (median 10 -> spike of 60 passes, 59 gated) ...
    C.append(("median_dup_pass", _with([10] * 60 + [0] * 40, i30=60), 1, [30]))
    C.append(("median_dup_gate", _with([10] * 60 + [0] * 40, i30=59), 1, []))
    # ... and different (50 zeros, 48 tens and two spikes -> median 5): 30 is the gate, 15 the height
    C.append(("median_split_pass", _with([10] * 50 + [0] * 50, i30=30, i20=15), 1, [20, 30]))
    C.append(("median_split_gate", _with([10] * 50 + [0] * 50, i30=29, i20=15), 1, []))
    C.append(("median_split_height", _with([10] * 50 + [0] * 50, i30=30, i20=14), 1, [30]))
    # negative values: keys of negative doubles order the other way round
    C.append(("negative", _with([-5] * 60 + [-20] * 41, i30=-1, i80=-2), 1, [30, 80]))
    C.append(("negative_even", _with([-5] * 60 + [-20] * 40, i30=-1, i80=-2), 1, [30, 80]))
    # min_dist 0, 1 and n
    sp = _with(_flat(200), i20=100, i21=10, i22=100, i24=101, i150=90)
    C.append(("dist_0", sp, 0, [20, 22, 24, 150]))
    C.append(("dist_1", sp, 1, [20, 22, 24, 150]))
    C.append(("dist_2", sp, 2, [20, 22, 24, 150]))
    C.append(("dist_3", sp, 3, [20, 24, 150]))
    C.append(("dist_n", sp, 200, [24]))
    # more than 256 equal candidates within min_dist of each other: a thread of the argmax loop then holds two tied candidates
    # itself (c and c + 256), and the later index must win there as well
    eq400 = spikes_track(400).tolist()
    C.append(("tie_400_candidates_d_n", eq400, len(eq400), [2 + 4 * 399]))
    C.append(("tie_400_candidates_d1200", eq400, 1200, [2 + 4 * 99, 2 + 4 * 399]))
    # dense ties and plateaus: small alphabets.  Uniform values 0..4 have median 2 and never pass the gate (4 < 12), so the
    # values are skewed: even seeds 0..4 with median 0 (gate open, height 0: every local maximum counts), odd seeds the values
    # (1, 0, 2, 3, 6) with median 1 (gate at 6, height 3: the 2s drop out, the 3s are exactly on the height)
    for n in (64, 300, 1025):
        p0 = 0.8 if n > 1000 else 0.55                 # fewer than 256 peaks also at n = 1025
        for seed in range(20):
            rng = np.random.default_rng(31 * n + seed)
            v = rng.choice(5, size=n, p=[p0] + [(1 - p0) / 4] * 4)
            if seed & 1:
                v = np.array([1, 0, 2, 3, 6])[v]
            C.append(("alphabet_n%d_s%d" % (n, seed), v.tolist(), int(rng.integers(0, 6)), None))
    return C


def spikes_track(k):
    """k one-point spikes, four points apart: z[2 : 2 + 4k : 4] = 1000"""
    z = np.zeros(2 + 4 * k + 2, dtype=np.int32)
    z[2:2 + 4 * k:4] = 1000
    return z

"""k_poa_pair: the alignment of subread 1 against the bare chain of subread 0 runs in a lean kernel of its own
ahead of the first k_poa pass, which then takes the stored vq for the reads that kernel has flagged.  That is a schedule, never a
change of result.  Every case asserts
  * default == C3_DEBUG_POA_PAIR=0 (kernel not launched) == the CPU oracle, bit for bit: consensus, draft (status, n_sub,
    draft_len, cons_len for batches), counted cells, n_poa_redo, n_poa_redo16 -- both GPU runs under C3_DEBUG_POISON;
  * n_pair is what the case expects: every read the kernel can take (worked out on the ORACLE side: subread 1 at most 1792 bases,
    every row of its alignment at most 128 columns), or zero where the kernel must not run.  No case passes with the kernel idle.
Subread lengths at the seams (40 ... 129 bases) cannot come out of the splitter (the splint alone is 284 bases), so the shapes
are injected pre-split through the determine_consensus probe, which runs the same POA stage on the same handle; batches of
synthetic reads cover the work list, many slots, the zero-repeat rescue and a reused handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c3poa_amd import _lib, synth  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = {"C3_DEBUG_POISON": "1"}
OFF = {"C3_DEBUG_POA_PAIR": "0"}
QMAX = 1792


class _env:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _acgt(rng, n):
    return synth._ACGT[rng.integers(0, 4, n)].tobytes().decode()


def _noisy(rng, clean):
    s, q = synth._mutate(rng, np.frombuffer(clean.encode(), dtype=np.uint8))
    return s.decode(), q.decode()


def _fit(rng, s, q, n):
    """(s, q) cut or padded to exactly n bases"""
    if len(s) < n:
        s += _acgt(rng, n - len(s)); q += "5" * (n - len(q))
    return s[:n], q[:n]


def _rows(s0, s1, **cfg):
    """oracle side: band widths of the rows of subread 1 against the chain of subread 0 ->
    dict(can = the kernel can take the pair, wide = rows of 65-128 columns, over = rows beyond 128 columns)"""
    lib = O.lib()
    S = (C.c_int64 * 64).in_dll(lib, "c3o_poa_rowstats")
    on = C.c_int.in_dll(lib, "c3o_poa_rowstats_on")
    for i in range(64):
        S[i] = 0
    on.value = 1
    try:
        P = O.default_params(**cfg)
        O.poa_msa([s0, s1], out_cons=False, out_msa=True, params=P)
    finally:
        on.value = 0
    w = P.poa_band_b + int(P.poa_band_f * len(s1))
    wd0 = min(len(s1), max(len(s1) - len(s0), 0) + w) + 1          # the source row
    wide, over = int(S[31] + S[32]), int(S[33]) + (1 if wd0 > 128 else 0)
    assert int(S[0]) == len(s0)
    return dict(can=len(s1) <= QMAX and over == 0, wide=wide + (1 if 64 < wd0 <= 128 else 0), over=over)


def _probe_runs(shapes, env=None, pair_runs=True, **cfg):
    """shapes: list of (subs, quals).  Runs them one after the other on ONE handle per GPU run (a reused handle: stale flags, a stale
    vq, reused slots), default and with the kernel off, and against the oracle.  Returns the oracle-side row facts per shape."""
    env = dict(env or {})
    P = O.default_params(**cfg)
    want = [O.determine_consensus(s, q, params=P, return_draft=True) for s, q in shapes]
    facts = [_rows(s[0], s[1], **cfg) if len(s) >= 2 else dict(can=False, wide=0, over=0) for s, _ in shapes]
    got = {}
    for name, extra in (("on", {}), ("off", OFF)):
        with _env(dict(POISON, **env, **extra)):
            h = _lib.Handle(**cfg)
            out = []
            for s, q in shapes:
                cons, draft = h.determine_consensus(s, q, return_draft=True)
                t = h.timing()
                out.append((cons, draft, int(t["cells_poa"]), int(t["n_poa_redo"]), int(t["n_poa_redo16"]), int(t["n_pair"]), int(t["n_pair_declined"])))
            h.close()
        got[name] = out
    for k, ((s, q), (wc, wdr, wcells), f) in enumerate(zip(shapes, want, facts)):
        a, b = got["on"][k], got["off"][k]
        lens = [len(x) for x in s]
        assert a[:5] == b[:5], (k, lens, env)
        assert a[0] == wc and a[1] == wdr and a[2] == wcells[0], (k, lens, env)
        assert b[5] == 0 and b[6] == 0, (k, lens, env)
        exp = 1 if (pair_runs and f["can"]) else 0
        assert a[5] == exp, (k, lens, env, f, a[5:])
        if pair_runs and len(s) >= 2:
            assert a[5] + a[6] == 1, (k, lens, env, a[5:])
    return facts


def _family(rng, n_ins, lens):
    """subreads of one random insert, noisy copies cut / padded to the given lengths"""
    ins = _acgt(rng, n_ins)
    subs, quals = [], []
    for n in lens:
        s, q = _fit(rng, *_noisy(rng, ins), n)
        subs.append(s); quals.append(q)
    return subs, quals


def test_seam_lengths():
    rng = np.random.default_rng(101)
    shapes = []
    for n in (40, 63, 64, 65, 127, 128, 129, 1500):
        shapes.append(_family(rng, n, (n, n - 1 if n % 2 else n + 1, n)))      # 3 subreads: heaviest bundling
        shapes.append(_family(rng, n, (n + 1, n)))                              # 2 subreads: pairwise merge
    shapes.append(_family(rng, 1790, (1785, QMAX, 1780)))                       # Q1 at the limit: taken
    shapes.append(_family(rng, 1790, (1785, QMAX - 1, 1780)))
    facts = _probe_runs(shapes)
    assert all(f["can"] for f in facts)
    # just above: the kernel declines.  (A batch with such a subread takes the WIDE instance, where the kernel does not run at
    # all; the NARROW instance is forced, as tests/test_gpu_poa16.py does for long subreads)
    facts = _probe_runs([_family(rng, 1790, (1785, QMAX + 1, 1780)), shapes[-1]], env={"C3_DEBUG_POA_WIDE": "0"})
    assert not facts[0]["can"] and facts[1]["can"]


def test_a_long_subread_takes_the_wide_instance():
    rng = np.random.default_rng(102)
    shapes = [_family(rng, 2600, (2600, 2590, 2605))]
    _probe_runs(shapes, pair_runs=False)


@pytest.mark.parametrize("ns", [2, 3, 5])
def test_subread_counts(ns):
    rng = np.random.default_rng(200 + ns)
    shapes = [_family(rng, 700, tuple(700 + 3 * k for k in range(ns))), _family(rng, 300, tuple(300 - 2 * k for k in range(ns)))]
    facts = _probe_runs(shapes)
    assert all(f["can"] for f in facts)


def _ragged_pair(rng, n_ins, delta, ns=3):
    """subread 1 loses (delta < 0) or doubles (delta > 0) a chunk of |delta| bases in the middle: the band drifts and widens"""
    ins = _acgt(rng, n_ins)
    at = n_ins // 2
    alt = ins[:at] + ins[at - delta:] if delta < 0 else ins[:at] + ins[at - delta:at] + ins[at:]
    subs, quals = [], []
    for k in range(ns):
        s, q = _noisy(rng, alt if k == 1 else ins)
        subs.append(s); quals.append(q)
    return subs, quals


def test_ragged_pairs():
    rng = np.random.default_rng(303)
    shapes = [_ragged_pair(rng, 800, d) for d in (-25, 25, -45, 45, -70, 70, -95, 95)]
    shapes.append(_ragged_pair(rng, 1000, -300))                                 # Q1 about 0.7 x Q0
    shapes.append(_ragged_pair(rng, 1000, 400))                                  # Q1 about 1.4 x Q0
    shapes.append(_ragged_pair(rng, 600, -60, ns=2))
    facts = _probe_runs(shapes)
    # the generator cannot hollow the case out: two-column rows in reads the kernel takes, and reads that drift past 128 columns
    assert any(f["can"] and f["wide"] > 0 for f in facts), facts
    assert any(f["over"] > 0 for f in facts), facts
    assert any(f["can"] for f in facts) and not all(f["can"] for f in facts)


def test_special_shapes():
    rng = np.random.default_rng(404)
    ins = _acgt(rng, 200)
    s0, q0 = _noisy(rng, ins)
    s2, q2 = _noisy(rng, ins)
    shapes = [
        ([ins, ins, ins], ["I" * 200, "5" * 200, "+" * 200]),                    # one diagonal run across block boundaries
        ([ins, ins], ["I" * 200, "5" * 200]),
        ([s0, "GATTACA" + s0, s2], [q0, "5" * 7 + q0, q2]),                      # subread 1 begins with an insertion
        ([s0, s0[:-9], s2], [q0, q0[:-9], q2]),                                  # ... ends in a deletion against subread 0
        ([s0, s0[6:], s2], [q0, q0[6:], q2]),                                    # ... begins with a deletion
        ([s0, s0 + "CCGTA", s2], [q0, q0 + "5" * 5, q2]),                        # ... ends with an insertion
    ]
    facts = _probe_runs(shapes)
    assert all(f["can"] for f in facts)


def test_moving_base():
    """C3_DEBUG_POA_RBSPAN=3300: the 16-bit base moves every few rows (the saturating rebase of all three row kinds)"""
    rng = np.random.default_rng(505)
    shapes = [_family(rng, 1500, (1500, 1490, 1510)), _ragged_pair(rng, 800, 45), _ragged_pair(rng, 800, -70), _family(rng, 90, (90, 91))]
    facts = _probe_runs(shapes, env={"C3_DEBUG_POA_RBSPAN": "3300"})
    assert any(f["can"] and f["wide"] > 0 for f in facts) and facts[0]["can"]


@pytest.mark.parametrize("env,cfg", [
    ({"C3_DEBUG_POA_SMALL": "64"}, {}),              # the first pass's slots hold 64 nodes: every read declined, redone by the second pass
    ({"C3_DEBUG_POA32": "1"}, {}),                   # every pass is the 32-bit instance
    ({"C3_DEBUG_POA_WIDE": "1"}, {}),                # the WIDE instance
    ({}, {"poa_match": 2}),                          # a non-default scoring
])
def test_other_instances_and_scorings_recompute(env, cfg):
    rng = np.random.default_rng(606)
    shapes = [_family(rng, 500, (500, 495, 505)), _ragged_pair(rng, 600, 45), _family(rng, 400, (400, 402))]
    _probe_runs(shapes, env=env, pair_runs=False, **cfg)


def _batch(recs, mdist, env):
    with _env(env):
        h = _lib.Handle(mdistcutoff=mdist)
        h.set_splints([synth.SPLINT1])
        out = []
        for rs in recs:                      # one handle, batch after batch
            h.upload([r[1] for r in rs], [r[2] for r in rs], [r[3] for r in rs])
            h.run()
            res, cons = h.results()
            out.append((res.copy(), cons, dict(h.timing())))
        h.close()
    return out


def _rescued_pair(seq, r, P):
    """oracle side: the two pseudo-subreads a zero-repeat read enters POA with (the overlap slices of its dangling pieces,
    DESIGN.md 4.7), or None when the read is not rescued"""
    if not P.zero or r.n_sub != 0 or r.n_peaks < 1 or not (r.has_front and r.has_tail) or r.front_end <= 0 or r.tail_beg >= len(seq):
        return None
    d0, d1 = seq[:r.front_end], seq[r.tail_beg:]
    if len(d0) * len(d1) > P.zr_max_cells:
        return None
    score, r_st, r_en, q_st, q_en = O.zero_local(d0, d1, params=P)
    if score < P.zr_min_score or r_en <= r_st or q_en <= q_st:
        return None
    return d0[r_st:r_en], d1[q_st:q_en]


def _check_batches(recs, mdist, n_zero=0):
    """n_zero: zero-repeat reads the oracle side must find rescued (the case cannot be hollowed out)"""
    P = O.default_params(mdistcutoff=mdist)
    on = _batch(recs, mdist, POISON)
    off = _batch(recs, mdist, dict(POISON, **OFF))
    for rs, (ra, ca, ta), (rb, cb, tb) in zip(recs, on, off):
        ores, ocons = O.process_batch(synth.SPLINT1, [(r[1], r[2]) for r in rs], [r[3] for r in rs], params=P, threads=8)
        can, jobs, rescued = 0, 0, 0               # reads the kernel can take / POA jobs of >= 2 (pseudo-)subreads / rescued reads
        for i, r in enumerate(rs):
            for f in ("status", "n_sub", "draft_len", "cons_len", "n_win"):
                assert ra[i][f] == rb[i][f], (i, f)
            assert ra[i]["status"] == ores[i].status and ra[i]["n_sub"] == ores[i].n_sub and ra[i]["cons_len"] == ores[i].cons_len, i
            assert ca[i] == cb[i] == ocons[i], i
            pair = None
            if ores[i].n_sub >= 2:
                pair = tuple(r[1][ores[i].sub_beg[k]:ores[i].sub_end[k]] for k in (0, 1))
            elif r[3] in "+-":
                pair = _rescued_pair(r[1], ores[i], P)
                rescued += pair is not None
            if pair is not None:
                jobs += 1
                can += _rows(*pair)["can"]
        for f in ("cells_poa", "n_poa_redo", "n_poa_redo16"):
            assert ta[f] == tb[f], f
        assert ta["cells_poa"] == sum(int(r.cells_poa) for r in ores)
        assert tb["n_pair"] == 0 and tb["n_pair_declined"] == 0
        assert rescued == n_zero, (rescued, n_zero)
        assert can > 0 and ta["n_pair"] == can, (can, jobs, ta["n_pair"], ta["n_pair_declined"])
        assert ta["n_pair"] + ta["n_pair_declined"] == jobs, (can, jobs, ta["n_pair"], ta["n_pair_declined"])
    return on


def test_batches_on_a_reused_handle():
    """the same handle runs two different batches in a row: flags, vq and slots of the first must not leak into the second"""
    a = list(synth.generate("cfg2", n_reads=24))
    b = list(synth.generate("cfg3", n_reads=32, seed=77))[8:]
    _check_batches([a, b, a[:7]], synth.CONFIGS["cfg2"]["mdist"])


def test_a_zero_repeat_read_in_the_batch():
    rng = np.random.default_rng(808)
    recs = list(synth.generate("cfg2", n_reads=10))
    for k in range(2):
        s, q, st, truth = synth.make_zero_read(rng, synth.SPLINT1, 1216, 200, 1000)
        recs.insert(3 + 4 * k, ("z%d" % k, s, q, st, truth))
    _check_batches([recs], synth.CONFIGS["cfg2"]["mdist"], n_zero=2)

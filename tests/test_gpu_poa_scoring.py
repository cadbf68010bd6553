"""k_poa away from abPOA's default scoring: the three kernel instances that read the scores from the parameters (DEF = false:
NARROW, WIDE, W32) instead of carrying 5/4/4/2/24/1 as immediate operands.  The drop-in msa_aligner of c3poa_amd/shims.py
defaults to match = 2, so these instances are what a bare msa_aligner().msa(...) runs.

Every configuration key a test moves goes to BOTH sides: _lib.Handle(**cfg) and O.default_params(**cfg).  The oracle is a sound
reference under these scorings: tests/test_independent_checkers.py holds it against an unbanded brute force for each of them.

  * stage probe (c3_poa_msa) under nine scorings x three shapes (fast / near rows, far predecessors and general rows, the WIDE
    ring) x four set-ups (default, WIDE forced, the 32-bit pass forced, the base of the 16-bit cells moving every few rows);
  * the whole path (k_poa inside the batch, the 2-sequence POA of the zero-repeat rescue) with counted cells, and how many reads
    the 16-bit instances hand to the 32-bit pass: a run in which that pass does all the work says nothing about them;
  * the shim with and without arguments;
  * the ends of the ranges c3_create admits: the last accepted value of every field equals the oracle;
  * poa_band_b / poa_band_f moved together, and pol_q, the last polish field no test moved."""
import contextlib
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c3poa_amd import _lib, shims, synth  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("poa_match", "poa_mismatch", "poa_o1", "poa_e1", "poa_o2", "poa_e2")
# (match, mismatch, o1, e1, o2, e2)
SCORINGS = [
    (5, 4, 4, 2, 24, 1),        # the default: the DEF = true instances, as a control
    (2, 4, 4, 2, 24, 1),        # the shim's default
    (1, 1, 1, 1, 1, 1),         # the two gap pieces identical: M / E1 / E2 and F1 / F2 tie at every gap
    (3, 5, 6, 3, 30, 1),        # an ordinary mix
    (10, 9, 8, 4, 48, 2),       # twice the default: the base moves twice as often, E2 sits 50 below H
    (5, 4, 4, 2, 4, 2),         # identical pieces again, default match
    (5, 4, 0, 3, 0, 3),         # zero open: open ties with extend at every gap
    (7, 2, 10, 1, 10, 1),       # an ordinary mix
    (15, 15, 20, 5, 60, 2),     # the large one
]
ENVS = [{}, {"C3_DEBUG_POA_WIDE": "1"}, {"C3_DEBUG_POA32": "1"}, {"C3_DEBUG_POA_RBSPAN": "3300"}]


def _sid(s):
    return "-".join(map(str, s))


def _cfg(scoring):
    return dict(zip(KEYS, scoring))


@contextlib.contextmanager
def _env(env):
    """the save and restore of test_gpu_poa16._run"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rand(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, n))


def _mut(rng, s):
    return synth._mutate(rng, np.frombuffer(s.encode(), dtype=np.uint8))[0].decode()


def _shape(kind):
    """the smallest inputs that reach each row kind of k_poa"""
    rng = np.random.default_rng({"noisy": 31, "ragged": 32, "long": 33}[kind])
    if kind == "noisy":                                      # 4 noisy copies of 300 bases: fast and near rows of the NARROW instance
        t = _rand(rng, 300)
        return [_mut(rng, t) for _ in range(4)]
    if kind == "ragged":                                     # two copies lose / double a 25-90 base chunk (the shape of test_gpu_poa16._ragged):
        t = _rand(rng, 300)                                  # far predecessors, general rows, the far arena
        out = []
        for k in range(4):
            s = t
            if k in (1, 3):
                at = int(rng.integers(60, 200)); ln = int(rng.integers(25, 90))
                s = s[:at] + s[at + ln:] if k == 1 else s[:at] + s[at:at + ln] + s[at:]
            out.append(_mut(rng, s))
        return out
    t = _rand(rng, 2000)                                     # beyond the 1 792-base LDS query copy: the WIDE instance by default
    return [_mut(rng, t) for _ in range(3)]


_SHAPES = {}
_WANT = {}


def _probe_input(kind):
    if kind not in _SHAPES:
        _SHAPES[kind] = _shape(kind)
    return _SHAPES[kind]


def _oracle_msa(kind, **cfg):
    """(consensus, MSA rows) of the oracle, computed once per (shape, configuration)"""
    key = (kind, tuple(sorted(cfg.items())))
    if key not in _WANT:
        _WANT[key] = O.poa_msa(_probe_input(kind), params=O.default_params(**cfg))[:2]
    return _WANT[key]


def _gpu_msa(kind, env, **cfg):
    with _env(env):
        h = _lib.Handle(**cfg)
        try:
            return h.poa_msa(_probe_input(kind))
        finally:
            h.close()


@pytest.mark.parametrize("kind", ["noisy", "ragged", "long"])
@pytest.mark.parametrize("scoring", SCORINGS, ids=_sid)
def test_stage_probe_equals_the_oracle(scoring, kind):
    cfg = _cfg(scoring)
    oc, om = _oracle_msa(kind, **cfg)
    assert len(om) == len(_probe_input(kind)) and oc
    for env in ENVS:
        gc, gm = _gpu_msa(kind, env, **cfg)
        assert gc == oc, (scoring, kind, env)
        assert gm == om, (scoring, kind, env, [i for i in range(len(om)) if gm[i] != om[i]])


def test_the_probes_depend_on_the_scoring():
    """the oracle's MSA of every probe under every non-default scoring differs from the default's on at least one shape: a kernel
    that ignored the configured scores could not pass test_stage_probe_equals_the_oracle (no GPU work here)"""
    for scoring in SCORINGS[1:]:
        assert any(_oracle_msa(kind, **_cfg(scoring)) != _oracle_msa(kind, **_cfg(SCORINGS[0])) for kind in ("noisy", "ragged", "long")), scoring


# ---- the whole path -----------------------------------------------------------------------------------------------------------

def _zero_recs(seed, n):
    """reads with one splint and two overlapping dangling pieces (as test_gpu_qv._zero_recs): the 2-sequence POA behind k_zero_finish"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        L = int(rng.integers(900, 1600))
        a, b = int(rng.integers(100, L // 3)), int(rng.integers(2 * L // 3, L - 50))
        s, q, st, t = synth.make_zero_read(rng, synth.SPLINT1, L, a, b)
        out.append(("zero%d" % k, s, q, st, t))
    return out


_RECS = {}


def _recs(which):
    if which not in _RECS:
        if which == "mix":
            _RECS[which] = list(synth.generate("cfg1", n_reads=24)) + list(synth.generate("cfg2", n_reads=32)) + _zero_recs(5, 8)
        else:
            _RECS[which] = list(synth.generate("cfg1", n_reads=24))
    return _RECS[which]


def _oracle_batch(recs, **cfg):
    return O.process_batch(synth.SPLINT1, [(r[1], r[2]) for r in recs], [r[3] for r in recs], params=O.default_params(**cfg), threads=8)


def _gpu_batch(recs, env, **cfg):
    with _env(env):
        h = _lib.Handle(**cfg)
        try:
            h.set_splints([synth.SPLINT1])
            h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
            h.run()
            res, cons = h.results()
            return res, cons, h.timing()
        finally:
            h.close()


def _same_reads(res, cons, ores, ocons, what):
    for i in range(len(ocons)):
        assert res[i]["status"] == ores[i].status and cons[i] == ocons[i], what + (i,)


@pytest.mark.parametrize("scoring", [SCORINGS[1], SCORINGS[2], SCORINGS[6], SCORINGS[4], SCORINGS[8]], ids=_sid)
def test_whole_path_equals_the_oracle_and_the_16_bit_instances_do_the_work(scoring):
    """status and consensus read for read, the counted POA cells (the same bands, row for row), and fewer than half of the reads
    with at least two subreads handed to the 32-bit pass (a read whose stored score leaves the 16-bit range is legitimately
    redone there; the counts are printed, -s, and listed in DESIGN.md 3)"""
    recs, cfg = _recs("mix"), _cfg(scoring)
    ores, ocons = _oracle_batch(recs, **cfg)
    cells = sum(int(r.cells_poa) for r in ores)
    multi = sum(1 for r in ores if r.n_sub >= 2)
    assert multi >= 40 and any(r.n_sub == 0 and c for r, c in zip(ores, ocons))          # ... and rescued zero-repeat reads
    for env in ENVS:
        res, cons, t = _gpu_batch(recs, env, **cfg)
        _same_reads(res, cons, ores, ocons, (scoring, env))
        assert t["cells_poa"] == cells, (scoring, env)
        print("scoring %s %s: n_poa_redo16 = %d of %d reads with >= 2 subreads" % (_sid(scoring), env, t["n_poa_redo16"], multi))
        if "C3_DEBUG_POA32" not in env:
            assert 2 * t["n_poa_redo16"] < multi, (scoring, env, t["n_poa_redo16"], multi)


def test_band_b_and_band_f_moved_together():
    """poa_band_b = 4, poa_band_f = 0.03 (w = 4 + 3 % of the subread instead of 10 + 1 %): the band rule with both terms away from
    the default and from (w, 0)"""
    recs, cfg = _recs("cfg1"), dict(poa_band_b=4, poa_band_f=0.03)
    ores, ocons = _oracle_batch(recs, **cfg)
    dres, _dcons = _oracle_batch(recs)
    cells = sum(int(r.cells_poa) for r in ores)
    assert cells != sum(int(r.cells_poa) for r in dres)                                   # other bands than the default's
    for env in ({}, {"C3_DEBUG_POA_RBSPAN": "3300"}):
        res, cons, t = _gpu_batch(recs, env, **cfg)
        _same_reads(res, cons, ores, ocons, (env,))
        assert t["cells_poa"] == cells and t["n_poa_redo16"] == 0, (env, t["n_poa_redo16"])


# ---- the shim -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [{}, {"match": 5}], ids=["bare", "match5"])
def test_msa_aligner_shim(kw):
    """msa_aligner() defaults to match = 2 as pyabpoa does; the reference's call site passes match = 5"""
    seqs = _probe_input("noisy")
    cfg = dict(poa_match=kw.get("match", 2))
    oc, om = _oracle_msa("noisy", **cfg)
    r = shims.msa_aligner(**kw).msa(seqs, True, True)
    assert r.cons_seq == oc and r.msa_seq == om and r.n_seq == len(seqs)
    assert _oracle_msa("noisy", poa_match=2) != _oracle_msa("noisy", poa_match=5)


# ---- the ends of the admitted ranges (c3_create; the refusals need no GPU: tests/test_cabi.py) ---------------------------------------

RANGES = {"poa_match": (1, 64), "poa_mismatch": (0, 64), "poa_o1": (0, 64), "poa_e1": (0, 16), "poa_o2": (0, 64), "poa_e2": (0, 16)}
EDGES = [{k: v} for k, (lo, hi) in RANGES.items() for v in (lo, hi)] + [
    {k: lo for k, (lo, hi) in RANGES.items()},               # every field at its lower end
    {k: hi for k, (lo, hi) in RANGES.items()},               # ... at its upper end
    dict(poa_match=3, poa_mismatch=5, poa_o1=30, poa_e1=1, poa_o2=6, poa_e2=3),      # the pieces of (3,5,6,3,30,1) swapped: o2 < o1 is admitted
]


@pytest.mark.parametrize("cfg", EDGES, ids=lambda c: ",".join("%s=%d" % (k[4:], v) for k, v in c.items()))
def test_last_accepted_value_of_every_field_equals_the_oracle(cfg):
    """on the 4 x 300 probe and on its ragged sibling: the long gaps of the second are what the second gap piece decides"""
    kinds = ("noisy", "ragged")
    assert any(_oracle_msa(k, **cfg) != _oracle_msa(k) for k in kinds), "the probe does not depend on this value"
    for kind in kinds:
        oc, om = _oracle_msa(kind, **cfg)
        for env in ({}, {"C3_DEBUG_POA_RBSPAN": "3300"}, {"C3_DEBUG_POA32": "1"}):
            gc, gm = _gpu_msa(kind, env, **cfg)
            assert gc == oc and gm == om, (cfg, kind, env)


@pytest.mark.parametrize("scoring", [SCORINGS[8], (24, 24, 24, 6, 64, 3), (32, 32, 32, 8, 64, 4), (64, 64, 64, 16, 64, 16)], ids=_sid)
def test_scores_that_leave_the_16_bit_range_are_handed_over_not_lost(scoring):
    """6 kb inserts (bands of 140-250 columns: the WIDE ring) under the large scoring, two scorings between it and the upper end
    of every range, and that upper end.  The oracle finds reachable cells 1 905 / 3 052 / 4 048 / 8 864 units below their row's
    maximum on these reads (c3o_poa_rowstats).  The 16-bit cells hold 2 296 units below the row's base, which sits up to 3 000
    below the row maximum and up to 400 above it: the first three fit or not with where the base stands when the deep cells occur
    (a row that moves its base up keeps only 2 296 below its maximum: DESIGN.md 4.3, R5; the counts are printed), the last one cannot fit
    (8 864 > 5 296) and MUST reach the 32-bit pass through the guard.  Every one of them ends with the oracle's result and cells"""
    shape = dict(reads=4, seed=66, insert=6000, n_lo=3, n_hi=3, k0=108, k1=108, mdist=500)
    recs, cfg = list(synth.generate(shape, n_reads=4)), _cfg(scoring)
    ores, ocons = _oracle_batch(recs, **cfg)
    assert all(r.status == 0 and r.n_sub >= 3 for r in ores)
    cells = sum(int(r.cells_poa) for r in ores)
    for env in ({}, {"C3_DEBUG_POA_RBSPAN": "3300"}, {"C3_DEBUG_POA32": "1"}):
        res, cons, t = _gpu_batch(recs, env, **cfg)
        _same_reads(res, cons, ores, ocons, (scoring, env))
        assert t["cells_poa"] == cells, (scoring, env)
        print("scoring %s %s, 6 kb inserts: n_poa_redo16 = %d of %d reads" % (_sid(scoring), env, t["n_poa_redo16"], len(recs)))
        if "C3_DEBUG_POA32" in env:
            assert t["n_poa_redo16"] == 0
        elif scoring[0] == 64:
            assert t["n_poa_redo16"] >= 1, (scoring, env)


# ---- pol_q --------------------------------------------------------------------------------------------------------------------

def _requalified(recs):
    """the cfg1 reads with constant qualities per piece: subread k at Phred 10 / 20 / 30 / 61 (k mod 4), the front piece at 61,
    the tail piece at 20.  A layer's mean quality over any window segment is then exactly its piece's Phred, so the polish's layer
    filter (qsum < pol_q * seglen drops the layer) has layers on both sides of pol_q = 20 and 60, and layers whose mean is
    EXACTLY 20, which are kept.  (The split does not read the qualities: the boundaries are the oracle's.)"""
    ores, _ = _oracle_batch(recs)
    out = []
    for r, o in zip(recs, ores):
        q = bytearray(chr(33 + 20).encode() * len(r[2]))
        if o.has_front:
            q[:o.front_end] = chr(33 + 61).encode() * o.front_end
        for k in range(o.n_sub):
            b, e = o.sub_beg[k], o.sub_end[k]
            q[b:e] = chr(33 + (10, 20, 30, 61)[k % 4]).encode() * (e - b)
        out.append((r[0], r[1], q.decode(), r[3], r[4]))
    assert any(o.n_sub >= 3 and o.has_front and o.has_tail for o in ores)
    return out


def test_pol_q_layer_filter():
    recs = _requalified(_recs("cfg1"))
    seen = {}
    for pol_q in (0, 20, 60):
        ores, ocons = _oracle_batch(recs, pol_q=pol_q)
        res, cons, t = _gpu_batch(recs, {}, pol_q=pol_q)
        _same_reads(res, cons, ores, ocons, (pol_q,))
        seen[pol_q] = sum(int(r.cells_polish) for r in ores)
        assert t["cells_polish"] == seen[pol_q], pol_q
    # layers fall on both sides: every step of pol_q drops layers (fewer polish cells), and at 20 the Phred-20 layers are still
    # there (dropping them as well -- a `<=` in place of `<` -- is what pol_q = 21 computes)
    assert seen[0] > seen[20] > seen[60]
    assert sum(int(r.cells_polish) for r in _oracle_batch(recs, pol_q=21)[0]) < seen[20]

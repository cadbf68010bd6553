"""The banded rows of k_window (win_rows_band, k_polish_band.h) at the seams of their row loop.  The rows of a layer run in
64-row descriptor blocks, word by word (8 rows per direction word at CB == 2, 4 at CB == 3 / 4); runs of fast rows of one band
shift are loops of their own, the general row stands between them; every 32 rows the parked band-edge cells become the
certificate bound and the edge-park offset wraps; a layer that does not fit its scratch returns -1 before its first row.
Every case goes through the pre-split determine_consensus probe and must equal the oracle (full matrix) in consensus, draft and
counted cells, in every mode below; one batch of concatemers goes through the whole pipeline and must equal it in status too.

Cases (each asserts on the oracle's window capture the shape it exists for):
  rows31 .. rows65, rows45   a last window of N backbone positions whose third layer is a query of 129 bases (an insertion of
            129 - N): R = N rows, Q = 129 -- the smallest query a band of 128 columns takes.  N = 31, 32, 33 (the edge-park wrap
            and the certificate every 32 rows), 63, 64, 65 (the descriptor block), 45 (the last, partial direction word)
  shorter / longer   subread 1 has 40 bases fewer / more than the backbone, spread evenly: band shifts 0 and 1 alternate, starting
            with the rows where the band still stands at column 0
  noisy6    six noisy copies: branches and joins between the fast rows -- a general row right before and right after a fast row,
            and fast rows with the `wr` bit (a later row other than the fast row below reads them from the ring)
  AC300     six noisy copies of (AC) x 300: layers in which more than a third of the rows are general rows (a layer of general
            rows ONLY cannot be built: the row below a row with one successor is a fast row by definition)
  noisy12   twelve noisy copies: later layers see R * 4 >= span * 5 and start at CB == 3
  scoring   noisy6 under the polish scoring (3, 4, -4)
  drift_hept_+8, runlen_hp_blocks_d15_n6   two families of tests/low_complexity_cases.py whose copies differ by whole repeat units or
            runs.  In the runlen family NO certificate holds: every layer is tried at every width from its first up to CB == 4
            and then redone unbanded, so the failed attempts the device counts must be the number of (layer, CB) pairs the
            capture gives -- 13, of which only 2 are at CB == 2
Modes: default; verify (C3_DEBUG_BAND=verify: every accepted band layer is aligned again with the full matrix on the device,
n_band_mismatch must stay 0); poison (C3_DEBUG_POISON=1); fail (C3_DEBUG_BAND=fail: every certificate counts as failed
and the layer is redone unbanded; the retries at CB 3 and 4 belong to the default mode alone, see the two families above; under
verify only the layers of noisy12 that START at CB == 3 run a wider instance); hcap (C3_DEBUG_HCAP_DIV: the first launch's scratch holds no layer,
the rows return -1 and the window is redone by the second launch).

Not covered: the exit INSIDE the row loop (a row with more than 64 predecessor rows: a read would need more than 64 subreads
branching at one backbone position) is checked by reading only; the hcap mode's -1 is returned before the first row.  The probe
has no status: per case consensus, draft and cells are compared, status in the batch at the end.  The expected layer counts come
from tests/test_band_certificate_model.py's restatement of the band rules under the default scoring."""
import collections
import os

import numpy as np
import pytest

from c3poa_amd import synth
from c3poa_amd.seqio import revcomp

import low_complexity_cases as LC
import test_band_certificate_model as M

pytestmark = pytest.mark.gpu

_HOOKS = ("C3_DEBUG_POISON", "C3_DEBUG_BAND", "C3_DEBUG_HCAP_DIV", "C3_DEBUG_WIN_CHAIN", "C3_DEBUG_WIN_LCAP", "C3_DEBUG_WIN_LDS")
MODES = collections.OrderedDict([
    ("default", {}),
    ("verify", {"C3_DEBUG_BAND": "verify"}),
    ("poison", {"C3_DEBUG_POISON": "1"}),
    ("fail", {"C3_DEBUG_BAND": "fail"}),
    ("hcap", {"C3_DEBUG_HCAP_DIV": "100000"}),
])
SEAM_ROWS = (31, 32, 33, 63, 64, 65, 45)
SCORING = (3, 4, -4)            # tests/test_gpu_pol_scoring.py: test_band_certificate_under_other_scorings
_COUNTERS = ("cells_poa", "cells_polish", "cells_polish_computed", "n_band_layers", "n_band_fallback", "n_band_mismatch", "n_windows",
             "n_win_redo")
Case = collections.namedtuple("Case", "name subs quals cfg")
_cache = {}


def _spread(rng, ins, n, insert):
    """ins with n single bases inserted (or deleted) at evenly spread places"""
    out, step = [], len(ins) // (n + 1)
    for k in range(n + 1):
        part = ins[k * step:(k + 1) * step] if k < n else ins[n * step:]
        out.append(part)
        if k < n:
            if insert:
                out.append(LC._acgt(rng, 1))
            else:
                out[-1] = part[:-1]
    return "".join(out)


def _cases():
    if "cases" in _cache:
        return _cache["cases"]
    cases = []

    def add(name, subs, quals=None, cfg=None):
        cases.append(Case(name, tuple(subs), tuple(quals or ["I" * len(s) for s in subs]), dict(cfg or {})))

    rng = np.random.default_rng(20280)
    for n in SEAM_ROWS:
        ins = LC._acgt(rng, 500 + n)
        at = 500 + n // 2
        alt = ins[:at] + LC._acgt(rng, 129 - n) + ins[at:]
        add("rows%d" % n, [ins, ins, alt, ins])
    ins = LC._acgt(rng, 500)
    add("shorter", [ins, _spread(rng, ins, 40, False), ins])
    add("longer", [ins, _spread(rng, ins, 40, True), ins])
    ins = LC._acgt(rng, 600)
    noisy6 = LC._family(rng, ins, 6)
    add("noisy6", *noisy6)
    add("AC300", *LC._family(rng, "AC" * 300, 6))
    add("noisy12", *LC._family(rng, LC._acgt(rng, 520), 12))
    add("scoring", *noisy6, cfg=dict(pol_match=SCORING[0], pol_mismatch=SCORING[1], pol_gap=SCORING[2]))
    for c in LC.CASES:
        if c.name in ("drift_hept_+8", "runlen_hp_blocks_d15_n6"):
            add(c.name, c.subs, c.quals)
    _cache["cases"] = tuple(cases)
    return _cache["cases"]


def _reference():
    """per case: the oracle's (consensus, draft, (cells_poa, cells_polish)) and its window capture, computed once"""
    from oracle import oracle_py as O
    if "ref" not in _cache:
        out = []
        for c in _cases():
            O.win_capture(True)
            try:
                r = O.determine_consensus(c.subs, c.quals, None, None, params=O.default_params(**c.cfg), return_draft=True)
                als = O.win_captured()
            finally:
                O.win_capture(False)
            for a in als:
                a["R"] = int(np.count_nonzero(a["mask"]))
            out.append((r, als))
        _cache["ref"] = tuple(out)
    return _cache["ref"]


class _hooks:
    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in _HOOKS}
        for k in _HOOKS:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(mode):
    """every case under one mode, one handle per scoring: [(consensus, draft, counters)], computed once"""
    from c3poa_amd import _lib
    if ("run", mode) not in _cache:
        handles, out = {}, []
        with _hooks(MODES[mode]):
            try:
                for c in _cases():
                    key = tuple(sorted(c.cfg.items()))
                    if key not in handles:
                        handles[key] = _lib.Handle(**c.cfg)
                    h = handles[key]
                    cons, draft = h.determine_consensus(list(c.subs), list(c.quals), None, None, return_draft=True)
                    t = h.timing()
                    out.append((cons, draft, {k: int(t[k]) for k in _COUNTERS}))
            finally:
                for h in handles.values():
                    h.close()
        _cache[("run", mode)] = out
    return _cache[("run", mode)]


def _widths(a):
    """the band widths the kernel tries for the layer, in order, when every certificate fails (win_rows_dispatch)"""
    rows, _rowof, _preds = M._rows(a)
    out, cb_min = [], 0
    while True:
        bd = M._band(a, rows, cb_min)
        if bd is None:
            return out
        out.append(bd[0]); cb_min = bd[0] + 1


def _model_accepts(a):
    """the certificate of the layer's first band width holds, by the model of tests/test_band_certificate_model.py"""
    rows, _rowof, preds = M._rows(a)
    cb, bw, lo = M._band(a, rows, 0)
    H, D, succ = M._band_dp(a, rows, preds, lo, bw)
    _ops, sb = M._trace(a, rows, succ, H, D)
    bound = M._certificate(a, rows, preds, succ, H, lo, bw, cb)
    return bound is not None and sb > M.NEG // 2 and bound < sb


def _kinds(a):
    """(fast[r], wr[r], R) of the layer's rows as win_build_desc_band classifies them, None when the layer takes no band"""
    rows, _rowof, preds = M._rows(a)
    bd = M._band(a, rows, 0)
    if bd is None:
        return None
    lo, R = bd[2], len(rows) - 1
    succ = [[] for _ in range(R + 2)]
    for r in range(1, R + 1):
        for p in preds[r]:
            succ[p].append(r)
    fast = [False] * (R + 2)
    for r in range(2, R + 1):
        fast[r] = preds[r] == [r - 1] and bool(succ[r]) and max(x - r for x in succ[r]) <= 4 and lo[r] - lo[r - 1] <= 1
    wr = [any(x != r + 1 for x in succ[r]) or ((r + 1) in succ[r] and not fast[r + 1]) for r in range(R + 1)]
    return fast, wr, R


def _expected_layers(name):
    """band-eligible layers of a case (default scoring)"""
    ref = dict(zip((c.name for c in _cases()), _reference()))
    return sum(bool(_widths(a)) for a in ref[name][1])


def test_the_cases_have_the_shapes_they_exist_for():
    ref = dict(zip((c.name for c in _cases()), _reference()))
    for n in SEAM_ROWS:
        _r, als = ref["rows%d" % n]
        hit = [a for a in als if a["R"] == n and a["Q"] == 129 and _widths(a)[:1] == [2]]
        assert len(hit) == 1, (n, [(a["R"], a["Q"]) for a in als])
        assert _model_accepts(hit[0]), n                                  # the layer is accepted, not redone unbanded
        assert _expected_layers("rows%d" % n) == 5, n                     # the four layers of window 0 and this one
    assert 45 % 8 and 45 % 4
    for name, sign in (("shorter", -1), ("longer", 1)):
        _r, als = ref[name]
        a = [a for a in als if a["layer"] == 1][0]
        span = a["end"] - a["begin"] + 1
        assert a["R"] == span and _widths(a)[:1] == [2] and (a["Q"] - span) * sign >= 30, (name, a["R"], a["Q"], span)
        lo = M._band(a, M._rows(a)[0], 0)[2]
        d = [int(lo[r] - lo[r - 1]) for r in range(1, a["R"] + 1)]
        # (the longer query also has rows of shift 2: general rows between the runs)
        assert set(d) <= {0, 1, 2} and d[0] == 0 and min(d.count(0), d.count(1)) >= 30, (name, d.count(0), d.count(1), d.count(2))
    for name in ("noisy6", "AC300"):
        _r, als = ref[name]
        k = [x for x in (_kinds(a) for a in als) if x]
        fw = sum(sum(1 for r in range(1, R + 1) if fast[r] and wr[r]) for fast, wr, R in k)
        gf = sum(sum(1 for r in range(1, R) if not fast[r] and fast[r + 1]) for fast, wr, R in k)
        fg = sum(sum(1 for r in range(1, R) if fast[r] and not fast[r + 1]) for fast, wr, R in k)
        assert min(fw, gf, fg) >= 100, (name, fw, gf, fg)
        if name == "AC300":
            assert max(sum(1 for r in range(1, R + 1) if not fast[r]) / R for fast, wr, R in k) > 1 / 3
    _r, als = ref["noisy12"]
    infl = [a for a in als if a["R"] * 4 >= (a["end"] - a["begin"] + 1) * 5 and _widths(a)[:1] in ([3], [4])]
    assert len(infl) >= 2, [(a["R"], a["end"] - a["begin"] + 1, a["Q"]) for a in als]
    w = [x for x in (_widths(a) for a in ref["runlen_hp_blocks_d15_n6"][1]) if x]
    assert sum(len(x) for x in w) == 13 and sum(x[:1] == [2] for x in w) == 2 and all(x[-1] == 4 for x in w), w


@pytest.mark.parametrize("mode", list(MODES))
def test_band_rows_equal_the_oracle(mode):
    got = _run(mode)
    for c, (cons, draft, t), ((wcons, wdraft, wcells), _als) in zip(_cases(), got, _reference()):
        assert draft == wdraft, (mode, c.name, len(draft), len(wdraft))
        assert cons == wcons, (mode, c.name, len(cons), len(wcons))
        assert t["cells_poa"] == wcells[0] and t["cells_polish"] == wcells[1], (mode, c.name, t, wcells)
        assert t["n_band_mismatch"] == 0, (mode, c.name, t)
        if mode in ("default", "verify", "poison", "hcap"):
            # (the two families of failed certificates may have no accepted layer at all: there the attempts count)
            assert t["n_band_layers"] + (t["n_band_fallback"] if c.name.startswith(("drift", "runlen")) else 0) > 0, (mode, c.name, t)
        if mode == "fail":
            assert t["n_band_layers"] == 0 and t["n_band_fallback"] > 0, (c.name, t)
        if mode == "default" and c.name.startswith(("drift", "runlen")):
            assert t["n_band_fallback"] > 0, (c.name, t)                  # failed certificates: retried at CB 3 and 4
        if mode in ("default", "poison", "hcap") and c.name == "runlen_hp_blocks_d15_n6":
            assert (t["n_band_layers"], t["n_band_fallback"]) == (0, 13), (mode, t)      # every width up to CB == 4 ran and failed
        if mode in ("default", "verify", "poison", "hcap") and c.name.startswith("rows"):
            # every eligible layer is accepted at its first width, the R = N layer among them
            assert (t["n_band_layers"], t["n_band_fallback"]) == (_expected_layers(c.name), 0), (mode, c.name, t)
        if mode == "hcap":
            assert t["n_win_redo"] > 0, (c.name, t)
    if mode != "default":
        for c, a, b in zip(_cases(), got, _run("default")):
            assert a[:2] == b[:2], (mode, c.name)
            # (fail and verify do not retry a failed certificate with a wider band, and verify fills every accepted layer's full
            # matrix as well: their layers and computed cells are not the default's)
            if mode in ("poison", "hcap"):
                for k in ("cells_polish_computed", "n_band_layers", "n_band_fallback"):
                    assert a[2][k] == b[2][k], (mode, c.name, k, a[2][k], b[2][k])


@pytest.mark.parametrize("mode", ["default", "verify"])
def test_one_batch_through_the_whole_pipeline(mode):
    """six concatemers of the inserts above, every third reverse-complemented: status, subreads, consensus and cells"""
    from c3poa_amd import _lib
    from oracle import oracle_py as O
    if "batch" not in _cache:
        rng = np.random.default_rng(20281)
        reads, strands = [], []
        for k, ins in enumerate((LC._acgt(rng, 531), LC._acgt(rng, 564), LC._acgt(rng, 565), "AC" * 300, LC._acgt(rng, 545), LC._acgt(rng, 1033))):
            s, q = LC.concatemer(rng, synth.SPLINT1, ins, 3 + k % 3, 150, 150)
            if k % 3 == 2:
                s, q, st = revcomp(s), q[::-1], "-"
            else:
                st = "+"
            reads.append((s, q)); strands.append(st)
        _cache["batch"] = (reads, strands, O.process_batch(synth.SPLINT1, reads, strands, threads=6))
    reads, strands, (ores, ocons) = _cache["batch"]
    with _hooks(MODES[mode]):
        h = _lib.Handle()
        try:
            h.set_splints([synth.SPLINT1])
            h.upload([r[0] for r in reads], [r[1] for r in reads], list(strands))
            h.run()
            res, cons = h.results()
            t = h.timing()
        finally:
            h.close()
    for i in range(len(reads)):
        assert res[i]["status"] == ores[i].status, (i, int(res[i]["status"]), ores[i].status)
        assert res[i]["n_sub"] == ores[i].n_sub, i
        assert cons[i] == ocons[i], i
    assert sum(o.status == 0 for o in ores) >= 5
    assert t["cells_polish"] == sum(int(r.cells_polish) for r in ores)
    assert t["n_band_layers"] > 0 and t["n_band_mismatch"] == 0

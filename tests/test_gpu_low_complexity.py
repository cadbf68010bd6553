"""k_poa, k_poa_pair, k_prep and k_window on homopolymers, tandem repeats and poly-A tails (tests/low_complexity_cases.py; that
the set holds the ties it exists for: tests/test_low_complexity_host.py).  The oracle states the tie rules and is the
specification: the first predecessor wins, M >= E1 >= E2, ht >= F1 >= F2, the last tied column is `right`, the lower quality
or sum goes to row B.  Every shape goes through the pre-split determine_consensus probe and the device's consensus, draft and
counted cells of both alignment stages must equal the oracle's bit for bit, in every mode below.  All runs poison fresh device
memory (C3_DEBUG_POISON) and use ONE handle per mode (and window length) for all shapes, one after the other: stale flags, a
stale vq, reused slots.

POA modes: default, the pair kernel off, the 32-bit instance, the WIDE instance forced on and off, a 16-bit base that moves every
few rows, no two-column rows, and first-pass slots of 64 nodes (every read is redone by the second pass).
Polish modes: default, the band off / every certificate failed / every accepted band layer verified on the device, the general
graph phases for first layers, the masked extension rows of k_prep, a first launch without DP scratch, the consensus sweep in
global scratch.
One batch of 24 concatemers of such inserts runs through the whole pipeline, default and with the band verified.

Band fallback share n_band_fallback / (n_band_layers + n_band_fallback) of the default mode, measured on an MI355X per family
group as failed attempts / (accepted layers + failed attempts); no cap is asserted, and two groups lie far above the 5 %
tests/test_gpu_band.py allows random inserts:
  tracts 0.9 % (2 / 225), noflank 0 % (0 / 69), runlen 81.6 % (31 / 38), drift 52.3 % (23 / 44), seam 3.5 % (6 / 171),
  equalq 0 % (0 / 7), dangling 7.7 % (1 / 13), control 0 % (0 / 3); all shapes 11.1 % (63 / 570).
Where copies differ by whole runs or repeat units the certificate fails on most layers and they are redone with wider bands or
the full matrix: results and counted cells still equal the oracle's, cells_polish_computed rises to 1.9 x cells_polish there."""
import collections
import os

import numpy as np
import pytest

from c3poa_amd import synth

import low_complexity_cases as LC
import test_gpu_poa_pair as PP

pytestmark = pytest.mark.gpu

_HOOKS = ("C3_DEBUG_POISON", "C3_DEBUG_POA_PAIR", "C3_DEBUG_POA32", "C3_DEBUG_POA_WIDE", "C3_DEBUG_POA_RBSPAN", "C3_DEBUG_POA_NO2COL",
          "C3_DEBUG_POA_SMALL", "C3_DEBUG_BAND", "C3_DEBUG_WIN_CHAIN", "C3_DEBUG_PREP_ROWS", "C3_DEBUG_HCAP_DIV", "C3_DEBUG_WIN_LCAP",
          "C3_DEBUG_WIN_LDS", "C3_DEBUG_PREP_WPC")
POA_MODES = collections.OrderedDict([
    ("default", {}),
    ("pair_off", {"C3_DEBUG_POA_PAIR": "0"}),
    ("poa32", {"C3_DEBUG_POA32": "1"}),
    ("wide_on", {"C3_DEBUG_POA_WIDE": "1"}),
    ("wide_off", {"C3_DEBUG_POA_WIDE": "0"}),
    ("rbspan", {"C3_DEBUG_POA_RBSPAN": "3300"}),
    ("no2col", {"C3_DEBUG_POA_NO2COL": "1"}),
    ("small64", {"C3_DEBUG_POA_SMALL": "64"}),
])
POL_MODES = collections.OrderedDict([
    ("default", {}),
    ("band_off", {"C3_DEBUG_BAND": "off"}),
    ("band_fail", {"C3_DEBUG_BAND": "fail"}),
    ("band_verify", {"C3_DEBUG_BAND": "verify"}),
    ("chain_off", {"C3_DEBUG_WIN_CHAIN": "0"}),
    ("prep_old", {"C3_DEBUG_PREP_ROWS": "old"}),
    ("hcap", {"C3_DEBUG_HCAP_DIV": "100000"}),
    ("lcap64", {"C3_DEBUG_WIN_LCAP": "64"}),
])
_COUNTERS = ("cells_poa", "cells_polish", "cells_polish_computed", "n_poa_redo", "n_poa_redo16", "n_pair", "n_pair_declined",
             "n_band_layers", "n_band_fallback", "n_band_mismatch", "n_windows", "n_win_redo")
_cache = {}


class _hooks:
    """the test hooks of one mode, and nothing else, in the environment"""

    def __init__(self, env):
        self.env = dict(env, C3_DEBUG_POISON="1")

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
    """every shape of the set under one mode, on one handle per window length: [(consensus, draft, counters)], computed once"""
    from c3poa_amd import _lib
    if mode not in _cache:
        env = POA_MODES[mode] if mode in POA_MODES else POL_MODES[mode]
        handles, out = {}, []
        with _hooks(env):
            try:
                for c in LC.CASES:
                    key = tuple(sorted(c.cfg.items()))
                    if key not in handles:
                        handles[key] = _lib.Handle(**c.cfg)
                    h = handles[key]
                    cons, draft = h.determine_consensus(list(c.subs), list(c.quals), c.front, c.tail, return_draft=True)
                    t = h.timing()
                    out.append((cons, draft, {k: int(t[k]) for k in _COUNTERS}))
            finally:
                for h in handles.values():
                    h.close()
        _cache[mode] = out
    return _cache[mode]


def _facts():
    """oracle side, per shape: what tests/test_gpu_poa_pair._rows reads of the alignment of subread 1 against subread 0"""
    if "facts" not in _cache:
        _cache["facts"] = [PP._rows(c.subs[0], c.subs[1]) for c in LC.CASES]
    return _cache["facts"]


def _equals_oracle(mode):
    got = _run(mode)
    for c, (cons, draft, t), (wcons, wdraft, wcells) in zip(LC.CASES, got, LC.reference()):
        assert draft == wdraft, (mode, c.name, len(draft), len(wdraft))
        assert cons == wcons, (mode, c.name, len(cons), len(wcons))
        assert t["cells_poa"] == wcells[0], (mode, c.name, t["cells_poa"], wcells[0])
        assert t["cells_polish"] == wcells[1], (mode, c.name, t["cells_polish"], wcells[1])
    return got


def _sum(run, key, group=None):
    return sum(t[key] for c, (_, _, t) in zip(LC.CASES, run) if group is None or c.group == group)


def fallback_shares(run):
    """group -> (share, n_band_layers, n_band_fallback) of one run"""
    out = collections.OrderedDict()
    for g in LC.GROUPS:
        lay, fb = _sum(run, "n_band_layers", g), _sum(run, "n_band_fallback", g)
        out[g] = (round(fb / max(lay + fb, 1), 4), lay, fb)
    return out


@pytest.mark.parametrize("mode", list(POA_MODES))
def test_poa_modes(mode):
    got = _equals_oracle(mode)
    if mode == "default":
        facts = _facts()
        for c, (_, _, t), f in zip(LC.CASES, got, facts):
            assert t["n_pair"] + t["n_pair_declined"] == 1, (c.name, t["n_pair"], t["n_pair_declined"])
            assert t["n_pair"] == (1 if f["can"] else 0), (c.name, f, t["n_pair"])
        assert _sum(got, "n_pair") > 0
        # reads the pair kernel takes that have rows of 65 - 128 columns: the copy-number drift
        wide = [c.name for c, (_, _, t), f in zip(LC.CASES, got, facts) if t["n_pair"] == 1 and f["wide"] > 0 and c.group == "drift"]
        assert len(wide) == 6, wide
    elif mode == "pair_off":
        for c, a, b in zip(LC.CASES, got, _run("default")):
            assert a[2]["n_pair"] == 0 and a[2]["n_pair_declined"] == 0, c.name
            assert a[:2] == b[:2], c.name
            for k in _COUNTERS:
                if k not in ("n_pair", "n_pair_declined"):
                    assert a[2][k] == b[2][k], (c.name, k, a[2][k], b[2][k])
    elif mode == "small64":
        for c, (_, _, t) in zip(LC.CASES, got):
            assert t["n_poa_redo"] == 1, (c.name, t["n_poa_redo"])                # 64 nodes hold none of these graphs


@pytest.mark.parametrize("mode", list(POL_MODES))
def test_polish_modes(mode):
    got = _equals_oracle(mode)
    for c, (_, _, t) in zip(LC.CASES, got):
        assert t["n_band_mismatch"] == 0, (mode, c.name, t["n_band_mismatch"])
        if mode == "band_off":
            assert t["n_band_layers"] == 0 and t["n_band_fallback"] == 0 and t["cells_polish_computed"] == t["cells_polish"], (c.name, t)
        if mode == "band_fail":
            assert t["n_band_layers"] == 0, (c.name, t)
    shares = fallback_shares(got)
    if mode in ("default", "band_verify"):
        assert _sum(got, "n_band_layers") > 0, shares                               # otherwise verify checks nothing
        print("band fallback share per group (%s): %s" % (mode, dict(shares)))
    if mode == "band_fail":
        assert _sum(got, "n_band_fallback") >= _sum(_run("default"), "n_band_layers") > 0, shares
    if mode == "hcap":
        assert _sum(got, "n_win_redo") >= 0.9 * _sum(got, "n_windows") > 0
        for c, a, b in zip(LC.CASES, got, _run("default")):
            for k in ("cells_polish_computed", "n_band_layers", "n_band_fallback"):
                assert a[2][k] == b[2][k], (c.name, k, a[2][k], b[2][k])
    if mode == "chain_off":
        for c, a, b in zip(LC.CASES, got, _run("default")):
            for k in ("cells_polish_computed", "n_band_layers", "n_band_fallback"):
                assert a[2][k] == b[2][k], (c.name, k, a[2][k], b[2][k])


@pytest.mark.parametrize("mode", ["default", "band_verify"])
def test_one_batch_through_the_whole_pipeline(mode):
    """24 tie-heavy reads side by side: many slots, the work lists, the cost-sorted queue; compared as
    tests/test_gpu_parity.test_full_batch_exact compares"""
    from c3poa_amd import _lib
    reads, strands = LC.BATCH
    ores, ocons = LC.batch_reference()
    with _hooks(POL_MODES[mode]):
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
        assert ores[i].status == 0 and res[i]["status"] == 0, (i, int(res[i]["status"]), ores[i].status)
        assert res[i]["n_sub"] == ores[i].n_sub, (i, int(res[i]["n_sub"]), ores[i].n_sub)
        assert res[i]["peaks"][:res[i]["n_peaks"]].tolist() == list(ores[i].peaks[:ores[i].n_peaks]), i
        assert cons[i] == ocons[i], i
    assert t["cells_poa"] == sum(int(r.cells_poa) for r in ores)
    assert t["cells_polish"] == sum(int(r.cells_polish) for r in ores)
    assert t["n_band_layers"] > 0 and t["n_band_mismatch"] == 0
    assert t["n_pair"] + t["n_pair_declined"] == len(reads) and t["n_pair"] > 0
    assert np.array_equal(res["cons_len"], [r.cons_len for r in ores])

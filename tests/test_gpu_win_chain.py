"""k_window's chain phases: the first layer aligned in a window meets the pristine backbone chain, so its sub-graph mask,
compaction, row descriptors (banded and unbanded), fusion, edge pass and reorder are closed-form (no graph look-ups).  The
default run must equal the run that sends first layers through the general phases (test hook C3_DEBUG_WIN_CHAIN=0), and both
must equal the CPU oracle, bit for bit: statuses, subread counts, consensus lengths and bytes, window counts, the counted
cells of both alignment stages, the cells actually computed and the band counters.  Every case states the shape it exists for
as an assertion on the oracle's window capture, so a change of the read generator cannot hollow it out.  Both GPU runs poison
fresh device memory (C3_DEBUG_POISON): an array the chain phases forgot to write does not read as zero."""
import os

import numpy as np
import pytest

from c3poa_amd import synth

pytestmark = pytest.mark.gpu

W_QCAP = 704                    # layers of more bases keep their row / node arrays in global memory
# inserts whose drafts (insert + splint, give or take the consensus errors) end in a last window of about 20 .. 480 bases
INSERTS = (722, 731, 741, 756, 766, 771, 781, 796, 801, 811, 826, 836, 846, 861, 876, 901, 951, 1016, 1116, 1216,
           725, 745, 760, 775, 790, 805, 820, 840)
INS_START = (29, 146, 299)      # cfg2 reads with a first layer whose first base is an insertion
_HOOKS = ("C3_DEBUG_WIN_CHAIN", "C3_DEBUG_POISON", "C3_DEBUG_BAND", "C3_DEBUG_HCAP_DIV")
_TIMING = ("cells_poa", "cells_polish", "cells_polish_computed", "n_band_layers", "n_band_fallback")
_cache = {}


def _batch():
    if "batch" not in _cache:
        reads, strands = [], []
        for k, ins in enumerate(INSERTS):
            s, q, st, _ = synth.make_read(np.random.default_rng([41, k]), synth.SPLINT1, ins, 3, 108, 108)
            reads.append((s, q)); strands.append(st)
        for i in INS_START:
            (_, s, q, st, _), = synth.generate("cfg2", n_reads=1, start=i)
            reads.append((s, q)); strands.append(st)
        # an error-free read with top qualities: every layer matches the backbone base for base
        rng = np.random.default_rng([41, 1000])
        ins = synth._ACGT[rng.integers(0, 4, 930)].tobytes().decode()
        clean = ins[-108:] + (synth.SPLINT1 + ins) * 3 + synth.SPLINT1 + ins[:108]
        reads.append((clean, "I" * len(clean))); strands.append("+")
        _cache["batch"] = (reads, strands)
    return _cache["batch"]


def _oracle(capture=False, **cfg):
    """oracle records, consensi (and the window capture) of the batch under one parameter set, computed once"""
    from oracle import oracle_py as O
    key = ("oracle", capture, tuple(sorted(cfg.items())))
    if key not in _cache:
        reads, strands = _batch()
        if capture:
            O.win_capture(True)
            try:
                ores, ocons = O.process_batch(synth.SPLINT1, reads, strands, params=O.default_params(**cfg), threads=1)
                als = O.win_captured()
            finally:
                O.win_capture(False)
        else:
            ores, ocons = O.process_batch(synth.SPLINT1, reads, strands, params=O.default_params(**cfg), threads=8)
            als = None
        _cache[key] = (ores, ocons, als)
    return _cache[key]


def _gpu_run(chain, cfg, env):
    from c3poa_amd import _lib
    reads, strands = _batch()
    keep = {k: os.environ.get(k) for k in _HOOKS}
    for k in _HOOKS:
        os.environ.pop(k, None)
    os.environ["C3_DEBUG_POISON"] = "1"
    if not chain:
        os.environ["C3_DEBUG_WIN_CHAIN"] = "0"
    os.environ.update(env)
    try:
        h = _lib.Handle(**cfg)
        h.set_splints([synth.SPLINT1])
        h.upload([r[0] for r in reads], [r[1] for r in reads], strands)
        h.run()
        res, cons = h.results()
        t = h.timing()
        h.close()
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return res, cons, t


def _check(env=None, oracle_cells=True, **cfg):
    """chain phases == general phases == oracle.  returns the timing counters of the default run"""
    ores, ocons, _ = _oracle(**cfg)
    new, new_cons, tn = _gpu_run(True, cfg, env or {})
    old, old_cons, to = _gpu_run(False, cfg, env or {})
    for i, o in enumerate(ores):
        for f in ("status", "n_sub", "cons_len", "n_win"):
            assert int(new[i][f]) == int(old[i][f]), (i, f, int(new[i][f]), int(old[i][f]))
        assert new_cons[i] == old_cons[i], i
        assert int(new[i]["status"]) == o.status, (i, int(new[i]["status"]), o.status)
        if o.status == 0:
            for f in ("n_sub", "cons_len"):
                assert int(new[i][f]) == getattr(o, f), (i, f, int(new[i][f]), getattr(o, f))
        assert new_cons[i] == ocons[i], i
    for k in _TIMING:
        assert tn[k] == to[k], (k, tn[k], to[k])
    for k in ("cells_poa", "cells_polish") if oracle_cells else ("cells_poa",):
        want = sum(int(getattr(o, k)) for o in ores)
        assert tn[k] == want, (k, tn[k], want)
    return tn


def _first_layers(als):
    return [a for a in als if a["layer"] == 0]


def test_first_layer_shapes_and_parity():
    """windows of exactly 500; last windows of less than 64, of 64-128 and of more bases that are no multiple of 64; last windows
    under 100 bases (offset 0: a first layer that is NOT full, a range of the chain shorter than the window or all of it) and of
    200 and more (full); first layers that begin with an insertion; a first layer without a single new node"""
    ores, _, als = _oracle(capture=True)
    first = _first_layers(als)
    assert all(a["n"] == a["blen"] for a in first)                        # the first layer always meets the bare backbone
    blens = [a["blen"] for a in first]
    assert blens.count(500) >= 30
    assert sum(b < 64 for b in blens) >= 3 and sum(64 <= b <= 128 for b in blens) >= 3
    assert sum(b > 128 and b % 64 != 0 and b != 500 for b in blens) >= 3
    assert sum(b < 100 for b in blens) >= 5 and sum(100 <= b < 500 for b in blens) >= 5
    assert sum(bool(a["full"]) for a in first) >= 5 and sum(not a["full"] for a in first) >= 5
    assert any(not a["full"] and a["end"] - a["begin"] + 1 < a["blen"] for a in first)     # fewer rows than backbone nodes
    # insertion first: the path's first step carries query base 0 and no node
    assert sum(int(a["ops"][0][1]) == 0 and int(a["ops"][0][0]) < 0 for a in first) >= 3
    # the error-free read (the last one; the capture numbers the windows in read order): its draft is the 1 214-base truth, three
    # windows, and no layer of them adds a node
    assert ores[-1].status == 0 and ores[-1].cons_len == 930 + len(synth.SPLINT1)
    clean = [a for a in als if a["win"] >= als[-1]["win"] - 2]
    assert [a["blen"] for a in clean if a["layer"] == 0] == [500, 500, 214] and len(clean) >= 9
    assert all(a["n"] == a["blen"] for a in clean)
    t = _check()
    assert t["n_band_layers"] > 0


@pytest.mark.parametrize("mode", ["off", "fail", "verify"])
def test_band_modes(mode):
    """off: the unbanded descriptor builder; fail: every attempt of the band fallback loop rebuilds the descriptors, then the
    unbanded rows; verify: band and full matrix of every accepted layer compared on the device"""
    # (verify counts the cells of an accepted layer twice, band and full matrix: there the two runs are compared with each other only)
    t = _check(env={"C3_DEBUG_BAND": mode}, oracle_cells=mode != "verify")
    if mode == "off":
        assert t["n_band_layers"] == 0 and t["n_band_fallback"] == 0
    elif mode == "fail":
        assert t["n_band_layers"] == 0 and t["n_band_fallback"] > 0
    else:
        assert t["n_band_layers"] > 0 and t["n_band_mismatch"] == 0


def test_second_launch():
    """a first launch without DP scratch for any layer (as tests/test_gpu_band.py sets it): every window is redone from its bare
    backbone by the k_window<true> instance"""
    t = _check(env={"C3_DEBUG_HCAP_DIV": "100000"})
    assert t["n_win_redo"] >= 0.9 * t["n_windows"] > 0


def test_layers_beyond_the_lds_query_arrays():
    """pol_window 1000: layers of more than W_QCAP bases keep rq / tq in global memory and take the linear fallback rows, which
    walk the graph themselves"""
    _, _, als = _oracle(capture=True, pol_window=1000)
    first = _first_layers(als)
    assert sum(a["Q"] > W_QCAP and a["n"] == a["blen"] for a in first) >= 20
    assert any(not a["full"] for a in first)
    _check(pol_window=1000)


@pytest.mark.parametrize("match,mismatch,gap", [(2, -5, -4), (7, -9, -6)])
def test_other_polish_scoring(match, mismatch, gap):
    """other substitution bytes and gap steps in the chain descriptors' band start and in the rows they feed"""
    _check(pol_match=match, pol_mismatch=mismatch, pol_gap=gap)

"""The polish stage under window lengths next to the guards the window length decides.  pol_window shapes the polish more than
any other number: run_polish (c3_stages.hip) sizes every capacity from it (wcap, NWcap, Ncap, wout_cap, the DP scratch of both
launches, k_window's dynamic LDS), prep_one (k_polish.hip) cuts the layers with it and drops segments below 2 % of it, k_window
calls a layer "full" by 1 % of the backbone, and win_rows_dispatch picks the row template by the layer's length (cpl 2 / 4 / 6 /
8 / 10 by need = (Q + 64) / 64, linear rows beyond, the band refused below need <= cb, rq / tq in global memory beyond W_QCAP).
c3_create admits 1 .. 18 458 (the ends: tests/test_cabi.py).  Every case runs a window length that puts layers
where one of these decides, first asserts on the oracle's window capture the shape it exists for (with thresholds of about
half of what the generator gives today, so a change of the generator fails loudly instead of hollowing the case out) and then
compares the GPU with the CPU oracle bit for bit: statuses, subread counts, consensus lengths and bytes, window counts and the
counted cells of both alignment stages.  All GPU runs poison fresh device memory (C3_DEBUG_POISON).  That the oracle itself is
the unbanded optimum at window lengths 7, 128 and 2000: tests/test_independent_checkers.py."""
import collections
import os

import numpy as np
import pytest

from c3poa_amd import synth

import test_gpu_win_chain as WC

pytestmark = pytest.mark.gpu

# sixteen reads of test_gpu_win_chain's batch: the first twelve of the insert sweep, the three insertion-first reads, the error-free read
SUBSET = tuple(range(12)) + (28, 29, 30, 31)
W_QCAP = WC.W_QCAP
POL_WINDOW_MAX = 18458          # c3_create: pol_window is 1 .. POL_WINDOW_MAX
LCAP_MAX = (6656 - 16) // 6     # run_polish: nodes the LDS arrays of the consensus sweep hold; larger graphs sweep in global scratch
OK16_MAX = 1546                 # win_rows_dispatch at the default scoring: 4 * 5 * (max(R, Q) + 4) >= 31000 from 1546 on
_HOOKS = ("C3_DEBUG_WIN_CHAIN", "C3_DEBUG_POISON", "C3_DEBUG_BAND", "C3_DEBUG_HCAP_DIV", "C3_DEBUG_WIN_LDS", "C3_DEBUG_WIN_LCAP")
_cache = {}


def _batch(which="sixteen"):
    if which not in _cache:
        if which == "sixteen":
            reads, strands = WC._batch()
            _cache[which] = ([reads[i] for i in SUBSET], [strands[i] for i in SUBSET])
        else:                   # the read of test_gpu_prep_rows.test_draft_beyond_lds: insert 4 300, two repeats
            s, q, st, _ = synth.make_read(np.random.default_rng([15, 0]), synth.SPLINT1, 4300, 2, 108, 108)
            _cache[which] = ([(s, q)], [st])
    return _cache[which]


def need(a):
    """copy of win_rows_dispatch's `need` (k_polish.hip): 64-column groups of the layer's DP row.  Keep the two in step."""
    return (a["Q"] + 1 + 63) // 64


def _oracle(wl, which="sixteen"):
    """oracle records, consensi and window capture of the batch under window length wl, computed once; every layer gets its
    row count R.  Every read must have a consensus: a case whose oracle has none compares nothing."""
    from oracle import oracle_py as O
    if ("oracle", wl, which) not in _cache:
        reads, strands = _batch(which)
        O.win_capture(True)
        try:
            ores, ocons = O.process_batch(synth.SPLINT1, reads, strands, params=O.default_params(pol_window=wl), threads=1)
            als = O.win_captured()
        finally:
            O.win_capture(False)
        for a in als:
            a["R"] = int(np.count_nonzero(a["mask"]))
        assert all(o.status == 0 for o in ores), (wl, [o.status for o in ores])
        _cache[("oracle", wl, which)] = (ores, ocons, als)
    return _cache[("oracle", wl, which)]


def _needs(als):
    return collections.Counter(need(a) for a in als)


def _gpu_run(wl, env, which="sixteen"):
    from c3poa_amd import _lib
    reads, strands = _batch(which)
    keep = {k: os.environ.get(k) for k in _HOOKS}
    for k in _HOOKS:
        os.environ.pop(k, None)
    os.environ["C3_DEBUG_POISON"] = "1"
    os.environ.update(env)
    try:
        h = _lib.Handle() if wl is None else _lib.Handle(pol_window=wl)
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


def _check(wl, env=None, oracle_cells=True, which="sixteen"):
    """GPU == oracle under window length wl, as test_gpu_win_chain._check compares; the oracle keeps no window count, so n_win
    is compared with the windows the GPU's own draft (whose polish is compared base for base) cuts into.  A C3_ST_LIMIT on
    the GPU where the oracle has a consensus fails here like any other difference.  returns (results, consensi, counters)"""
    ores, ocons, _ = _oracle(500 if wl is None else wl, which)
    res, cons, t = _gpu_run(wl, env or {}, which)
    WL = 500 if wl is None else wl
    for i, o in enumerate(ores):
        assert int(res[i]["status"]) == o.status, (wl, i, int(res[i]["status"]), o.status)
        for f in ("n_sub", "cons_len"):
            assert int(res[i][f]) == getattr(o, f), (wl, i, f, int(res[i][f]), getattr(o, f))
        assert int(res[i]["n_win"]) == (int(res[i]["draft_len"]) + WL - 1) // WL, (wl, i, int(res[i]["n_win"]), int(res[i]["draft_len"]))
        assert cons[i] == ocons[i], (wl, i)
    for k in ("cells_poa", "cells_polish") if oracle_cells else ("cells_poa",):
        want = sum(int(getattr(o, k)) for o in ores)
        assert t[k] == want, (wl, k, t[k], want)
    return res, cons, t


def _same(a, b, wl):
    """two GPU runs of one window length agree: records, consensi, counted and computed cells, band counters"""
    for i in range(len(a[0])):
        for f in ("status", "n_sub", "cons_len", "n_win"):
            assert int(a[0][i][f]) == int(b[0][i][f]), (wl, i, f, int(a[0][i][f]), int(b[0][i][f]))
        assert a[1][i] == b[1][i], (wl, i)
    for k in WC._TIMING:
        assert a[2][k] == b[2][k], (wl, k, a[2][k], b[2][k])


@pytest.mark.parametrize("wl,qmax,nmax,least,least_two", [(1, 1, 3, 29000, 1000), (2, 4, 5, 15000, 100), (7, 10, 11, 4500, 0)])
def test_windows_of_a_few_bases(wl, qmax, nmax, least, least_two):
    """windows of 1, 2 and 7 backbone bases: a thousand and more windows per read (NWcap, wcap, the window records and layer lists,
    t / WL), graphs of 3 .. 11 nodes, offset 0 so that no layer is full; at 1 and 2 there are layers that skip a window
    altogether (a deletion at its only bases: windows of two layers in reads whose other windows have three and four)"""
    _, _, als = _oracle(wl)
    assert len(als) >= least, len(als)
    assert max(a["Q"] for a in als) <= qmax and max(a["n"] for a in als) <= nmax, (max(a["Q"] for a in als), max(a["n"] for a in als))
    assert max(a["n"] for a in als) >= 3 and max(a["blen"] for a in als) == wl
    assert not any(a["full"] for a in als)
    per_win = collections.Counter(a["win"] for a in als)
    assert len(per_win) >= 16 * 900 // wl
    assert sum(n == 2 for n in per_win.values()) >= least_two and max(per_win.values()) >= 4
    res, _, t = _check(wl)
    assert min(int(r["n_win"]) for r in res) >= 900 // wl
    assert t["n_band_layers"] == 0


def test_first_window_length_that_drops_a_one_base_segment():
    """50: seglen < 0.02 * WL never fires (one-base segments are layers); 51: it drops exactly the segments of one base"""
    a50, a51 = _oracle(50)[2], _oracle(51)[2]
    assert sum(a["Q"] == 1 for a in a50) >= 1 and min(a["Q"] for a in a51) == 2, (min(a["Q"] for a in a50), min(a["Q"] for a in a51))
    assert len(a50) >= 650 and len(a51) >= 650
    _check(50)
    _check(51)


def test_every_layer_in_the_narrowest_rows():
    """100: every layer has need <= 2, so cpl = 2 runs on whole windows and the band is refused by need <= cb; no layer is full"""
    _, _, als = _oracle(100)
    n = _needs(als)
    assert set(n) == {1, 2} and n[1] >= 36 and n[2] >= 300, n
    assert not any(a["full"] for a in als)
    t = _check(100)[2]
    assert t["n_band_layers"] == 0 and t["n_band_fallback"] == 0


def test_both_sides_of_127_bases():
    """128: layers of up to 127 bases (cpl 2, never banded) and of 128 and more (cpl 4, banded) in one batch"""
    _, _, als = _oracle(128)
    n = _needs(als)
    assert n[2] >= 200 and n[3] >= 50 and max(n) == 3, n
    t = _check(128)[2]
    assert t["n_band_layers"] > 0


def test_first_window_length_with_a_full_layer():
    """offset = (int)(0.01 * blen) is 1 below 200 backbone bases, and l.end > blen - 1 never holds: 199 has no full layer, 200 has
    them (begin < 2 and end = 199), first layers among them"""
    a199, a200 = _oracle(199)[2], _oracle(200)[2]
    assert max(a["blen"] for a in a199) == 199 and not any(a["full"] for a in a199) and len(a199) >= 180
    assert sum(bool(a["full"]) for a in a200) >= 120 and sum(bool(a["full"]) for a in a200 if a["layer"] == 0) >= 40
    assert sum(not a["full"] for a in a200 if a["blen"] == 200) >= 20 and _needs(a200)[4] >= 110
    _check(199)
    _check(200)


@pytest.mark.parametrize("wl,lo,least_lo,least_hi", [(256, 4, 100, 10), (384, 6, 60, 5), (512, 8, 50, 3), (640, 10, 27, 2)])
def test_both_sides_of_a_row_template(wl, lo, least_lo, least_hi):
    """256, 384, 512: layers on both sides of cpl 4 / 6, 6 / 8 and 8 / 10; 640: of cpl 10 / the linear rows"""
    _, _, als = _oracle(wl)
    n = _needs(als)
    assert n[lo] >= least_lo and n[lo + 1] >= least_hi, (wl, n)
    _check(wl)


def test_both_sides_of_the_lds_query_arrays():
    """704: layers of exactly W_QCAP bases (rq / tq in LDS) and, at 710, of more (in global memory), all beyond cpl = 10"""
    a704, a710 = _oracle(704)[2], _oracle(710)[2]
    assert max(a["Q"] for a in a704) == W_QCAP and sum(a["Q"] == W_QCAP for a in a704) >= 1
    assert sum(need(a) >= 11 for a in a704) >= 28
    assert sum(a["Q"] > W_QCAP for a in a710) >= 2 and sum(W_QCAP - 64 < a["Q"] <= W_QCAP for a in a710) >= 25
    _check(704)
    _check(710)


def test_one_window_per_read():
    """2000: one window per read, graphs more than three times the default's, every long layer beyond cpl = 10"""
    _, _, als = _oracle(2000)
    assert len({a["win"] for a in als}) == 16
    assert max(a["Q"] for a in als) >= 1400 and max(a["n"] for a in als) >= 1700
    assert sum(need(a) > 10 for a in als) >= 24
    assert any(a["n"] > LCAP_MAX for a in als)                               # the consensus sweep in global scratch
    res, _, _ = _check(2000)
    assert all(int(r["n_win"]) == 1 for r in res)


def test_one_window_of_a_long_read():
    """pol_window 5000 and a draft of 4 474 bases: one window whose layers have more than 4 096 bases, more rows than the
    16-bit rows take at the default scoring and more nodes than the LDS consensus arrays hold"""
    _, _, als = _oracle(5000, "long")
    assert len({a["win"] for a in als}) == 1
    big = [a for a in als if a["Q"] > 4096]
    assert len(big) >= 2 and all(a["n"] > LCAP_MAX and max(a["R"], a["Q"]) > OK16_MAX for a in big)
    assert als[-1]["n"] > 4096 + 500
    res, _, _ = _check(5000, which="long")
    assert int(res[0]["n_win"]) == 1 and int(res[0]["draft_len"]) > 4096


def test_the_largest_admitted_window_length():
    """18 458: one window per read, node capacity 55 374 + 40 per layer, the dangling pieces of 108 bases are
    below 2 % of the window and dropped"""
    _, _, als = _oracle(POL_WINDOW_MAX)
    per_win = collections.Counter(a["win"] for a in als)
    assert len(per_win) == 16 and max(per_win.values()) <= 4 and min(a["Q"] for a in als) >= 0.02 * POL_WINDOW_MAX
    assert len(_oracle(2000)[2]) >= len(als) + 16                            # the layers 2000 keeps and this length drops
    res, _, _ = _check(POL_WINDOW_MAX)
    assert all(int(r["n_win"]) == 1 for r in res)


@pytest.mark.parametrize("wl", [100, 200, 640])
@pytest.mark.parametrize("mode", ["off", "verify"])
def test_band_modes(wl, mode):
    """off: the unbanded descriptor builder and rows for every layer; verify: band and full matrix of every accepted layer compared
    on the device (the second alignment of a layer is computed, not counted: cells_polish stays the oracle's)"""
    _oracle(wl)
    t = _check(wl, env={"C3_DEBUG_BAND": mode})[2]
    assert t["n_band_mismatch"] == 0
    if mode == "off" or wl == 100:
        assert t["n_band_layers"] == 0 and t["n_band_fallback"] == 0
    else:
        assert t["n_band_layers"] > 0


@pytest.mark.parametrize("wl", [7, 128, 200])
def test_chain_phases_off(wl):
    """first layers through the general graph phases (C3_DEBUG_WIN_CHAIN=0): the closed-form phases of the default run must leave
    what these leave, on windows of 7 bases, on first layers that are ranges of the chain (128) and on full first layers (200)"""
    _, _, als = _oracle(wl)
    first = [a for a in als if a["layer"] == 0]
    assert all(a["n"] == a["blen"] for a in first)
    if wl == 200:
        assert sum(bool(a["full"]) for a in first) >= 40 and sum(not a["full"] for a in first) >= 10
    else:
        assert sum(a["end"] - a["begin"] + 1 < a["blen"] for a in first) >= 10
    new = _check(wl)
    old = _check(wl, env={"C3_DEBUG_WIN_CHAIN": "0"})
    _same(new, old, wl)


def test_window_lengths_back_to_back():
    """fresh handles of different window lengths in one process, and a default run after them: nothing sized for one window
    length survives into the next"""
    _check(7)
    _check(2000)
    _check(100)
    res, _, t = _check(None)
    assert t["n_band_layers"] > 0 and all(int(r["n_win"]) >= 2 for r in res)

"""CPU side of the peak-calling edge tests: the oracle against the reference fixtures of tests/golden/make_golden_peaks.py
(other windows, pass counts and orders than the default, lengths around the window / the 256-key median exit / the
1024-point smoothing tile), and the oracle against a plain-Python restatement of the specification on exact-arithmetic
tracks (ties, plateaus, gate and height boundaries).  The GPU tests (test_gpu_peaks_edges.py) compare the kernel with the same
oracle on the same inputs, so what is expected there is settled here first."""
import numpy as np
import pytest

import peaks_edge_tracks as T
from oracle import oracle_py as O


@pytest.fixture(scope="module")
def fx():
    return T.load_fixtures()


def test_fixture_is_complete(fx):
    """every case of the grid is either pinned from the reference or listed as an exact tie; nothing is missing"""
    js, npz = fx
    assert [tuple(s) for s in js["settings"]] == T.SETTINGS and tuple(js["min_dists"]) == T.MIN_DISTS
    want = {T.case_key(s, name, md) for s in T.SETTINGS for name, _t in T.grid_tracks(s) for md in T.MIN_DISTS}
    assert set(js["peaks"]) | set(js["ties"]) == want
    assert not set(js["peaks"]) & set(js["ties"])
    assert len(js["ties"]) <= 3 and all("/step/d500" in k for k in js["ties"])
    for s in T.SETTINGS:
        for name, t in T.grid_tracks(s):
            assert np.array_equal(npz["track/" + name], t), name          # the builders still make the stored inputs
            assert len(npz["sm/%s/%s" % (T.setting_id(s), name)]) == len(t)


@pytest.mark.parametrize("setting", T.SETTINGS, ids=T.setting_id)
def test_oracle_against_reference_edges(fx, setting):
    js, npz = fx
    iters, window, order = setting
    for name, t in T.grid_tracks(setting):
        ref_sm = npz["sm/%s/%s" % (T.setting_id(setting), name)]
        for md in T.MIN_DISTS:
            pk, sm = O.call_peaks(t, md, iters, window, order, return_smoothed=True)
            key = T.case_key(setting, name, md)
            if key not in js["ties"]:
                assert pk.tolist() == js["peaks"][key], key
            # tolerance of test_call_peaks_against_reference_golden / test_savgol_matches_reference: numpy dot with pinv
            # coefficients against closed-form coefficients in a fixed fma order
            np.testing.assert_allclose(sm, ref_sm, rtol=1e-9, atol=1e-7, err_msg=key)


def test_grid_reaches_the_branches():
    """the inputs do what they were chosen for (all on the oracle's track): negative smoothed values on the step track,
    a tile whose first output is the last point of the track, tracks of exactly half + 1 points"""
    _pk, sm = O.call_peaks(T.step_track(), 50, 3, 41, 2, return_smoothed=True)
    assert sm.min() < -200
    for _i, w, _o in T.SETTINGS:
        half = (w - 1) // 2
        assert {half + 1, 1025, 2049, 3073, 1024 + 3 * half + 1} <= set(T.lengths(w))
    _pk, sm = O.call_peaks(T.equal_track(), 50, 3, 41, 2, return_smoothed=True)
    assert len(set(sm.tolist())) == 1 and len(sm) > 256              # the median select never narrows such keys down


def test_python_restatement_against_oracle():
    cases = T.exact_cases()
    assert len(cases) > 100
    n_open = 0
    for name, x, md, want in cases:
        got = T.py_call_peaks(x, md)
        assert len(got) <= 255, name                                     # what one GPU read can keep
        if name.startswith("alphabet"):
            n_open += len(got) > 3
        if want is not None:
            assert got == want, name
        assert O.call_peaks(np.asarray(x, dtype=np.int32), md, 0, 41, 2).tolist() == got, name
    assert n_open >= 55                                                  # the small-alphabet tracks are not simply gated


def test_python_restatement_on_reference_cases(fx):
    """the restatement itself against the reference: every iters = 0 case of the fixtures"""
    js, _npz = fx
    n = 0
    for s in T.SETTINGS:
        if s[0] != 0:
            continue
        for name, t in T.grid_tracks(s):
            for md in T.MIN_DISTS:
                assert T.py_call_peaks(t, md) == js["peaks"][T.case_key(s, name, md)], (name, md)
                n += 1
    assert n >= 60


def test_spike_tracks():
    for k in (255, 256):
        z = T.spikes_track(k)
        want = list(range(2, 2 + 4 * k, 4))
        assert T.py_call_peaks(z, 1) == want
        assert O.call_peaks(z, 1, 0, 41, 2).tolist() == want

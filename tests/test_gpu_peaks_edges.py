"""k_peaks at the settings, lengths and tracks that default runs never reach: every smoothing code path (unrolled half = 20,
generic tiled, untiled, no smoothing), track lengths around the window, the 256-key exit of the median select and the
1024-point LDS tile with its halo, plateaus across the threads' chunk boundaries, exact ties, the gate and height
boundaries, and the capacity of 255 peaks.  The kernel is compared with the CPU oracle bit for bit (fp64 smoothed track as
uint64), with the reference's own peaks (tests/golden/peaks_edges*) and, without smoothing, with the plain-Python
restatement of the specification in peaks_edge_tracks.py.  All calls go through Handle(...).call_peaks, one read per launch."""
import numpy as np
import pytest

import peaks_edge_tracks as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def O():
    from oracle import oracle_py
    return oracle_py


@pytest.fixture(scope="module")
def handles():
    from c3poa_amd import _lib
    made = {}

    def get(setting):
        if setting not in made:
            made[setting] = _lib.Handle(sg_iters=setting[0], sg_window=setting[1], sg_order=setting[2])
        return made[setting]
    yield get
    for h in made.values():
        h.close()


@pytest.fixture(scope="module")
def fx():
    return T.load_fixtures()


@pytest.mark.parametrize("setting", T.SETTINGS, ids=T.setting_id)
def test_grid_against_oracle_and_reference(handles, O, fx, setting):
    js, _npz = fx
    h = handles(setting)
    iters, window, order = setting
    n_ref = 0
    for name, t in T.grid_tracks(setting):
        for md in T.MIN_DISTS:
            key = T.case_key(setting, name, md)
            want, want_sm = O.call_peaks(t, md, iters, window, order, return_smoothed=True)
            got, got_sm = h.call_peaks(t, md, return_smoothed=True)
            bad = np.flatnonzero(want_sm.view(np.uint64) != got_sm.view(np.uint64))
            assert bad.size == 0, (key, bad[:8].tolist(), float(np.abs(want_sm - got_sm).max()))
            assert got.tolist() == want.tolist(), key
            if key not in js["ties"]:
                assert got.tolist() == js["peaks"][key], key
                n_ref += 1
    assert n_ref >= 3 * len(T.lengths(window)) + 5


def test_exact_arithmetic_cases(handles, O):
    h = handles((0, 41, 2))
    for name, x, md, want in T.exact_cases():
        x = np.asarray(x, dtype=np.int32)
        got, sm = h.call_peaks(x, md, return_smoothed=True)
        assert np.array_equal(sm, x.astype(np.float64)), name           # no smoothing: the track itself
        assert got.tolist() == T.py_call_peaks(x, md), name
        assert got.tolist() == O.call_peaks(x, md, 0, 41, 2).tolist(), name
        if want is not None:
            assert got.tolist() == want, name


def test_exact_arithmetic_cases_after_one_handle_served_longer_tracks(handles, O):
    """the scratch rows and candidate lists are reused between calls: a short track after a long one sees no leftovers"""
    h = handles((0, 41, 2))
    cases = T.exact_cases()
    for (name, x, md, _w), (_n2, x2, md2, _w2) in zip(cases[:40], cases[::-1][:40]):
        for z, d in ((x2, md2), (x, md)):
            z = np.asarray(z, dtype=np.int32)
            assert h.call_peaks(z, d).tolist() == T.py_call_peaks(z, d), name


def test_capacity_255_peaks(handles, O):
    h = handles((0, 41, 2))
    z = T.spikes_track(255)
    want = O.call_peaks(z, 1, 0, 41, 2).tolist()
    assert len(want) == 255 and want == list(range(2, 2 + 4 * 255, 4))
    assert h.call_peaks(z, 1).tolist() == want


def test_capacity_256_peaks_is_an_error_not_zero(handles, O):
    from c3poa_amd import _lib, shims
    h = handles((0, 41, 2))
    z = T.spikes_track(256)
    assert len(O.call_peaks(z, 1, 0, 41, 2)) == 256
    with pytest.raises(_lib.C3Error) as e:
        h.call_peaks(z, 1)
    assert e.value.code == _lib.E_LIMIT
    assert "255 peaks" in str(e.value)
    assert "255 peaks" in h.lib.c3_last_error(h.h).decode()
    # the handle goes on working, and a gated track is still 0 peaks without an error
    assert len(h.call_peaks(T.spikes_track(255), 1)) == 255
    assert h.call_peaks(np.full(300, 7, dtype=np.int32), 1).tolist() == []
    # the reference-shaped shim passes the error on
    with pytest.raises(_lib.C3Error) as e2:
        shims.call_peaks(z, 1, 0, 41, 2)
    assert e2.value.code == _lib.E_LIMIT


@pytest.mark.parametrize("window", [41, 5])
def test_too_short(window):
    """n = half: 0 peaks from call_peaks, C3_ST_TOO_SHORT in a batch (include/c3poa.h says what the reference does there);
    n = half + 1 is served"""
    from c3poa_amd import _lib
    half = (window - 1) // 2
    h = _lib.Handle(sg_window=window)
    h.set_splints(["ACGT"])
    x = np.arange(half, dtype=np.int32) * 100
    assert h.call_peaks(x, 1).tolist() == []
    reads = ["ACGT" * 8, ("ACGT" * 8)[:half], ("ACGT" * 8)[:half + 1], "ACGT" * 8]
    h.upload(reads, ["I" * len(r) for r in reads], ["+"] * 4)
    h.run(_lib.STAGE_CONK | _lib.STAGE_PEAKS)
    res, _ = h.results(with_consensus=False)
    assert res[1]["status"] == _lib.ST_TOO_SHORT and res[1]["n_peaks"] == 0
    assert res[2]["status"] != _lib.ST_TOO_SHORT
    assert res[0]["status"] != _lib.ST_TOO_SHORT and res[3]["status"] != _lib.ST_TOO_SHORT
    h.close()

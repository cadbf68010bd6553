"""k_poa's two-column rows: a row whose only predecessor is the row above, with a band of up to 128 columns (or
a row above whose cells are not in the fast row's registers), is computed with two band columns per lane, the row above read
from its LDS ring slot.  That is a schedule, never a change of result:
  * GPU == oracle with the two-column rows on and off (C3_DEBUG_POA_NO2COL) on cfg2 / cfg3 / cfg4 / cfgL samples, counted cells
    equal, no read handed to the 32-bit pass,
  * the same with the 16-bit base moving every few rows (C3_DEBUG_POA_RBSPAN: the rare re-basing branch of the row),
  * MSA rows equal the oracle's when the band half-width puts rows at 64 / 65 / 127 / 128 columns (and every band shift the
    drifting maxima give), on the NARROW ring (where the rows live) and on the instance the library picks."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from c3poa_amd import _lib, synth  # noqa: E402
from oracle import oracle_py as O  # noqa: E402

pytestmark = pytest.mark.gpu


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


def _run(recs, mdist, env):
    with _env(env):
        h = _lib.Handle(mdistcutoff=mdist)
        h.set_splints([synth.SPLINT1])
        h.upload([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs])
        h.run()
        res, cons = h.results()
        t = h.timing()
        h.close()
    return res, cons, t


def _ragged(recs, seed):
    """every third read loses or doubles a 25-90 base chunk in one repeat: wider, drifting bands"""
    rng = np.random.default_rng(seed)
    out = []
    for k, r in enumerate(recs):
        name, seq, qual, strand, truth = r
        if k % 3 == 0 and len(seq) > 3000:
            at = int(rng.integers(1800, len(seq) - 400)); ln = int(rng.integers(25, 90))
            if k % 2:
                seq, qual = seq[:at] + seq[at + ln:], qual[:at] + qual[at + ln:]
            else:
                seq, qual = seq[:at] + seq[at:at + ln] + seq[at:], qual[:at] + qual[at:at + ln] + qual[at:]
        out.append((name, seq, qual, strand, truth))
    return out


NO2COL = {"C3_DEBUG_POA_NO2COL": "1"}


@pytest.mark.parametrize("cfg,n,base", [("cfg2", 128, {}), ("cfg3", 96, {}), ("cfg4", 24, {}),
                                        ("cfgL", 8, {"C3_DEBUG_POA_WIDE": "0"})])
def test_two_column_rows_equal_the_oracle(cfg, n, base):
    recs = _ragged(list(synth.generate(cfg, n_reads=n)), seed=11)
    md = synth.CONFIGS[cfg]["mdist"]
    ores, ocons = O.process_batch(synth.SPLINT1, [(r[1], r[2]) for r in recs], [r[3] for r in recs],
                                  params=O.default_params(mdistcutoff=md), threads=8)
    cells = sum(int(r.cells_poa) for r in ores)
    for extra in ({}, NO2COL, {"C3_DEBUG_POA_RBSPAN": "3300"}, dict(NO2COL, C3_DEBUG_POA_RBSPAN="3300")):
        env = dict(base, **extra)
        res, cons, t = _run(recs, md, env)
        for i in range(n):
            assert res[i]["status"] == ores[i].status and cons[i] == ocons[i], (cfg, env, i)
        assert t["cells_poa"] == cells, (cfg, env)
        assert t["n_poa_redo16"] == 0, (cfg, env, t["n_poa_redo16"])


def _subread_groups(n_groups, seed):
    """3-4 subreads of ~1.5 kb per group, cut from synthetic reads, some with a chunk lost or doubled (band drift)"""
    recs = _ragged(list(synth.generate("cfg2", n_reads=3 * n_groups)), seed=seed)
    groups = []
    for r in recs[:n_groups]:
        seq = r[1]
        k = 3 + (len(groups) % 2)
        step = max(600, (len(seq) - 300) // k)
        groups.append([seq[150 + step * i: 150 + step * (i + 1)] for i in range(k) if 150 + step * (i + 1) <= len(seq)])
    return [g for g in groups if len(g) >= 2]


@pytest.mark.parametrize("half_width", [31, 32, 63, 64])
def test_band_edges_64_65_127_128(half_width):
    """w = band_b with band_f = 0: a row holds 2w+1 columns plus the drift of the maxima, and fewer where the band is clipped
    (the first rows, the query ends), so w = 31 / 32 / 63 / 64 put rows on both sides of 64 and of 128 columns"""
    groups = _subread_groups(6, seed=half_width)
    P = O.default_params(poa_band_b=half_width, poa_band_f=0.0)
    want = [O.poa_msa(g, params=P)[:2] for g in groups]
    for env in ({"C3_DEBUG_POA_WIDE": "0"}, dict(NO2COL, C3_DEBUG_POA_WIDE="0"), {"C3_DEBUG_POA_WIDE": "0", "C3_DEBUG_POA_RBSPAN": "3300"}, {}):
        with _env(env):
            h = _lib.Handle(poa_band_b=half_width, poa_band_f=0.0)
            for g, (oc, om) in zip(groups, want):
                gc, gm = h.poa_msa(g)
                assert gc == oc and gm == om, (half_width, env, [len(s) for s in g])
            h.close()

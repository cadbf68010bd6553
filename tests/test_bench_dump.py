"""bench.py --dump-outputs: what the timed path delivered for its last batch, as float32 / float64 .npy files of at most 64 MB,
for a seeded sample of reads that depends on the input only (CPU); end to end against an independent run of the same reads (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from c3poa_amd import _lib, synth  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def _fake_batch(rng, n, garbage):
    """records whose array tails hold `garbage` (they are unspecified in what c3_batch_results delivers)"""
    lens = rng.integers(500, 6000, n).astype(np.int64)
    res = np.zeros(n, dtype=_lib.RESULT_DTYPE)
    res["status"] = rng.integers(0, 4, n)
    res["n_peaks"] = rng.integers(0, 8, n)
    res["n_sub"] = np.maximum(res["n_peaks"] - 1, 0)
    for f in ("peaks", "sub_beg", "sub_end"):
        res[f] = garbage
        for i in range(n):
            m = res["n_peaks"][i] if f == "peaks" else res["n_sub"][i]
            res[f][i, :m] = np.sort(rng.integers(0, lens[i], m))
    res["cons_len"] = np.where(res["status"] == 0, lens // 4, 0)
    coff = np.concatenate(([0], np.cumsum(res["cons_len"]))).astype(np.int64)
    cbuf = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), int(coff[-1]) + 16)
    return res, cbuf, coff, lens


def test_dump_is_a_fixed_sample_within_the_budget(tmp_path):
    rng = np.random.default_rng(7)
    res, cbuf, coff, lens = _fake_batch(rng, 3000, garbage=12345)
    budget = 4 << 20                                                    # forces a sample: 3000 reads need ~48 MB
    s = bench.dump_outputs(str(tmp_path / "a"), res, cbuf, coff, lens, budget=budget)
    assert 0 < s["reads"] < 3000 and s["bytes"] <= budget
    d = _load(str(tmp_path / "a"))
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in d) == s["bytes"]
    assert all(v.dtype in (np.float32, np.float64) for v in d.values())
    idx = d["read_index"].astype(np.int64)
    assert len(idx) == s["reads"] and np.all(np.diff(idx) > 0)
    for f in bench.DUMP_FIELDS:
        assert np.array_equal(d[f], res[f][idx])
    for f, cnt in (("peaks", "n_peaks"), ("sub_beg", "n_sub"), ("sub_end", "n_sub")):
        for j, i in enumerate(idx):
            m = res[cnt][i]
            assert np.array_equal(d[f][j, :m], res[f][i, :m]) and np.all(d[f][j, m:] == -1)
    co = d["consensus_offsets"].astype(np.int64)
    for j, i in enumerate(idx):
        assert np.array_equal(d["consensus"][co[j]:co[j + 1]], cbuf[coff[i]:coff[i + 1]])
    # other results (and other tail garbage) for the same input: the same reads are sampled, the tails dump the same
    res2, cbuf2, coff2, _ = _fake_batch(np.random.default_rng(7), 3000, garbage=-777)
    res2["status"] = 1 - res2["status"]
    bench.dump_outputs(str(tmp_path / "b"), res2, cbuf2, coff2, lens, budget=budget)
    d2 = _load(str(tmp_path / "b"))
    assert np.array_equal(d2["read_index"], d["read_index"])
    assert np.array_equal(d2["peaks"], d["peaks"]) and not np.array_equal(d2["status"], d["status"])


def test_dump_keeps_every_read_of_a_small_batch(tmp_path):
    res, cbuf, coff, lens = _fake_batch(np.random.default_rng(1), 64, garbage=0)
    s = bench.dump_outputs(str(tmp_path), res, cbuf, coff, lens)
    assert s["reads"] == 64 and s["bytes"] <= bench.DUMP_BYTES
    d = _load(str(tmp_path))
    assert np.array_equal(d["read_index"], np.arange(64)) and len(d["consensus"]) == coff[-1]


def test_steps_and_warmup_are_checked():
    assert bench.parse_args(["--steps", "1", "--warmup", "0"]).steps == 1
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    assert bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"


@pytest.mark.gpu
def test_bench_dump_equals_a_run_of_the_same_reads(tmp_path):
    n = 512
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--reads", str(n), "--steps", "2", "--warmup", "1",
           "--no-cpu", "--other-configs", "none", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["dump_outputs"]["reads"] == n
    d = _load(str(tmp_path))
    recs = list(synth.generate("cfg2", n_reads=n))
    h = _lib.Handle(mdistcutoff=synth.CONFIGS["cfg2"]["mdist"])
    h.set_splints([synth.SPLINT1])
    h.upload([x[1] for x in recs], [x[2] for x in recs], [x[3] for x in recs])
    h.run()
    res, cbuf, coff = h.results_raw()
    assert (res["status"] == 0).sum() >= n - 2
    for f in bench.DUMP_FIELDS:
        assert np.array_equal(d[f], res[f]), f
    for j in range(n):
        assert np.array_equal(d["peaks"][j, :res["n_peaks"][j]], res["peaks"][j, :res["n_peaks"][j]])
        assert np.array_equal(d["sub_end"][j, :res["n_sub"][j]], res["sub_end"][j, :res["n_sub"][j]])
    assert bytes(d["consensus"].astype(np.uint8)) == cbuf.tobytes()[:int(coff[-1])]
    h.close()

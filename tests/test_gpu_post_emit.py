"""GPU tests of --emit gpu (k_post): the device against its host statement on the hand-made tables of the host test, the real
pipeline (scan_adapters -> c3_post_emit) and the CLI against the Python path, batching, --keep-quals and the four fallbacks."""
import gzip
import os
import shutil

import numpy as np
import pytest

import post_emit_cases as K
from c3poa_amd import postprocess as PP
from c3poa_amd import synth
from c3poa_amd.seqio import revcomp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    from c3poa_amd import _lib
    h = _lib.Handle()
    yield h
    h.close()


def _same(dev, host):
    return np.array_equal(dev[1], host[1]) and dev[2] == host[2] and \
        np.array_equal(dev[0][:int(dev[1][-1])], host[0][:int(host[1][-1])])


@pytest.mark.parametrize("with_quals", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("combo", list(K.COMBOS))
def test_device_equals_host_statement(handle, combo, with_quals):
    from c3poa_amd import _lib
    names, seqs, quals, tab = K.make_reads(combo)
    plan, batch = K.plan_of(combo), _lib.PostBatch.from_lists(names, seqs, quals if with_quals else None)
    host = _lib.post_emit_host(plan, batch, tab)
    assert host[2] > 0.3 * len(names) and host[1][-1] > 0
    assert _same(handle.post_emit(plan, batch, tab), host)


def test_device_long_read_and_empty_batches(handle):
    """a read above the length at which the four waves of a workgroup share the body segments (32768), both directions and
    with qualities; a batch with no kept read; an empty batch"""
    from c3poa_amd import _lib
    rng = np.random.default_rng(5)
    names, seqs, quals, tab = K.make_reads("bt", seed=11, n_random=6)
    tab = tab.copy()
    for i, L in ((1, 40001), (2, 33000)):                                      # read 1 goes '-' (plus hit on 3Prime_adapter), read 2 '+'
        seqs[i] = "".join(K.ODD[k] for k in rng.integers(0, len(K.ODD), L))
        quals[i] = "".join(chr(33 + int(k)) for k in rng.integers(0, 61, L))
        tab[i, :, :, 0] = 0
        ap, am = (0, 1) if i == 1 else (1, 0)
        tab[i, ap, 0] = K._hit(rng, K.AD_DIR[ap][1], 0, 37 + i)
        tab[i, am, 1] = K._hit(rng, K.AD_DIR[am][1], 1, L - 41 - i)
    for combo in ("bt", "b"):
        for q in (None, quals):
            plan, batch = K.plan_of(combo), _lib.PostBatch.from_lists(names, seqs, q)
            host = _lib.post_emit_host(plan, batch, tab)
            assert host[2] >= 2 and host[1][-1] > 40001 + 33000 - 400             # both long reads are kept and written
            assert _same(handle.post_emit(plan, batch, tab), host)
    none = tab.copy()
    none[:, :, 1, 5] = 10                                                      # no '-' row counts
    plan, batch = K.plan_of("bt"), _lib.PostBatch.from_lists(names, seqs)
    host = _lib.post_emit_host(plan, batch, none)
    assert host[2] == 0 and _same(handle.post_emit(plan, batch, none), host)
    empty = (_lib.PostBatch.from_lists([], []), np.zeros((0, 2, 2, 12), np.int32))
    assert _same(handle.post_emit(plan, *empty), _lib.post_emit_host(plan, *empty))
    t = handle.post_emit_timing()
    assert t["n_reads"] == 0 and t["out_bytes"] == 0


# ---- real alignments ---------------------------------------------------------------------------------------------------
def _rand(rng, L):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, L))


def _noisy(rng, s, err):
    out, _q = synth._mutate(rng, np.frombuffer(s.encode(), dtype=np.uint8), sub=err * 0.4, ins=err * 0.25, dele=err * 0.35)
    return out.decode()


def _dataset(seed, n, kind, idx=None, err=0.06):
    """consensus-like reads with planted adapters: (records [(name, seq, qual)], adapters [(name, seq)])"""
    rng = np.random.default_rng(seed)
    a5, a3, und = _rand(rng, 33), _rand(rng, 36), _rand(rng, 40)
    recs = []
    for i in range(n):
        cdna = _rand(rng, int(rng.integers(60, 500)))
        pre, post = _rand(rng, int(rng.integers(0, 45))), _rand(rng, int(rng.integers(0, 45)))
        if kind == "und":
            tag = idx[i % (len(idx) + 1)][1] if idx and i % (len(idx) + 1) < len(idx) else _rand(rng, 16)
            seq = pre + _noisy(rng, und, err) + (tag + cdna if i % 2 else cdna + revcomp(tag)) + _noisy(rng, revcomp(und), err) + post
        else:
            l, r = (a3, a5) if i % 3 == 0 else (a5, a3)
            seq = pre + _noisy(rng, l, err) + cdna + _noisy(rng, revcomp(r), err) + post
        if i % 17 == 5:
            seq = _rand(rng, int(rng.integers(30, 300)))                        # no adapter at all
        if i % 19 == 7:
            seq = seq[:int(rng.integers(1, 40))]                                # a stub
        if i % 23 == 3:
            seq = seq.lower() if i % 2 else seq.replace("A", "N", 3)
        recs.append(("c%04d_11.%d_5000_%d_%d" % (i, i % 10, 1 + i % 5, len(seq)), seq,
                     "".join(chr(65 + int(k)) for k in rng.integers(0, 29, len(seq)))))
    adapters = [("Adapter", und)] if kind == "und" else [("3Prime_adapter", a3), ("5Prime_adapter", a5)]
    return recs, adapters


def _write_fa(path, recs):
    with open(path, "w") as fh:
        for r in recs:
            fh.write(">%s\n%s\n" % (r[0], r[1]))


def _write_fq(path, recs):
    with open(path, "w") as fh:
        for r in recs:
            fh.write("@%s\n%s\n+\n%s\n" % (r[0], r[1], r[2]))


def test_real_pipeline_equals_python_path(handle, tmp_path):
    """a few hundred reads with noisy planted adapters through scan_adapters, then c3_post_emit against the Python path"""
    from c3poa_amd import _lib
    recs, adapters = _dataset(21, 300, "dir")
    names, seqs, quals = [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]
    handle.set_splints([a[1] for a in adapters])
    handle.upload(seqs, ["!" * len(s) for s in seqs], "?" * len(seqs))
    tab = handle.scan_adapters()
    try:
        for combo, base in (("real_t", "t"), ("real_b", "b")):
            K.COMBOS[combo] = dict(K.COMBOS[base], adapters=[(a[0], len(a[1])) for a in adapters])
            for q in (False, True):
                exp, keep, _d = K.expected_streams(combo, names, seqs, quals, tab, tmp_path, q)
                assert len(keep) > 200
                got = handle.post_emit(K.plan_of(combo), _lib.PostBatch.from_lists(names, seqs, quals if q else None), tab)
                assert got[2] == len(keep) and K.split(got[0], got[1]) == exp
    finally:
        K.COMBOS.pop("real_t", None)
        K.COMBOS.pop("real_b", None)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def _tree(root):
    out = {}
    for base, _d, files in os.walk(root):
        for f in files:
            p = os.path.join(base, f)
            data = gzip.open(p, "rb").read() if f.endswith(".gz") else open(p, "rb").read()
            out[os.path.relpath(p, root)] = data
    return out


def _cli(argv):
    import C3POa_postprocessing as P
    return P.main(P.parse_args(argv))


def _inputs(tmp_path, kind, n=150, idx=None, seed=33):
    recs, adapters = _dataset(seed, n, kind, idx)
    fa, fq, ad = str(tmp_path / "cons.fasta"), str(tmp_path / "cons.fastq"), str(tmp_path / "adapters.fasta")
    _write_fa(fa, recs); _write_fq(fq, recs); _write_fa(ad, adapters)
    return recs, adapters, fa, fq, ad


IDX3 = [("dT_A", "GAGGTAAAGCAGGGAA"), ("dT_B", "TCATCCGCGTACTTCC"), ("dT_C", "CTCAAAATCTGAATTC")]


@pytest.mark.parametrize("case", ["dir_t", "und_x", "10x"])
def test_cli_trees_are_equal(tmp_path, case):
    if case == "und_x":
        recs, adapters, fa, fq, ad = _inputs(tmp_path, "und", idx=IDX3)
        ix = str(tmp_path / "idx.fasta")
        _write_fa(ix, IDX3)
        opts = ["-u", "-t", "-x", ix, "-n", "2", "-co"]
    else:
        recs, adapters, fa, fq, ad = _inputs(tmp_path, "dir")
        opts = ["-t"] if case == "dir_t" else ["-b"]
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    n_host = _cli(["-i", fa, "-a", ad, "-o", host] + opts)
    n_dev = _cli(["-i", fa, "-a", ad, "-o", dev, "--emit", "gpu"] + opts)
    th, td = _tree(host), _tree(dev)
    assert n_host == n_dev and n_host > 80
    assert sorted(th) == sorted(td) and PP.PSL_NAME in td
    for f in th:
        assert th[f] == td[f], f
    if case == "und_x":
        assert sum(len(v) > 0 for f, v in td.items() if f.endswith("reads.fasta.gz")) == 4      # three indexes + no_index_found
    # FASTQ input gives the same files (-i accepts FASTQ as before)
    dev2 = str(tmp_path / "dev_fq")
    _cli(["-i", fq, "-a", ad, "-o", dev2, "--emit", "gpu"] + opts)
    assert _tree(dev2) == td


def test_cli_batches_do_not_show(tmp_path):
    recs, adapters, fa, fq, ad = _inputs(tmp_path, "dir", n=60)
    one, many = str(tmp_path / "one"), str(tmp_path / "many")
    _cli(["-i", fa, "-a", ad, "-o", one, "--emit", "gpu", "-b"])
    _cli(["-i", fa, "-a", ad, "-o", many, "--emit", "gpu", "-b", "--post-batch", "7"])
    assert _tree(one) == _tree(many) and len(_tree(one)) == 5


def test_cli_keep_quals(tmp_path, capsys):
    recs, adapters, fa, fq, ad = _inputs(tmp_path, "dir", n=120)
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    _cli(["-i", fa, "-a", ad, "-o", host, "-t"])
    n = _cli(["-i", fq, "-a", ad, "-o", dev, "-t", "--emit", "gpu", "--keep-quals", "--post-batch", "50"])
    # the Python quality model on the host path's own PSL
    reads, quals = {r[0]: r[1] for r in recs}, {r[0]: r[2] for r in recs}
    opts = K.opts_of("t")
    keep = K.classify(opts, PP.parse_blat(host + "/" + PP.PSL_NAME, reads), reads, {}, {})
    model = K.fastq_model(opts, keep, reads, quals)
    td = _tree(dev)
    assert n == len(keep) > 60
    assert sorted(td) == sorted([PP.PSL_NAME] + [f.replace(".fasta", ".fastq") for f in (PP.FLC, PP.FLC_LEFT, PP.FLC_RIGHT)])
    for k, f in enumerate((PP.FLC, PP.FLC_LEFT, PP.FLC_RIGHT)):
        assert td[f.replace(".fasta", ".fastq")] == model[("", k)].encode(), f
    assert td[PP.PSL_NAME] == _tree(host)[PP.PSL_NAME]
    # FASTA input has no qualities to keep
    with pytest.raises(SystemExit) as e:
        _cli(["-i", fa, "-a", ad, "-o", str(tmp_path / "dev_fa"), "-t", "--emit", "gpu", "--keep-quals"])
    assert e.value.code not in (0, None) and "no quality line" in str(e.value.code)
    import C3POa_postprocessing as P
    with pytest.raises(SystemExit):
        P.parse_args(["-i", fq, "-a", ad, "-o", dev, "--keep-quals"])           # needs --emit gpu
    capsys.readouterr()


@pytest.mark.parametrize("case", ["psl", "dup", "high", "limit"])
def test_cli_fallbacks_give_the_host_tree(tmp_path, capsys, case):
    recs, adapters, fa, fq, ad = _inputs(tmp_path, "dir", n=40)
    opts, note = ["-t"], None
    host, dev = str(tmp_path / "host"), str(tmp_path / "dev")
    if case == "dup":
        recs[7] = (recs[3][0],) + recs[7][1:]
        note = "share a name"
    elif case == "high":
        recs[5] = ("réad_" + recs[5][0],) + recs[5][1:]
        note = "0x80"
    elif case == "limit":                                                       # 17 indexes: beyond the device matcher; no read reaches it here
        recs = [(r[0], "N" * (150 + i), "I" * (150 + i)) for i, r in enumerate(recs)]
        ix = str(tmp_path / "idx.fasta")
        _write_fa(ix, [("i%02d" % k, _rand(np.random.default_rng(100 + k), 16)) for k in range(17)])
        opts, note = ["-t", "-x", ix], "more than 16 indexes"
    _write_fa(fa, recs); _write_fq(fq, recs)
    _cli(["-i", fa, "-a", ad, "-o", host] + opts)
    if case == "psl":
        os.makedirs(dev)
        shutil.copy(host + "/" + PP.PSL_NAME, dev + "/" + PP.PSL_NAME)
        note = "is reused"
    capsys.readouterr()
    _cli(["-i", fa, "-a", ad, "-o", dev, "--emit", "gpu"] + opts)
    err = capsys.readouterr().err
    assert "--emit gpu:" in err and note in err and "using the host path" in err
    assert _tree(dev) == _tree(host)
    if case == "psl":
        os.makedirs(str(tmp_path / "dev_q"))
        shutil.copy(host + "/" + PP.PSL_NAME, str(tmp_path / "dev_q" / PP.PSL_NAME))
    with pytest.raises(SystemExit) as e:                                        # no silent FASTA under --keep-quals
        _cli(["-i", fq, "-a", ad, "-o", str(tmp_path / "dev_q"), "--emit", "gpu", "--keep-quals"] + opts)
    assert e.value.code not in (0, None)

"""c3_post_emit_host (the host statement of k_post) against the existing Python path, stream by stream, byte for byte, on
hand-made adapter tables (tests/post_emit_cases.py).  Expected bytes come from psl_line -> parse_blat -> write_fasta_file and,
for qualities, from the same Python slices; never from the code under test.  No GPU."""
import numpy as np
import pytest

import post_emit_cases as K
from c3poa_amd import _lib

STREAM_KIND = ("main", "left", "right")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """per combination: the reads, the table and the expected streams with and without qualities (computed once)"""
    tmp = tmp_path_factory.mktemp("post_emit_truth")
    out = {}
    for combo in K.COMBOS:
        names, seqs, quals, tab = K.make_reads(combo)
        exp, keep, dests = K.expected_streams(combo, names, seqs, quals, tab, tmp, False)
        exp_q, keep_q, _d = K.expected_streams(combo, names, seqs, quals, tab, tmp, True)
        assert keep == keep_q
        out[combo] = dict(names=names, seqs=seqs, quals=quals, tab=tab, exp=exp, exp_q=exp_q, keep=keep, dests=dests)
    return out


def _compare(c, combo, with_quals):
    plan = K.plan_of(combo)
    batch = _lib.PostBatch.from_lists(c["names"], c["seqs"], c["quals"] if with_quals else None)
    arena, so, kept = _lib.post_emit_host(plan, batch, c["tab"])
    assert plan.dests == c["dests"] and len(so) == 3 * len(plan.dests) + 4
    assert kept == len(c["keep"])
    got, exp = K.split(arena, so), c["exp_q" if with_quals else "exp"]
    for s in range(len(exp)):
        assert got[s] == exp[s], "stream %d of %s differs" % (s, combo)


@pytest.mark.parametrize("with_quals", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("combo", list(K.COMBOS))
def test_host_statement_equals_python_path(cases, combo, with_quals):
    _compare(cases[combo], combo, with_quals)


def test_python_path_covers_the_cases(cases):
    """the chosen seed meets the issue's coverage conditions on the Python path alone"""
    lens = {n: len(s) for n, s in zip(cases["t"]["names"], cases["t"]["seqs"])}
    for combo, c in cases.items():
        assert len(c["keep"]) >= 0.3 * len(c["names"]), combo
    for combo in ("t", "bt", "main"):
        keep = cases[combo]["keep"]
        L = {n: len(s) for n, s in zip(cases[combo]["names"], cases[combo]["seqs"])}
        cnt = dict(p13=0, m2_15=0, m16_39=0, m40=0, m4=0, pL=0, mL=0, short=0)
        seq_lens, bodies = set(), ""
        reads = dict(zip(cases[combo]["names"], cases[combo]["seqs"]))
        for name, p, m, _d, _dest in keep:
            s = reads[name]
            cnt["p13"] += 1 <= p <= 3
            cnt["m2_15"] += 2 <= m <= 15
            cnt["m16_39"] += 16 <= m <= 39
            cnt["m40"] += m + 40 > L[name]
            cnt["m4"] += m + 4 > L[name]
            cnt["pL"] += p >= L[name]
            cnt["mL"] += m > L[name]
            cnt["short"] += L[name] <= 16 and (len(s[p - 4:p + 16]) > 0 or len(s[m - 16:m + 4]) > 0 or len(s[m - 40:m]) > 0)
            seq_lens.add(len(s[p:m]))
            bodies += s[p:m]
        assert all(v >= 1 for v in cnt.values()), (combo, cnt)
        assert {0, 9, 10, 99, 100, 999} <= seq_lens                              # digit counts of the name suffix
        assert {0, 1, 63, 64, 65, 255, 256, 257} <= seq_lens                     # copy-tail lengths (-t: the body is seq)
        for ch in "NacgtRYKMBDHVU*-":
            assert ch in bodies, ch
    for s, b in enumerate(cases["main"]["exp"]):                                # every kind of stream at once, none empty
        assert len(b) > 0, s
    assert len(cases["b"]["exp"][3]) > 0 and len(cases["x_dir"]["exp"][-2]) > 0 and len(cases["none"]["exp"][-1]) > 0
    unused = cases["x_unused"]
    d = unused["dests"].index("dT_never")
    assert unused["exp"][3 * d:3 * d + 3] == [b"", b"", b""]                    # a destination no read goes to
    assert cases["main"]["dests"] == ["dT_A", "dT_B", "dT_C", "no_index_found"]  # two index sequences share dT_A
    dirs = {k[3] for k in cases["no5"]["keep"]}
    assert dirs == {"-"}                                                        # no adapter is called 5Prime_adapter
    assert {k[3] for k in cases["main"]["keep"]} == {"+", "-"}


def test_drop_rules_sit_between_kept_reads(cases):
    c = cases["t"]
    kept = {k[0] for k in c["keep"]}
    first = len(K.SPECIAL)
    for r in range(4):
        a, b, d = c["names"][first + 3 * r: first + 3 * r + 3]
        assert a in kept and b not in kept and d in kept, r
    edge = c["names"][first + 12: first + 18]                                   # qBaseInsert 50 / 49, matches 10 / 11, score 21 / 22
    assert [n in kept for n in edge] == [True, False, True, False, True, False]
    dup = cases["dup"]
    kd = {k[0] for k in dup["keep"]}
    assert [n in kd for n in dup["names"][first + 18: first + 22]] == [False, False, True, True]


def test_batch_without_a_kept_read(tmp_path):
    """all streams but the PSL are empty; the Python path creates its files empty as well"""
    names, seqs, quals, tab = K.make_reads("bt", seed=3, n_random=0)
    tab = tab.copy()
    tab[:, :, 1, 0] = np.minimum(tab[:, :, 1, 0], 30)
    tab[:, :, 1, 5] = 10                                                        # no '-' row counts any more
    exp, keep, _d = K.expected_streams("bt", names, seqs, quals, tab, tmp_path, False)
    assert keep == [] and exp[:5] == [b""] * 5 and len(exp[5]) > 0
    arena, so, kept = _lib.post_emit_host(K.plan_of("bt"), _lib.PostBatch.from_lists(names, seqs), tab)
    assert kept == 0 and K.split(arena, so) == exp
    arena, so, kept = _lib.post_emit_host(K.plan_of("bt"), _lib.PostBatch.from_lists([], []), np.zeros((0, 2, 2, 12), np.int32))
    assert kept == 0 and list(so) == [0] * 7


def test_limits_and_arena_size():
    names, seqs, quals, tab = K.make_reads("t", n_random=5)
    plan, batch = K.plan_of("t"), _lib.PostBatch.from_lists(names, seqs)
    arena, so, kept = _lib.post_emit_host(plan, batch, tab)
    lib = _lib.load()
    import ctypes as C
    # a short arena: C3_E_LIMIT, the needed size reported, nothing written
    calls = []

    def fn(a, arena_p, cap, so_p, kept_p):
        guard = np.full(64, 0xEE, dtype=np.uint8)
        so2 = np.zeros(7, dtype=np.int64)
        rc = lib.c3_post_emit_host(a, guard.ctypes.data, 64, so2.ctypes.data, kept_p)
        calls.append((rc, int(so2[6]), bool((guard == 0xEE).all()), lib.c3_last_error(None).decode()))
        return lib.c3_post_emit_host(a, arena_p, cap, so_p, kept_p)
    _lib._post_call(fn, lambda: b"", plan, batch, tab)
    assert calls[0][0] == _lib.E_LIMIT and calls[0][1] == int(so[6]) and calls[0][2] and "arena too small" in calls[0][3]
    # the limits of c3_match_index_batch: 16 indexes of at most 32 bases
    for idx in ([("i%d" % k, "ACGT" * 4 + "ACGTACGTACGTACGT"[k:] + "C" * k) for k in range(17)], [("a", "A" * 33), ("b", "C" * 16)]):
        i2s, s2i = {n: s for n, s in idx}, {s: n for n, s in idx}
        big = _lib.PostPlan([("3Prime_adapter", "A" * 36), ("5Prime_adapter", "A" * 33)], (i2s, s2i), trim=True)
        with pytest.raises(_lib.C3Error) as e:
            _lib.post_emit_host(big, batch, tab)
        assert e.value.code == _lib.E_LIMIT

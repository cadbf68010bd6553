"""The output tree of a C3POa.py run (c3poa_amd/stream.py: OutputTree) on its own: no thread, no handle, no device.

Which files exist before and after a run in the three modes (plain, -co, --bgzf), with and without --consensus-fastq, and
in the fused mode (no PSL yet).  Two splints, SplA and SplB; only SplA is used.  The expected listings and bytes are
written out: they are what stream.run did to the tree before OutputTree was cut out of it.
"""
import gzip
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from c3poa_amd import _lib, stream  # noqa: E402

NAMES = ["SplA", "SplB"]
PLAIN = ["R2C2_Consensus.fasta", "R2C2_Subreads.fastq"]
PLAIN_QV = ["R2C2_Consensus.fasta", "R2C2_Consensus.fastq", "R2C2_Subreads.fastq"]
GZ = ["R2C2_Consensus.fasta.gz", "R2C2_Subreads.fastq.gz"]
GZ_QV = ["R2C2_Consensus.fasta.gz", "R2C2_Consensus.fastq.gz", "R2C2_Subreads.fastq.gz"]
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
MODES = {"plain": {}, "co": {"compress": True}, "bgzf": {"bgzf": True}}


def _tree(tmp_path, mode, qv, **kw):
    out = str(tmp_path) + "/out/"
    os.makedirs(out, exist_ok=True)
    return out, stream.OutputTree(out, NAMES, qv=qv, **MODES[mode], **kw)


def _put(path, data):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(data)


def _get(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("qv", [False, True])
@pytest.mark.parametrize("mode", ["plain", "co", "bgzf"])
def test_prepare_truncates_and_removes_the_stale_counterpart(tmp_path, mode, qv):
    out, tree = _tree(tmp_path, mode, qv)
    for f in PLAIN_QV + GZ_QV:                                         # an earlier run in either form left bytes behind
        _put(out + "SplA/" + f, b"stale bytes")
    tree.prepare({"SplA"})
    want = {("plain", False): PLAIN, ("plain", True): PLAIN_QV, ("co", False): PLAIN, ("co", True): PLAIN_QV,
            ("bgzf", False): GZ, ("bgzf", True): GZ_QV}[mode, qv]
    # X when writing X.gz, X.gz when writing X: gone.  (Without QVs nobody owns R2C2_Consensus.fastq[.gz]: it is left alone.)
    left = [] if qv else ["R2C2_Consensus.fastq", "R2C2_Consensus.fastq.gz"]
    assert sorted(os.listdir(out + "SplA")) == sorted(want + left)
    assert [os.path.getsize(out + "SplA/" + f) for f in want] == [0] * len(want)
    assert os.listdir(out) == ["SplA"]                                 # the splint nobody used gets no directory
    made = ["R2C2_Consensus.fasta.gz", "R2C2_Subreads.fastq.gz"] + ["R2C2_Consensus.fastq.gz"] * qv       # in the order they were made
    assert tree.gz_made == ([out + "SplA/" + f for f in made] if mode == "bgzf" else [])


def test_paths_and_emit_order(tmp_path):
    out, tree = _tree(tmp_path, "plain", False)
    assert tree.names == NAMES
    assert tree.cons_paths == tree.cons_w == [out + "SplA/R2C2_Consensus.fasta", out + "SplB/R2C2_Consensus.fasta"]
    assert tree.sub_paths == tree.sub_w == [out + "SplA/R2C2_Subreads.fastq", out + "SplB/R2C2_Subreads.fastq"]
    assert tree.fq_paths == tree.fq_w == []
    assert tree.emit_paths == [out + "SplA/R2C2_Consensus.fasta", out + "SplA/R2C2_Subreads.fastq",
                               out + "SplB/R2C2_Consensus.fasta", out + "SplB/R2C2_Subreads.fastq"]
    out, tree = _tree(tmp_path, "co", True)                           # -co writes plain files; stream s * 3 + kind with QVs
    assert tree.fq_paths == tree.fq_w == [out + "SplA/R2C2_Consensus.fastq", out + "SplB/R2C2_Consensus.fastq"]
    assert tree.emit_paths == [out + "SplA/R2C2_Consensus.fasta", out + "SplA/R2C2_Subreads.fastq", out + "SplA/R2C2_Consensus.fastq",
                               out + "SplB/R2C2_Consensus.fasta", out + "SplB/R2C2_Subreads.fastq", out + "SplB/R2C2_Consensus.fastq"]
    out, tree = _tree(tmp_path, "bgzf", True)
    assert tree.cons_paths == [out + "SplA/R2C2_Consensus.fasta", out + "SplB/R2C2_Consensus.fasta"]
    assert tree.cons_w == [out + "SplA/R2C2_Consensus.fasta.gz", out + "SplB/R2C2_Consensus.fasta.gz"]
    assert tree.emit_paths == [out + "SplA/R2C2_Consensus.fasta.gz", out + "SplA/R2C2_Subreads.fastq.gz", out + "SplA/R2C2_Consensus.fastq.gz",
                               out + "SplB/R2C2_Consensus.fasta.gz", out + "SplB/R2C2_Subreads.fastq.gz", out + "SplB/R2C2_Consensus.fastq.gz"]


@pytest.mark.parametrize("qv", [False, True])
def test_finish_plain_leaves_the_files_alone(tmp_path, qv):
    out, tree = _tree(tmp_path, "plain", qv)
    tree.prepare({"SplA"})
    _put(out + "SplA/R2C2_Consensus.fasta", b">r\nACGT\n")
    tree.finish()
    assert sorted(os.listdir(out + "SplA")) == (PLAIN_QV if qv else PLAIN)
    assert _get(out + "SplA/R2C2_Consensus.fasta") == b">r\nACGT\n" and _get(out + "SplA/R2C2_Subreads.fastq") == b""


@pytest.mark.parametrize("qv", [False, True])
def test_finish_bgzf_appends_the_eof_member_once_to_what_prepare_made(tmp_path, qv):
    assert _lib.BGZF_EOF == EOF
    out, tree = _tree(tmp_path, "bgzf", qv)
    tree.prepare({"SplA"})
    _put(out + "SplA/R2C2_Consensus.fasta.gz", b"members")
    os.remove(out + "SplA/R2C2_Subreads.fastq.gz")                     # made by prepare, gone since: not made again
    _put(out + "SplA/other.gz", b"x")                                  # not made by prepare: not touched
    tree.finish()
    assert sorted(os.listdir(out + "SplA")) == ["R2C2_Consensus.fasta.gz"] + ["R2C2_Consensus.fastq.gz"] * qv + ["other.gz"]
    assert _get(out + "SplA/R2C2_Consensus.fasta.gz") == b"members" + EOF
    assert _get(out + "SplA/other.gz") == b"x"
    if qv:
        assert _get(out + "SplA/R2C2_Consensus.fastq.gz") == EOF


@pytest.mark.parametrize("qv", [False, True])
def test_finish_co_gzips_every_file_and_removes_the_plain_one(tmp_path, qv):
    out, tree = _tree(tmp_path, "co", qv)
    tree.prepare({"SplA"})
    data = {"R2C2_Consensus.fasta": b">r\nACGT\n" * 1000, "R2C2_Subreads.fastq": b"", "R2C2_Consensus.fastq": b"@r\nACGT\n+\nIIII\n"}
    for f in (PLAIN_QV if qv else PLAIN):
        _put(out + "SplA/" + f, data[f])
    tree.finish()
    assert sorted(os.listdir(out + "SplA")) == (GZ_QV if qv else GZ) and os.listdir(out) == ["SplA"]
    for f in (PLAIN_QV if qv else PLAIN):
        assert gzip.decompress(_get(out + "SplA/" + f + ".gz")) == data[f]


@pytest.mark.parametrize("qv", [False, True])
@pytest.mark.parametrize("mode", ["plain", "co", "bgzf"])
def test_fused_finish_drops_the_unseen_splint_before_the_eof_members_and_renames_the_psl(tmp_path, mode, qv):
    psl = str(tmp_path) + "/finder.psl"
    out, tree = _tree(tmp_path, mode, qv, finder_psl=psl)
    tree.prepare(set())                                                # nothing is known yet: every splint gets its files
    gz = ".gz" if mode == "bgzf" else ""
    want = {"": PLAIN_QV if qv else PLAIN, ".gz": GZ_QV if qv else GZ}
    assert sorted(os.listdir(out)) == NAMES and sorted(os.listdir(out + "SplB")) == want[gz]
    assert _get(psl + ".part") == b"" and not os.path.exists(psl)
    _put(psl + ".part", b"psl rows\n")
    _put(out + "SplA/R2C2_Consensus.fasta" + gz, b"bytes")
    tree.finish({"SplA"})
    # SplB's files were empty, so they and the directory are gone -- under --bgzf only because this comes BEFORE the EOF members
    assert os.listdir(out) == ["SplA"]
    assert _get(psl) == b"psl rows\n" and not os.path.exists(psl + ".part")
    assert sorted(os.listdir(out + "SplA")) == want["" if mode == "plain" else ".gz"]
    got = _get(out + "SplA/R2C2_Consensus.fasta" + ("" if mode == "plain" else ".gz"))
    assert (gzip.decompress(got) if mode == "co" else got) == (b"bytes" + EOF if mode == "bgzf" else b"bytes")
    if mode == "bgzf":                                                 # a seen splint's empty .gz still gets its EOF member
        assert _get(out + "SplA/R2C2_Subreads.fastq.gz") == EOF


def test_fused_finish_keeps_an_unseen_directory_that_holds_something(tmp_path):
    psl = str(tmp_path) + "/finder.psl"
    out, tree = _tree(tmp_path, "plain", False, finder_psl=psl)
    tree.prepare(set())
    _put(out + "SplB/R2C2_Subreads.fastq", b"not empty")
    tree.finish(set())
    assert sorted(os.listdir(out)) == ["SplB"] and os.listdir(out + "SplB") == ["R2C2_Subreads.fastq"]

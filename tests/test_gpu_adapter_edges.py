"""k_adapter at its edges: the 64-column chunk seams, gaps across them, equal maxima, and waves that take several items from the
queue one after the other.  Every batch of adapter_edge_cases.py is scanned (Handle.set_splints / upload / scan_adapters) and
the table must equal the oracle's bit for bit over all (read, adapter, strand); test_adapter_oracle_host.py shows that the
oracle is the first optimum of the textbook recurrence on the same batches and that every designed case reaches the code it
is for.  All runs poison fresh device memory (C3_DEBUG_POISON): a direction byte nobody wrote does not read as zero."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

import adapter_edge_cases as AC

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _handle(**cfg):
    """a Handle whose whole lifetime runs under C3_DEBUG_POISON=1; the variable is restored afterwards"""
    from c3poa_amd import _lib
    keep = os.environ.get("C3_DEBUG_POISON")
    os.environ["C3_DEBUG_POISON"] = "1"
    h = None
    try:
        h = _lib.Handle(**cfg)
        yield h
    finally:
        if h is not None:
            h.close()
        if keep is None:
            os.environ.pop("C3_DEBUG_POISON", None)
        else:
            os.environ["C3_DEBUG_POISON"] = keep


def _scan(h, adapters, reads):
    h.set_splints(adapters)
    h.upload(reads, ["!" * len(r) for r in reads], "?" * len(reads))
    return h.scan_adapters()


def _assert_equal(b, tab, exp):
    bad = np.argwhere((tab != exp).any(axis=3))
    assert bad.size == 0, (b.name, [(i, len(b.reads[i]), len(b.adapters[a]), s, tab[i, a, s].tolist(), exp[i, a, s].tolist()) for i, a, s in bad[:4].tolist()])
    assert np.array_equal(tab, exp)


GROUPS = AC.groups()


def _check_group(name):
    for b in GROUPS[name]:
        assert b.scratch_bytes(1 << 20) < (1 << 30), b
        with _handle() as h:
            tab = _scan(h, b.adapters, b.reads)
        _assert_equal(b, tab, AC.oracle_table(b))
        AC.check_table(b, tab)


def test_seams():
    """adapters of 1, 2, 63 .. 65, 127 .. 129, 191 .. 193, 511 and 512 bases; exact, substituted at columns 64 / 65 / 128 / 129,
    shorter reads, an empty read: the diagonal and left-neighbour carries from lane 63 to lane 0 of the next chunk"""
    _check_group("seams")


def test_hgaps():
    """one horizontal gap of 1 .. 20 columns around a seam, and of 80 columns over a whole chunk: the carried prefix maximum"""
    _check_group("hgaps")


def test_vgaps():
    """one vertical gap of 1 .. 40 rows after columns 63, 64 and 100: the extend flag and E row at the last lane / first lane"""
    _check_group("vgaps")


def test_ties():
    """the first maximum in row-major order among equal ones in other rows, other chunks, other lanes; no positive cell at all"""
    _check_group("ties")


def _cu_count():
    """torch.cuda.get_device_properties(0).multi_processor_count, asked in a child process: torch brings a HIP runtime of its
    own, which finds no device in a process where the library's runtime is already at work"""
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         stdout=subprocess.PIPE, timeout=120, check=True).stdout
    cus = int(out.split()[-1])
    assert 1 <= cus <= 4096, cus
    return cus


def test_queue_reuses_waves():
    """at least three items per wave of the launch (grid = min(items, 16 * CUs)): every wave re-initialises its LDS rows and
    reuses its direction bytes under another row stride; a second scan of the same handle starts from a fresh queue counter"""
    cus = _cu_count()
    b = AC.queue(16 * cus)
    print("queue batch: %d items (%d reads x %d adapters x 2), %d CUs, grid %d" % (b.n_items(), len(b.reads), len(b.adapters), cus, 16 * cus))
    assert b.n_items() >= 3 * 16 * cus
    assert b.scratch_bytes(16 * cus) < (1 << 30)
    with _handle() as h:
        tab = _scan(h, b.adapters, b.reads)
        again = h.scan_adapters()
    _assert_equal(b, tab, AC.oracle_table(b))
    assert np.array_equal(again, tab)
    AC.check_table(b, tab)


def test_row_independent_of_the_table():
    """a (read, adapter, strand) row depends on nothing else in the adapter table: not on the order of the adapters, not on
    the longest one (max_spl sizes each wave's slice of the direction bytes)"""
    for b in GROUPS["seams"]:
        n_ad = len(b.adapters)
        assert n_ad >= 3
        with _handle() as h:
            full = _scan(h, b.adapters, b.reads)
        by_len = sorted(range(n_ad), key=lambda a: len(b.adapters[a]))
        assert len(b.adapters[by_len[1]]) < len(b.adapters[by_len[-1]])          # the subset's longest adapter is shorter
        for order in (list(range(n_ad))[::-1], by_len[:2]):
            with _handle() as h:
                tab = _scan(h, [b.adapters[a] for a in order], b.reads)
            for k, a in enumerate(order):
                assert np.array_equal(tab[:, k], full[:, a]), (b.name, order, k, a)


def test_refused_adapter_tables_leave_the_handle_usable():
    """an adapter of 513 bases or of none is C3_E_LIMIT (the code itself: test_gpu_edge_cases.py pins it at the C ABI for 513);
    the table of the last successful call stays in force, with the scratch sizes that go with it"""
    from c3poa_amd import _lib
    b = GROUPS["seams"][1]
    with _handle() as h:
        tab = _scan(h, b.adapters, b.reads)
        for bad in (["A" * 513], [""], ["ACGT" * 5, ""], ["ACGT" * 5, "C" * 513, "ACGT"]):
            with pytest.raises(_lib.C3Error) as e:
                h.set_splints(bad)
            assert e.value.code == _lib.E_LIMIT and "1..512" in str(e.value)
            assert np.array_equal(h.scan_adapters(), tab), bad
        h.set_splints(b.adapters[:1])                       # and a good table after a refused one
        assert np.array_equal(h.scan_adapters(), tab[:, :1])
    _assert_equal(b, tab, AC.oracle_table(b))

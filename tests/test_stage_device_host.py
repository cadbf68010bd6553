"""CPU tests of the reader's device groups (include/c3poa.h "Groups kept on the device"): the new symbols and the
argument and state checks that need no device.  The device side is tests/test_gpu_stage_device.py."""
import ctypes as C
import pytest

from c3poa_amd import _lib

NEW = ["c3_reader_stage_on_device", "c3_reader_device_group", "c3_reader_stage_stats"]
THREE = b"@a x\nACGTACGT\n+\nIIIIIIII\n@b\nAC\n+\nII\n@c\nGGGTTT\n+\n!!!!!!\n"


def test_symbols_are_exported():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(lib, name)
    assert [f[0] for f in _lib.DeviceBatchStruct._fields_] == ["d_seqs", "d_quals", "device", "bytes"]


def test_null_arguments():
    lib = _lib.load()
    g = _lib.DeviceBatchStruct(None, None, 0, 4)
    assert lib.c3_reader_stage_on_device(None, 1) == _lib.E_ARG
    assert lib.c3_reader_device_group(None, 0, C.byref(g)) == _lib.E_ARG
    assert lib.c3_reader_stage_stats(None, None, None, None) == _lib.E_ARG


def test_reader_state(tmp_path):
    p = str(tmp_path / "three.fastq")
    open(p, "wb").write(THREE)
    lib = _lib.load()
    with pytest.raises(_lib.C3Error) as e:                        # a plain-text reader has no device parser in force
        _lib.Reader(p, stage_device=True)
    assert e.value.code == _lib.E_STATE and "c3_reader_parse_on_device" in str(e.value)
    rd = _lib.Reader(p, n_sets=2)
    assert lib.c3_reader_stage_on_device(rd.r, 1) == _lib.E_STATE
    assert b"c3_reader_stage_on_device" in lib.c3_reader_error(rd.r)
    assert lib.c3_reader_stage_on_device(rd.r, 0) == _lib.E_STATE   # asking to switch it off is the same question
    assert rd.stage_stats() == (0, 0, 0)
    hb = rd.next(10)
    assert hb.n == 3 and hb.dev is None and hb.c.seqs and hb.c.quals            # an ordinary host group, untouched
    g = _lib.DeviceBatchStruct(1, 1, 7, 7)
    assert lib.c3_reader_device_group(rd.r, 0, C.byref(g)) == 0                 # ... which has no device side
    assert (g.d_seqs, g.d_quals, g.device, g.bytes) == (None, None, -1, 0)
    for bad_set in (-1, 2):
        assert lib.c3_reader_device_group(rd.r, bad_set, C.byref(g)) == _lib.E_ARG
    assert lib.c3_reader_device_group(rd.r, 0, None) == _lib.E_ARG
    assert lib.c3_reader_stage_on_device(rd.r, 1) == _lib.E_STATE               # and after the first group it is too late anyway
    assert rd.stage_stats() == (0, 0, 0) and rd.reserved_bytes() > 0
    rd.close()

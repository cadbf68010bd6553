"""CPU tests of what every wrapper of c3poa_amd/_lib.py shares: the guarded output arrays, the error path and the owner base."""
import ctypes as C

import numpy as np
import pytest

from c3poa_amd import _lib


class _Info(_lib._Info):
    _fields_ = [("n", C.c_int64)]


class _Out:
    pass


def _write(ptr, at, n, value=0x11):
    """what a C call does: n bytes at ptr + at"""
    if n:
        C.memset(ptr + at, value, n)


@pytest.mark.parametrize("size", [0, 1, 65])
def test_guarded_outputs_with_a_fake_call(size):
    """a call that writes exactly `used` bytes leaves both findings true; one byte past `used` makes untouched_beyond_results false
    (also where that byte is the first of the back guard: used == size); a byte of either guard makes guards_intact false"""
    G = _lib.GUARD
    assert G == 64 == _lib.FASTQ_GUARD == _lib.FASTA_GUARD
    for used in sorted({0, size // 2, size}):
        o = _lib._Outputs({"a": size, "b": 8})
        assert o.cap("a") == size and all(bool((v == 0xA5).all()) and len(v) == o.cap(k) + 2 * G for k, v in o.arr.items())
        assert o.ptr["a"] == o.arr["a"].ctypes.data + G
        _write(o.ptr["a"], 0, used)
        assert o.check({"a": used}) == (True, True)
        out = _Out()
        o.settle(out, 0, None, _Info(used), {"a": used, "b": 0})
        assert (out.guards_intact, out.untouched_beyond_results, out.info) == (True, True, {"n": used})
        o.take(out, a=None)
        assert out.a == b"\x11" * used and o.view("a").tobytes() == out.a

        o = _lib._Outputs({"a": size, "b": 8})
        _write(o.ptr["a"], 0, used + 1)                                    # one byte past the results
        assert o.check({"a": used}) == (used < size, False)               # ... which is a guard byte when the results fill the array
        assert o.check({"a": used + 1})[1] is True

    for at in (-1, -G, size, size + G - 1):                                # the last / first byte of the front guard, the back guard
        o = _lib._Outputs({"a": size, "b": 8})
        _write(o.ptr["a"], at, 1)
        assert o.check({"a": size})[0] is False, at
    o = _lib._Outputs({"a": size, "b": 8})
    _write(o.ptr["b"], 8, 1)                                               # any array of the set counts
    assert o.check({"a": 0}) == (False, False)


def test_guarded_outputs_slices_and_refusal():
    """take() gives bytes, an int64 copy or a uint64 copy of the used part; a refused call (rc != 0) counts every byte as beyond the
    results and raises with .code, .info, .guards_intact, .untouched and the caller's attributes"""
    o = _lib._Outputs({"out": 2})                                           # an array may be called what take() calls its object
    o.settle(_Out(), 0, None, _Info(0), {"out": 2})
    res = _Out()
    o.take(res, out=None)
    assert res.out == b"\xa5\xa5"
    o = _lib._Outputs({"t": 5, "i": 24, "u": 16})
    C.memmove(o.ptr["t"], b"hello", 5)
    for k, dt, vals in (("i", np.int64, [-1, 2]), ("u", np.uint64, [2 ** 64 - 1, 7])):
        a = np.array(vals, dtype=dt)
        C.memmove(o.ptr[k], a.ctypes.data, 16)
    out = _Out()
    o.settle(out, 0, None, _Info(2), {"t": 5, "i": 16, "u": 16}, intact=False)
    assert out.guards_intact is False and out.untouched_beyond_results is True        # `intact`: a guard of the caller's own
    o.take(out, t=None, i=np.int64, u=np.uint64)
    assert out.t == b"hello" and out.i.dtype == np.int64 and out.i.tolist() == [-1, 2]
    assert out.u.dtype == np.uint64 and out.u.tolist() == [2 ** 64 - 1, 7]
    out.i[0] = 5                                                            # copies: the arrays are not views of the guarded ones
    assert o.view("i").view(np.int64)[0] == -1

    for wrote, untouched in ((0, True), (1, False)):
        o = _lib._Outputs({"t": 5})
        _write(o.ptr["t"], 0, wrote)
        with pytest.raises(_lib.C3Error) as e:
            o.settle(_Out(), _lib.E_LIMIT, lambda: b"too small", _Info(9), {"t": 5}, stream_off=[0])
        assert str(e.value) == "c3 error -6: too small" and e.value.code == _lib.E_LIMIT and e.value.info == {"n": 9}
        assert (e.value.guards_intact, e.value.untouched, e.value.stream_off) == (True, untouched, [0])

    keep = {}
    o = _lib._Outputs({"t": 5}, keep=keep)                                  # kept arrays: no guards, grow only, nothing to find
    first = keep["t"]
    assert o.cap("t") == 5 == len(first) and o.ptr["t"] == first.ctypes.data and o.check({"t": 0}) == (True, True)
    assert _lib._Outputs({"t": 3}, keep=keep).arr["t"] is first and _lib._Outputs({"t": 6}, keep=keep).cap("t") == 6


def test_one_error_path_for_the_three_sources():
    """_c3_error gives .code == rc and the exact message for c3_last_error(h), c3_last_error(NULL) and c3_reader_error(r)"""
    lib = _lib.load()
    with pytest.raises(_lib.C3Error) as e:
        _lib.Handle(poa_match=0)                                            # refused before a device is looked for
    text = lib.c3_last_error(None).decode()
    assert "poa_match = 0" in text and e.value.code == _lib.E_ARG and str(e.value) == "c3_create failed (-3): " + text
    err = _lib._c3_error(-3)                                                # c3_last_error(NULL)
    assert str(err) == "c3 error -3: " + text and err.code == -3 and isinstance(err, RuntimeError)

    h = _lib.Handle.__new__(_lib.Handle)                                    # Handle._chk: c3_last_error(h), here of a null handle
    h.lib, h.h = lib, C.c_void_p()
    with pytest.raises(_lib.C3Error) as e:
        h._chk(-5)
    assert str(e.value) == "c3 error -5: " + text and e.value.code == -5
    assert h._chk(0) == 0 and h._chk(7) == 7

    r = _lib.Reader(__file__)                                               # c3_reader_error(r): a refused c3_reader_parse_on_device
    rc = lib.c3_reader_parse_on_device(r.r, 1)
    rtext = lib.c3_reader_error(r.r).decode()
    assert rc == _lib.E_STATE and rtext
    err = _lib._c3_error(rc, r._err, "c3_reader_parse_on_device")
    assert str(err) == "c3_reader_parse_on_device failed (-5): " + rtext and err.code == rc
    r.close()
    with pytest.raises(_lib.C3Error) as e:
        _lib.Reader(__file__, parse_device=True)
    assert str(e.value) == str(err) and e.value.code == _lib.E_STATE

    err = _lib._c3_error(-6, False, "c3_batch_emit_fetch", stream_off=3)    # a call that leaves no text
    assert str(err) == "c3_batch_emit_fetch failed (-6)" and err.code == -6 and err.stream_off == 3


@pytest.mark.parametrize("call,args", [(_lib.demux_host, ([b"A" * 300], [b"ACGT"], [b"ACGT", b"TTGA"])),
                                       (_lib.consensus_qv_host, ("", [])), (_lib.bgzf_decompress_host, (b"not bgzf",))])
def test_host_refusals_carry_their_code(call, args):
    with pytest.raises(_lib.C3Error) as e:
        call(*args)
    assert e.value.code in (_lib.E_ARG, _lib.E_DATA) and str(e.value).startswith("c3 error %d: " % e.value.code)
    assert str(e.value) == "c3 error %d: %s" % (e.value.code, _lib.load().c3_last_error(None).decode())


def test_owner_base_closes_once():
    """close() twice, then __del__ after close(); `with` closes on the way out"""
    pb = _lib.PinnedBytes(100)
    assert isinstance(pb, _lib._Owned) and pb.size == 100 and len(pb.arr) == 100 and pb.ptr
    pb.arr[:] = 7
    pb.close()
    assert pb.arr is None and not pb._p
    pb.close()
    pb.__del__()
    with _lib.PinnedBytes(1) as q:
        assert q.ptr and q.arr is not None
    assert q.arr is None and not q._p
    for cls in (_lib.Handle, _lib.ResultBuffers, _lib.PinnedBatch, _lib.Reader, _lib.Assigner, _lib.PinnedBytes, _lib.Bgzf):
        assert issubclass(cls, _lib._Owned) and "__del__" not in vars(cls) and "close" not in vars(cls), cls
    _lib.Reader.__new__(_lib.Reader).__del__()                             # an object whose __init__ never ran: nothing raised
    rb = _lib.ResultBuffers(pinned=True)
    res, buf, coff = rb.fit(3, 10)
    first = dict(rb._p)
    rb.fit(300, 1000)                                                      # grown: the old blocks are retired, not yet freed
    assert len(rb._retired) == 3 and all(p in rb._retired for p in first.values())
    rb.fit(3, 10)                                                          # the next fit() frees them
    assert rb._retired == []
    rb.close()
    rb.close()
    assert rb._p == {} and rb.res is None

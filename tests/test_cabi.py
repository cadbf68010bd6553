"""CPU tests of the C-ABI shared library: it loads, exports every symbol declared in
include/c3poa.h, and fails loudly (no CPU fallback) when there is no GPU.  No compute calls."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "c3poa.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(c3_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from c3poa_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), "missing export %s" % n
    assert set(_lib.EXPORTS) <= set(names)


def _header():
    """(prototypes {name: (return type, [parameter types])}, structs {name: [(field, type, is_array)]}) of include/c3poa.h.  A
    statement that is none of a prototype, a struct, an enum or an opaque typedef is an AssertionError naming it."""
    txt = open(os.path.join(ROOT, "include", "c3poa.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"^\s*#.*$", " ", txt, flags=re.M)
    txt = re.sub(r'extern\s+"C"\s*\{', " ", txt).rstrip()
    assert txt.endswith("}"), txt[-40:]
    txt = txt[:-1]
    structs = {}

    def struct(m):
        fields = []
        for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
            first, *more = [p.strip() for p in decl.split(",")]
            f = re.fullmatch(r"(.*[\s*])(\w+)\s*(\[[^\]]*\])?", first)
            assert f, "unreadable field %r of %s" % (decl, m.group(2))
            fields.append((f.group(2), f.group(1).strip(), bool(f.group(3))))
            for p in more:
                g = re.fullmatch(r"(\w+)\s*(\[[^\]]*\])?", p)
                assert g, "unreadable field %r of %s" % (decl, m.group(2))
                fields.append((g.group(1), f.group(1).strip(), bool(g.group(2))))
        structs[m.group(2)] = fields
        return " "

    txt = re.sub(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", struct, txt, flags=re.S)
    txt = re.sub(r"typedef\s+enum\s*\{[^}]*\}\s*\w+\s*;", " ", txt)
    protos = {}
    for stmt in filter(None, (" ".join(s.split()) for s in txt.split(";"))):
        if re.fullmatch(r"typedef struct (\w+) \1", stmt):
            continue
        m = re.fullmatch(r"([\w\s*]+?[\s*])(c3_\w+) ?\(([^()]*)\)", stmt)
        assert m, "unreadable declaration: %r" % stmt
        params = [] if m.group(3).strip() == "void" else [p.strip() for p in m.group(3).split(",")]
        types = []
        for p in params:
            t = re.fullmatch(r"(.*[\s*])(\w+)", p)
            assert t, "unreadable parameter %r of %s" % (p, m.group(2))
            types.append(t.group(1).strip())
        assert m.group(2) not in protos, m.group(2)
        protos[m.group(2)] = (m.group(1).strip(), types)
    return protos, structs


def _c_class(ctype):
    """the class of a C type of the header: ptr, i32, i64, f32, f64 or void"""
    if "*" in ctype:
        return "ptr"
    t = ctype.replace("const", "").strip()
    assert t in ("int", "int32_t", "int64_t", "float", "double", "void"), "a type the test does not know: %r" % ctype
    return {"int": "i32", "int32_t": "i32", "int64_t": "i64", "float": "f32", "double": "f64", "void": "void"}[t]


def _ctypes_class(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "ptr"
    for k, ts in (("i32", (C.c_int, C.c_int32)), ("i64", (C.c_int64,)), ("f32", (C.c_float,)), ("f64", (C.c_double,))):
        if t in ts:
            return k
    raise AssertionError("a ctypes type the test does not know: %r" % (t,))


def test_prototype_table_agrees_with_the_header():
    """every entry of the binding's prototype table against the declaration of include/c3poa.h: the number of parameters, and the
    class of every parameter and of the return value (int / int32_t: c_int or c_int32; int64_t: c_int64; double: c_double; any
    pointer: a pointer type; void: None; const char* returned: c_char_p).  load() applies exactly this table, and EXPORTS is
    its key list."""
    from c3poa_amd import _lib
    protos, _structs = _header()
    assert len(protos) >= 100
    assert list(_lib._PROTOTYPES) == _lib.EXPORTS and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS)
    assert set(_lib._PROTOTYPES) == set(protos), sorted(set(_lib._PROTOTYPES) ^ set(protos))
    lib = _lib.load()
    for name, (ret, params) in protos.items():
        restype, argtypes = _lib._PROTOTYPES[name]
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        assert len(argtypes) == len(params), (name, len(argtypes), params)
        assert _ctypes_class(restype) == _c_class(ret), (name, ret, restype)
        if _c_class(ret) == "ptr":
            assert " ".join(ret.split()) == "const char*" and restype is C.c_char_p, (name, ret, restype)
        for k, (p, a) in enumerate(zip(params, argtypes)):
            assert _ctypes_class(a) == _c_class(p), (name, k, p, a)


def test_structures_agree_with_the_header():
    """every struct of include/c3poa.h against its ctypes Structure: the field names in order and the class of every field (the
    rule of the prototype test, with float: c_float).  c3_read_result has arrays: its names are compared here, its size in
    test_default_config_matches_reference_call_sites and against RESULT_DTYPE at import."""
    from c3poa_amd import _lib
    _protos, structs = _header()
    binding = {"c3_config": _lib.Config, "c3_read_result": _lib.ReadResult, "c3_timing": _lib.Timing, "c3_host_batch": _lib.HostBatchStruct,
               "c3_qv_timing": _lib.QvTiming, "c3_fastq_info": _lib.FastqInfo, "c3_bam_info": _lib.BamInfo, "c3_post_args": _lib.PostArgs,
               "c3_post_timing": _lib.PostTiming, "c3_fasta_info": _lib.FastaInfo, "c3_demux_info": _lib.DemuxInfo,
               "c3_demux_timing": _lib.DemuxTiming, "c3_emit_timing": _lib.EmitTiming, "c3_fastx_info": _lib.FastxInfo,
               "c3_post_text_info": _lib.PostTextInfo, "c3_post_text_timing": _lib.PostTextTiming, "c3_demux_sets": _lib.DemuxSetsStruct,
               "c3_demux_text_info": _lib.DemuxTextInfo, "c3_demux_text_timing": _lib.DemuxTextTiming,
               "c3_device_batch": _lib.DeviceBatchStruct}
    assert set(structs) == set(binding), sorted(set(structs) ^ set(binding))
    for name, fields in structs.items():
        got = binding[name]._fields_
        assert [f[0] for f in got] == [f[0] for f in fields], name
        for (fname, ctype, is_array), (_n, t) in zip(fields, got):
            if is_array:
                assert name == "c3_read_result" and issubclass(t, C.Array) and _ctypes_class(t._type_) == _c_class(ctype), (name, fname)
            else:
                assert _ctypes_class(t) == _c_class(ctype), (name, fname, ctype, t)


def test_default_config_matches_reference_call_sites():
    from c3poa_amd import _lib
    c = _lib.default_config()
    assert (c.conk_penalty, c.sg_iters, c.sg_window, c.sg_order) == (20, 3, 41, 2)       # C3POa.py:111
    assert c.mdistcutoff == 500 and c.poa_match == 5                                         # C3POa.py:45, determine_consensus.py:30
    assert (c.poa_mismatch, c.poa_o1, c.poa_e1, c.poa_o2, c.poa_e2, c.poa_band_b) == (4, 4, 2, 24, 1, 10)
    assert abs(c.poa_band_f - 0.01) < 1e-15
    assert (c.pol_window, c.pol_q) == (500, 5)                                               # racon -q 5
    assert C.sizeof(_lib.ReadResult) == 4 * (10 + 3 * 256)


def test_no_gpu_means_loud_failure_not_fallback():
    import torch
    from c3poa_amd import _lib
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.C3Error) as e:
        _lib.Handle()
    assert "no CPU fallback" in str(e.value)


POA_RANGES = {"poa_match": (1, 64), "poa_mismatch": (0, 64), "poa_o1": (0, 64), "poa_e1": (0, 16), "poa_o2": (0, 64), "poa_e2": (0, 16)}


@pytest.mark.parametrize("field", sorted(POA_RANGES))
def test_create_refuses_poa_scoring_outside_the_exact_range(field):
    """the ranges of DESIGN.md 4.3 / include/c3poa.h: the first value beyond either end of every POA scoring field is refused with
    C3_E_ARG and a message naming the field and its bounds; the ends themselves are not (the scoring is checked before a device
    is looked for, so this needs no GPU; that the ends compute what the oracle computes: tests/test_gpu_poa_scoring.py)"""
    from c3poa_amd import _lib
    lo, hi = POA_RANGES[field]
    for v in (lo - 1, hi + 1, -1000, 1 << 20):
        with pytest.raises(_lib.C3Error) as e:
            _lib.Handle(**{field: v})
        assert e.value.code == _lib.E_ARG, (field, v, str(e.value))
        assert "%s = %d" % (field, v) in str(e.value) and "%d..%d" % (lo, hi) in str(e.value)
    for v in (lo, hi):
        try:
            _lib.Handle(**{field: v}).close()
        except _lib.C3Error as err:                       # without a GPU the accepted value gets as far as the device query
            assert err.code != _lib.E_ARG and "no CPU fallback" in str(err), (field, v, str(err))


POL_MAX = 8191


def _create(**cfg):
    """None if c3_create gets past its argument checks (without a GPU: as far as the device query), else the C3_E_ARG error"""
    from c3poa_amd import _lib
    try:
        _lib.Handle(**cfg).close()
    except _lib.C3Error as err:
        if err.code == _lib.E_ARG:
            return err
        assert "no CPU fallback" in str(err), (cfg, str(err))
    return None


@pytest.mark.parametrize("field", ["pol_gap", "pol_match", "pol_mismatch"])
def test_create_refuses_polish_scoring_outside_the_exact_range(field):
    """the range of DESIGN.md 4.6a / include/c3poa.h: the first value beyond either end of every polish scoring field is refused
    with C3_E_ARG and a message naming the field and its bounds; the ends themselves are not (checked before a device is looked
    for, so this needs no GPU; that the ends compute what the oracle computes: tests/test_gpu_pol_scoring.py).  The other two
    fields are set so that the match stays above two gaps."""
    other = {"pol_gap": dict(pol_match=POL_MAX), "pol_match": dict(pol_gap=-POL_MAX), "pol_mismatch": {}}[field]
    for v in (-POL_MAX - 1, POL_MAX + 1, -1000000, 1000000, -(1 << 31), (1 << 31) - 1):
        err = _create(**other, **{field: v})
        assert err is not None, (field, v)
        assert "%s = %d" % (field, v) in str(err) and "%d..%d" % (-POL_MAX, POL_MAX) in str(err), str(err)
    lo, hi = {"pol_gap": (-POL_MAX, 4095), "pol_match": (-POL_MAX, POL_MAX), "pol_mismatch": (-POL_MAX, POL_MAX)}[field]
    for v in (lo, hi, 0):
        assert _create(**other, **{field: v}) is None, (field, v)


@pytest.mark.parametrize("match,gap,ok", [(3, 1, True), (3, 2, False), (-7, -4, True), (-8, -4, False), (0, -1, True), (-2, -1, False),
                                          (-14, -1, False), (3, 8191, False), (-8191, -4, False), (8191, 4095, True), (8191, 4096, False)])
def test_create_refuses_a_match_that_does_not_beat_two_gaps(match, gap, ok):
    """pol_match > 2 * pol_gap: with the other two fields at their defaults the last admitted values are
    pol_gap = 1 and pol_match = -7"""
    err = _create(pol_match=match, pol_gap=gap)
    assert (err is None) == ok, (match, gap, str(err))
    if err is not None:
        assert "pol_match = %d" % match in str(err) and "2 * pol_gap = %d" % (2 * gap) in str(err), str(err)


POL_WINDOW_MAX = 18458


def test_create_refuses_a_window_length_outside_the_exact_range():
    """the range of DESIGN.md 4.6b / include/c3poa.h: pol_window 1 .. 18 458.  Below it run_polish would divide by zero or size
    negative capacities, above it a window graph's node ids leave the 16 bits k_window's consensus keeps them in.  Refused with
    C3_E_ARG and a message naming the field and its bounds, before a device is looked for; the ends themselves are not (that
    they compute what the oracle computes: tests/test_gpu_pol_window.py)"""
    assert POL_WINDOW_MAX == (65534 - 40 * (250 + 4)) // 3
    for v in (0, POL_WINDOW_MAX + 1, -1, -500, 100000, -(1 << 31), (1 << 31) - 1):
        err = _create(pol_window=v)
        assert err is not None, v
        assert "pol_window = %d" % v in str(err) and "%d..%d" % (1, POL_WINDOW_MAX) in str(err), str(err)
    for v in (1, POL_WINDOW_MAX, 500):
        assert _create(pol_window=v) is None, v


def test_create_refuses_a_negative_extension_band():
    """dang_band 0 is the diagonal alone (a band of one offset, which the kernel's rows and the oracle both define); a negative
    half width is no band.  Refused with C3_E_ARG before a device is looked for (the upper end, 255, is a capacity of k_prep
    and refused with C3_E_LIMIT: tests/test_gpu_prep_rows.py)"""
    for v in (-1, -128, -(1 << 31)):
        err = _create(dang_band=v)
        assert err is not None, v
        assert "dang_band = %d" % v in str(err) and "0..255" in str(err), str(err)
    for v in (0, 1, 128, 255):
        assert _create(dang_band=v) is None, v


def test_product_never_imports_the_oracle():
    """the oracle is test infrastructure: nothing under c3poa_amd/ or the CLI may reference it"""
    bad = []
    for base, _d, files in os.walk(os.path.join(ROOT, "c3poa_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(base, f), errors="ignore").read()
                if re.search(r"(from|import)\s+oracle|libc3oracle|c3o_[a-z]+\s*\(", txt):
                    bad.append(f)
    txt = open(os.path.join(ROOT, "C3POa.py")).read()
    if re.search(r"(from|import)\s+oracle|libc3oracle", txt):
        bad.append("C3POa.py")
    assert not bad, bad

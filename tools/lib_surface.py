"""The visible surface of two versions of c3poa_amd/_lib.py side by side (for a change that must keep it):

    git show HEAD~1:c3poa_amd/_lib.py > /tmp/_lib_parent.py
    python tools/lib_surface.py /tmp/_lib_parent.py c3poa_amd/_lib.py

Compares the public module names, inspect.signature of every public function and method (and of _demux_args, _post_call,
__init__ and _chk), _fields_ of every Structure, and (restype, argtypes) of every export of the first file after load();
prints one line per kind, with the differences.  Both files load the built library of this tree."""
import ctypes as C
import importlib.util
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("C3POA_LIB", os.path.join(ROOT, "c3poa_amd", "lib", "libc3poa_hip.so"))


def tn(t):
    return None if t is None else t.__name__


def surface(path, exports=None):
    spec = importlib.util.spec_from_file_location("lib_surface_%d" % len(sys.modules), path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    s = {"names": {n: None for n in vars(m) if not n.startswith("_")}, "signatures": {}, "fields": {}, "prototypes": {}}
    for n in list(s["names"]) + ["_demux_args", "_post_call"]:
        o = getattr(m, n)
        if inspect.isfunction(o):
            s["signatures"][n] = str(inspect.signature(o))
        elif inspect.isclass(o):
            if issubclass(o, C.Structure):
                s["fields"][n] = [(f[0], tn(f[1])) for f in o._fields_]
            for k, v in inspect.getmembers(o, inspect.isfunction):
                if not k.startswith("_") or k in ("__init__", "_chk"):
                    s["signatures"]["%s.%s" % (n, k)] = str(inspect.signature(v))
    lib = m.load()
    for n in exports or m.EXPORTS:
        f = getattr(lib, n)
        s["prototypes"][n] = (tn(f.restype), None if f.argtypes is None else [tn(a) for a in f.argtypes])
    return s, list(m.EXPORTS)


if __name__ == "__main__":
    a, exports = surface(sys.argv[1])
    b, exports_b = surface(sys.argv[2], exports)
    print("exports: %d, %s" % (len(exports), "same names" if sorted(exports) == sorted(exports_b) else "DIFFERENT names"))
    for kind in a:
        diff = {k: (a[kind].get(k, "absent"), b[kind].get(k, "absent")) for k in {**a[kind], **b[kind]} if a[kind].get(k, "absent") != b[kind].get(k, "absent")}
        print("%s: %d, %s" % (kind, len(a[kind]), "equal" if not diff else "%d differ: %s" % (len(diff), diff)))

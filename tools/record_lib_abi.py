#!/usr/bin/env python3
"""Records the public surface of jxl_rs_amd.lib as tests/golden/lib_public_abi.json, which tests/test_py_binding.py holds
every later jxl_rs_amd.lib to: each public module-level name with its kind; the value of every integer constant (and of
the small dicts and lists of names); for every ctypes.Structure its [field, ctypes type name, offset, size] rows; for
every function of the loaded library that carries a signature its per-argument classes (i4, i8, f4, ptr) and its
return class.  Run it on the commit whose surface is to be pinned; it needs the built library and no GPU.

  python tools/record_lib_abi.py [--check] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def type_class(t):
    """i4 / i8 / f4 for the scalars by width, ptr for everything that travels as an address, void for no result"""
    if t is None:
        return "void"
    if isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ not in "PzZ":
        return ("f" if t._type_ in "fd" else "i") + str(C.sizeof(t))
    return "ptr"


def struct_rows(cls):
    return [[f[0], f[1].__name__, getattr(cls, f[0]).offset, getattr(cls, f[0]).size] for f in cls._fields_]


def snapshot(lib):
    names = {}
    for name, v in sorted(vars(lib).items()):
        if name.startswith("_"):
            continue
        if isinstance(v, bool) or not isinstance(v, (int, str, list, dict, type, types.ModuleType, types.FunctionType)):
            names[name] = {"kind": type(v).__name__}
        elif isinstance(v, int):
            names[name] = {"kind": "int", "value": v}
        elif isinstance(v, dict):
            names[name] = {"kind": "dict", "value": {str(k): x for k, x in v.items()}}
        elif isinstance(v, list):
            names[name] = {"kind": "list", "value": sorted(v)}
        elif isinstance(v, type) and issubclass(v, C.Structure):
            names[name] = {"kind": "struct", "size": C.sizeof(v), "fields": struct_rows(v)}
        else:
            names[name] = {"kind": "class" if isinstance(v, type) else type(v).__name__}
    L = lib.load()
    functions = {}
    for name in lib.ABI_SYMBOLS + lib.DEV_SYMBOLS:
        fn = getattr(L, name, None)
        if fn is not None and (fn.argtypes is not None or fn.restype is not C.c_int):
            functions[name] = {"args": None if fn.argtypes is None else [type_class(t) for t in fn.argtypes],
                               "ret": type_class(fn.restype)}
    return {"names": names, "functions": functions}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare against the file instead of writing it")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lib_public_abi.json"))
    a = ap.parse_args()
    from jxl_rs_amd import lib
    got = snapshot(lib)
    n = sum(v["kind"] == "struct" for v in got["names"].values())
    print(f"{len(got['names'])} names ({n} structs), {len(got['functions'])} functions")
    if a.check:
        same = got == json.load(open(a.out))
        print(("reproduces " if same else "differs from ") + a.out)
        return 0 if same else 1
    with open(a.out, "w") as f:
        json.dump(got, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

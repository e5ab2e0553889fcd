"""Dump what a binding.py tells ctypes about the library: argtypes and restype of every function the headers declare, and the layout of
every ctypes.Structure and numpy record dtype the module holds.  Two dumps of two versions of binding.py against the same built library
diff to nothing when the ABI they state is the same (profiles/binding_header_zero_diff.txt).

    python scripts/binding_abi_dump.py                      # the tree's binding
    python scripts/binding_abi_dump.py --binding OLD.py     # another version of binding.py, a file outside the package, on the tree's library
"""
import argparse
import ctypes as C
import importlib
import importlib.util
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def type_name(t):
    if t is None:
        return "None"
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return "POINTER(%s)" % type_name(t._type_)
    if isinstance(t, type) and issubclass(t, C.Array):
        return "%s[%d]" % (type_name(t._type_), t._length_)
    return t.__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--binding", help="a binding.py outside the package (default: the package's)")
    a = ap.parse_args()
    pkg = importlib.import_module("opendlv-logic-cfsd18-sensation-slam_amd")
    if a.binding:
        os.environ["GS_LIB"] = pkg.binding.LIB_PATH
        spec = importlib.util.spec_from_file_location("binding_under_dump", a.binding)
        B = importlib.util.module_from_spec(spec); spec.loader.exec_module(B)
    else:
        B = pkg.binding
    L = B.lib()
    names = set()
    for h in (pkg.binding.HEADER, pkg.binding.DEBUG_HEADER):
        names |= set(re.findall(r"\b(gs_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)))
    for fn in sorted(names):
        f = getattr(L, fn)
        args = "unset" if f.argtypes is None else "(%s)" % ", ".join(type_name(t) for t in f.argtypes)
        print("function %s: %s -> %s" % (fn, args, type_name(f.restype)))
    for k in sorted(vars(B)):
        v = getattr(B, k)
        if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure:
            print("struct %s: %d bytes: %s" % (k, C.sizeof(v), ", ".join("%s %s" % (type_name(t), n) for n, t in v._fields_)))
        elif isinstance(v, np.dtype) and v.names:
            print("record %s: %d bytes: %s" % (k, v.itemsize, v.descr))


if __name__ == "__main__":
    main()

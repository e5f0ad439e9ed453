#!/usr/bin/env python3
"""Writes tests/golden/g26_ctypes_signatures.json: for every function the headers under include/ declare, the restype and argtypes
the loaded library's ctypes function carries, as type names (an unset restype is ctypes' default c_int; unset argtypes are null).
Run at the commit whose declarations are the reference; tests/test_abi_and_host.py compares _lib.lib() against the file.

    python tools/dump_ctypes_signatures.py"""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cspn_monodepth_amd import _lib  # noqa: E402

names = set()
for header in glob.glob(os.path.join(ROOT, "include", "*.h")):
    names |= set(re.findall(r"\b(cspn\w*)\s*\(", re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)))
sigs = {}
for name in sorted(names):
    fn = getattr(_lib.lib(), name)
    sigs[name] = {"restype": getattr(fn.restype, "__name__", None), "argtypes": fn.argtypes and [t.__name__ for t in fn.argtypes]}
with open(os.path.join(ROOT, "tests", "golden", "g26_ctypes_signatures.json"), "w") as fh:
    fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in sigs.items()) + "\n}\n")

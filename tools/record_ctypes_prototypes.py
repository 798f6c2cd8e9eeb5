"""Record what micromix_amd._lib binds, as plain names: (restype, argtypes) of every mm_* symbol that load() and load_diag() gave a
prototype, and every MM_* integer of the module.  tests/test_ctypes_prototypes.py holds the binding to the record; re-record only when
the C ABI itself changes, from a tree whose binding is known to be right:

    python tools/record_ctypes_prototypes.py > tests/golden/ctypes_prototypes_v1.json

Needs the built libraries, no GPU."""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from micromix_amd import _lib  # noqa: E402


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", text)))


def bound(lib, header):
    out = {}
    for name in declared(header):
        fn = getattr(lib, name, None)
        if fn is not None and fn.argtypes is not None:
            out[name] = [fn.restype.__name__ if fn.restype is not None else None, [t.__name__ for t in fn.argtypes]]
    return out


record = {"libmicromix_hip": bound(_lib.load(), "micromix_hip.h"), "libmicromix_diag": bound(_lib.load_diag(), "micromix_diag.h"),
          "constants": {k: v for k, v in sorted(vars(_lib).items()) if re.fullmatch(r"MM_[A-Z0-9_]+", k) and isinstance(v, int)}}
json.dump(record, sys.stdout, indent=1, sort_keys=True)
print()

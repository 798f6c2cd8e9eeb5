"""CPU tests of the ctypes binding: the prototypes micromix_amd._lib gives the two libraries equal, symbol for symbol, the record of
the hand-written binding it replaced (tests/golden/ctypes_prototypes_v1.json, tools/record_ctypes_prototypes.py), every exported
symbol has one, every MM_* integer keeps its value, and the header reader refuses what it does not understand.  A wrong prototype
does not fail by itself: it hands a truncated pointer or a shifted argument to a launch."""
import json
import os
import re

import pytest

from micromix_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "ctypes_prototypes_v1.json")))


def declared(header):
    """every function name of a header, the instrumented variant's included (the independent regex of tests/test_abi.py)"""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mm_[a-z0-9_]+)\s*\(", text)))


def bound(lib, header):
    out = {}
    for name in declared(header):
        fn = getattr(lib, name, None)
        if fn is not None and fn.argtypes is not None:
            out[name] = [fn.restype.__name__ if fn.restype is not None else None, [t.__name__ for t in fn.argtypes]]
    return out


@pytest.mark.parametrize("key, load, header, exports", [("libmicromix_hip", "load", "micromix_hip.h", "EXPORTS"),
                                                         ("libmicromix_diag", "load_diag", "micromix_diag.h", "DIAG_EXPORTS")])
def test_prototypes_equal_the_record(key, load, header, exports):
    lib = getattr(_lib, load)()
    got, want = bound(lib, header), GOLDEN[key]
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    for name in getattr(_lib, exports):                    # every exported symbol has a prototype
        assert getattr(lib, name).argtypes is not None, name
    for name in declared(header):
        assert not hasattr(lib, name) or getattr(lib, name).argtypes is not None, name


def test_constants_equal_the_record():
    got = {k: v for k, v in vars(_lib).items() if re.fullmatch(r"MM_[A-Z0-9_]+", k) and isinstance(v, int)}
    assert got == GOLDEN["constants"]


def test_reader_refuses_what_it_does_not_understand():
    good = "int mm_a(const void *p, int n, mm_stream_t stream);\nsize_t mm_b(void);\n"
    protos = _lib.prototypes(good)
    assert [(n, r.__name__, [t.__name__ for t in a]) for n, (r, a) in protos.items()] == \
        [("mm_a", "c_int", ["c_void_p", "c_int", "c_void_p"]), ("mm_b", "c_ulong", [])]
    with pytest.raises(_lib.MicroMixLibraryError, match=r"mm_c.*double"):
        _lib.prototypes(good + "int mm_c(double x);\n")                      # a type outside the table
    with pytest.raises(_lib.MicroMixLibraryError, match=r"mm_c.*short"):
        _lib.prototypes(good + "short mm_c(int x);\n")                       # ... as the return type
    with pytest.raises(_lib.MicroMixLibraryError, match=r"mm_c"):
        _lib.prototypes("int mm_c(int x)\n" + good)                          # a declaration without its ';'
    with pytest.raises(_lib.MicroMixLibraryError, match=r"MM_X"):
        _lib.constants("enum e { MM_X = MM_Y | 1 };\n")
    assert _lib.constants("enum e { MM_A = 3, MM_B = 0x10 };\n#define MM_C (1 << 4)\n#define MM_D 7    \n") == \
        {"MM_A": 3, "MM_B": 16, "MM_C": 16, "MM_D": 7}
    with pytest.raises(_lib.MicroMixLibraryError, match=r"no_such_header\.h"):
        _lib.header_text("no_such_header.h")

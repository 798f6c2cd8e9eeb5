"""ctypes binding of libmicromix_hip.so (the C ABI declared in include/micromix_hip.h).

There is deliberately NO fallback: if the HIP library is missing or fails to load, every
op raises.  A CPU path would silently void the parity claims of the GPU tests.
"""
from __future__ import annotations

import ctypes
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
# MICROMIX_HIP_LIB lets a kernel developer A/B an experimental build of the same C ABI (never a fallback).
LIB_PATH = os.environ.get("MICROMIX_HIP_LIB") or os.path.join(_PKG, "lib", "libmicromix_hip.so")
DIAG_LIB_PATH = os.environ.get("MICROMIX_DIAG_LIB") or os.path.join(_PKG, "lib", "libmicromix_diag.so")


class MicroMixLibraryError(RuntimeError):
    pass


class MMGroup(ctypes.Structure):
    """mm_group of include/micromix_hip.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("AN", "AS", "AO", "SFAN", "SFAS", "SFAO", "BN", "BS", "BO", "SFBN", "SFBS", "SFBO",
                                              "bias_bf16", "D")] + [("M", ctypes.c_int)]


class MMQuantGroup(ctypes.Structure):
    """mm_quant_group of include/micromix_hip.h"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("src_bf16", "reorder_index", "oN", "oS", "oO", "sfN", "sfS", "sfO")] + [("rows", ctypes.c_int)]


# ---- the C ABI is read from its headers: one copy of every prototype and constant (tests/test_ctypes_prototypes.py pins them) ----

_INCLUDE = os.path.join(os.path.dirname(_PKG), "include")
_SCALARS = {"int": ctypes.c_int, "unsigned": ctypes.c_uint, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64,
            "long long": ctypes.c_longlong, "mm_stream_t": ctypes.c_void_p}
_POINTERS = {"char": ctypes.c_char_p, "mm_group": ctypes.POINTER(MMGroup), "mm_quant_group": ctypes.POINTER(MMQuantGroup)}    # every other: c_void_p
_INSTRUMENT = re.compile(r"#ifdef MM_INSTRUMENT.*?#endif", re.S)        # declarations of the -DMM_INSTRUMENT developer variant only
_HEAD = re.compile(r"\b(mm_[a-z0-9_]+)\s*\(")
_DECLARATION = re.compile(r"([A-Za-z_][\w\s*]*?)\b(mm_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")
_CONSTANT = re.compile(r"\b(MM_[A-Z0-9_]+)[ \t]*=[ \t]*([^,}\n]*)|^[ \t]*#[ \t]*define[ \t]+(MM_[A-Z0-9_]+)[ \t]+(\S[^\n]*)", re.M)
_VALUE = re.compile(r"(\d+|0[xX][0-9a-fA-F]+)|\(1 << (\d+)\)")


def header_text(name):
    """a header of include/, without its comments"""
    path = os.path.join(_INCLUDE, name)
    if not os.path.exists(path):
        raise MicroMixLibraryError(f"{path} is missing: the ctypes prototypes of micromix_amd are read from it")
    with open(path) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _ctype(text, named, decl):
    """the ctypes type of one parameter (`named`) or return type, from the closed table above"""
    base, star, _ = text.partition("*")
    words = [w for w in base.split() if w != "const"]
    if star:
        return _POINTERS.get(" ".join(words), ctypes.c_void_p)
    if named:
        words = words[:-1]
    if " ".join(words) not in _SCALARS:
        raise MicroMixLibraryError(f"{decl}: no ctypes type for '{text.strip()}'")
    return _SCALARS[" ".join(words)]


def prototypes(text):
    """{name: (restype, argtypes)} of every `ret mm_name(args);` of comment-free header text; raises on a type outside the table and when
    a `mm_name(` is left that is no such declaration"""
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    out = {}
    for ret, name, args in _DECLARATION.findall(text):
        decl = f"{' '.join(ret.split())} {name}({' '.join(args.split())})"
        params = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (_ctype(ret, False, decl), [_ctype(a, True, decl) for a in params])
    heads = _HEAD.findall(text)
    if len(heads) != len(out):
        raise MicroMixLibraryError(f"{len(heads)} mm_*( in the header, {len(out)} declarations understood: "
                                   f"{sorted(set(heads) - set(out)) or 'a name is declared twice'}")
    return out


def constants(text):
    """{name: value} of every `MM_NAME = value` enum entry and `#define MM_NAME value` of comment-free header text; a value is decimal,
    hex or (1 << n), anything else raises"""
    out = {}
    for enum_name, enum_value, define_name, define_value in _CONSTANT.findall(text):
        name, value = enum_name or define_name, (enum_value or define_value).strip()
        m = _VALUE.fullmatch(value)
        if not m:
            raise MicroMixLibraryError(f"{name} = {value}: not a decimal, hex or (1 << n) value")
        out[name] = int(m.group(1), 0) if m.group(1) else 1 << int(m.group(2))
    return out


def _read(name):
    text = header_text(name)
    protos = prototypes(text)
    variant_only = set(_HEAD.findall(" ".join(_INSTRUMENT.findall(text))))
    return protos, tuple(n for n in protos if n not in variant_only), constants(text)


def _bind(lib, protos):
    """a symbol gets its prototype when the loaded library exports it: an older build, or the default one next to the instrumented
    variant, lacks some, and the wrappers say so when they are called"""
    for name, (restype, argtypes) in protos.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


# EXPORTS / DIAG_EXPORTS: every symbol include/micromix_hip.h / micromix_diag.h declares outside #ifdef MM_INSTRUMENT (libmicromix_diag.so:
# hardware probes for tests/tools, never used by the ops); the MM_* integers of the headers become attributes of this module
_PROTOS, EXPORTS, _consts = _read("micromix_hip.h")
_DIAG_PROTOS, DIAG_EXPORTS, _diag_consts = _read("micromix_diag.h")
globals().update(_consts, **_diag_consts)
# CALIB_EXPORTS: the entries of include/micromix_calib.h, exported by the product library next to EXPORTS; the header defines no constant
_CALIB_PROTOS, CALIB_EXPORTS, _ = _read("micromix_calib.h")
# LOGPROB_EXPORTS: the entries of include/micromix_logprob.h, exported and bound the same way; the header defines no constant either
_LOGPROB_PROTOS, LOGPROB_EXPORTS, _ = _read("micromix_logprob.h")
# LOGITS_EXPORTS: the entry of include/micromix_logits.h, likewise
_LOGITS_PROTOS, LOGITS_EXPORTS, _ = _read("micromix_logits.h")
# SPEC_EXPORTS: the entries of include/micromix_spec.h, likewise
_SPEC_PROTOS, SPEC_EXPORTS, _ = _read("micromix_spec.h")
# KVSTEP_EXPORTS: the entries of include/micromix_kvstep.h, likewise.  Its integers stay out of the module's MM_* attributes (those are the
# two headers' above): KV_STEP holds them by name -- the limits, the state's header size, the statuses of a step -- and KV_STEP_STATUS
# names a status value
_KVSTEP_PROTOS, KVSTEP_EXPORTS, KV_STEP = _read("micromix_kvstep.h")
KV_STEP_STATUS = {v: n for n, v in KV_STEP.items() if n not in ("MM_KV_STEP_MAX_BATCH", "MM_KV_STEP_HEADER_INTS")}
# TOKENS_EXPORTS: the entries of include/micromix_tokens.h, likewise; TOKENS holds its integers by name (the limits, the n-gram part, the
# values of `finished`)
_TOKENS_PROTOS, TOKENS_EXPORTS, TOKENS = _read("micromix_tokens.h")
# RANDOM_EXPORTS: the entry of include/micromix_random.h, likewise; RANDOM holds its two limits by name
_RANDOM_PROTOS, RANDOM_EXPORTS, RANDOM = _read("micromix_random.h")

_lib = None


def load():
    """Load (once) and return the ctypes handle; raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MicroMixLibraryError(
            f"{LIB_PATH} is missing: build it with `python -m micromix_amd.build` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for protos in (_PROTOS, _CALIB_PROTOS, _LOGPROB_PROTOS, _LOGITS_PROTOS, _SPEC_PROTOS, _KVSTEP_PROTOS, _TOKENS_PROTOS, _RANDOM_PROTOS):
        _bind(lib, protos)
    _lib = lib
    return _lib


_diag = None


def load_diag():
    """libmicromix_diag.so (include/micromix_diag.h): hardware probes and microbenchmarks for tests/ and tools/."""
    global _diag
    if _diag is not None:
        return _diag
    if not os.path.exists(DIAG_LIB_PATH):
        raise MicroMixLibraryError(f"{DIAG_LIB_PATH} is missing: build it with `python -m micromix_amd.build`")
    _diag = _bind(ctypes.CDLL(DIAG_LIB_PATH), _DIAG_PROTOS)
    return _diag


def check(status: int, what: str):
    """Map an mm_status to the exception the reference's binding raises."""
    if status == MM_OK:
        return
    lib = load()
    msg = lib.mm_strerror(status).decode()
    if status == MM_ERR_BAD_SPLIT:
        # reference: throw std::runtime_error("Value error in run_reorder_quantize_x") (bindings.cpp:145-148)
        raise RuntimeError(f"Value error in run_{what}: {msg}")
    if status == MM_ERR_LAUNCH:
        raise RuntimeError(f"{what}: {msg}: {lib.mm_last_error().decode()}")
    raise RuntimeError(f"{what}: {msg}")

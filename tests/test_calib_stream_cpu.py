"""CPU tests of the streaming calibration (include/micromix_calib.h, micromix_amd.calib.accumulate / Calibrator): the statuses that
come back without device work, the ABI record, the host arithmetic of Calibrator.finish from planted state, and the Python argument
errors that need no device."""
import ctypes
import math

import pytest
import torch

from micromix_amd import _lib, calib
import calib_oracle as co
from test_ctypes_prototypes import test_constants_equal_the_record, test_prototypes_equal_the_record  # noqa: F401  (EXPORTS and MM_* as they were)

OK, BAD_ARG, UNSUPPORTED = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


def call(x=0x1000, dtype=0, rows=16, k=256, ld=None, lamda=1.0, score=0x2000, counts=0x3000, ws=0x4000, ws_bytes=None):
    """mm_calib_accumulate with made-up addresses: every case below returns before any launch"""
    lib = _lib.load()
    ws_bytes = lib.mm_calib_workspace_bytes(rows, k) if ws_bytes is None else ws_bytes
    return lib.mm_calib_accumulate(x, dtype, rows, k, k if ld is None else ld, lamda, score, counts, ws, ws_bytes, None)


def test_bad_arguments_without_device_work():
    for kw in (dict(x=None), dict(score=None), dict(counts=None), dict(ws=None),            # a null pointer
               dict(x=0x1008), dict(ld=260), dict(ld=257),                                   # x or ld * 2 not at 16 bytes
               dict(ld=255), dict(ld=0), dict(rows=-1), dict(k=-128),                        # ld < K, negative sizes
               dict(ws_bytes=0), dict(ws_bytes=2 * (4 * 256 + 16) - 1), dict(ws=0x4008),     # a workspace too small or misaligned
               dict(score=0x2002), dict(counts=0x3004),
               dict(lamda=0.0), dict(lamda=-1.0), dict(lamda=math.inf), dict(lamda=math.nan)):
        assert call(**kw) == BAD_ARG, kw


def test_unsupported_without_device_work():
    for kw in (dict(k=192), dict(k=64), dict(k=0), dict(k=32768 + 128), dict(rows=(1 << 20) + 1, ws_bytes=1 << 40), dict(dtype=2), dict(dtype=-1)):
        assert call(**kw) == UNSUPPORTED, kw
    assert call(rows=1 << 20, ws_bytes=0) == BAD_ARG and call(k=32768, ws_bytes=0) == BAD_ARG      # the limits themselves are accepted


def test_no_rows_is_ok_and_touches_nothing():
    assert call(rows=0, x=None, score=None, counts=None, ws=None, ws_bytes=0) == OK
    assert call(rows=0, k=192) == UNSUPPORTED and call(rows=0, lamda=0.0) == BAD_ARG                # but the sizes are still looked at


def test_workspace_bytes():
    f = _lib.load().mm_calib_workspace_bytes
    for rows, k in ((-1, 256), (0, 256), (16, 192), (16, 64), (16, 0), (16, -128), (16, 32768 + 128), ((1 << 20) + 1, 256)):
        assert f(rows, k) == 0, (rows, k)
    for rows, k in ((1, 128), (8, 128), (9, 128), (2048, 4096), (1 << 20, 32768)):
        assert f(rows, k) == (rows + 7) // 8 * (4 * k + 16) > 0, (rows, k)


def test_abi_record():
    lib = _lib.load()
    assert _lib.CALIB_EXPORTS == ("mm_calib_workspace_bytes", "mm_calib_accumulate")
    assert not set(_lib.CALIB_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS))
    f, g = lib.mm_calib_workspace_bytes, lib.mm_calib_accumulate
    assert f.restype is ctypes.c_size_t and f.argtypes == [ctypes.c_int, ctypes.c_int]
    v = ctypes.c_void_p
    assert g.restype is ctypes.c_int
    assert g.argtypes == [v, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, v, v, v, ctypes.c_size_t, v]
    assert _lib.constants(_lib.header_text("micromix_calib.h")) == {}                              # the header defines no MM_* constant
    assert lib.mm_version() == 660


def planted(k, count4, count6, numel, score=None, key="a"):
    c = calib.Calibrator()
    c.set_stats(key, torch.zeros(k) if score is None else score, count4, count6, numel)
    return c


def test_finish_uses_the_reference_fp32_ratios():
    """K = 4096, numel = 12288, counts (3649, 9409): the reference's fp32 tensor arithmetic and double arithmetic part at a ceil"""
    a = 3649 / 12288
    b = 9409 / 12288 - a
    assert (math.ceil(4096 * b / 128) * 128, math.ceil(4096 * (1 - a - b) / 128) * 128) == (2048, 1024)
    assert co.split(3649, 9409, 12288, 4096) == (1920, 1024)
    order, p6, p8, bits = planted(4096, 3649, 9409, 12288).finish(report=True)
    assert (p6["a"], p8["a"]) == (1920, 1024)
    ra = torch.tensor(3649) / 12288
    rb = torch.tensor(9409) / 12288 - ra
    assert bits["a"] == float(4 * ra + 6 * rb + 8 * (1 - ra - rb))
    assert len(planted(4096, 3649, 9409, 12288).finish()) == 3


def test_finish_clamps():
    # count6 < count4 (a lamda for which the p6 threshold lies below the p4 one): a negative p6 ratio, clamped to 0; p8 then to K - p6
    _, p6, p8 = planted(256, 1000, 0, 1000).finish()
    assert (p6["a"], p8["a"]) == (0, 256)
    _, p6, p8 = planted(256, 0, 1000, 1000).finish()              # everything in p6: p8 = 0
    assert (p6["a"], p8["a"]) == (256, 0)
    _, p6, p8 = planted(256, 0, 0, 1000).finish()                 # everything in p8
    assert (p6["a"], p8["a"]) == (0, 256)
    _, p6, p8 = planted(256, 1, 601, 1000).finish()               # both rounded up, 256 + 128 > K: p8 clamped to K - p6
    assert (p6["a"], p8["a"]) == (256, 0)


def test_finish_leaves_out_a_key_without_elements():
    c = planted(256, 10, 20, 100)
    c.set_stats("empty", torch.zeros(384), 0, 0, 0)
    order, p6, p8 = c.finish()
    assert list(order) == list(p6) == list(p8) == ["a"] and c.keys() == ["a", "empty"]
    assert calib.Calibrator().finish() == ({}, {}, {})


def test_finish_orders_ties_stably_and_round_trips(tmp_path):
    score = torch.tensor([3.0, 1.0, 2.0, 1.0] * 64)
    order, p6, p8 = planted(256, 10, 20, 100, score=score).finish()
    ones, twos, threes = (torch.arange(256)[score == v].tolist() for v in (1.0, 2.0, 3.0))
    assert order["a"].tolist() == ones + twos + threes and order["a"].dtype is torch.int64
    calib.validate(order, p6, p8)
    calib.save_calibration(str(tmp_path), "m", order, p6, p8)
    o2, p6b, p8b = calib.load_calibration(str(tmp_path), "m")
    assert torch.equal(o2["a"], order["a"]) and p6b == p6 and p8b == p8
    s, c4, c6, n = planted(256, 10, 20, 100, score=score).stats("a")
    assert torch.equal(s, score) and (c4, c6, n) == (10, 20, 100)


def test_argument_errors():
    score, counts = torch.zeros(256), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        calib.accumulate(torch.zeros(4, 256, dtype=torch.bfloat16), score, counts)
    with pytest.raises(RuntimeError, match="no CPU path"):
        calib.Calibrator().observe("a", torch.zeros(4, 256, dtype=torch.float16))
    with pytest.raises(TypeError, match="bfloat16 or torch.float16"):
        calib.accumulate(torch.zeros(4, 256), score, counts)
    with pytest.raises(TypeError):
        calib.accumulate([[0.0] * 256], score, counts)
    for lamda in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="lamda"):
            calib.Calibrator(lamda)

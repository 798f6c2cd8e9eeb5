"""mm_add_rmsnorm_quantize without a GPU: the add rule of tests/add_rms_oracle.py against torch's CPU bf16 `x + r`, bit for bit, and the
statuses the entry returns before any device work."""
import ctypes

import numpy as np
import pytest

import add_rms_oracle as ar
from micromix_amd import _lib
from oracle import mx_oracle as o


@pytest.fixture(autouse=True)
def library_with_the_entries():
    """every test here is about mm_add_rmsnorm_quantize's rule: without a library that has the entry there is nothing to state it for"""
    assert _lib.load().mm_version() >= 660 and hasattr(_lib.load(), "mm_add_rmsnorm_quantize")


def torch_add(x_bits, r_bits):
    import torch
    t = lambda b: torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).view(torch.bfloat16)
    return (t(x_bits) + t(r_bits)).view(torch.int16).numpy().view(np.uint16)


def is_nan(b):
    return (np.asarray(b) & 0x7FFF) > 0x7F80


def same_as_torch(got, want):
    """bit-equal wherever torch's sum is a number, a NaN -- the rule's one pattern -- wherever torch's is a NaN (torch's own NaN pattern is
    0x7FC0 from its scalar conversion and 0xFFFF from its vectorised one: the rule cannot equal both)"""
    nan = is_nan(want)
    return np.array_equal(got[~nan], want[~nan]) and np.all(got[nan] == ar.CANONICAL_NAN) and np.array_equal(is_nan(got), nan)


def test_the_rule_is_torchs_bf16_add_on_random_data():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 1 << 16, size=(64, 4096), dtype=np.uint32).astype(np.uint16)      # every pattern, NaN and inf included
    r = rng.integers(0, 1 << 16, size=(64, 4096), dtype=np.uint32).astype(np.uint16)
    want = torch_add(x, r)
    assert is_nan(want).sum() > 1000 and same_as_torch(ar.add_bf16(x, r), want)
    g = o.f32_to_bf16(rng.standard_normal((64, 4096)).astype(np.float32)), o.f32_to_bf16((3 * rng.standard_normal((64, 4096))).astype(np.float32))
    assert np.array_equal(ar.add_bf16(*g), torch_add(*g))


def test_the_rule_on_every_finite_bf16_against_its_partners():
    b = ar.all_finite_bf16()
    assert b.size == 2 * 255 * 128
    for name, p in ar.partners(b).items():
        got, want = ar.add_bf16(b, p), torch_add(b, p)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        assert np.array_equal(ar.add_bf16(p, b), got), name                       # commutative, bit for bit
    s = ar.add_bf16(b, ar.partners(b)["negation"])
    assert np.all(s == 0)                                                         # x + (-x) = +0 under round to nearest
    over = ar.add_bf16(np.uint16(0x7F7F), np.uint16(0x7F7F))
    assert over == 0x7F80 and ar.add_bf16(np.uint16(0xFF7F), np.uint16(0xFF7F)) == 0xFF80      # overflow to +-inf
    assert ar.add_bf16(np.uint16(0x0001), np.uint16(0x0001)) == 0x0002            # subnormals are kept, not flushed
    assert ar.add_bf16(np.uint16(0x0040), np.uint16(0x0040)) == 0x0080            # ... and grow into the smallest normal


def test_inf_minus_inf_and_nan_operands_give_the_one_nan():
    inf, ninf = np.uint16(0x7F80), np.uint16(0xFF80)
    for a, b in ((inf, ninf), (ninf, inf), (np.uint16(0x7FC1), np.uint16(0x3F80)), (np.uint16(0xFFFF), np.uint16(0x0000)), (np.uint16(0x7F81), inf)):
        assert ar.add_bf16(a, b) == ar.CANONICAL_NAN
        assert is_nan(torch_add(np.array([a]), np.array([b]))[0])
        wide = torch_add(np.full(64, a), np.full(64, b))                         # (torch's vectorised path: another NaN pattern)
        assert np.all(is_nan(wide)) and same_as_torch(ar.add_bf16(np.full(64, a), np.full(64, b)), wide)
    assert ar.add_bf16(inf, inf) == inf and ar.add_bf16(inf, np.uint16(0xFF7F)) == inf


def test_the_expectation_for_the_six_buffers_is_the_oracle_on_the_sum():
    rng = np.random.default_rng(2)
    rows, k, split = 3, 384, (128, 128, 128)
    x = o.f32_to_bf16(rng.standard_normal((rows, k)).astype(np.float32))
    r = o.f32_to_bf16(rng.standard_normal((rows, k)).astype(np.float32))
    r[1] = x[1] ^ 0x8000
    w = o.f32_to_bf16((1 + 0.1 * rng.standard_normal(k)).astype(np.float32))
    idx = rng.permutation(k).astype(np.int16)
    s, six = ar.add_rmsnorm_quantize(x, r, w, 1e-5, idx, *split)
    want = o.rmsnorm_quantize(torch_add(x, r), w, 1e-5, idx, *split)
    assert np.array_equal(s, torch_add(x, r)) and all(np.array_equal(a, b) for a, b in zip(six, want))
    assert np.all(s[1] == 0)
    zero = o.rmsnorm_quantize(np.zeros((1, k), np.uint16), w, 1e-5, idx, *split)
    assert all(np.array_equal(six[i][1], zero[i][0]) for i in range(3))           # x = -r: the zero row's bytes


def test_status_codes_without_device_work():
    lib = _lib.load()
    assert lib.mm_version() >= 660
    B, S = _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_BAD_SPLIT
    rows, K = 4, 256
    nbytes = rows * K * 2
    base = 0x7F0000000000         # never dereferenced: every call below returns before a launch
    X, R, So, W, IDX = base, base + 0x100000, base + 0x200000, base + 0x300000, base + 0x400000
    outs = [base + 0x500000 + 0x10000 * i for i in range(6)]

    def call(x=X, r=R, s=So, w=W, idx=IDX, rows=rows, K=K, split=(128, 0, 128), o_=None):
        o_ = list(outs) if o_ is None else o_
        return lib.mm_add_rmsnorm_quantize(x, r, s, w, 1e-5, rows, K, idx, *split, 0, *o_, None)

    for nul in ("x", "r", "s", "w", "idx"):
        assert call(**{nul: None}) == B, nul
    no_on, no_sfo = list(outs), list(outs)
    no_on[0], no_sfo[5] = None, None
    assert call(o_=no_on) == B and call(o_=no_sfo) == B
    no_os = list(outs)
    no_os[1] = no_os[4] = None
    assert call(o_=no_os, rows=0) == _lib.MM_OK                                    # KS = 0: the S buffers may be null (rows = 0: no launch)
    # S_out over X and over R: the same pointer, and partial overlaps from either side
    for other in ("x", "r"):
        p = X if other == "x" else R
        assert call(s=p) == B, other
        assert call(s=p + nbytes - 16) == B and call(s=p - nbytes + 16) == B, other
        assert call(s=p + 16) == B, other
    # misaligned operands
    for name in ("x", "r", "s", "w"):
        assert call(**{name: dict(x=X, r=R, s=So, w=W)[name] + 2}) == B, name
    # K and the split: the statuses of mm_rmsnorm_quantize
    plain = lambda K, split, rows=rows: lib.mm_rmsnorm_quantize(X, W, 1e-5, rows, K, IDX, *split, 0, *outs, None)
    for K_, split in ((192, (128, 0, 64)), (256, (128, 0, 0)), (0, (0, 0, 0)), (256, (-128, 256, 128)), (32768 + 128, (32768, 0, 128))):
        assert call(K=K_, split=split) == plain(K_, split), (K_, split)
    assert call(K=192, split=(128, 0, 64)) == S and call(K=32768 + 128, split=(32768, 0, 128)) == B
    assert call(rows=-1) == B == plain(256, (128, 0, 128), rows=-1)
    # rows == 0: success, whatever the pointers -- nothing is read or written
    assert call(rows=0) == _lib.MM_OK and call(rows=0, x=None, r=None, s=None) == _lib.MM_OK
    assert call(rows=0, s=X) == _lib.MM_OK


def test_status_codes_of_the_decode_entries_without_device_work():
    lib = _lib.load()
    B, S, U = _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_BAD_SPLIT, _lib.MM_ERR_UNSUPPORTED
    base = 0x7F0000000000         # never dereferenced: every call below returns before a launch
    X, R, So, W, IDX, D, WS = (base + 0x100000 * i for i in range(7))
    wts = [base + 0x1000000 + 0x100000 * i for i in range(6)]
    outs = [base + 0x2000000 + 0x100000 * i for i in range(6)]
    M, K, split = 2, 256, (128, 0, 128)
    nbytes = M * K * 2

    def lin(x=X, r=R, s=So, w=W, idx=IDX, M=M, N=256, split=split, wmode=_lib.MM_W_FP4, flags=0, d=D, wt=None):
        return lib.mm_add_rmsnorm_qlinear_decode(x, r, s, w, 1e-5, idx, *(wts if wt is None else wt), M, N, *split, wmode, flags, None, d, None)

    def gate_up(x=X, r=R, s=So, w=W, idx=IDX, M=M, I=128, split=split, dsplit=(128, 0, 0), flags=0, o_=None, ws=WS, wsb=1 << 20):
        return lib.mm_add_rmsnorm_gate_up_activate_decode(x, r, s, w, 1e-5, idx, *wts, M, I, *split, *dsplit, flags, *(outs if o_ is None else o_), ws, wsb, None)

    for call in (lin, gate_up):
        for nul in ("x", "r", "s", "w", "idx"):
            assert call(**{nul: None}) == B, (call.__name__, nul)
        for other in (X, R):                                                     # S_out over X and over R: equal, and partial from both sides
            for sp in (other, other + 16, other + nbytes - 16, other - nbytes + 16):
                assert call(s=sp) == B, (call.__name__, hex(sp))
        for name, p in (("x", X), ("r", R), ("s", So), ("w", W)):
            assert call(**{name: p + 2}) == B, (call.__name__, name)
        assert call(split=(128, 0, 64)) == S and call(split=(0, 0, 0)) == S       # K % 128 != 0; no K at all
        assert call(M=-1) == B
        assert call(M=0) == _lib.MM_OK and call(M=0, x=None, r=None, s=X) == _lib.MM_OK
        assert call(M=9) == U                                                     # the plain forms' own limit, answered by their queries
        assert call(flags=0x40) == B
    # the statuses of the plain entries for the same bad arguments
    assert lib.mm_rmsnorm_qlinear_decode(X, W, 1e-5, IDX, *wts, M, 256, 128, 0, 64, _lib.MM_W_FP4, 0, None, D, None) == S
    assert lib.mm_rmsnorm_qlinear_decode(None, W, 1e-5, IDX, *wts, M, 256, *split, _lib.MM_W_FP4, 0, None, D, None) == B
    assert lin(d=None) == B and lin(wmode=7) == B and lin(N=0) == _lib.MM_OK
    no_bn = list(wts)
    no_bn[0] = None
    assert lin(wt=no_bn) == B
    assert gate_up(dsplit=(64, 0, 64)) == S and gate_up(dsplit=(128, 128, 0)) == S   # the down split must be multiples of 128 that sum to I
    no_on = list(outs)
    no_on[0] = None
    assert gate_up(o_=no_on) == B
    assert gate_up(ws=None) == B and gate_up(wsb=16) == B                         # a narrow layer: the two-launch form needs its scratch


def test_the_header_declares_the_entry_and_the_python_ops_exist():
    import os
    from micromix_amd import mixedgemm, qlinear
    import inspect
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "micromix_hip.h")).read()
    for name in ("mm_add_rmsnorm_quantize", "mm_add_rmsnorm_qlinear_decode", "mm_add_rmsnorm_gate_up_activate_decode"):
        assert f"int {name}(" in header and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert "_supported" not in " ".join(e for e in _lib.EXPORTS if e.startswith("mm_add_"))        # the plain forms' queries answer for these
    sig = inspect.signature(mixedgemm.add_rmsnorm_quantize_x)
    assert list(sig.parameters)[:9] == ["x", "residual", "weight", "eps", "reorder_index", "KN", "KS", "KO", "out_sum"]
    for fn in (qlinear.QLinearLayer.forward_norm, qlinear.FusedQLinear.forward_norm, qlinear.FusedMLP.forward):
        assert inspect.signature(fn).parameters["residual"].default is None
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm", os.path.join(root, "micromix_amd", "dropin", "mixedgemm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("add_rmsnorm_quantize_x", "add_rmsnorm_qlinear_decode", "add_rmsnorm_gate_up_activate_decode"):
        assert getattr(mod, name) is getattr(mixedgemm, name)

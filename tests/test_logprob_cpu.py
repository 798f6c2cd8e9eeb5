"""CPU tests of the token log-probabilities: the host side of mm_logprob_rows (include/micromix_logprob.h: symbols, every status
without device work, the workspace sizes, the Python argument errors), the numpy oracle itself (tests/logprob_oracle.py against
torch.log_softmax in fp64 and against hand-written rows) and the cap on E / S that keeps its bound honest.  No kernel is launched."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
import logprob_oracle as lo
import sample_oracle as so

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
C = _lib.MM_ARGMAX_CHUNK
BIG = 1 << 40


def call(logits=16, rows=3, vocab=100, ld=None, target=16, T=16, logprob=16, rank=16, lse=16, top_n=2, top_idx=16, top_logprob=16, ws=64,
         ws_bytes=BIG):
    """mm_logprob_rows with made-up addresses: every case below returns before any launch"""
    return _lib.load().mm_logprob_rows(logits, rows, vocab, vocab if ld is None else ld, target, T, logprob, rank, lse, top_n, top_idx,
                                       top_logprob, ws, ws_bytes, None)


# ---- the C ABI and the Python ops ------------------------------------------------------------------------------------------------------------
def test_symbols_and_the_abi_record():
    lib = _lib.load()
    assert _lib.LOGPROB_EXPORTS == ("mm_logprob_rows_workspace_bytes", "mm_logprob_rows")
    assert not set(_lib.LOGPROB_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS) | set(_lib.CALIB_EXPORTS))
    for name in _lib.LOGPROB_EXPORTS:
        assert hasattr(lib, name), name
    f, g = lib.mm_logprob_rows_workspace_bytes, lib.mm_logprob_rows
    v, i = ctypes.c_void_p, ctypes.c_int
    assert f.restype is ctypes.c_size_t and f.argtypes == [i, i, i]
    assert g.restype is i and g.argtypes == [v, i, i, ctypes.c_longlong, v, v, v, v, v, i, v, v, v, ctypes.c_size_t, v]
    assert _lib.constants(_lib.header_text("micromix_logprob.h")) == {}             # no constant of the header reaches _lib
    assert not [n for n in vars(_lib) if n.startswith("MM_LOGPROB")]
    assert lib.mm_version() == 660


def test_python_surface():
    for name in ("logprob_rows", "logprob_rows_workspace_bytes", "cross_entropy"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name)), name
    sig = inspect.signature(mixedgemm.logprob_rows).parameters
    assert list(sig) == ["logits", "targets", "temperature", "top_n", "workspace"] and sig["targets"].default is None
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in list(sig)[2:]) and sig["top_n"].default == 0
    sig = inspect.signature(mixedgemm.cross_entropy).parameters
    assert list(sig) == ["logits", "labels", "ignore_index", "reduction"]
    assert sig["ignore_index"].default == -100 and sig["reduction"].default == "mean"
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm_lp", inspect.getsourcefile(_lib).replace("_lib.py", "dropin/mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.logprob_rows is mixedgemm.logprob_rows and dropin.cross_entropy is mixedgemm.cross_entropy
    assert dropin.logprob_rows_workspace_bytes is mixedgemm.logprob_rows_workspace_bytes
    assert "bf16" in mixedgemm.cross_entropy.__doc__ and "reference" in mixedgemm.cross_entropy.__doc__


def test_bad_arguments_without_device_work():
    for kw in (dict(logits=None), dict(logits=17), dict(logits=31),                 # null, odd
               dict(rows=-1), dict(vocab=0), dict(vocab=-5), dict(ld=99),
               dict(target=18), dict(T=18), dict(logprob=18), dict(rank=18), dict(lse=18), dict(top_idx=18), dict(top_logprob=18),
               dict(target=None), dict(logprob=None),                               # one without the other
               dict(target=None, logprob=None),                                     # rank without a target
               dict(top_n=-1), dict(top_n=33), dict(top_idx=None), dict(top_logprob=None),
               dict(target=None, logprob=None, rank=None, lse=None, top_n=0),       # nothing asked for
               dict(target=None, logprob=None, rank=None, lse=None, top_n=0, top_idx=None, top_logprob=None),
               dict(ws=None), dict(ws=68), dict(ws_bytes=0), dict(ws=None, ws_bytes=0)):
        assert call(**kw) == BAD, kw
    need = _lib.load().mm_logprob_rows_workspace_bytes(3, 100, 2)
    assert need > 0 and call(ws_bytes=need - 1) == BAD
    # the sizes are looked at before the pointers, and top_n before the limits
    assert call(rows=0, top_n=33) == BAD and call(rows=0, vocab=0) == BAD and call(vocab=(1 << 20) + 1, top_n=40) == BAD


def test_unsupported_and_no_rows_without_device_work():
    assert call(vocab=(1 << 20) + 1) == UNS and call(rows=_lib.MM_ARGMAX_MAX_ROWS + 1) == UNS
    assert call(rows=0) == OK
    assert call(rows=0, logits=None, target=None, T=None, logprob=None, rank=None, lse=None, top_n=0, top_idx=None, top_logprob=None, ws=None,
                ws_bytes=0) == OK
    assert call(rows=0, vocab=(1 << 20) + 1) == UNS


def test_workspace_bytes():
    f = _lib.load().mm_logprob_rows_workspace_bytes
    for rows, vocab, n in ((0, 100, 0), (-1, 100, 0), (3, 0, 0), (3, -1, 0), (3, (1 << 20) + 1, 0), (_lib.MM_ARGMAX_MAX_ROWS + 1, 100, 0),
                           (3, 100, -1), (3, 100, 33)):
        assert f(rows, vocab, n) == 0, (rows, vocab, n)
    one = f(3, 100, 0)
    assert one > 0 and one % 8 == 0 and one == f(3, C, 0)
    assert f(3, C + 1, 0) > one                                                     # a second part
    assert f(3, 100, 1) > one and f(3, 100, 32) > f(3, 100, 20) > f(3, 100, 1)      # the candidates of top_n
    assert all(f(r, v, n) % 8 == 0 for r in (1, 2, 5) for v in (1, C + 1) for n in (0, 1, 5))
    parts = -(-128256 // C)
    assert f(2047, 128256, 20) <= 2047 * (parts * (24 + 8 * 20) + 8) + 8            # no [rows, vocab] array
    assert f(_lib.MM_ARGMAX_MAX_ROWS, 1 << 20, 32) > 0                              # the limits themselves are accepted
    assert mixedgemm.logprob_rows_workspace_bytes(3, 100) == one and mixedgemm.logprob_rows_workspace_bytes(3, 100, 5) == f(3, 100, 5)


def test_python_argument_errors():
    lg = torch.zeros((3, 100), dtype=torch.bfloat16)
    y = torch.zeros((3,), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.logprob_rows(lg, y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.cross_entropy(lg, y)
    with pytest.raises(TypeError, match="bfloat16"):
        mixedgemm.logprob_rows(lg.float())
    with pytest.raises(TypeError, match="bfloat16"):
        mixedgemm.cross_entropy(lg.float(), y)
    with pytest.raises(TypeError):
        mixedgemm.logprob_rows(None)
    with pytest.raises(ValueError, match="reduction"):
        mixedgemm.cross_entropy(lg, y, reduction="batchmean")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------
def to_torch(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def test_the_oracle_equals_torch_log_softmax_in_fp64():
    rng = np.random.default_rng(3)
    for vocab, T in ((1, 1.0), (7, 1.0), (1000, 0.5), (C + 1, 2.0), (32000, 1.0)):
        bits = so.bf16_bits(rng.standard_normal(vocab) * 3.0)
        bits[rng.integers(0, vocab, vocab // 10)] = 0xFF80                          # some -inf
        bits[0] = so.bf16_bits(np.float32(2.5))                                     # and a finite one for certain
        x = to_torch(bits).double() / T
        want, want_lse = torch.log_softmax(x, dim=0).numpy(), float(torch.logsumexp(x, dim=0))
        lse, lp = lo.values(bits, T)
        assert lse == pytest.approx(want_lse, rel=1e-13, abs=1e-13)
        finite = np.isfinite(want)
        assert np.array_equal(np.isneginf(lp), np.isneginf(want)) and np.allclose(lp[finite], want[finite], rtol=1e-12, atol=1e-12)
        r = lo.row(bits, 0, T, 5)
        assert r["logprob"] == lp[0] and r["lse"] == lse
        top = r["top_idx"][r["top_idx"] >= 0]
        assert len(top) == min(5, vocab) and x[top].tolist() == torch.topk(x, len(top)).values.tolist()
        assert r["rank"] == int((x > x[0]).sum())


def test_the_oracle_on_hand_written_rows():
    ninf, nan = 0xFF80, 0x7FC0
    bits = np.concatenate([so.bf16_bits(np.array([1.0, 3.0, 3.0, 2.0, -0.0, 0.0], dtype=np.float32)), np.array([ninf], dtype=np.uint16)])
    bits[4] = 0x8000                                                                # -0 next to +0: one class, the lower index first
    r = lo.row(bits, 3, None, 9)
    assert r["top_idx"].tolist() == [1, 2, 3, 0, 4, 5, 6, -1, -1] and r["rank"] == 2
    S = 2 + math.exp(-1) + math.exp(-2) + 2 * math.exp(-3)
    assert r["lse"] == pytest.approx(3 + math.log(S), rel=1e-15) and r["logprob"] == pytest.approx(-1 - math.log(S), rel=1e-15)
    assert r["top_logprob"][6] == -np.inf and r["top_logprob"][7] == -np.inf and r["top_logprob"][0] == pytest.approx(-math.log(S))
    assert lo.row(bits, 6)["logprob"] == -np.inf and lo.row(bits, 6)["rank"] == 6 and lo.row(bits, 5)["rank"] == 4
    for ignored in (-100, -1, 7, 2 ** 31 - 1):
        r = lo.row(bits, ignored)
        assert r["logprob"] == 0.0 and r["rank"] == -1
    assert lo.row(bits)["logprob"] is None and lo.row(bits)["rank"] is None
    # T' : None, 0, negative and NaN are 1; T = 2 halves the logits
    for T in (None, 0.0, -1.0, math.nan):
        assert lo.t_prime(T) == 1.0 and lo.row(bits, 3, T)["lse"] == lo.row(bits, 3)["lse"]
    assert lo.row(bits, 3, 2.0)["lse"] == pytest.approx(1.5 + math.log(2 + math.exp(-0.5) + math.exp(-1) + 2 * math.exp(-1.5)))
    # degenerate rows: NaN values, the integers stand
    for special, first in ((nan, 2), (0x7F80, 2), (0xFFC0, 2)):
        b = bits.copy()
        b[2] = special
        r = lo.row(b, 3, None, 3)
        assert math.isnan(r["lse"]) and math.isnan(r["logprob"]) and np.isnan(r["top_logprob"]).all()
        assert r["top_idx"].tolist() == [first, 1, 3] and r["rank"] == 2
    r = lo.row(np.full(4, ninf, dtype=np.uint16), 1, None, 2)
    assert math.isnan(r["lse"]) and math.isnan(r["logprob"]) and r["rank"] == 0 and r["top_idx"].tolist() == [0, 1]
    b = bits.copy()
    b[[0, 5]] = nan, 0xFFC0                                                          # NaNs of both signs are one class
    assert lo.row(b, 5, None, 3)["top_idx"].tolist() == [0, 5, 1] and lo.row(b, 5)["rank"] == 0


def test_the_bound_is_what_the_docstring_states():
    assert lo.bound(1e-6, 0.0) == 1e-6 + 2.0 ** -40 + 2.0 ** -149
    assert lo.bound(1e-6, -10.0) == 1e-6 + 2.0 ** -40 + 10 * 2.0 ** -23
    assert lo.check_value(np.float32(-10.0), -10.0, 0.0) is None and lo.check_value(np.float32(-10.0), -10.00001, 0.0) is not None
    assert lo.check_value(math.nan, math.nan, 0.0) is None and lo.check_value(1.0, math.nan, 0.0) is not None
    assert lo.check_value(-math.inf, -math.inf, 0.0) is None and lo.check_value(-1e30, -math.inf, 0.0) is not None
    # n equal tokens: E / S is the relative error of a weight at t = 0 plus the truncation
    bits = np.full(1000, so.bf16_bits(np.float32(4.0)), dtype=np.uint16)
    assert lo.e_over_s(bits) == pytest.approx(2.0 ** -23 * (1 + 2.0 ** -10) + 2.0 ** -43, rel=1e-9)


@pytest.mark.parametrize("vocab,rows", [(32000, lo.GAUSSIAN_ROWS), (2 * C + 5, lo.GAUSSIAN_ROWS), (128256, 1), (152064, 1)])
def test_e_over_s_stays_under_the_cap_on_every_gaussian_row(vocab, rows):
    """the condition under which the bound cannot hide an error: E / S <= 8e-6 on every row the value tests use"""
    expected = lo.gaussian_expected(vocab, rows)
    assert len(expected) == rows
    worst = max(e for _, e in expected)
    print(f"vocab {vocab}: max E / S = {worst:.3e}")
    assert 0 < worst <= lo.E_OVER_S_CAP
    bits, T, target = lo.long_row(vocab) if rows == 1 else lo.gaussian_case(vocab, rows)
    assert len(set(T.tolist())) == rows                                              # temperatures that all differ within the call
    if rows > 1:
        assert expected[0][0]["rank"] == 0                                          # one target is a greedy token


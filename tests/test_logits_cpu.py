"""CPU tests of the logits processing: the host side of mm_process_logits (include/micromix_logits.h: the symbol, its prototype, every
status without device work, the overlap decision, the Python argument errors) and the numpy oracle itself (tests/logits_oracle.py
against torch's fp32 chain on the CPU, against hand-written rows, and the planted rounding cases the GPU test uses).  No kernel is
launched."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
import logits_oracle as lg

OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
A = 1 << 28                                                                         # a made-up, well aligned address
TOO_MANY = 65536                                                                    # rows beyond the limit


def call(logits=A, rows=TOO_MANY, vocab=100, ld_in=None, out=2 * A, ld_out=None, tokens=3 * A, ld_tok=64, n_seq=3, row_seq=4 * A,
         prompt_len=5 * A, total_len=6 * A, rep=7 * A, freq=8 * A, pres=9 * A, bias_idx=10 * A, bias_val=11 * A, n_bias=4, mask=12 * A,
         ld_mask=None):
    """mm_process_logits with made-up addresses.  No call of this file may reach a launch: the header puts every MM_ERR_BAD_ARG before
    every MM_ERR_UNSUPPORTED, so a call with rows > 0 carries something beyond a limit (by default the rows) and answers
    MM_ERR_UNSUPPORTED exactly when nothing about it is refused"""
    assert rows <= 0 or rows > 65535 or vocab > 1 << 20 or n_bias > 1 << 20 or (tokens and ld_tok > 1 << 24), "this call would launch"
    return _lib.load().mm_process_logits(logits, rows, vocab, vocab if ld_in is None else ld_in, out, vocab if ld_out is None else ld_out,
                                         tokens, ld_tok, n_seq, row_seq, prompt_len, total_len, rep, freq, pres, bias_idx, bias_val, n_bias,
                                         mask, (vocab + 31) // 32 if ld_mask is None else ld_mask, None)


ACCEPTED = UNS                                                                      # what call() answers when nothing is refused
NO_HISTORY = dict(tokens=None, row_seq=None, prompt_len=None, total_len=None, rep=None, freq=None, pres=None)
NO_BIAS = dict(bias_idx=None, bias_val=None, n_bias=0)


# ---- the C ABI and the Python op ---------------------------------------------------------------------------------------------------------
def test_symbol_prototype_and_python_surface():
    """fails without the feature: the symbol, LOGITS_EXPORTS and mixedgemm.process_logits do not exist there"""
    lib = _lib.load()
    assert _lib.LOGITS_EXPORTS == ("mm_process_logits",)
    assert not set(_lib.LOGITS_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.DIAG_EXPORTS) | set(_lib.CALIB_EXPORTS) | set(_lib.LOGPROB_EXPORTS))
    assert hasattr(lib, "mm_process_logits")
    f = lib.mm_process_logits
    v, i, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    assert f.restype is i
    assert f.argtypes == [v, i, i, ll, v, ll, v, ll, i, v, v, v, v, v, v, v, v, i, v, ll, v]
    assert _lib.constants(_lib.header_text("micromix_logits.h")) == {}              # no constant of the header reaches _lib
    assert lib.mm_version() == 660
    assert "process_logits" in mixedgemm.__all__ and callable(mixedgemm.process_logits)
    sig = inspect.signature(mixedgemm.process_logits).parameters
    assert list(sig) == ["logits", "out", "tokens", "prompt_len", "total_len", "row_seq", "repetition_penalty", "frequency_penalty",
                         "presence_penalty", "bias_idx", "bias_val", "allowed_mask"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in list(sig)[1:])
    assert sig["logits"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD


def test_no_new_mm_constant():
    have = {n for n in vars(_lib) if n.startswith("MM_") and isinstance(getattr(_lib, n), int)}
    want = set(_lib.constants(_lib.header_text("micromix_hip.h"))) | set(_lib.constants(_lib.header_text("micromix_diag.h")))
    assert have == want


def test_no_rows_and_every_optional_input_null():
    assert call(rows=0) == OK
    assert call(rows=0, logits=None, out=None, **NO_HISTORY, **NO_BIAS, mask=None) == OK
    assert call(rows=0, logits=A + 1) == OK                                         # the pointers are not looked at
    assert call() == ACCEPTED                                                       # everything given
    assert call(**NO_HISTORY, **NO_BIAS, mask=None) == ACCEPTED                     # the copy
    assert call(**NO_HISTORY) == ACCEPTED and call(**NO_BIAS) == ACCEPTED and call(mask=None) == ACCEPTED
    assert call(rep=None, freq=None, pres=None, row_seq=None) == ACCEPTED
    assert call(ld_in=103, ld_out=100, logits=A + 2, out=2 * A + 6) == ACCEPTED     # strides and alignments of their own


def test_bad_arguments_without_device_work():
    for kw in (dict(rows=-1), dict(vocab=0), dict(vocab=-3), dict(ld_in=99), dict(ld_out=99),
               dict(logits=None), dict(out=None), dict(logits=A + 1), dict(out=2 * A + 1),
               dict(prompt_len=None), dict(total_len=None), dict(prompt_len=None, total_len=None),     # tokens without both lengths
               dict(NO_HISTORY, prompt_len=5 * A), dict(NO_HISTORY, total_len=6 * A), dict(NO_HISTORY, row_seq=4 * A),
               dict(NO_HISTORY, rep=7 * A), dict(NO_HISTORY, freq=8 * A), dict(NO_HISTORY, pres=9 * A),
               dict(n_seq=0), dict(n_seq=-1), dict(ld_tok=0), dict(ld_tok=-5),
               dict(bias_idx=None), dict(bias_val=None), dict(n_bias=-1), dict(bias_idx=None, bias_val=None),  # n_bias 4, null arrays
               dict(n_bias=0),                                                      # arrays, no entries
               dict(ld_mask=3), dict(ld_mask=0), dict(vocab=97, ld_in=100, ld_out=100, ld_mask=3),
               dict(tokens=3 * A + 2), dict(row_seq=4 * A + 2), dict(prompt_len=5 * A + 1), dict(total_len=6 * A + 2), dict(rep=7 * A + 2),
               dict(freq=8 * A + 1), dict(pres=9 * A + 3), dict(bias_idx=10 * A + 2), dict(bias_val=11 * A + 2), dict(mask=12 * A + 2)):
        assert call(**kw) == BAD, kw
    # a refusal comes before a limit, and the sizes before rows == 0
    assert call(rows=0, vocab=0) == BAD and call(vocab=(1 << 20) + 1, n_bias=-1) == BAD and call(rows=0, ld_mask=3) == BAD
    assert call(vocab=(1 << 20) + 1, logits=None) == BAD
    assert call(ld_mask=4) == ACCEPTED and call(vocab=97, ld_in=100, ld_out=100, ld_mask=4) == ACCEPTED and call(vocab=96, ld_mask=3) == ACCEPTED


def test_unsupported_without_device_work():
    assert call(rows=0, vocab=(1 << 20) + 1) == UNS and call(rows=TOO_MANY) == UNS and call(rows=3, vocab=(1 << 20) + 1) == UNS
    assert call(rows=0, ld_tok=(1 << 24) + 1) == UNS and call(rows=0, n_bias=(1 << 20) + 1) == UNS
    assert call(rows=3, ld_tok=(1 << 24) + 1) == UNS and call(rows=3, n_bias=(1 << 20) + 1) == UNS
    assert call(rows=0, ld_tok=1 << 24, n_bias=1 << 20, vocab=1 << 20) == OK        # the limits themselves are accepted
    assert call(rows=0, **dict(NO_HISTORY, ld_tok=(1 << 24) + 1)) == OK             # no history: ld_tok says nothing


def test_the_overlap_decision():
    """identical is the in-place form; anything else that shares an element is refused; disjoint is allowed.  Decided from the addresses:
    3 rows of 100 columns, 120 apart, are a span of 340 elements = 680 bytes"""
    def decide(out, ld_out=120, ld_in=120, rows=3):
        return call(rows=rows, logits=A, ld_in=ld_in, out=out, ld_out=ld_out, ld_tok=(1 << 24) + 1)

    assert decide(A) == ACCEPTED                                                    # identical
    for out, ld_out in ((A + 2 * 120, 120),                                         # shifted by one row
                        (A + 2, 120), (A - 2, 120), (A + 678, 120), (A - 678, 120),  # by one element; the last shared element
                        (A, 121), (A, 100),                                         # the same start, another stride: not the in-place form
                        (A + 2 * 100, 240)):                                        # interleaved rows still share the span
        assert decide(out, ld_out) == BAD, (out - A, ld_out)
        assert overlap(A, 120, out, ld_out, 3, 100)
    for out, ld_out in ((A + 680, 120), (A - 680, 120), (A + 680, 100), (A - 2 * (2 * 333 + 100), 333), (2 * A, 120)):   # disjoint, touching included
        assert decide(out, ld_out) == ACCEPTED, (out - A, ld_out)
        assert not overlap(A, 120, out, ld_out, 3, 100)
    assert decide(A + 2 * 120, rows=1) == ACCEPTED and decide(A + 2 * 99, rows=1) == BAD   # one row of 100 columns


def overlap(a, ld_a, b, ld_b, rows, vocab):
    """the header's words: the spans of (rows - 1) ld + vocab elements meet, and it is not the in-place form"""
    ea, eb = a + 2 * ((rows - 1) * ld_a + vocab), b + 2 * ((rows - 1) * ld_b + vocab)
    return not (a == b and ld_a == ld_b) and a < eb and b < ea


def test_python_argument_errors():
    lgt = torch.zeros((3, 100), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.process_logits(lgt)
    with pytest.raises(TypeError, match="bfloat16"):
        mixedgemm.process_logits(lgt.float())
    with pytest.raises(TypeError, match="logits"):
        mixedgemm.process_logits(None)
    with pytest.raises(TypeError):
        mixedgemm.process_logits(lgt, 3)                                            # keyword-only


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------------
def to_torch(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def from_torch(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_the_conversions_are_torchs():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(1 << 16).astype(np.float32) * np.float32(100.0)
    x[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 3.4e38, 1e-40, -1e-45]        # overflow to inf, subnormals
    x[8] = np.frombuffer(np.uint32(0x3F808000).tobytes(), dtype=np.float32)[0]      # a tie: to even, down
    x[9] = np.frombuffer(np.uint32(0x3F818000).tobytes(), dtype=np.float32)[0]      # a tie: to even, up
    got = lg.f32_to_bf16(x)
    want = from_torch(torch.from_numpy(x).to(torch.bfloat16))
    assert got[8] == 0x3F80 and got[9] == 0x3F82 and got[4] == 0x7FC0 and got[5] == 0x7F80
    is_nan = np.isnan(x)                                                            # torch's NaN bits depend on the path its conversion takes
    assert np.array_equal(got[~is_nan], want[~is_nan]) and np.isnan(lg.bf16_to_f32(want[is_nan])).all() and is_nan.sum() == 1
    every = np.arange(1 << 16, dtype=np.uint16)
    back = lg.f32_to_bf16(lg.bf16_to_f32(every))
    nan = np.isnan(lg.bf16_to_f32(every))
    assert np.array_equal(back[~nan], every[~nan]) and (back[nan] == 0x7FC0).all()   # a copy, up to the NaN


def torch_chain(bits, tokens, P, N, theta, a_f, a_p, bias_idx, bias_val, mask_bool):
    """what a caller writes today, on the CPU in fp32"""
    vocab = len(bits)
    x = to_torch(bits).float()
    ids = torch.from_numpy(tokens[:N].astype(np.int64))
    seen = torch.zeros(vocab, dtype=torch.bool)
    seen[ids] = True
    counts = torch.zeros(vocab, dtype=torch.float32).scatter_add(0, ids[P:], torch.ones(N - P))
    x = torch.where(seen, torch.where(x < 0, x * theta, x / theta), x)
    x = x - a_f * counts
    x = x - a_p * (counts > 0)
    x = x.index_put((torch.from_numpy(bias_idx.astype(np.int64)),), x[torch.from_numpy(bias_idx.astype(np.int64))] + torch.from_numpy(bias_val))
    x = x.masked_fill(~torch.from_numpy(mask_bool), float("-inf"))
    return from_torch(x.to(torch.bfloat16))


@pytest.mark.parametrize("vocab", [33, 1000, 8193, 32000])
def test_the_oracle_equals_the_torch_chain_on_gaussian_rows(vocab):
    rng = np.random.default_rng(vocab)
    for trial in range(4):
        bits = lg.f32_to_bf16((rng.standard_normal(vocab) * 3.0).astype(np.float32))
        ld_tok = 300
        tokens = rng.integers(0, min(vocab, 50 + 40 * trial), (1, ld_tok)).astype(np.int32)   # heavy repeats
        P, N = 100, 280
        theta, a_f, a_p = np.float32(1.0 + 0.3 * (trial + 1)), np.float32(0.1 * (trial + 1)), np.float32(0.37 * trial)
        bias_idx = rng.permutation(vocab)[:min(vocab, 20)].astype(np.int32)         # distinct: index_put has no rule for duplicates
        bias_val = (rng.standard_normal(len(bias_idx)) * 5.0).astype(np.float32)
        mask_bool = rng.random(vocab) < 0.7
        words = np.zeros((vocab + 31) // 32 * 32, dtype=np.uint8)
        words[:vocab] = mask_bool
        mask_words = np.packbits(words.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).view(np.int32)
        got = lg.row(bits, tokens=tokens, s=0, prompt_len=P, total_len=N, theta=theta, alpha_f=a_f, alpha_p=a_p, bias_idx=bias_idx,
                     bias_val=bias_val, mask_words=mask_words)
        want = torch_chain(bits, tokens[0], P, N, float(theta), float(a_f), float(a_p), bias_idx, bias_val, mask_bool)
        assert np.array_equal(got, want), (vocab, trial, int((got != want).sum()))
        assert (got != bits).sum() > vocab // 4                                     # and the row did change


def test_the_oracle_on_hand_written_rows():
    b = lambda *xs: lg.f32_to_bf16(np.array(xs, dtype=np.float32))
    f = lambda bits: lg.bf16_to_f32(bits).tolist()
    bits = b(2.0, -2.0, 4.0, -4.0, 1.0, 0.5)
    tokens = np.array([[0, 1, 9, -1, 2, 2, 3, 2 ** 31 - 1, 6, 0]], dtype=np.int32)  # prompt [0, 1, 9, -1], output [2, 2, 3, ..]
    kw = dict(tokens=tokens, s=0, prompt_len=4, total_len=8)
    assert f(lg.row(bits, **kw)) == [2.0, -2.0, 4.0, -4.0, 1.0, 0.5]                # nothing asked for
    assert f(lg.row(bits, theta=2.0, **kw)) == [1.0, -4.0, 2.0, -8.0, 1.0, 0.5]     # prompt and output, 4 and 5 unseen
    assert f(lg.row(bits, alpha_f=0.5, **kw)) == [2.0, -2.0, 3.0, -4.5, 1.0, 0.5]   # output only, c = 2 and 1
    assert f(lg.row(bits, alpha_p=0.25, **kw)) == [2.0, -2.0, 3.75, -4.25, 1.0, 0.5]
    assert f(lg.row(bits, theta=2.0, alpha_f=0.5, alpha_p=0.25, **kw)) == [1.0, -4.0, 0.75, -8.75, 1.0, 0.5]
    for off in (1.0, 0.0, -1.0, np.inf, np.nan):                                    # theta: 1 is the identity, the others are off
        assert np.array_equal(lg.row(bits, theta=off, **kw), bits)
    assert np.array_equal(lg.row(bits, alpha_f=np.nan, alpha_p=np.nan, **kw), bits)
    # the lengths: clamped; total_len 10 reaches the 0 at the end (c_0 = 1) and the 6 (outside the vocabulary)
    assert f(lg.row(bits, alpha_p=1.0, tokens=tokens, s=0, prompt_len=4, total_len=99)) == [1.0, -2.0, 3.0, -5.0, 1.0, 0.5]
    assert f(lg.row(bits, theta=2.0, alpha_p=1.0, tokens=tokens, s=0, prompt_len=9, total_len=3)) == [1.0, -4.0, 2.0, -8.0, 1.0, 0.5]   # P = N = 9
    assert np.array_equal(lg.row(bits, theta=2.0, alpha_p=1.0, tokens=tokens, s=0, prompt_len=-5, total_len=-5), bits)          # N = 0
    assert np.array_equal(lg.row(bits, theta=2.0, alpha_p=1.0, tokens=tokens, s=1, prompt_len=4, total_len=8), bits)            # no such sequence
    assert np.array_equal(lg.row(bits, theta=2.0, alpha_p=1.0, tokens=tokens, s=-1, prompt_len=4, total_len=8), bits)
    # bias: the highest j wins, ids outside are ignored, inf - inf is NaN, written 0x7FC0
    assert f(lg.row(bits, bias_idx=[1, 1, -1, 6, 4], bias_val=[10.0, 20.0, 5.0, 5.0, -np.inf])) == [2.0, 18.0, 4.0, -4.0, -np.inf, 0.5]
    assert f(lg.row(bits, bias_idx=[4, 6, -1, 1, 1], bias_val=[-np.inf, 5.0, 5.0, 20.0, 10.0])) == [2.0, 8.0, 4.0, -4.0, -np.inf, 0.5]
    ninf = bits.copy()
    ninf[0] = lg.NINF_BITS
    assert lg.row(ninf, bias_idx=[0], bias_val=[np.inf])[0] == lg.NAN_BITS
    ninf[0] = 0xFFC1                                                                 # a negative NaN with a payload
    assert lg.row(ninf)[0] == lg.NAN_BITS
    # mask: bits beyond the vocabulary are garbage; the mask wins over a bias
    words = np.array([0b100101 | ~0b111111], dtype=np.int64).astype(np.int32)
    assert f(lg.row(bits, mask_words=words)) == [2.0, -np.inf, 4.0, -np.inf, -np.inf, 0.5]
    assert f(lg.row(bits, bias_idx=[1, 2], bias_val=[np.inf, 1.0], mask_words=words)) == [2.0, -np.inf, 5.0, -np.inf, -np.inf, 0.5]
    # rows(): row_seq maps rows onto one buffer under their own lengths
    out = lg.rows(np.stack([bits, bits]), tokens=tokens, row_seq=[0, 0], prompt_len=[4, 4], total_len=[5, 6], alpha_f=[1.0, 1.0])
    assert f(out[0]) == [2.0, -2.0, 3.0, -4.0, 1.0, 0.5] and f(out[1]) == [2.0, -2.0, 2.0, -4.0, 1.0, 0.5]


def test_the_planted_rounding_cases_exist():
    """the only inputs on which a reciprocal-based divide or a contracted fma shows after the bf16 rounding; kept for the GPU test"""
    xb, theta = lg.division_cases()
    print(f"division cases: {len(xb)} of {lg.DRAWS} draws")
    assert len(xb) >= 128
    q = lg.bf16_to_f32(xb) / theta
    b = lg.f32_to_bf16(q)
    assert ((lg.f32_to_bf16(np.nextafter(q, np.float32(np.inf))) != b) | (lg.f32_to_bf16(np.nextafter(q, np.float32(-np.inf))) != b)).all()
    assert (lg.bf16_to_f32(xb) > 0).all() and np.isfinite(theta).all() and (theta > 0).all()
    xb, alpha, c = lg.fma_cases()
    print(f"fma cases: {len(xb)} of {lg.DRAWS} draws")
    assert len(xb) >= 128
    x = lg.bf16_to_f32(xb)
    two = x - alpha * c.astype(np.float32)
    one = (x.astype(np.float64) - alpha.astype(np.float64) * c).astype(np.float32)
    assert (lg.f32_to_bf16(two) != lg.f32_to_bf16(one)).all() and (c >= 1).all()
    # and the oracle takes the two-rounding side on them
    k = 0
    tokens = np.full((1, int(c[k])), 0, dtype=np.int32)
    assert lg.row(xb[k:k + 1], tokens=tokens, s=0, prompt_len=0, total_len=int(c[k]), alpha_f=alpha[k])[0] == lg.f32_to_bf16(two[k:k + 1])[0]

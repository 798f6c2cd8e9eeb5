"""GPU tests of mixedgemm.process_logits.  The reference is tests/logits_oracle.py, the rule of include/micromix_logits.h in numpy
float32, and EVERY comparison is bit equality with it: there is no tolerance in this file.

1 walk        vocab in {1, 7, 33, C - 1, C, C + 1, 2 C + 7} (C = MM_ARGMAX_CHUNK = 8192), 1 - 3 rows, pointer offsets 0 .. 7 elements for
              logits and for out independently (64 pairs), odd and even row strides that differ between the two, NaN around the logits, a
              sentinel around out that must survive; every feature on, so each path of the store is taken with the history, bias and mask
2 history     tokens at columns 0, C - 1, C, vocab - 1; ids -1, vocab, 2^31 - 1; P = 0, P = N, N = 0, clamped lengths; a token of the
              prompt only; 1, 2, 300 and 70 000 repeats; three rows on one buffer; a row_seq out of range
3 parameters  each penalty alone and all together; theta in {1, 0, -1, inf, NaN}; NaN alpha; negative, +-0, +-inf and NaN logits; the
              planted rounding cases of tests/logits_oracle.py (a divide one ulp off, or x - a c as one fma, would differ on each)
4 bias        duplicates and the reversed list, ids out of range, +-inf, +inf onto -inf, n_bias 1 and 5 000
5 mask        garbage bits beyond the vocabulary, one allowed token at every part edge, an all-clear row (then sample_rows gives
              argmax_rows' answer), mask over bias
6 forms       in place == out of place, all null == a copy, two runs identical
7 capture     one hipGraph of process_logits -> sample_rows replayed after everything was rewritten in place
8 wrapper     shape and dtype of a valid call; argument errors before any launch"""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
import logits_oracle as lg

pytestmark = pytest.mark.gpu

C = _lib.MM_ARGMAX_CHUNK
NAN_BITS, NINF_BITS, PINF_BITS, SENTINEL = 0x7FC0, 0xFF80, 0x7F80, 0x1234
DEV = "cuda:0"

f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)
i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(DEV)
opt = lambda a, conv: None if a is None else conv(a)
bits_of = lambda x: lg.f32_to_bf16(np.asarray(x, dtype=np.float32))


def place(bits, ld, offset, fill):
    """bits [rows, vocab] as a bf16 device view at element `offset` of its 16-byte aligned allocation, rows ld apart, `fill`
    everywhere else; returns (view, whole allocation)"""
    rows, vocab = bits.shape
    buf = np.full(offset + rows * ld + 16, fill, dtype=np.uint16)
    buf[offset: offset + rows * ld].reshape(rows, ld)[:, :vocab] = bits
    t = torch.from_numpy(buf.view(np.int16)).to(DEV).view(torch.bfloat16)
    view = t[offset: offset + rows * ld].view(rows, ld)[:, :vocab]
    assert view.data_ptr() == t.data_ptr() + 2 * offset and t.data_ptr() % 16 == 0
    return view, t


def to_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def run(bits, *, ld_in=None, off_in=0, ld_out=None, off_out=0, inplace=False, **p):
    """mixedgemm.process_logits on `bits` laid out as asked, the parameters of lg.rows() uploaded as they are; returns the out bits
    after checking that nothing around them was written"""
    rows, vocab = bits.shape
    x, x_whole = place(bits, vocab if ld_in is None else ld_in, off_in, NAN_BITS)
    if inplace:
        out, whole, ld_out, off_out = x, x_whole, vocab if ld_in is None else ld_in, off_in
    else:
        ld_out = vocab if ld_out is None else ld_out
        out, whole = place(np.full((rows, vocab), SENTINEL, dtype=np.uint16), ld_out, off_out, SENTINEL)
    got = mixedgemm.process_logits(x, out=out, tokens=opt(p.get("tokens"), i32), prompt_len=opt(p.get("prompt_len"), i32),
                                   total_len=opt(p.get("total_len"), i32), row_seq=opt(p.get("row_seq"), i32),
                                   repetition_penalty=opt(p.get("theta"), f32), frequency_penalty=opt(p.get("alpha_f"), f32),
                                   presence_penalty=opt(p.get("alpha_p"), f32), bias_idx=opt(p.get("bias_idx"), i32),
                                   bias_val=opt(p.get("bias_val"), f32), allowed_mask=opt(p.get("mask"), i32))
    torch.cuda.synchronize()
    assert got is out
    result = to_bits(out)
    around = to_bits(whole).copy()
    around[off_out: off_out + rows * ld_out].reshape(rows, ld_out)[:, :vocab] = NAN_BITS if inplace else SENTINEL
    assert (around == (NAN_BITS if inplace else SENTINEL)).all(), "something outside the rows of out was written"
    if not inplace:
        assert np.array_equal(to_bits(x), bits), "the logits were written"
    return result


def same(got, want):
    assert got.shape == want.shape
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{len(bad)} elements differ, first at {bad[0].tolist()}: got {int(got[tuple(bad[0])]):#06x}, want {int(want[tuple(bad[0])]):#06x}"


def gaussian(rng, rows, vocab, scale=3.0):
    return bits_of(rng.standard_normal((rows, vocab)) * scale)


def everything(rng, rows, vocab, ld_tok=96, n_bias=9):
    """parameters with every feature on, the history dense enough to repeat"""
    span = min(vocab, 40)
    tokens = rng.integers(-1, vocab + 1, (rows, ld_tok)).astype(np.int32)
    tokens[:, ::2] = (rng.integers(0, span, (rows, ld_tok // 2)) * (vocab // span)).astype(np.int32)
    tokens[:, 1] = vocab - 1
    bias_idx = rng.integers(-2, vocab + 2, (rows, n_bias)).astype(np.int32)
    bias_idx[:, 0] = bias_idx[:, -1] = tokens[:, 0]                                 # a duplicate, on a penalised column
    return dict(tokens=tokens, prompt_len=rng.integers(0, ld_tok // 2, rows), total_len=rng.integers(ld_tok // 2, ld_tok + 5, rows),
                theta=(1.0 + rng.random(rows)).astype(np.float32), alpha_f=rng.random(rows).astype(np.float32),
                alpha_p=rng.random(rows).astype(np.float32), bias_idx=bias_idx,
                bias_val=(rng.standard_normal((rows, n_bias)) * 4).astype(np.float32),
                mask=rng.integers(-2 ** 31, 2 ** 31, (rows, (vocab + 31) // 32 + 1)).astype(np.int32))


def first_rows(p, rows):
    return {k: v[:rows] for k, v in p.items()}


# ---- 1. the edges of the walk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1, 7, 33, C - 1, C, C + 1, 2 * C + 7])
def test_walk_at_every_pair_of_alignments(vocab):
    rng = np.random.default_rng(vocab)
    bits = gaussian(rng, 3, vocab)
    p = everything(rng, 3, vocab)
    want = lg.rows(bits, **p)                                                       # once: the layout is no input of the rule
    assert (want != bits).any() or vocab == 1
    odd = lambda n: n | 1
    for off_in in range(8):
        for off_out in range(8):
            k = 8 * off_in + off_out
            rows = 1 + k % 3
            ld_in, ld_out = (odd(vocab + 3), odd(vocab + 5)) if k % 2 else (vocab + 8, vocab + (off_in & 2))
            got = run(bits[:rows], ld_in=ld_in, off_in=off_in, ld_out=ld_out, off_out=off_out, **first_rows(p, rows))
            same(got, want[:rows])
    for off in (0, 3):                                                              # and the copy, over the same store paths
        same(run(bits, ld_in=odd(vocab + 3), off_in=off, ld_out=vocab, off_out=1), lg.rows(bits))


# ---- 2. history --------------------------------------------------------------------------------------------------------------------------------
def test_history():
    vocab, ld_tok = 2 * C + 7, 70400
    rng = np.random.default_rng(2)
    once, twice, many, flood, prompt_only = 5, C + 9, 2 * C + 1, 77, 4000
    seq0 = np.full(ld_tok, -1, dtype=np.int32)
    seq0[:10] = [prompt_only, 0, C - 1, C, vocab - 1, -1, vocab, 2 ** 31 - 1, -2 ** 31, prompt_only]
    seq0[10:20] = [0, C - 1, C, vocab - 1, once, twice, twice, vocab, -1, 2 ** 31 - 1]
    seq0[20:320] = many
    seq0[320:70320] = flood
    seq1 = rng.integers(0, 64, ld_tok).astype(np.int32) * 257                       # a second buffer, read by three rows
    tokens = np.stack([seq0, seq1])
    cases = [  # (sequence, prompt_len, total_len)
        (0, 0, ld_tok),            # P = 0: everything is output; counts 1, 2, 300, 70 000
        (0, 10, 70320),            # a prompt of 10: prompt_only is seen, never counted
        (0, 321, 321),             # P = N: repetition only
        (0, 0, 0),                 # N = 0
        (0, 10, ld_tok + 1000),    # total_len beyond the buffer: clamped
        (0, 500, 100),             # prompt_len > total_len: N = P = 500
        (0, -7, 15),               # a negative prompt_len is 0
        (1, 5, 50), (1, 0, 300), (1, 200, 70000),                                   # three rows, three lengths, one buffer
        (2, 10, 100), (-1, 10, 100), (2 ** 31 - 1, 10, 100),                        # no such sequence: an empty history
    ]
    rows = len(cases)
    bits = gaussian(rng, rows, vocab)
    p = dict(tokens=tokens, row_seq=[c[0] for c in cases], prompt_len=[c[1] for c in cases], total_len=[c[2] for c in cases],
             theta=np.full(rows, 1.25, np.float32), alpha_f=np.full(rows, 0.0078125 * 3, np.float32), alpha_p=np.full(rows, 0.4, np.float32))
    want = lg.rows(bits, **p)
    # the oracle sees what the case is about
    seen, c = lg.history(tokens, 0, 0, ld_tok, vocab)
    assert [int(c[i]) for i in (once, twice, many, flood)] == [1, 2, 300, 70000] and c[prompt_only] == 2 and c.sum() == 70000 + 300 + 13
    seen, c = lg.history(tokens, 0, 10, 70320, vocab)
    assert seen[prompt_only] and c[prompt_only] == 0 and want[1, prompt_only] != bits[1, prompt_only]
    assert np.array_equal(want[3], bits[3]) and all(np.array_equal(want[r], bits[r]) for r in (10, 11, 12))
    assert (want[0] != bits[0]).sum() >= 5
    same(run(bits, **p), want)
    same(run(bits, ld_in=vocab + 3, off_in=5, inplace=True, **p), want)
    # without row_seq row r reads sequence r, and rows beyond n_seq have none
    q = dict(p, row_seq=None)
    want = lg.rows(bits, **q)
    assert all(np.array_equal(want[r], bits[r]) for r in range(2, rows)) and not np.array_equal(want[1], bits[1])
    same(run(bits, **q), want)


# ---- 3. parameters -----------------------------------------------------------------------------------------------------------------------------
SPECIAL = [NAN_BITS, 0xFFC1, PINF_BITS, NINF_BITS, 0x0000, 0x8000, 0x0001, 0x8001, 0x7F7F, 0xFF7F]   # NaNs, infs, zeros, subnormals, the largest


@pytest.mark.parametrize("given", ["theta", "alpha_f", "alpha_p", "theta alpha_f", "alpha_f alpha_p", "theta alpha_p", "theta alpha_f alpha_p"])
def test_penalties_alone_and_together(given):
    vocab, ld_tok = C + 1, 64
    rng = np.random.default_rng(3)
    theta = np.array([1.0, 0.0, -1.0, np.inf, np.nan, 1.5, 0.75, 3.0, -np.inf, 1e-30, 1.3], np.float32)
    alpha_f = np.array([0.5, np.nan, -0.25, 0.0, np.inf, 0.1, 1e-40, 2.0, 0.3, -np.inf, 1e30], np.float32)
    alpha_p = np.array([np.nan, 0.5, -0.25, 0.0, 0.7, np.inf, 1e-40, 2.0, -np.inf, 0.3, 1e38], np.float32)
    rows = len(theta)
    bits = gaussian(rng, rows, vocab)
    cols = rng.permutation(vocab)[:2 * len(SPECIAL)]
    cols[:4] = [0, C - 1, C, 7]
    bits[:, cols[:len(SPECIAL)]] = SPECIAL                                          # special values that the history names ...
    bits[:, cols[len(SPECIAL):]] = SPECIAL                                          # ... and that it does not
    tokens = rng.integers(0, vocab, (rows, ld_tok)).astype(np.int32)
    tokens[:, :len(SPECIAL)] = cols[:len(SPECIAL)]                                  # in the prompt
    tokens[:, 20:20 + len(SPECIAL)] = cols[:len(SPECIAL)]                           # and in the output,
    tokens[:, 40:45] = cols[:5]                                                     # some of them twice
    p = dict(tokens=tokens, prompt_len=np.full(rows, 15), total_len=np.full(rows, 60))
    for name in given.split():
        p[name] = dict(theta=theta, alpha_f=alpha_f, alpha_p=alpha_p)[name]
    want = lg.rows(bits, **p)
    if given == "theta":
        for r in (0, 1, 2, 3, 4, 8):                                                # 1 is the identity, the others are off: a copy up to NaN
            assert np.array_equal(want[r], lg.rows(bits[r:r + 1])[0])
        assert (want[5] != bits[5]).sum() > 30
    if given == "alpha_f":
        assert np.array_equal(want[1], lg.rows(bits[1:2])[0]) and (want[0] != bits[0]).sum() > 20
    assert (want[:, cols[0]] == NAN_BITS).all() and (want[:, cols[1]] == NAN_BITS).all()                 # 0x7FC0 out, whatever came in
    same(run(bits, **p), want)


def test_the_planted_rounding_cases():
    """theta and alpha are per-row parameters, so a case takes a row of its own; its column is the case number mod the vocabulary"""
    vocab = 7
    xb, theta = lg.division_cases()
    n = len(xb)
    assert n >= 128
    rng = np.random.default_rng(4)
    bits = gaussian(rng, n, vocab)
    col = np.arange(n) % vocab
    bits[np.arange(n), col] = xb
    tokens = col[:, None].astype(np.int32)
    p = dict(tokens=tokens, prompt_len=np.ones(n), total_len=np.ones(n), theta=theta)
    want = lg.rows(bits, **p)
    q = lg.bf16_to_f32(xb) / theta
    assert np.array_equal(want[np.arange(n), col], lg.f32_to_bf16(q))
    same(run(bits, **p), want)

    xb, alpha, c = lg.fma_cases()
    n = len(xb)
    assert n >= 128
    bits = gaussian(rng, n, vocab)
    col = np.arange(n) % vocab
    bits[np.arange(n), col] = xb
    tokens = np.where(np.arange(64)[None, :] < c[:, None], col[:, None], -1).astype(np.int32)
    p = dict(tokens=tokens, prompt_len=np.zeros(n), total_len=np.full(n, 64), alpha_f=alpha)
    want = lg.rows(bits, **p)
    two = lg.bf16_to_f32(xb) - alpha * c.astype(np.float32)
    assert np.array_equal(want[np.arange(n), col], lg.f32_to_bf16(two))
    same(run(bits, **p), want)


# ---- 4. bias -----------------------------------------------------------------------------------------------------------------------------------
def test_bias():
    vocab = 2 * C + 7
    rng = np.random.default_rng(5)
    bits = gaussian(rng, 2, vocab)
    bits[:, 11] = NINF_BITS
    idx = np.array([[3, 3, C, 3, -1, vocab, 2 ** 31 - 1, -2 ** 31, C - 1, vocab - 1, 11, 12, 13, C, 0]] * 2, dtype=np.int32)
    val = np.array([[1.0, 2.0, 5.0, 4.0, 9.0, 9.0, 9.0, 9.0, -1.5, 0.25, np.inf, np.inf, -np.inf, -5.0, 1e-3]] * 2, dtype=np.float32)
    want = lg.rows(bits, bias_idx=idx, bias_val=val)
    x = lg.bf16_to_f32(bits)
    assert want[0, 3] == bits_of(x[0, 3] + np.float32(4.0)) and want[0, C] == bits_of(x[0, C] + np.float32(-5.0))   # the highest j
    assert want[0, 11] == NAN_BITS and want[0, 12] == PINF_BITS and want[0, 13] == NINF_BITS
    same(run(bits, bias_idx=idx, bias_val=val), want)
    back = lg.rows(bits, bias_idx=idx[:, ::-1], bias_val=val[:, ::-1])              # the reversed list: the other duplicate wins
    assert back[0, 3] == bits_of(x[0, 3] + np.float32(1.0)) and back[0, 3] != want[0, 3] and back[0, C] != want[0, C]
    same(run(bits, bias_idx=idx[:, ::-1], bias_val=val[:, ::-1]), back)
    same(run(bits, bias_idx=idx[:, :1], bias_val=val[:, :1]), lg.rows(bits, bias_idx=idx[:, :1], bias_val=val[:, :1]))   # n_bias = 1
    idx = rng.integers(-5, vocab + 5, (2, 5000)).astype(np.int32)                   # n_bias = 5 000, with its share of duplicates
    val = (rng.standard_normal((2, 5000)) * 3).astype(np.float32)
    assert len(np.unique(idx[0])) < 5000
    want = lg.rows(bits, bias_idx=idx, bias_val=val)
    same(run(bits, ld_in=vocab + 1, off_in=1, ld_out=vocab + 2, off_out=6, bias_idx=idx, bias_val=val), want)


# ---- 5. mask -----------------------------------------------------------------------------------------------------------------------------------
def words_of(allowed_cols, vocab, n_words, garbage):
    w = np.zeros(n_words * 32, dtype=np.uint8)
    w[list(allowed_cols)] = 1
    w[vocab:] = garbage                                                             # bits at and beyond the vocabulary
    return np.packbits(w.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).view(np.int32)


def test_mask():
    vocab = 2 * C + 7
    assert vocab % 32
    n_words = (vocab + 31) // 32 + 2                                                # ld_mask beyond what is needed
    edges = [0, 1, 31, 32, C - 1, C, 2 * C - 1, 2 * C, vocab - 1]
    rng = np.random.default_rng(6)
    rows = len(edges) + 2
    bits = gaussian(rng, rows, vocab)
    mask = np.stack([words_of([e], vocab, n_words, 1) for e in edges] + [words_of([], vocab, n_words, 1),
                                                                        words_of(range(0, vocab, 3), vocab, n_words, 0)])
    want = lg.rows(bits, mask=mask)
    for r, e in enumerate(edges):                                                   # one token left, at a part edge
        assert (want[r] != NINF_BITS).sum() == 1 and want[r, e] == bits[r, e]
    assert (want[len(edges)] == NINF_BITS).all()                                    # all clear, whatever the garbage says
    got = run(bits, ld_in=vocab + 1, off_in=3, ld_out=vocab + 5, off_out=2, mask=mask)
    same(got, want)
    # an all -inf row: sample_rows falls back to argmax_rows' answer
    dead = torch.from_numpy(got[len(edges):len(edges) + 1].view(np.int16).copy()).to(DEV).view(torch.bfloat16)
    u = torch.full((1,), 0.7, dtype=torch.float32, device=DEV)
    assert torch.equal(mixedgemm.sample_rows(dead, u), mixedgemm.argmax_rows(dead))
    # the mask wins over a bias on the same column
    idx = np.array([[edges[4], 5, 6]] * rows, dtype=np.int32)
    val = np.array([[np.inf, np.inf, 2.0]] * rows, dtype=np.float32)
    want = lg.rows(bits, mask=mask, bias_idx=idx, bias_val=val)
    assert want[0, 5] == NINF_BITS and want[4, edges[4]] == PINF_BITS and want[len(edges), 6] == NINF_BITS
    same(run(bits, mask=mask, bias_idx=idx, bias_val=val), want)


# ---- 6. forms ----------------------------------------------------------------------------------------------------------------------------------
def test_forms():
    vocab = 2 * C + 7
    rng = np.random.default_rng(7)
    bits = gaussian(rng, 3, vocab)
    bits[0, :len(SPECIAL)] = SPECIAL
    p = everything(rng, 3, vocab, ld_tok=600, n_bias=40)
    want = lg.rows(bits, **p)
    apart = run(bits, ld_in=vocab + 3, off_in=1, ld_out=vocab + 4, off_out=5, **p)
    again = run(bits, ld_in=vocab + 3, off_in=1, ld_out=vocab + 4, off_out=5, **p)
    inplace = run(bits, ld_in=vocab + 3, off_in=1, inplace=True, **p)
    assert apart.tobytes() == again.tobytes() == inplace.tobytes() == want.tobytes()
    copy = run(bits, ld_in=vocab + 3, off_in=1, ld_out=vocab, off_out=0)            # all null: a copy, up to the NaN
    expect = bits.copy()
    expect[np.isnan(lg.bf16_to_f32(bits))] = NAN_BITS
    assert copy.tobytes() == expect.tobytes() and (copy != bits).sum() == 1         # 0xFFC1 became 0x7FC0
    # out = None allocates; two disjoint views of one allocation are accepted, a shifted one is refused
    x, _ = place(bits, vocab, 0, NAN_BITS)
    out = mixedgemm.process_logits(x)
    assert out.data_ptr() != x.data_ptr() and to_bits(out).tobytes() == expect.tobytes()
    both = torch.zeros((6, vocab), dtype=torch.bfloat16, device=DEV)
    both[:3] = x
    assert mixedgemm.process_logits(both[:3], out=both[3:]) .data_ptr() == both[3:].data_ptr() and to_bits(both[3:]).tobytes() == expect.tobytes()
    with pytest.raises(RuntimeError, match="process_logits"):
        mixedgemm.process_logits(both[:3], out=both[1:4])
    torch.cuda.synchronize()


# ---- 7. capture --------------------------------------------------------------------------------------------------------------------------------
def test_one_graph_serves_rewritten_requests():
    vocab, rows, ld_tok, n_bias = 2 * C + 7, 3, 200, 12
    rng = np.random.default_rng(8)
    n_words = (vocab + 31) // 32

    def request(k):
        p = everything(np.random.default_rng(100 + k), rows, vocab, ld_tok=ld_tok, n_bias=n_bias)
        p["mask"] = p["mask"][:, :n_words]
        keep = np.random.default_rng(200 + k).permutation(vocab)[:50]               # few tokens allowed: the filters matter to the draw
        p["mask"] = np.stack([words_of(keep, vocab, n_words, 1)] * rows)
        return gaussian(np.random.default_rng(300 + k), rows, vocab), p, np.random.default_rng(400 + k).random(rows).astype(np.float32)

    bits, p, u = request(0)
    dev = dict(logits=torch.from_numpy(bits.view(np.int16).copy()).to(DEV).view(torch.bfloat16), u=f32(u),
               tokens=i32(p["tokens"]), prompt_len=i32(p["prompt_len"]), total_len=i32(p["total_len"]), theta=f32(p["theta"]),
               alpha_f=f32(p["alpha_f"]), alpha_p=f32(p["alpha_p"]), bias_idx=i32(p["bias_idx"]), bias_val=f32(p["bias_val"]), mask=i32(p["mask"]))
    processed = torch.empty((rows, vocab), dtype=torch.bfloat16, device=DEV)
    picked = torch.empty((rows,), dtype=torch.int32, device=DEV)
    ws = torch.empty((mixedgemm.sample_rows_workspace_bytes(rows, vocab),), dtype=torch.uint8, device=DEV)
    temperature = torch.full((rows,), 0.8, dtype=torch.float32, device=DEV)

    def step():
        mixedgemm.process_logits(dev["logits"], out=processed, tokens=dev["tokens"], prompt_len=dev["prompt_len"], total_len=dev["total_len"],
                                 repetition_penalty=dev["theta"], frequency_penalty=dev["alpha_f"], presence_penalty=dev["alpha_p"],
                                 bias_idx=dev["bias_idx"], bias_val=dev["bias_val"], allowed_mask=dev["mask"])
        mixedgemm.sample_rows(processed, dev["u"], temperature=temperature, out=picked, workspace=ws)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    answers = []
    for k in range(3):
        bits, p, u = request(k)
        dev["logits"].copy_(torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16))
        dev["u"].copy_(torch.from_numpy(u))
        for name, conv in (("tokens", np.int32), ("prompt_len", np.int32), ("total_len", np.int32), ("theta", np.float32), ("alpha_f", np.float32),
                           ("alpha_p", np.float32), ("bias_idx", np.int32), ("bias_val", np.float32), ("mask", np.int32)):
            dev[name].copy_(torch.from_numpy(np.ascontiguousarray(p[name], dtype=conv)))
        graph.replay()
        torch.cuda.synchronize()
        want = lg.rows(bits, **p)
        same(to_bits(processed), want)
        oracle_logits = torch.from_numpy(want.view(np.int16).copy()).to(DEV).view(torch.bfloat16)
        expect = mixedgemm.sample_rows(oracle_logits, dev["u"], temperature=temperature)
        assert torch.equal(picked, expect)
        allowed = set(np.flatnonzero(lg.bf16_to_f32(want[0]) > -np.inf).tolist())
        assert int(picked[0]) in allowed and len(allowed) <= 50
        answers.append(picked.cpu().tolist())
    assert len({tuple(a) for a in answers}) > 1                                     # the replays did read what was rewritten


# ---- 8. the wrapper ----------------------------------------------------------------------------------------------------------------------------
def test_wrapper_returns_and_refuses():
    rows, vocab = 2, 100
    x = torch.randn((rows, vocab), device=DEV).to(torch.bfloat16)
    tokens = torch.zeros((rows, 8), dtype=torch.int32, device=DEV)
    lens = torch.full((rows,), 8, dtype=torch.int32, device=DEV)
    pen = torch.full((rows,), 1.5, dtype=torch.float32, device=DEV)
    out = mixedgemm.process_logits(x, tokens=tokens, prompt_len=lens, total_len=lens, repetition_penalty=pen)
    assert out.dtype is torch.bfloat16 and tuple(out.shape) == (rows, vocab) and out.device == x.device and out.is_contiguous()
    assert mixedgemm.process_logits(x, out=x) is x
    before = to_bits(x).copy()
    mask = torch.full((rows, 4), -1, dtype=torch.int32, device=DEV)
    bidx = torch.zeros((rows, 2), dtype=torch.int32, device=DEV)
    bval = torch.zeros((rows, 2), dtype=torch.float32, device=DEV)
    for kw, exc, match in (
            (dict(tokens=tokens), RuntimeError, "prompt_len"), (dict(tokens=tokens, prompt_len=lens), RuntimeError, "total_len"),
            (dict(prompt_len=lens), RuntimeError, "prompt_len needs tokens"), (dict(repetition_penalty=pen), RuntimeError, "repetition_penalty needs tokens"),
            (dict(row_seq=lens), RuntimeError, "row_seq needs tokens"),
            (dict(tokens=tokens.long(), prompt_len=lens, total_len=lens), TypeError, "tokens"),
            (dict(tokens=tokens[0], prompt_len=lens, total_len=lens), RuntimeError, "tokens"),
            (dict(tokens=tokens, prompt_len=lens.float(), total_len=lens), TypeError, "prompt_len"),
            (dict(tokens=tokens, prompt_len=lens[:1], total_len=lens), RuntimeError, "prompt_len"),
            (dict(tokens=tokens, prompt_len=lens, total_len=lens, frequency_penalty=pen.double()), TypeError, "frequency_penalty"),
            (dict(tokens=tokens, prompt_len=lens, total_len=lens, presence_penalty=1.0), TypeError, "presence_penalty"),
            (dict(tokens=tokens.cpu(), prompt_len=lens, total_len=lens), RuntimeError, "tokens"),
            (dict(bias_idx=bidx), RuntimeError, "bias_val"), (dict(bias_val=bval), RuntimeError, "bias_idx"),
            (dict(bias_idx=bidx, bias_val=bval[:, :1]), RuntimeError, "bias_val"), (dict(bias_idx=bidx.long(), bias_val=bval), TypeError, "bias_idx"),
            (dict(bias_idx=bidx[:1], bias_val=bval[:1]), RuntimeError, "bias_idx"),
            (dict(allowed_mask=mask[:, :3]), RuntimeError, "allowed_mask"), (dict(allowed_mask=mask.bool()), TypeError, "allowed_mask"),
            (dict(allowed_mask=mask[:1]), RuntimeError, "allowed_mask"),
            (dict(out=torch.empty((rows, vocab), device=DEV)), TypeError, "out"), (dict(out=torch.empty((rows, vocab + 1), dtype=torch.bfloat16, device=DEV)), RuntimeError, "out"),
            (dict(out=torch.empty((rows, vocab), dtype=torch.bfloat16)), RuntimeError, "out")):
        with pytest.raises(exc, match=match):
            mixedgemm.process_logits(x, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(to_bits(x), before)                                       # nothing was launched on the way

"""GPU tests of the logits family on rows that start past 2^31 and 2^32 bytes and past 2^31 and 2^32 elements of their buffer: nine rows
far_cases.LD = 2^29 + 24 elements apart (and LD_ODD = 2^29 + 27, rows at every 2-byte alignment) in one bf16 buffer of about 8 GiB from
torch.empty, of which only the rows and a NaN guard band of 64 elements on each side of every row are ever written or read back.
tests/test_far_cpu.py proves which thresholds each row crosses and that a start computed in 32 bits lands in another row or in a guard.

Every call is compared with its oracle on the same nine rows; where the existing tests hold a value to a derived bound
(logprob_rows' fp32 values, cross_entropy), the far call is also bit-equal to the same call on the rows packed contiguously.

argmax_rows, sample_rows, logprob_rows (top_n 0 and 20, targets, per-row temperature), cross_entropy, calib.accumulate on a bf16 and an
fp16 far view, and process_logits:
  in place        nine rows: the kernel's own row products pass every threshold of the logits, and 2^31 bytes of the mask (row 8)
  own buffer      nine rows into an output view of a buffer of its own, rows 2^28 + 24 apart: the output's products pass 2^31 and 2^32
                  bytes and 2^31 elements
  second view     mm_process_logits refuses input and output spans that meet, so two views of ONE buffer are used in halves, rows 0 .. 3
                  of one into rows 5 .. 8 of the other and back: the kernel sees a moved base and forms offsets up to 3 ld, past 2^31
                  bytes only; what this case adds is that nothing outside the rows named is written
  histories       sequences that start at and past 2^31 bytes of a [34, 2^24] token buffer, in all three
  bias lists      2056 rows of n_bias = 2^20 entries (8 GiB each for bias_idx and bias_val, over small logits): the lists of rows 512,
                  1024 and 2048 start at 2^31 and 2^32 bytes and 2^31 elements; only the compared rows' lists are filled.  It runs
                  first and releases its buffers before the others are allocated"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from micromix_amd import calib, mixedgemm
import calib_oracle as co
import far_cases as fc
import kv_verify_oracle as vo
import logits_oracle as lgo
import logprob_oracle as lo

pytestmark = pytest.mark.gpu

ROWS = 9
f32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


@pytest.fixture(scope="module")
def far(dev):
    """the buffers of this file, allocated once and released at its end: logits and the output of its own (bf16), tokens and mask
    (int32); uninitialised"""
    need, free = fc.logits_need_bytes(), torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the far logits tests need {need / fc.GIB:.1f} GiB of device memory (tests/far_cases.py), {free / fc.GIB:.1f} GiB are free")
    box = dict(logits=torch.empty(fc.LOGIT_BUFFER_ELEMENTS, dtype=torch.bfloat16, device=dev),
               out=torch.empty(fc.FAR_OUT_OWN.numel(), dtype=torch.bfloat16, device=dev),
               tokens=torch.empty((fc.TOK_SEQS, fc.LD_TOK), dtype=torch.int32, device=dev),
               mask=torch.empty((ROWS, fc.LD_MASK), dtype=torch.int32, device=dev))
    yield box
    box.clear()
    torch.cuda.empty_cache()


def place(buf, g, bits, nan=fc.NAN_BITS):
    """write bits [rows, width] (uint16) as the rows of geometry g into buf, NaN into every guard band; returns the strided view"""
    raw = buf.view(torch.int16)
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(buf.device)
    nan = int(np.array(nan, dtype=np.uint16).view(np.int16))
    for r in range(g.rows):
        s = g.start(r)
        raw[s - g.guard: s] = nan
        raw[s + g.width: s + g.width + g.guard] = nan
        raw[s: s + g.width] = t[r]
    view = torch.as_strided(buf, (g.rows, g.width), (g.ld, 1), g.base)
    assert view.data_ptr() == buf.data_ptr() + 2 * g.base and view.stride(0) == g.ld
    assert (view.data_ptr() - buf.data_ptr()) + 2 * ((g.rows - 1) * g.ld + g.width) <= buf.numel() * 2          # inside the allocation
    return view


def read(buf, g):
    """(rows [rows, width] uint16, True when every guard band still holds the NaN pattern) of geometry g"""
    raw = buf.view(torch.int16)
    rows = torch.stack([raw[g.start(r): g.start(r) + g.width] for r in range(g.rows)]).cpu().numpy().view(np.uint16)
    guards = torch.cat([raw[g.start(r) - g.guard: g.start(r)] for r in range(g.rows)]
                       + [raw[g.start(r) + g.width: g.start(r) + g.width + g.guard] for r in range(g.rows)]).cpu().numpy().view(np.uint16)
    return rows, guards


def packed(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    a, b = a.view(np.int32) if a.dtype == np.float32 else a, b.view(np.int32) if b.dtype == np.float32 else b
    assert np.array_equal(a, b), (what, np.argwhere(a != b)[:4].tolist())


# ---- process_logits: far bias lists (before the `far` fixture exists) -------------------------------------------------------------------
def bias_list(r):
    """(bias_idx, bias_val) of row r, n_bias entries: padding (-1) but for 64 entries at the start, in the middle and at the end, ids in
    -1 .. vocab (both ends padding) with repeats, every row its own"""
    rng = np.random.default_rng(7000 + r)
    n = fc.BIAS.cols
    idx, val = np.full(n, -1, dtype=np.int32), rng.standard_normal(n).astype(np.float32) * 4
    for at in (0, n // 2, n - 64):
        idx[at: at + 64] = rng.integers(-1, fc.BIAS_VOCAB + 1, 64)
    return idx, val


def test_process_logits_bias_lists_past_b31_b32_and_e31(dev):
    need, free = fc.bias_need_bytes(), torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the far bias lists need {need / fc.GIB:.1f} GiB of device memory (tests/far_cases.py), {free / fc.GIB:.1f} GiB are free")
    b, rows = fc.BIAS, fc.closure(fc.BIAS)
    bits = fc.logit_rows(b.rows, fc.BIAS_VOCAB, seed=61, planted=list(range(b.rows)))
    lists = {r: bias_list(r) for r in rows}
    box = [torch.empty((b.rows, b.cols), dtype=torch.int32, device=dev), torch.empty((b.rows, b.cols), dtype=torch.float32, device=dev)]
    try:
        for r, (idx, val) in lists.items():
            box[0][r], box[1][r] = torch.from_numpy(idx).to(dev), torch.from_numpy(val).to(dev)
        out = mixedgemm.process_logits(packed(bits, dev), bias_idx=box[0], bias_val=box[1])
        got = out[torch.tensor(rows, device=dev)].view(torch.int16).cpu().numpy().view(np.uint16)
    finally:
        box.clear()
        torch.cuda.empty_cache()
    for i, r in enumerate(rows):
        want = lgo.row(bits[r], bias_idx=lists[r][0], bias_val=lists[r][1])
        assert np.array_equal(got[i], want), (r, np.flatnonzero(got[i] != want)[:4].tolist())
        for what, w in b.wraps(r).items():                        # the list a 32-bit offset would read gives this row another answer
            live = lists[w][0] >= 0
            assert not np.array_equal(lgo.row(bits[r], bias_idx=lists[w][0][live], bias_val=lists[w][1][live]), want), (r, what, w)


VIEWS = pytest.mark.parametrize("g", [fc.FAR_IN, fc.FAR_ODD], ids=["ld_aligned", "ld_odd"])


@VIEWS
def test_argmax_rows(dev, far, g):
    bits = fc.logit_rows()
    x = place(far["logits"], g, bits)
    ws = torch.full((mixedgemm.argmax_rows_workspace_bytes(ROWS, fc.VOCAB),), 0xFF, dtype=torch.uint8, device=dev)
    got = mixedgemm.argmax_rows(x, workspace=ws).cpu().numpy()
    assert got.tolist() == vo.argmax_rows(bits).tolist() == list(fc.PLANTED), got.tolist()


@VIEWS
def test_sample_rows(dev, far, g):
    bits = fc.sample_rows_bits()
    x = place(far["logits"], g, bits)
    u = f32((np.arange(ROWS) + 0.5) / ROWS, dev)
    for filtered in (False, True):
        kw = dict(top_k=i32([ROWS] * ROWS, dev), top_p=f32([0.999] * ROWS, dev), min_p=f32([0.5] * ROWS, dev)) if filtered else {}
        got = mixedgemm.sample_rows(x, u, **kw).cpu().numpy()
        assert got.tolist() == list(fc.PLANTED), (filtered, got.tolist())
    # Gaussian rows under a temperature and all three filters: the far call draws what the call on the packed rows draws
    bits = fc.logit_rows(seed=6, planted=[0] * 9)
    bits[:, [0, 13]] = fc.bf16_bits(np.float32([3.0, 2.5]))
    x = place(far["logits"], g, bits)
    kw = dict(temperature=f32(np.linspace(0.5, 2.0, ROWS), dev), top_k=i32([50] * ROWS, dev), top_p=f32([0.9] * ROWS, dev),
              min_p=f32([0.01] * ROWS, dev))
    same(mixedgemm.sample_rows(x, u, **kw), mixedgemm.sample_rows(packed(bits, dev), u, **kw), "sample_rows, far and packed")


def logprob_inputs():
    bits = fc.logit_rows()
    rng = np.random.default_rng(17)
    target = rng.integers(0, fc.VOCAB, ROWS).astype(np.int32)
    target[0], target[4], target[8], target[6] = fc.PLANTED[0], fc.PLANTED[4], fc.VOCAB - 1, -1
    T = np.linspace(0.5, 2.0, ROWS).astype(np.float32)
    return bits, target, T


@VIEWS
@pytest.mark.parametrize("top_n", [0, 20])
def test_logprob_rows(dev, far, g, top_n):
    bits, target, T = logprob_inputs()
    x = place(far["logits"], g, bits)
    got = mixedgemm.logprob_rows(x, i32(target, dev), temperature=f32(T, dev), top_n=top_n)
    near = mixedgemm.logprob_rows(packed(bits, dev), i32(target, dev), temperature=f32(T, dev), top_n=top_n)
    for name, a, b in zip(got._fields, got, near):
        assert (a is None) == (b is None) == (top_n == 0 and name.startswith("top")), name
        if a is not None:
            same(a, b, f"logprob_rows.{name}, far and packed")
    out = type(got)(*(None if o is None else o.cpu().numpy() for o in got))
    for r in range(ROWS):
        want, e_s = lo.row(bits[r], int(target[r]), T[r], top_n), lo.e_over_s(bits[r], T[r])
        assert out.rank[r] == want["rank"], (r, out.rank[r], want["rank"])
        pairs = [("logprob", out.logprob[r], want["logprob"]), ("lse", out.lse[r], want["lse"])]
        if top_n:
            assert out.top_idx[r].tolist() == want["top_idx"].tolist() and out.top_idx[r, 0] == fc.PLANTED[r], r
            pairs += [(f"top_logprob[{j}]", a, b) for j, (a, b) in enumerate(zip(out.top_logprob[r], want["top_logprob"]))]
        for name, a, b in pairs:
            assert lo.check_value(a, b, e_s) is None, (r, name, lo.check_value(a, b, e_s))


@VIEWS
def test_cross_entropy(dev, far, g):
    bits, target, _ = logprob_inputs()
    labels = target.astype(np.int64)
    labels[6] = -100
    x, y = place(far["logits"], g, bits), torch.from_numpy(labels).to(dev)
    ref_x = torch.from_numpy(lgo.bf16_to_f32(bits).copy())
    B = max(lo.bound(lo.e_over_s(bits[r]), lo.row(bits[r], int(labels[r]))["logprob"]) for r in range(ROWS) if labels[r] >= 0)
    for reduction in ("mean", "sum", "none"):
        got = mixedgemm.cross_entropy(x, y, reduction=reduction)
        same(got, mixedgemm.cross_entropy(packed(bits, dev), y, reduction=reduction), f"cross_entropy {reduction}, far and packed")
        want = F.cross_entropy(ref_x, torch.from_numpy(labels), reduction=reduction).double()
        err = (got.cpu().double() - want).abs()
        assert bool((err <= B + 2.0 ** -22 * want.abs()).all()), (reduction, float(err.max()))


# ---- process_logits --------------------------------------------------------------------------------------------------------------------
def process_inputs(far, dev):
    """the per-row operands of process_logits over the nine rows: (keywords of the oracle, keywords of the call)"""
    rng = np.random.default_rng(23)
    hist = rng.integers(-3, fc.VOCAB + 3, (fc.TOK_SEQS, fc.TOKENS.width)).astype(np.int32)       # every sequence its own tokens
    hist[:, :8] = np.array(fc.PLANTED[:8]) + (np.arange(fc.TOK_SEQS)[:, None] % 3)                # some near each row's maximum
    far["tokens"][:, : fc.TOKENS.width] = torch.from_numpy(hist).to(dev)
    row_seq = np.array(fc.ROW_SEQ, dtype=np.int32)
    prompt_len = rng.integers(0, 20, ROWS).astype(np.int32)
    total_len = (prompt_len + rng.integers(1, fc.HIST_LEN - 20, ROWS)).astype(np.int32)
    theta = np.float32([1.3, 1.0, 2.0, 1.7, np.nan, 1.1, 1.5, 1.2, 3.0])
    alpha_f = np.float32([0.5, 0.25, np.nan, 1.0, 0.1, 0.7, 0.3, 0.2, 0.9])
    alpha_p = np.float32([0.1, np.nan, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8])
    bias_idx = rng.integers(-1, fc.VOCAB + 1, (ROWS, 16)).astype(np.int32)
    bias_idx[:, 3] = bias_idx[:, 11] = np.array(fc.PLANTED)                                      # twice: the later entry counts
    bias_val = (rng.standard_normal((ROWS, 16)) * 4).astype(np.float32)
    bias_val[2, 11] = -np.inf
    mask = rng.integers(-2 ** 31, 2 ** 31, (ROWS, fc.MASK.width), dtype=np.int64).astype(np.int32)
    far["mask"][:, : fc.MASK.width] = torch.from_numpy(mask).to(dev)
    oracle = dict(tokens=hist, row_seq=row_seq, prompt_len=prompt_len, total_len=total_len, theta=theta, alpha_f=alpha_f, alpha_p=alpha_p,
                  bias_idx=bias_idx, bias_val=bias_val, mask=mask)

    def call(rows):
        sl = lambda a, conv: conv(a[rows], dev)
        return dict(tokens=far["tokens"], row_seq=sl(row_seq, i32), prompt_len=sl(prompt_len, i32), total_len=sl(total_len, i32),
                    repetition_penalty=sl(theta, f32), frequency_penalty=sl(alpha_f, f32), presence_penalty=sl(alpha_p, f32),
                    bias_idx=sl(bias_idx, i32), bias_val=sl(bias_val, f32), allowed_mask=far["mask"][rows])
    return oracle, call


def test_process_logits_into_a_second_far_view(dev, far):
    bits = fc.logit_rows()
    oracle, call = process_inputs(far, dev)
    want = lgo.rows(bits, **oracle)
    assert (want != bits).any(axis=1).all()                                                       # every row is changed by its operands
    x = place(far["logits"], fc.FAR_IN, bits)
    out = place(far["logits"], fc.FAR_OUT, np.full_like(bits, 0x1234))
    for src, dst in ((slice(0, 4), slice(5, 9)), (slice(5, 9), slice(0, 4))):
        assert mixedgemm.process_logits(x[src], out=out[dst], **call(src)) is not None
    torch.cuda.synchronize()
    got, out_guards = read(far["logits"], fc.FAR_OUT)
    kept, in_guards = read(far["logits"], fc.FAR_IN)
    assert np.array_equal(got[5:9], want[0:4]) and np.array_equal(got[0:4], want[5:9])
    assert (got[4] == 0x1234).all(), "a row of the output view that no call names was written"
    assert np.array_equal(kept, bits), "rows 0 to 8 of the input changed"
    assert (out_guards == fc.NAN_BITS).all() and (in_guards == fc.NAN_BITS).all(), "a guard band was written"


def test_process_logits_into_a_buffer_of_its_own(dev, far):
    bits = fc.logit_rows()
    oracle, call = process_inputs(far, dev)
    x = place(far["logits"], fc.FAR_IN, bits)
    out = place(far["out"], fc.FAR_OUT_OWN, np.full_like(bits, 0x1234))
    assert mixedgemm.process_logits(x, out=out, **call(slice(0, ROWS))) is out
    torch.cuda.synchronize()
    got, out_guards = read(far["out"], fc.FAR_OUT_OWN)
    kept, in_guards = read(far["logits"], fc.FAR_IN)
    assert np.array_equal(got, lgo.rows(bits, **oracle)) and np.array_equal(kept, bits)
    assert (out_guards == fc.NAN_BITS).all() and (in_guards == fc.NAN_BITS).all(), "a guard band was written"


@VIEWS
def test_process_logits_in_place(dev, far, g):
    bits = fc.logit_rows()
    oracle, call = process_inputs(far, dev)
    x = place(far["logits"], g, bits)
    assert mixedgemm.process_logits(x, out=x, **call(slice(0, ROWS))) is x
    torch.cuda.synchronize()
    got, guards = read(far["logits"], g)
    assert np.array_equal(got, lgo.rows(bits, **oracle)) and (guards == fc.NAN_BITS).all()


# ---- calib.accumulate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_calib_accumulate(dev, far, dtype):
    g, k = fc.FAR_IN, fc.CALIB_K
    x = torch.from_numpy(fc.integer_rows(ROWS, g.width, 31))
    x[:, k:] = float("nan")                                                                       # columns the kernel must not read
    x[:, :k] += torch.arange(ROWS).float()[:, None] * 16                                          # row r around 16 r: its own mean
    host = x.to(dtype)
    buf = far["logits"].view(dtype)
    view = place(buf, g, host.view(torch.int16).numpy().view(np.uint16), nan=0x7E00 if dtype is torch.float16 else fc.NAN_BITS)[:, :k]
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0                                   # taken as a view, not copied
    score, counts = torch.zeros(k, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    calib.accumulate(view, score, counts)
    want = co.run([host[:, :k]])
    assert torch.equal(score.cpu().view(torch.int32), want["score"].view(torch.int32))
    assert counts.tolist() == [want["count4"], want["count6"]] and 0 < counts[0] < counts[1] < want["numel"]

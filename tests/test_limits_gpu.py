"""GPU tests that launch every entry point of the logits family, calib.accumulate and the paged KV cache at the limits their headers
promise (tests/far_cases.py holds the numbers, tests/test_far_cpu.py checks them against the library):

rows    MM_ARGMAX_MAX_ROWS = 65535 rows (a full gridDim.y) at vocab 8 and MM_ARGMAX_CHUNK + 1 (two parts): argmax_rows, sample_rows,
        logprob_rows, process_logits.  The rows are 257 distinct rows tiled as distinct[r % 257]; the oracle runs on the 257 and every
        one of the 65535 results is compared
vocab   MM_ARGMAX_MAX_VOCAB = 2^20 columns (128 parts), 2 rows: the planted answer in part 0, part 64, part 127 and the last column;
        logprob_rows with top_n = 32, the top tokens spread over the parts; process_logits with n_bias = 2^20 entries
calib   rows = 2^20 at K = 128, and K = 32768
kv      B = 65535 sequences of one token each, one kv head, one query head, pages of one token: kv_append, rope_kv_append, paged_decode,
        paged_prefill.  Softmax over one token is 1, so the output is the sequence's V row as the cache holds it

Integers and bytes are compared exactly.  The int4 cache's attention output is bit-equal to the same call on slices of the batch and
within the bounds of tests/test_kvcache_gpu.py / tests/test_kvprefill_gpu.py of the dequantized V row (the prefill kernel multiplies
bf16(p * scale) by the codes).  logprob_rows' fp32 values are bit-equal to the call on the 257 distinct rows, which is held to
tests/logprob_oracle.py's bound."""
import numpy as np
import pytest
import torch

from micromix_amd import calib, mixedgemm
import calib_oracle as co
import far_cases as fc
import kv_fp8_oracle as fo
import kv_oracle as ko
import kv_verify_oracle as vo
import logits_oracle as lgo
import logprob_oracle as lo
import rope_oracle as ro
import test_kvcache_gpu as t_dec
import test_kvprefill_gpu as t_pre

pytestmark = pytest.mark.gpu

R, D = fc.MAX_ROWS, fc.DISTINCT
f32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


@pytest.fixture(scope="module", autouse=True)
def memory(dev):
    need, free = max(fc.limits_need_bytes(), 2 * fc.GIB), torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f"the limit tests need {need / fc.GIB:.1f} GiB of device memory (tests/far_cases.py), {free / fc.GIB:.1f} GiB are free")
    yield
    torch.cuda.empty_cache()


def bf16(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(dev).view(torch.bfloat16)


def tile(a, dev):
    """a [257, ...] on the host -> [65535, ...] on the device, row r = a[r % 257]"""
    t = bf16(a, dev) if a.dtype == np.uint16 else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t[torch.arange(R, device=dev) % D].contiguous()


def all_rows_equal(got, want257, what):
    """every one of the 65535 rows of `got` equals row r % 257 of the expected values, bit for bit"""
    want = tile(np.ascontiguousarray(want257), got.device)
    got, want = (t.view(torch.int32) if t.dtype is torch.float32 else t.view(torch.int16) if t.dtype is torch.bfloat16 else t for t in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = (got != want).reshape(R, -1).any(dim=1)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {R} rows differ, the first is row {int(bad.nonzero()[0])}"


# ---- the row limit ---------------------------------------------------------------------------------------------------------------------
VOCABS = pytest.mark.parametrize("vocab", fc.LIMIT_VOCABS)


@VOCABS
def test_argmax_rows_at_the_row_limit(dev, vocab):
    bits = fc.logit_rows(D, vocab, seed=vocab, planted=list(range(7, 7 + 31 * D, 31)))
    want = vo.argmax_rows(bits)
    assert len(set(want.tolist())) == min(vocab, D) and (want == (7 + 31 * np.arange(D)) % vocab).all()
    all_rows_equal(mixedgemm.argmax_rows(tile(bits, dev)), want.astype(np.int32), "argmax_rows")


@VOCABS
def test_sample_rows_at_the_row_limit(dev, vocab):
    planted = list(range(7, 7 + 31 * D, 31))
    x = tile(fc.sample_rows_bits(D, vocab, planted), dev)
    u = torch.rand(R, generator=torch.Generator().manual_seed(vocab)).to(dev)
    want = (np.array(planted) % vocab).astype(np.int32)
    all_rows_equal(mixedgemm.sample_rows(x, u), want, "sample_rows")
    all_rows_equal(mixedgemm.sample_rows(x, u, top_k=i32([5] * R, dev), top_p=f32([0.999] * R, dev), min_p=f32([0.5] * R, dev)), want,
                   "sample_rows, filtered")


@VOCABS
def test_logprob_rows_at_the_row_limit(dev, vocab):
    top_n = 5
    bits = fc.logit_rows(D, vocab, seed=vocab + 1, planted=list(range(7, 7 + 31 * D, 31)))
    rng = np.random.default_rng(vocab)
    target = rng.integers(-1, vocab, D).astype(np.int32)
    T = (0.5 + rng.random(D) * 1.5).astype(np.float32)
    near = mixedgemm.logprob_rows(bf16(bits, dev), i32(target, dev), temperature=f32(T, dev), top_n=top_n)
    near = type(near)(*(o.cpu().numpy() for o in near))
    for r in range(D):
        want, e_s = lo.row(bits[r], int(target[r]), T[r], top_n), lo.e_over_s(bits[r], T[r])
        assert near.rank[r] == want["rank"] and near.top_idx[r].tolist() == want["top_idx"].tolist(), r
        pairs = [(near.logprob[r], want["logprob"]), (near.lse[r], want["lse"])] + list(zip(near.top_logprob[r], want["top_logprob"]))
        assert all(lo.check_value(a, b, e_s) is None for a, b in pairs), (r, [lo.check_value(a, b, e_s) for a, b in pairs])
    got = mixedgemm.logprob_rows(tile(bits, dev), tile(target, dev), temperature=tile(T, dev), top_n=top_n)
    for name, a, b in zip(got._fields, got, near):
        all_rows_equal(a, b, f"logprob_rows.{name}")


@VOCABS
def test_process_logits_at_the_row_limit(dev, vocab):
    rng = np.random.default_rng(vocab + 2)
    bits = fc.logit_rows(D, vocab, seed=vocab + 2, planted=list(range(7, 7 + 31 * D, 31)))
    hist = rng.integers(-2, vocab + 2, (D, 24)).astype(np.int32)
    prompt_len = rng.integers(0, 10, D).astype(np.int32)
    total_len = (prompt_len + rng.integers(0, 14, D)).astype(np.int32)
    row_seq = rng.permutation(D).astype(np.int32)
    theta, alpha_f, alpha_p = ((lo_ + rng.random(D) * 1.5).astype(np.float32) for lo_ in (1.0, 0.0, 0.0))
    bias_idx = rng.integers(-1, vocab + 1, (D, 4)).astype(np.int32)
    bias_val = (rng.standard_normal((D, 4)) * 4).astype(np.float32)
    mask = rng.integers(-2 ** 31, 2 ** 31, (D, (vocab + 31) // 32), dtype=np.int64).astype(np.int32)
    want = lgo.rows(bits, tokens=hist, row_seq=row_seq, prompt_len=prompt_len, total_len=total_len, theta=theta, alpha_f=alpha_f,
                    alpha_p=alpha_p, bias_idx=bias_idx, bias_val=bias_val, mask=mask)
    got = mixedgemm.process_logits(tile(bits, dev), tokens=i32(hist, dev), row_seq=tile(row_seq, dev), prompt_len=tile(prompt_len, dev),
                                   total_len=tile(total_len, dev), repetition_penalty=tile(theta, dev), frequency_penalty=tile(alpha_f, dev),
                                   presence_penalty=tile(alpha_p, dev), bias_idx=tile(bias_idx, dev), bias_val=tile(bias_val, dev),
                                   allowed_mask=tile(mask, dev))
    all_rows_equal(got, want, "process_logits")


# ---- the vocabulary limit --------------------------------------------------------------------------------------------------------------
V = fc.MAX_VOCAB


@pytest.mark.parametrize("cols", [fc.LIMIT_PLANTED[:2], fc.LIMIT_PLANTED[2:]], ids=["parts_0_64", "part_127_last_column"])
def test_argmax_and_sample_at_the_vocabulary_limit(dev, cols):
    assert mixedgemm.argmax_rows_workspace_bytes(2, V) == 2 * fc.VOCAB_PARTS * 8
    bits = fc.logit_rows(2, V, seed=cols[0] + 3, planted=list(cols))
    assert vo.argmax_rows(bits).tolist() == list(cols)
    assert mixedgemm.argmax_rows(bf16(bits, dev)).tolist() == list(cols)
    u = f32([0.25, 0.75], dev)
    assert mixedgemm.sample_rows(bf16(fc.sample_rows_bits(2, V, list(cols)), dev), u).tolist() == list(cols)


def test_logprob_rows_at_the_vocabulary_limit(dev):
    top_n = 32
    bits = fc.bf16_bits(np.random.default_rng(41).standard_normal((2, V)) * 3.0)
    cols = np.array([[(4 * j + r) * fc.CHUNK + (37 * j + r) % fc.CHUNK for j in range(top_n)] for r in range(2)])   # parts 0, 4, .. 124 (+ 1)
    for r in range(2):
        bits[r, cols[r][::-1] if r else cols[r]] = fc.bf16_bits(np.float32(40.0 - 0.25 * np.arange(top_n)))       # descending; row 1 from the end
    target, T = np.array([cols[0][3], V - 1], dtype=np.int32), np.float32([0.7, 1.5])
    got = mixedgemm.logprob_rows(bf16(bits, dev), i32(target, dev), temperature=f32(T, dev), top_n=top_n)
    got = type(got)(*(o.cpu().numpy() for o in got))
    for r in range(2):
        want, e_s = lo.row(bits[r], int(target[r]), T[r], top_n), lo.e_over_s(bits[r], T[r])
        assert want["top_idx"].tolist() == (cols[r][::-1] if r else cols[r]).tolist() and len({c // fc.CHUNK for c in cols[r]}) == top_n
        assert got.rank[r] == want["rank"] and got.top_idx[r].tolist() == want["top_idx"].tolist(), r
        pairs = [(got.logprob[r], want["logprob"]), (got.lse[r], want["lse"])] + list(zip(got.top_logprob[r], want["top_logprob"]))
        assert all(lo.check_value(a, b, e_s) is None for a, b in pairs), (r, [lo.check_value(a, b, e_s) for a, b in pairs])


def test_process_logits_with_the_longest_bias_list_at_the_vocabulary_limit(dev):
    """n_bias = 2^20: row 0's list names every column once, row 1's names every second column twice, where the higher index counts"""
    n = fc.MAX_BIAS
    rng = np.random.default_rng(43)
    bits = fc.bf16_bits(rng.standard_normal((2, V)) * 3.0)
    bias_idx = np.stack([rng.permutation(V), rng.permutation(n) % (V // 2) * 2]).astype(np.int32)
    assert n == V and np.array_equal(np.sort(bias_idx[0]), np.arange(V)) and (np.bincount(bias_idx[1], minlength=V)[0::2] == 2).all()
    bias_val = (rng.standard_normal((2, n)) * 4).astype(np.float32)
    want = lgo.rows(bits, bias_idx=bias_idx, bias_val=bias_val)
    got = mixedgemm.process_logits(bf16(bits, dev), bias_idx=i32(bias_idx, dev), bias_val=f32(bias_val, dev))
    got = got.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert (want[0] != bits[0]).mean() > 0.9 and np.array_equal(want[1, 1::2], bits[1, 1::2])


# ---- calib.accumulate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,k", [(fc.CALIB_MAX_ROWS, 128), (3, fc.CALIB_MAX_K)], ids=["rows_2^20", "K_32768"])
def test_calib_accumulate_at_its_limits(dev, rows, k):
    x = torch.randint(-100, 101, (rows, k), generator=torch.Generator().manual_seed(k), dtype=torch.int16).to(torch.bfloat16)
    x[:, 5] *= 2                                                                                  # one channel above the others
    score, counts = torch.zeros(k, dtype=torch.float32, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    calib.accumulate(x.to(dev), score, counts)
    want = co.run([x])
    assert torch.equal(score.cpu().view(torch.int32), want["score"].view(torch.int32))
    assert counts.tolist() == [want["count4"], want["count6"]] and 0 < counts[0] < counts[1] < rows * k


# ---- B = 65535 sequences ---------------------------------------------------------------------------------------------------------------
B = fc.KV_MAX_B


def pool(kind, dev):
    """an empty cache of B + 3 pages of one token, one layer, one kv head; (data, param, its host copies as the oracles take them)"""
    shape = (B + 3, 1, 2, 1, 1)
    if kind == "bf16":
        return torch.zeros(shape + (128,), dtype=torch.bfloat16, device=dev), None, np.zeros(shape + (128,), dtype=np.uint16), None
    width = 64 if kind == "int4" else 128
    return (torch.zeros(shape + (width,), dtype=torch.uint8, device=dev), torch.zeros(shape + (2,), dtype=torch.float16, device=dev),
            np.zeros(shape + (width,), dtype=np.uint8), np.zeros(shape + (2,), dtype=np.float16))


def host(data, param):
    d = data.cpu()
    return (d.view(torch.int16).numpy().view(np.uint16) if d.dtype is torch.bfloat16 else d.numpy()), None if param is None else param.cpu().numpy()


@pytest.mark.parametrize("kind", ["int4", "fp8", "bf16"])
def test_the_paged_kv_entry_points_at_65535_sequences(dev, kind):
    rng = np.random.default_rng(B)
    pages = rng.permutation(B + 3)[:B].astype(np.int32)                                           # sequence b owns page pages[b]
    tbl = [i32(np.arange(B + 1), dev), i32(pages, dev), i32(np.ones(B), dev)]
    one_seq = (np.array([0, B]), pages, np.array([1]))              # the same slots as one sequence of B tokens: what the oracle loops over
    per_seq = i32(np.arange(B + 1), dev)
    kb, vb, qb = (fc.bf16_bits(rng.standard_normal((B, 1, 128)) * s) for s in (2.0, 0.5, 1.0))
    oracle_append = ko.append if kind != "fp8" else fo.append

    def check_cache(data, param, want_d, want_p, what):
        got_d, got_p = host(data, param)
        assert np.array_equal(got_d, want_d), f"{what}: {int((got_d != want_d).any(axis=-1).sum())} cache rows differ"
        assert param is None or np.array_equal(got_p.view(np.uint16), want_p.view(np.uint16)), f"{what}: params differ"

    # kv_append
    data, param, want_d, want_p = pool(kind, dev)
    mixedgemm.kv_append(data, param, *tbl, bf16(kb, dev), bf16(vb, dev), per_seq, 0)
    oracle_append(want_d, want_p, *one_seq, kb, vb, np.array([0, B]), 0)
    check_cache(data, param, want_d, want_p, "kv_append")
    # what every sequence's one V row decodes to, as bf16 bits
    if kind == "bf16":
        v_rows = vb
    elif kind == "fp8":
        v_rows = fo.dequantize(want_d, want_p)[pages, 0, 1, :, 0]
    else:
        v_rows = None                                              # int4: held to the same call on slices of the batch instead
    if v_rows is not None:                                         # the sum starts at +0.0, and +0.0 + 1 * -0.0 is +0.0
        v_rows = np.where(v_rows == 0x8000, 0, v_rows).astype(np.uint16)
    # paged_decode and paged_prefill with one query token per sequence
    q = bf16(qb, dev)
    for name, o in (("paged_decode", mixedgemm.paged_decode(q, data, param, *tbl, 0, 1)),
                    ("paged_prefill", mixedgemm.paged_prefill(q, data, param, *tbl, per_seq, 0, 1))):
        assert tuple(o.shape) == (B, 1, 128)
        if v_rows is not None:
            got = o.view(torch.int16).cpu().numpy().view(np.uint16)
            bad = (got != v_rows).any(axis=(1, 2))
            assert not bad.any(), f"{name}: {int(bad.sum())} of {B} outputs are not their V row, the first is sequence {int(bad.nonzero()[0][0])}"
        else:
            step = 8192
            for b0 in range(0, B, step):
                n = min(step, B - b0)
                sub = [i32(np.arange(n + 1), dev), i32(pages[b0: b0 + n], dev), i32(np.ones(n), dev)]
                part = (mixedgemm.paged_decode(q[b0: b0 + n], data, param, *sub, 0, 1) if name == "paged_decode" else
                        mixedgemm.paged_prefill(q[b0: b0 + n], data, param, *sub, sub[0], 0, 1))
                assert torch.equal(part.view(torch.int16), o[b0: b0 + n].view(torch.int16)), (name, b0)
            prm = want_p[pages, 0, 1, :, 0].astype(np.float64)                                    # [B, 1, 2]
            deq = ko.unpack_codes(want_d[pages, 0, 1, :, 0]).astype(np.float64) * prm[..., 0:1] - prm[..., 1:2]
            if name == "paged_decode":                                                            # the bounds of the existing tests
                t_dec.check_attention(o, deq, float(np.abs(deq).max()))
            else:
                t_pre.check(o, deq, np.abs(deq).max(axis=-1, keepdims=True), name)
    # rope_kv_append into a fresh cache
    cos, sin = ro.llama3_tables(np.arange(B) % 4096)
    data, param, want_d, want_p = pool(kind, dev)
    q_rot = mixedgemm.rope_kv_append(data, param, *tbl, q, bf16(kb, dev), bf16(vb, dev), bf16(cos, dev), bf16(sin, dev), per_seq, 0)
    oracle_append(want_d, want_p, *one_seq, ro.rope(kb, cos, sin), vb, np.array([0, B]), 0)
    check_cache(data, param, want_d, want_p, "rope_kv_append")
    assert np.array_equal(q_rot.view(torch.int16).cpu().numpy().view(np.uint16), ro.rope(qb, cos, sin)), "rope_kv_append: the rotated q"

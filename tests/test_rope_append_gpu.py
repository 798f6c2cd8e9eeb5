"""GPU tests of the fused RoPE + KV append (mixedgemm.rope_kv_append, PagedKVCache.append_rope) against tests/rope_oracle.py.
Every comparison is bit equality: the op is specified bit for bit (include/micromix_hip.h, mm_rope_kv_append)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_oracle as ko
import rope_oracle as ro

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, LAYER = 2, 1          # a layer offset fault shows


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def from_bits(b, dev):
    return torch.from_numpy(np.ascontiguousarray(b).view(np.int16).copy()).view(torch.bfloat16).to(dev)


def empty_cache(kind, max_pages, Hkv, P, dev, poison=0xA5):
    """the poisoned cache of test_kvcache_gpu.empty_cache"""
    if kind == "int4":
        data = torch.full((max_pages, L, 2, Hkv, P, 64), poison, dtype=torch.uint8, device=dev)
        param = torch.full((max_pages, L, 2, Hkv, P, 2), -7.0, dtype=torch.float16, device=dev)
    else:
        data = torch.full((max_pages, L, 2, Hkv, P, 128), 0x5A5A, dtype=torch.int16, device=dev).view(torch.bfloat16)
        param = None
    return data, param


def host(data, param):
    d = data.cpu()
    d = d.numpy() if d.dtype == torch.uint8 else d.view(torch.int16).numpy().view(np.uint16)
    return d.copy(), (param.cpu().numpy().copy().view(np.uint16) if param is not None else None)


def same_cache(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None or np.array_equal(a[1], b[1]))


def page_table(lens, P, max_pages, rng):
    """shuffled, non-contiguous pages for sequences of the given lengths"""
    npg = [-(-n // P) for n in lens]
    perm = rng.permutation(max_pages)[: sum(npg)]
    indptr = np.concatenate([[0], np.cumsum(npg)]).astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    return indptr, perm.astype(np.int32), last


def dev_i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def rand_bf16(shape, rng, dev, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale).to(torch.bfloat16).to(dev)


def packed_qkv(T, Hq, Hkv, rng, dev):
    """a [T, (Hq + 2 Hkv) * 128] projection as FusedQLinear leaves it, and its q | k | v views"""
    buf = torch.cat([rand_bf16((T, Hq * 128), rng, dev), rand_bf16((T, Hkv * 128), rng, dev, 2.0), rand_bf16((T, Hkv * 128), rng, dev, 0.5)], 1)
    return buf, buf[:, : Hq * 128], buf[:, Hq * 128: (Hq + Hkv) * 128], buf[:, (Hq + Hkv) * 128:]


def torch_rope(x, cos, sin):
    """HF apply_rotary_pos_emb on bf16 device tensors: x [T, H, 128], cos / sin [T, 128]"""
    cos, sin = cos.unsqueeze(1), sin.unsqueeze(1)
    return (x * cos) + (torch.cat((-x[..., 64:], x[..., :64]), dim=-1) * sin)


def run_exact(kind, Hq, Hkv, P, prior, new, rng, dev, tables=None):
    """appends new[b] tokens to sequences holding prior[b]; the whole cache (target slots and poison alike) and q_rot against the
    oracle and against kv_append(oracle rope(k), v); views of a packed projection and three contiguous tensors give the same bytes"""
    lens = [a + n for a, n in zip(prior, new)]
    max_pages = sum(-(-n // P) for n in lens) + 3
    assert max_pages <= 64
    indptr, indices, last = page_table(lens, P, max_pages, rng)
    app = np.concatenate([[0], np.cumsum(new)]).astype(np.int32)
    T = int(app[-1])
    buf, q, k, v = packed_qkv(T, Hq, Hkv, rng, dev)
    keep = buf.clone()
    if tables is None:
        pos = rng.integers(0, 131072, T)          # rows that differ per token, in no order
        pos[-1] = 131071
        tables = ro.llama3_tables(pos)
    cos_b, sin_b = tables
    cos, sin = from_bits(cos_b, dev), from_bits(sin_b, dev)
    tbl = [dev_i32(a, dev) for a in (indptr, indices, last)]
    app_d = dev_i32(app, dev)

    data, param = empty_cache(kind, max_pages, Hkv, P, dev)
    want_d, want_p = host(data, param)
    if want_p is not None:
        want_p = want_p.view(np.float16)
    qb, kb, vb = (bits(t).reshape(T, -1, 128) for t in (q, k, v))
    want_q = ro.rope_append(want_d, want_p, indptr, indices, last, qb, kb, vb, cos_b, sin_b, app, LAYER)
    want = (want_d, want_p.view(np.uint16) if want_p is not None else None)

    q_rot = mixedgemm.rope_kv_append(data, param, *tbl, q, k, v, cos, sin, app_d, LAYER)
    torch.cuda.synchronize()
    assert q_rot.shape == (T, Hq, 128) and q_rot.is_contiguous()
    assert np.array_equal(bits(q_rot), want_q), f"{int((bits(q_rot) != want_q).sum())} q elements differ from the oracle"
    got = host(data, param)
    assert np.array_equal(got[0], want[0]), f"{int((got[0] != want[0]).sum())} cache bytes differ from the oracle"
    assert same_cache(got, want), "params differ from the oracle"
    assert torch.equal(buf.view(torch.int16), keep.view(torch.int16)), "the packed input was written"

    data2, param2 = empty_cache(kind, max_pages, Hkv, P, dev)
    mixedgemm.kv_append(data2, param2, *tbl, from_bits(ro.rope(kb, cos_b, sin_b), dev), v.reshape(T, Hkv, 128).contiguous(), app_d, LAYER)
    assert same_cache(host(data2, param2), got), "differs from kv_append(rope(k), v)"

    data3, param3 = empty_cache(kind, max_pages, Hkv, P, dev)
    q3 = mixedgemm.rope_kv_append(data3, param3, *tbl, q.reshape(T, Hq, 128).contiguous(), k.contiguous(), v.reshape(T, Hkv, 128).contiguous(),
                                  cos, sin, app_d, LAYER)
    torch.cuda.synchronize()
    assert torch.equal(q3.view(torch.int16), q_rot.view(torch.int16)) and same_cache(host(data3, param3), got), \
        "three contiguous tensors give other bytes than views of the packed projection"
    return dict(q=q, k=k, v=v, q_rot=q_rot, cache=got, tbl=tbl, app=app_d, max_pages=max_pages)


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("heads", [(32, 8), (40, 8), (4, 4), (128, 8), (3, 1)])
def test_byte_exact(dev, kind, heads):
    """ragged appends of 0, 1, 5 and 17 tokens over 0, 15, 16 and 40 cached ones: they cross page edges, one sequence is empty.  With
    one token per page (P = 1) the four sequences need more than the 64 pages a test cache may have, so they come in two batches."""
    Hq, Hkv = heads
    rng = np.random.default_rng(Hq * 100 + Hkv)
    for P in (16, 24):
        run_exact(kind, Hq, Hkv, P, [0, 15, 16, 40], [0, 17, 5, 1], rng, dev)
    run_exact(kind, Hq, Hkv, 1, [0, 40, 0], [0, 1, 17], rng, dev)
    run_exact(kind, Hq, Hkv, 1, [15, 0, 16], [5, 0, 17], rng, dev)


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_identity_and_rotate_half_tables(dev, kind):
    rng = np.random.default_rng(2)
    Hq, Hkv, T = 32, 8, 23
    one, zero = np.full((T, 128), 0x3F80, np.uint16), np.zeros((T, 128), np.uint16)
    # cos = 1, sin = 0: q and K pass through (run_exact: the cache equals kv_append(rope(k), v), and here rope(k) must be k)
    r = run_exact(kind, Hq, Hkv, 16, [0, 15, 16, 40], [0, 17, 5, 1], rng, dev, tables=(one, zero))
    assert np.array_equal(bits(r["q_rot"]).reshape(T, -1), bits(r["q"]))
    data, param = empty_cache(kind, r["max_pages"], Hkv, 16, dev)
    mixedgemm.kv_append(data, param, *r["tbl"], r["k"].reshape(T, Hkv, 128).contiguous(), r["v"].reshape(T, Hkv, 128).contiguous(), r["app"], LAYER)
    assert same_cache(host(data, param), r["cache"]), "K did not pass through"
    # cos = 0, sin = 1: exactly rotate_half (the partner, its sign, its half)
    r = run_exact(kind, Hq, Hkv, 16, [0, 15, 16, 40], [0, 17, 5, 1], rng, dev, tables=(zero, one))
    qb = bits(r["q"]).reshape(T, Hq, 128)
    assert np.array_equal(bits(r["q_rot"]), np.concatenate([qb[..., 64:] ^ 0x8000, qb[..., :64]], axis=-1))


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_table_rows_follow_the_flat_token_not_the_slot(dev, kind):
    """positions that run against the slot order, cos / sin as strided rows of one [T, 256] tensor and in HF's [1, T, 128] shape"""
    rng = np.random.default_rng(3)
    Hq, Hkv, P, prior, new = 32, 8, 16, [20, 3], [6, 14]
    T = sum(new)
    pos = np.arange(T)[::-1] * 997 + 11                        # decreasing, while every sequence's slots increase
    cos_b, sin_b = ro.llama3_tables(pos)
    r = run_exact(kind, Hq, Hkv, P, prior, new, rng, dev, tables=(cos_b, sin_b))
    both = torch.cat([from_bits(cos_b, dev), from_bits(sin_b, dev)], dim=1)             # [T, 256]
    ones = torch.ones((T, Hkv, 128), dtype=torch.bfloat16, device=dev)                  # a V of its own: q, k, v go through the packing copy
    for cos, sin in ((both[:, :128], both[:, 128:]), (from_bits(cos_b, dev).unsqueeze(0), from_bits(sin_b, dev).unsqueeze(0))):
        data, param = empty_cache(kind, r["max_pages"], Hkv, P, dev)
        q2 = mixedgemm.rope_kv_append(data, param, *r["tbl"], r["q"], r["k"], ones, cos, sin, r["app"], LAYER)
        torch.cuda.synchronize()
        assert torch.equal(q2.view(torch.int16), r["q_rot"].view(torch.int16))
        got = host(data, param)
        assert np.array_equal(got[0][:, LAYER, 0], r["cache"][0][:, LAYER, 0]), "K rows differ"
        assert got[1] is None or np.array_equal(got[1][:, LAYER, 0], r["cache"][1][:, LAYER, 0]), "K params differ"


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_guards_write_nothing_and_still_rotate_q(dev, kind):
    rng = np.random.default_rng(4)
    Hq, Hkv, P, max_pages, T = 32, 8, 16, 8, 3
    buf, q, k, v = packed_qkv(T, Hq, Hkv, rng, dev)
    cos_b, sin_b = ro.llama3_tables([5, 6, 7])
    cos, sin = from_bits(cos_b, dev), from_bits(sin_b, dev)
    want_q = ro.rope(bits(q).reshape(T, Hq, 128), cos_b, sin_b)
    i32 = lambda a: dev_i32(np.array(a), dev)
    cases = {"a table that does not count the tokens": (i32([0, 0]), i32([2]), i32([0])),
             "page -1": (i32([0, 1]), i32([-1]), i32([3])),
             "page max_pages": (i32([0, 1]), i32([max_pages]), i32([3]))}
    for what, tbl in cases.items():
        data, param = empty_cache(kind, max_pages, Hkv, P, dev)
        clean = host(data, param)
        q_rot = mixedgemm.rope_kv_append(data, param, *tbl, q, k, v, cos, sin, i32([0, T]), LAYER)
        torch.cuda.synchronize()
        assert same_cache(host(data, param), clean), f"{what}: the cache was written"
        assert np.array_equal(bits(q_rot), want_q), f"{what}: q is not the full rotated q"


def test_operands_at_the_end_of_their_allocations(dev):
    """T = 1 with every operand ending where its own allocation ends (a child process, as tests/test_stream_bounds_gpu.py does)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "rope_bounds_probe.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "done" in p.stdout, (p.stdout[-1500:], p.stderr[-1500:])
    cases = [l.split() for l in p.stdout.splitlines() if l.startswith("case")]
    assert len(cases) == 2
    for c in cases:
        assert c[-1] == c[-2], c            # the same bytes as with the operands in the middle of torch's pool


def twin_caches(kind, B, prior, rng, dev, Hkv=8):
    """two caches in the same state: the same pages, the same `prior` tokens in both layers"""
    caches = [PagedKVCache(L, Hkv, 16, 64, B, kind=kind, device=dev) for _ in range(2)]
    n = sum(prior)
    pk, pv = rand_bf16((L, n, Hkv, 128), rng, dev), rand_bf16((L, n, Hkv, 128), rng, dev)
    for c in caches:
        c.extend(prior)
        for layer in range(L):
            c.append(layer, pk[layer], pv[layer])
    return caches


@pytest.mark.parametrize("kind", ["int4", "bf16"])
@pytest.mark.parametrize("new", [(1, 1, 1), (17, 1, 0)])
def test_drop_in_for_torch_rope_then_append(dev, kind, new):
    """append_rope -> attend / attend_new against torch bf16 RoPE -> append -> attend / attend_new: decode B = 3, prefill (17, 1, 0)"""
    rng = np.random.default_rng(6)
    Hq, Hkv = 32, 8
    a, b = twin_caches(kind, 3, [40, 5, 23], rng, dev)
    T = sum(new)
    buf, q, k, v = packed_qkv(T, Hq, Hkv, rng, dev)
    cos_b, sin_b = ro.llama3_tables(rng.integers(0, 131072, T))
    cos, sin = from_bits(cos_b, dev), from_bits(sin_b, dev)
    for c in (a, b):
        c.extend(list(new))
    q3, k3, v3 = q.reshape(T, Hq, 128), k.reshape(T, Hkv, 128), v.reshape(T, Hkv, 128)
    a.append(LAYER, torch_rope(k3, cos, sin).contiguous(), v3.contiguous())
    qa = torch_rope(q3, cos, sin).contiguous()
    qb = b.append_rope(LAYER, q, k, v, cos, sin)
    attend = (lambda c, x: c.attend(LAYER, x)) if new == (1, 1, 1) else (lambda c, x: c.attend_new(LAYER, x))
    oa, ob = attend(a, qa), attend(b, qb)
    torch.cuda.synchronize()
    assert torch.equal(qa.view(torch.int16), qb.view(torch.int16)), "the rotated q differs from torch's"
    assert same_cache(host(a.kv_data, a.kv_param), host(b.kv_data, b.kv_param)), "the caches differ"
    assert torch.equal(oa.view(torch.int16), ob.view(torch.int16)), "the attention outputs differ"


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_graph_capture_over_extend_steps(dev, kind):
    B, Hq, Hkv = 2, 32, 8
    rng = np.random.default_rng(11)
    cache, = twin_caches(kind, B, [40, 5], rng, dev)[:1]
    bound = 256
    buf, q, k, v = packed_qkv(B, Hq, Hkv, rng, dev)
    cos, sin = (from_bits(t, dev) for t in ro.llama3_tables([40, 5]))
    cache.extend(1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.attend(LAYER, cache.append_rope(LAYER, q, k, v, cos, sin), max_seq_len=bound)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        q_out = cache.append_rope(LAYER, q, k, v, cos, sin)
        out = cache.attend(LAYER, q_out, max_seq_len=bound)
    for step in range(4):
        if step:
            cache.extend(1)
        buf.copy_(packed_qkv(B, Hq, Hkv, rng, dev)[0])
        tabs = ro.llama3_tables([40 + step, 5 + step])
        cos.copy_(from_bits(tabs[0], dev))
        sin.copy_(from_bits(tabs[1], dev))
        graph.replay()
        torch.cuda.synchronize()
        got_q, got, got_cache = q_out.clone(), out.clone(), host(cache.kv_data, cache.kv_param)
        eager_q = cache.append_rope(LAYER, q, k, v, cos, sin)
        eager = cache.attend(LAYER, eager_q, max_seq_len=bound)
        torch.cuda.synchronize()
        assert np.array_equal(bits(got_q), ro.rope(bits(q).reshape(B, Hq, 128), *tabs)), f"replay {step}: q differs from the oracle"
        assert torch.equal(got_q.view(torch.int16), eager_q.view(torch.int16)), f"replay {step}: q differs from eager"
        assert same_cache(got_cache, host(cache.kv_data, cache.kv_param)), f"replay {step}: the cache differs from eager"
        assert torch.equal(got.view(torch.int16), eager.view(torch.int16)), f"replay {step} differs from eager"


@pytest.mark.parametrize("kind", ["int4", "bf16"])
def test_two_launches_are_bit_equal(dev, kind):
    rng = np.random.default_rng(8)
    Hq, Hkv, P, lens = 40, 8, 24, [30, 9]
    indptr, indices, last = page_table(lens, P, 8, rng)
    T = sum(lens)
    buf, q, k, v = packed_qkv(T, Hq, Hkv, rng, dev)
    cos, sin = (from_bits(t, dev) for t in ro.llama3_tables(rng.integers(0, 131072, T)))
    res = []
    for _ in range(2):
        data, param = empty_cache(kind, 8, Hkv, P, dev)
        q_rot = mixedgemm.rope_kv_append(data, param, dev_i32(indptr, dev), dev_i32(indices, dev), dev_i32(last, dev), q, k, v, cos, sin,
                                         dev_i32([0, lens[0], T], dev), LAYER)
        torch.cuda.synchronize()
        res.append((bits(q_rot), host(data, param)))
    assert np.array_equal(res[0][0], res[1][0]) and same_cache(res[0][1], res[1][1])

"""GPU tests of page sharing in the paged KV cache (mixedgemm.kv_copy_pages, PagedKVCache.fork / truncate / copy-on-write).

1 copy     mm_kv_copy_pages against a numpy oracle over the WHOLE cache, every byte poisoned, the three kinds, odd page sizes, rows
           below / at / above the page size, skipped pairs; and with the cache ending where its allocation ends
2 twin     a cache that forks and truncates against one that never shares, rebuilt from the rows a model says each sequence holds:
           attend and attend_new bit-equal after every step, no tolerance
3 owner    after a fork and a diverging step, nothing but the new rows and the copied page has changed
4 graph    one hipGraph of append + attend replayed across a copying extend and a truncate

No bound here comes from what a kernel produced: every comparison is equality."""
import ctypes

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache

pytestmark = pytest.mark.gpu

KINDS = ["int4", "bf16", "fp8_e4m3"]
WIDTH = {"int4": 64, "fp8_e4m3": 128, "bf16": 256}                   # bytes of codes per row
CODE = {"int4": _lib.MM_KV_INT4, "bf16": _lib.MM_KV_BF16, "fp8_e4m3": _lib.MM_KV_FP8_E4M3}


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def rand_bf16(shape, rng, dev, scale=1.0):
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32) * scale).to(torch.bfloat16).to(dev)


def same_bits(a, b, what):
    assert a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16)), f"{what}: {int((a.view(torch.int16) != b.view(torch.int16)).sum())} values differ"


# ---- 1. the copy kernel, byte for byte ---------------------------------------------------------------------------------------------------
def poison(kind, max_pages, L, Hkv, P, seed):
    """host arrays: every code byte from a per-byte pattern; params (int16 pairs) with the exponent field never all ones"""
    rng = np.random.default_rng(seed)
    shape = (max_pages, L, 2, Hkv, P)
    n = int(np.prod(shape)) * WIDTH[kind]
    data = ((np.arange(n, dtype=np.int64) * 131 + 7) % 251 + rng.integers(0, 5, n)).astype(np.uint8).reshape(shape + (WIDTH[kind],))
    param = None if kind == "bf16" else (rng.integers(0, 0x7C00, shape + (2,)) | (rng.integers(0, 2, shape + (2,)) << 15)).astype(np.uint16)
    return data, param


def to_dev(kind, data, param, dev):
    d = torch.from_numpy(data.copy()).to(dev)
    if kind == "bf16":
        d = d.view(torch.bfloat16)
    return d, None if param is None else torch.from_numpy(param.view(np.int16).copy()).to(dev).view(torch.float16)


def to_host(d, p):
    return d.view(torch.uint8).cpu().numpy(), None if p is None else p.view(torch.int16).cpu().numpy().view(np.uint16)


def copy_oracle(data, param, pairs, P):
    """the rule of include/micromix_hip.h, mm_kv_copy_pages, on host arrays [pages, L, 2, Hkv, P, bytes]; rows None: whole pages"""
    n = data.shape[0]
    for src, dst, r in pairs:
        r = P if r is None else min(r, P)
        if not (0 <= src < n and 0 <= dst < n) or src == dst or r <= 0:
            continue
        data[dst, :, :, :, :r] = data[src, :, :, :, :r]
        if param is not None:
            param[dst, :, :, :, :r] = param[src, :, :, :, :r]


def copy_calls(P, n):
    """three calls of up to 6 pairs over n = 12 pages: the row counts, the skipped pairs, whole pages"""
    return [[(0, 5, 1), (1, 6, P - 1), (2, 7, P), (3, 8, P + 3), (4, 9, 0), (2, 10, -2)],
            [(n, 5, P), (0, -1, P), (0, n, P), (11, 11, P), (-1, 6, P), (1, 10, 2)],
            [(0, 9, None), (3, 10, None), (n + 7, 5, None), (11, 11, None), (7, 4, None)]]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [1, 5, 16])
def test_copy_pages_byte_for_byte(dev, kind, P):
    n, L, Hkv = 12, 3, 2
    hd, hp = poison(kind, n, L, Hkv, P, 7 * P)
    d, p = to_dev(kind, hd, hp, dev)
    for pairs in copy_calls(P, n):
        src, dst, rows = zip(*pairs)
        assert len(pairs) <= 6 and len({x for x in dst if 0 <= x < n}) == len([x for x in dst if 0 <= x < n])
        assert mixedgemm.kv_copy_pages(d, p, i32(src, dev), i32(dst, dev), None if rows[0] is None else i32(rows, dev)) is None
        torch.cuda.synchronize()
        before = hd.copy()
        copy_oracle(hd, hp, pairs, P)
        assert (hd != before).any(), "the call must move something"
        gd, gp = to_host(d, p)
        assert np.array_equal(gd, hd), f"{int((gd != hd).sum())} code bytes differ from the oracle"
        assert hp is None or np.array_equal(gp, hp), "params differ from the oracle"
    mixedgemm.kv_copy_pages(d, p, i32([], dev), i32([], dev))                     # no pairs: nothing happens
    torch.cuda.synchronize()
    assert np.array_equal(to_host(d, p)[0], hd)


@pytest.mark.parametrize("kind", KINDS)
def test_copy_pages_at_the_end_of_the_allocation(dev, kind):
    """kv_data and kv_param each END where a hipMalloc allocation of whole 2 MiB pages ends; the cache's last page is a source in one
    call and a destination in the next, whole pages and P + 3 rows, so the last rows of both arrays are read and then written"""
    lib = _lib.load()
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    PAGE = 2 << 20
    n, L, Hkv, P = 4, 2, 2, 5
    hd, hp = poison(kind, n, L, Hkv, P, 3)
    d, p = to_dev(kind, hd, hp, dev)
    allocs, ends = [], {"param": None}
    try:
        for name, t in (("data", d), ("param", p)):
            if t is None:
                continue
            nbytes = t.numel() * t.element_size()
            size = (nbytes + PAGE - 1) // PAGE * PAGE
            ptr = ctypes.c_void_p()
            assert hip.hipMalloc(ctypes.byref(ptr), size) == 0
            allocs.append(ptr)
            ends[name] = ptr.value + size - nbytes
            assert ends[name] % (16 if name == "data" else 4) == 0
            assert hip.hipMemcpy(ends[name], t.data_ptr(), nbytes, 3) == 0           # device to device
        st = torch.cuda.current_stream().cuda_stream
        for pairs in ([(n - 1, 0, None), (1, 2, None)], [(1, n - 1, P + 3), (n - 1, n - 1, P)], [(0, n - 1, 2), (1, n, P), (n, n - 1, P)]):
            src, dst, rows = zip(*pairs)
            r = None if rows[0] is None else i32(rows, dev)
            s_, d_ = i32(src, dev), i32(dst, dev)
            assert lib.mm_kv_copy_pages(ends["data"], ends["param"], CODE[kind], n, L, Hkv, P, 128, s_.data_ptr(), d_.data_ptr(),
                                        None if r is None else r.data_ptr(), len(pairs), st) == 0
            torch.cuda.synchronize()
            copy_oracle(hd, hp, pairs, P)
        for name, t in (("data", d), ("param", p)):
            if t is not None:
                assert hip.hipMemcpy(t.data_ptr(), ends[name], t.numel() * t.element_size(), 3) == 0
        torch.cuda.synchronize()
        gd, gp = to_host(d, p)
        assert np.array_equal(gd, hd) and (hp is None or np.array_equal(gp, hp))
    finally:
        torch.cuda.synchronize()
        for ptr in allocs:
            hip.hipFree(ptr)


def test_python_argument_errors_on_the_device(dev):
    d = torch.full((4, 2, 2, 2, 4, 64), 7, dtype=torch.uint8, device=dev)
    p = torch.ones((4, 2, 2, 2, 4, 2), dtype=torch.float16, device=dev)
    for src, dst, rows in (([0, 1], [2], None), ([0, 1], [2, 3], [4])):
        with pytest.raises(RuntimeError, match="one length"):
            mixedgemm.kv_copy_pages(d, p, i32(src, dev), i32(dst, dev), None if rows is None else i32(rows, dev))
    with pytest.raises(TypeError):
        mixedgemm.kv_copy_pages(d, p, i32([0], dev).long(), i32([1], dev))
    with pytest.raises(RuntimeError, match="contiguous"):
        mixedgemm.kv_copy_pages(d, p, i32([0, 9, 1, 9], dev)[::2], i32([2, 3], dev))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.kv_copy_pages(d, p, i32([0], dev), torch.zeros((1,), dtype=torch.int32))
    with pytest.raises(RuntimeError, match="kv_param"):
        mixedgemm.kv_copy_pages(d, p[:3].contiguous(), i32([0], dev), i32([1], dev))
    with pytest.raises(TypeError):
        mixedgemm.kv_copy_pages(d, None, i32([0], dev), i32([1], dev))           # without params the data must be bf16
    torch.cuda.synchronize()
    assert bool((d == 7).all()) and bool((p == 1).all())


def extend_counting_copies(cache, new):
    """extend, and the number of sequences whose partly filled last page was swapped for a fresh one"""
    old = [(n, p[-1] if p else None) for n, p in zip(cache.seq_lens, cache._pages)]
    cache.extend(new)
    return sum(1 for s, (n, last) in enumerate(old) if n % cache.page_size and cache._pages[s][(n - 1) // cache.page_size] != last)


# ---- 2. twin equality ----------------------------------------------------------------------------------------------------------------------
class Pair:
    """cache `a` forks and truncates; cache `b` never shares: after a fork or truncate the sequence is emptied and appended again from
    the K / V rows the model (self.k, self.v: per sequence, per layer) says it holds"""

    def __init__(self, dev, kind, P, Hkv, g, W, pools, seed, L=2, layers=None, batch=3, bound=None):
        self.dev, self.L, self.Hkv, self.Hq, self.P, self.W, self.batch, self.bound = dev, L, Hkv, g * Hkv, P, W, batch, bound
        self.layers = list(range(L)) if layers is None else layers
        self.a = PagedKVCache(L, Hkv, P, pools[0], batch, kind=kind, device=dev, window=W, max_seq_len=256)
        self.b = PagedKVCache(L, Hkv, P, pools[1], batch, kind=kind, device=dev, window=W, max_seq_len=256)
        self.rng = np.random.default_rng(seed)
        empty = lambda: {layer: torch.zeros((0, Hkv, 128), dtype=torch.bfloat16, device=dev) for layer in self.layers}
        self.k, self.v = [empty() for _ in range(batch)], [empty() for _ in range(batch)]

    def lens(self):
        return [int(self.k[s][self.layers[0]].size(0)) for s in range(self.batch)]

    def record(self, new, layer, k, v):
        at = 0
        for s, n in enumerate(new):
            self.k[s][layer] = torch.cat([self.k[s][layer], k[at:at + n]])
            self.v[s][layer] = torch.cat([self.v[s][layer], v[at:at + n]])
            at += n

    def extend(self, new, what):
        new = [new] * self.batch if isinstance(new, int) else new
        self.copied = extend_counting_copies(self.a, new)
        self.b.extend(new)
        for layer in self.layers:
            k, v = (rand_bf16((sum(new), self.Hkv, 128), self.rng, self.dev, s) for s in (1.0, 0.5))
            self.a.append(layer, k, v)
            self.b.append(layer, k, v)
            self.record(new, layer, k, v)
        assert self.a.seq_lens == self.b.seq_lens == self.lens()
        self.compare(what, new)

    def rebuild(self, seq):
        self.b.reset(seq)
        n = self.lens()[seq]
        if n:
            self.b.extend([n if s == seq else 0 for s in range(self.batch)])
            for layer in self.layers:
                self.b.append(layer, self.k[seq][layer], self.v[seq][layer])

    def fork(self, src, dst, length, what):
        self.a.fork(src, dst, length)
        for layer in self.layers:
            self.k[dst][layer], self.v[dst][layer] = self.k[src][layer][:length], self.v[src][layer][:length]
        self.rebuild(dst)
        self.compare(what)

    def refused(self, seq, length):
        """the window condition, from the rule: released pages the shorter sequence would keep must lie wholly below its window"""
        kept = min(self.a._released[seq], -(-length // self.P))
        return kept * self.P > max(0, length - (self.W or 0))

    def truncate(self, seq, length, what):
        self.a.truncate(seq, length)
        for layer in self.layers:
            self.k[seq][layer], self.v[seq][layer] = self.k[seq][layer][:length], self.v[seq][layer][:length]
        self.rebuild(seq)
        self.compare(what)

    def reset(self, seq, what):
        self.a.reset(seq)
        self.b.reset(seq)
        for layer in self.layers:
            self.k[seq][layer], self.v[seq][layer] = self.k[seq][layer][:0], self.v[seq][layer][:0]
        self.compare(what)

    def compare(self, what, new=None):
        """attend on both; attend_new on both for the tokens an extend announced; and, whatever the step was, the multi-token kernel
        with one query at each sequence's last position (what a sequence may attend whatever its window has released)"""
        lens = self.lens()
        assert self.a.seq_lens == lens == self.b.seq_lens
        bound = self.bound or max(lens + [1])
        one = [int(n > 0) for n in lens]
        qo = i32(np.concatenate([[0], np.cumsum(one)]), self.dev)
        for layer in self.layers:
            q = rand_bf16((self.batch, self.Hq, 128), self.rng, self.dev, 2.0)
            same_bits(self.a.attend(layer, q, max_seq_len=bound), self.b.attend(layer, q, max_seq_len=bound), f"{what}: attend, layer {layer}")
            if new is not None and sum(new):
                q = rand_bf16((sum(new), self.Hq, 128), self.rng, self.dev, 2.0)
                same_bits(self.a.attend_new(layer, q, max_seq_len=bound), self.b.attend_new(layer, q, max_seq_len=bound), f"{what}: attend_new, layer {layer}")
            if sum(one):
                q = rand_bf16((sum(one), self.Hq, 128), self.rng, self.dev, 2.0)
                o = [mixedgemm.paged_prefill(q, c.kv_data, c.kv_param, c.kv_indptr, c.kv_indices, c.last_page_len, qo, layer, bound, window=c.window)
                     for c in (self.a, self.b)]
                same_bits(*o, f"{what}: one query per sequence through the multi-token kernel, layer {layer}")
        if max(self.a._ref) > 1:
            assert self.a.pages_in_use < self.b.pages_in_use, f"{what}: sharing must save pages"
        assert self.a.pages_in_use <= self.b.pages_in_use


POOLS = {1: (72, 200), 4: (24, 60), 16: (12, 24)}


def script(t):
    """prefill, two forks (full; 21 tokens: mid-page for P = 4 and 16, a page edge for P = 1), diverging decode steps, a truncate, a
    5-token draft of which 3 are taken back, a reset of the sequence whose pages the others still share, more decode"""
    t.extend([37, 0, 0], "prefill")
    t.fork(0, 1, None, "fork 0 -> 1")
    t.fork(0, 2, 21, "fork 0 -> 2, 21 tokens")
    assert t.a._pages[1] == t.a._pages[0] and t.a._pages[2] == t.a._pages[0][: -(-21 // t.P)] and t.a.pages_in_use == -(-37 // t.P)
    for step in range(3):
        t.extend(1, f"decode {step}")
        # 37 and 21 both end mid-page unless P = 1: sequences 0 and 1 share their last page (one copy, the second to be served owns it
        # alone), sequence 2 shares its last page with both (one copy); after that every sequence writes into pages of its own
        assert t.copied == (2 if step == 0 and t.P > 1 else 0)
    n = t.lens()[1]
    if t.refused(1, n - 3):                              # with a window the decode steps released what tokens n - 4 .. would attend
        assert t.W
        with pytest.raises(ValueError, match="released"):
            t.a.truncate(1, n - 3)
        t.compare("refused truncate")
    else:
        assert not t.W
        t.truncate(1, n - 3, "truncate 1 by 3")
    t.extend([0, 5, 0], "5 tokens on sequence 1")
    t.truncate(1, t.lens()[1] - 3, "3 of the 5 taken back")
    assert max(t.a._ref) > 1
    t.reset(0, "reset 0 while its pages are shared")
    t.extend([0, 1, 1], "decode after the reset")
    t.extend(1, "decode, sequence 0 starting again")
    t.fork(1, 0, None, "fork 1 -> 0")
    t.extend([2, 0, 1], "two tokens on the fork")
    assert t.copied == (t.lens()[1] % t.P != 0)


@pytest.mark.parametrize("W", [None, 24])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [1, 4, 16])
@pytest.mark.parametrize("g", [1, 4])
def test_forked_cache_equals_a_cache_that_never_shares(dev, g, P, kind, W):
    script(Pair(dev, kind, P, 2, g, W, POOLS[P], seed=1000 * g + 10 * P + len(kind)))


def test_forked_cache_on_the_split_kv_path(dev):
    """one kv head and a bound of 1024 tokens: decode and prefill both cut the range into chunks and merge them"""
    B, Hq, Hkv, bound = 3, 4, 1, 1024
    assert mixedgemm.paged_decode_workspace_bytes(B, Hq, Hkv, bound) > 0
    for T in (1, 2, 3, 5, 37):
        assert mixedgemm.paged_prefill_workspace_bytes(T, B, Hq, Hkv, bound) > 0
    script(Pair(dev, "int4", 16, Hkv, 4, None, POOLS[16], seed=5, bound=bound))


# ---- 3. the sole-owner rule on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [4, 16])
def test_only_the_new_rows_and_the_copied_page_change(dev, kind, P):
    L, Hkv, n0 = 2, 2, 37
    rng = np.random.default_rng(P)
    c = PagedKVCache(L, Hkv, P, 16, 2, kind=kind, device=dev)
    r = PagedKVCache(L, Hkv, P, 4, 2, kind=kind, device=dev)          # where the two new tokens' rows are written on their own
    hd, hp = poison(kind, 16, L, Hkv, P, 11)
    d, p = to_dev(kind, hd, hp, dev)
    c.kv_data.copy_(d)
    if p is not None:
        c.kv_param.copy_(p)
    c.extend([n0, 0])
    for layer in range(L):
        c.append(layer, rand_bf16((n0, Hkv, 128), rng, dev), rand_bf16((n0, Hkv, 128), rng, dev, 0.5))
    torch.cuda.synchronize()
    snap_d, snap_p = to_host(c.kv_data, c.kv_param)
    snap_d, snap_p = snap_d.copy(), None if snap_p is None else snap_p.copy()
    pages, rows = list(c._pages[0]), n0 % P
    assert 0 < rows < P
    c.fork(0, 1)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(c.kv_data, c.kv_param)[0], snap_d), "fork copies nothing"
    c.extend([1, 1])
    r.extend([1, 1])
    for layer in range(L):
        k, v = rand_bf16((2, Hkv, 128), rng, dev), rand_bf16((2, Hkv, 128), rng, dev, 0.5)
        c.append(layer, k, v)
        r.append(layer, k, v)
    torch.cuda.synchronize()
    # sequence 0 was served first: it moved to a fresh page; sequence 1 was then the old page's sole owner and wrote into it
    new, old = c._pages[0][-1], pages[-1]
    assert c._pages[0][:-1] == pages[:-1] and new not in pages and c._pages[1] == pages and c._ref[old] == 1 and c._ref[new] == 1
    assert all(c._ref[q] == 2 for q in pages[:-1]) and c.pages_in_use == len(pages) + 1
    rd, rp = to_host(r.kv_data, r.kv_param)
    want_d, want_p = snap_d.copy(), None if snap_p is None else snap_p.copy()
    for arr, ref in ((want_d, rd), (want_p, rp)):
        if arr is not None:
            arr[new, :, :, :, :rows] = arr[old, :, :, :, :rows]                   # the copied rows
            arr[new, :, :, :, rows] = ref[r._pages[0][0], :, :, :, 0]             # sequence 0's token
            arr[old, :, :, :, rows] = ref[r._pages[1][0], :, :, :, 0]             # sequence 1's token
    got_d, got_p = to_host(c.kv_data, c.kv_param)
    assert np.array_equal(got_d, want_d), f"{int((got_d != want_d).sum())} bytes differ: shared pages or rows outside the copy were touched"
    assert want_p is None or np.array_equal(got_p, want_p)
    assert np.array_equal(got_d[pages[:-1]], snap_d[pages[:-1]]) and np.array_equal(got_d[old, :, :, :, :rows], snap_d[old, :, :, :, :rows])


# ---- 4. graph ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replays_across_a_copying_extend_and_a_truncate(dev, kind):
    """append + attend of layer 1 captured once on a forked cache; every replay against the eager twin"""
    layer, bound = 1, 128
    t = Pair(dev, kind, 16, 2, 4, None, POOLS[16], seed=77, layers=[layer], bound=bound)
    a, b = t.a, t.b
    t.extend([37, 0, 0], "prefill")
    t.fork(0, 1, None, "fork 0 -> 1")
    t.fork(0, 2, 21, "fork 0 -> 2")
    sk, sv, sq = (rand_bf16((3, h, 128), t.rng, dev) for h in (t.Hkv, t.Hkv, t.Hq))
    assert extend_counting_copies(a, [1, 1, 1]) == 2
    b.extend(1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.append(layer, sk, sv)
        a.attend(layer, sq, max_seq_len=bound)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.append(layer, sk, sv)
        out = a.attend(layer, sq, max_seq_len=bound)
    steps = [(None, 0),                                                                            # the tokens announced before the capture
             (lambda: t.fork(0, 2, None, "fork 0 -> 2 again"), 1),                                 # 0 and 2 share a partly filled page
             (lambda: t.truncate(1, t.lens()[1] - 3, "truncate 1 by 3"), 0),                       # its own page: overwritten in place
             (lambda: t.fork(1, 0, t.lens()[1] - 2, "fork 1 -> 0 mid-page"), 1)]
    for i, (before, copies) in enumerate(steps):
        if before:
            before()
            assert extend_counting_copies(a, [1, 1, 1]) == copies, f"step {i}"
            b.extend(1)
        for x in (sk, sv, sq):
            x.copy_(rand_bf16(tuple(x.shape), t.rng, dev))
        graph.replay()
        torch.cuda.synchronize()
        got = out.clone()
        b.append(layer, sk, sv)
        t.record([1, 1, 1], layer, sk.clone(), sv.clone())
        same_bits(got, b.attend(layer, sq, max_seq_len=bound), f"replay {i} against the eager twin")
        same_bits(got, a.attend(layer, sq, max_seq_len=bound), f"replay {i} against eager on the same cache")

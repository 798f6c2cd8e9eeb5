"""CPU tests of page sharing in the paged KV cache: the host side of mm_kv_copy_pages (symbol, statuses without device work, Python
argument errors) and PagedKVCache's reference counts, fork, truncate and copy-on-write, driven on a CPU cache next to a model that
holds every sequence as a list of token ids.  No kernel is launched here.

The no-fork identity literals (BASIC_TRACE, WINDOW_TRACES) were recorded from the class as it was before it counted references: run
this file as a script (PYTHONPATH = the repository root and tests/) against a checkout to print them."""
import hashlib
import inspect

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache

L, HKV = 2, 2
SEGS = L * 2 * HKV


# ---- the C ABI and the Python op -----------------------------------------------------------------------------------------------------
def test_symbol_declared_and_exported_and_the_version_stays():
    lib = _lib.load()
    header = open(inspect.getsourcefile(_lib).replace("micromix_amd/_lib.py", "include/micromix_hip.h")).read()
    assert "mm_kv_copy_pages" in _lib.EXPORTS and hasattr(lib, "mm_kv_copy_pages") and "int mm_kv_copy_pages(" in header
    assert lib.mm_version() == 660
    assert "kv_copy_pages" in mixedgemm.__all__ and callable(mixedgemm.kv_copy_pages)
    assert list(inspect.signature(mixedgemm.kv_copy_pages).parameters) == ["kv_data", "kv_param", "src_pages", "dst_pages", "rows"]
    assert inspect.signature(mixedgemm.kv_copy_pages).parameters["rows"].default is None


def test_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes (16) or null"""
    lib = _lib.load()
    OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED

    def copy(kind=0, data=16, param=16, max_pages=4, L=2, Hkv=8, P=16, hd=128, src=16, dst=16, rows=16, n=0):
        return lib.mm_kv_copy_pages(data, param, kind, max_pages, L, Hkv, P, hd, src, dst, rows, n, None)

    for kind in (_lib.MM_KV_INT4, _lib.MM_KV_BF16, _lib.MM_KV_FP8_E4M3):
        assert copy(kind) == OK and copy(kind, src=None, dst=None, rows=None) == OK              # no pairs: nothing to do
        assert copy(kind, data=None) == BAD
        assert copy(kind, param=None) == (OK if kind == _lib.MM_KV_BF16 else BAD)                # int4 and fp8 need their params
        for bad in (dict(max_pages=0), dict(L=0), dict(Hkv=0), dict(P=0), dict(hd=0), dict(L=-1), dict(P=-3), dict(n=-1)):
            assert copy(kind, **bad) == BAD, bad
        for hd in (64, 127, 256):
            assert copy(kind, hd=hd) == UNS and copy(kind, hd=hd, n=1, data=None) == UNS
        # with pairs, the index arrays are needed (rows may be null: whole pages); the null data pointer is the backstop of these rows
        assert copy(kind, n=1, src=None) == BAD and copy(kind, n=1, dst=None) == BAD
        assert copy(kind, n=1, data=None, rows=None) == BAD
        assert copy(kind, data=24) == BAD                                                        # kv_data not 16-byte aligned
    assert copy(_lib.MM_KV_INT4, param=18) == BAD                                                # kv_param not 4-byte aligned
    for kind in (2, 4, -1, 255):
        assert copy(kind) == BAD and not lib.mm_kv_dtype_supported(kind)
    assert copy(L=1 << 13, Hkv=1 << 10, P=1 << 3) == UNS and copy(L=1 << 12, Hkv=1 << 10, P=1 << 3) == OK    # 2 L Hkv P below 2^27


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.uint8)
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.kv_copy_pages(data, param, i32(2), i32(2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.kv_copy_pages(torch.zeros((4, 2, 2, 8, 16, 128), dtype=torch.bfloat16), None, i32(2), i32(2), i32(2))
    with pytest.raises(TypeError):
        mixedgemm.kv_copy_pages(data.float(), param, i32(2), i32(2))
    with pytest.raises(TypeError):
        mixedgemm.kv_copy_pages(None, None, i32(2), i32(2))


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def row_bytes(tids, width):
    """[n, SEGS, width] uint8: what each token holds in its (layer, K / V, head) rows -- the whole id, in every four bytes"""
    j = np.arange(width)
    seg = np.arange(SEGS)[:, None]
    return (((np.asarray(tids).reshape(-1, 1, 1) >> (8 * (j % 4))) & 255) + 37 * seg + j).astype(np.uint8)


def param_bits(tids):
    """[n, SEGS, 2] int16"""
    seg, t = np.arange(SEGS), np.asarray(tids).reshape(-1, 1)
    return np.stack([(t * 31 + seg) & 0x7FFF, ((t >> 3) + 5 * seg) & 0x7FFF], -1).astype(np.int16)


class Twin:
    """a CPU cache and the model next to it: tokens[b] = the ids sequence b holds"""

    def __init__(self, P, max_pages, B, kind, window):
        self.c = PagedKVCache(L, HKV, P, max_pages, B, kind=kind, device="cpu", window=window)
        self.P, self.B, self.W = P, B, self.c.window
        self.tokens = [[] for _ in range(B)]
        self.next_id = 1
        self.data = self.c.kv_data.view(torch.uint8).numpy()                      # [pages, L, 2, Hkv, P, bytes]: the cache's own memory
        self.param = None if self.c.kv_param is None else self.c.kv_param.view(torch.int16).numpy()
        self.copies = self.failed = self.refused = self.most_released = 0

    def state(self):
        c = self.c
        return repr((c._pages, c._free, c._ref, c._released, c.seq_lens, c.num_new_tokens, c.kv_indptr.tolist(), c.kv_indices.tolist(),
                     c.last_page_len.tolist(), c.append_indptr.tolist())), self.data.tobytes(), None if self.param is None else self.param.tobytes()

    def table(self, b):
        indptr = self.c.kv_indptr.tolist()
        return self.c.kv_indices.tolist()[indptr[b]:indptr[b + 1]]

    def slots(self, b, lo, hi):
        """(page, slot) of positions lo .. hi - 1 of sequence b, by the table on the "device"""""
        pos = np.arange(lo, hi)
        return np.asarray(self.table(b), dtype=np.int64)[pos // self.P], pos % self.P

    def extend(self, new):
        before = self.state()
        old_pages = [list(p) for p in self.c._pages]
        try:
            self.c.extend(new)
        except RuntimeError as e:
            assert "out of pages" in str(e)
            assert self.state() == before, "a failed extend changed something"
            self.failed += 1
            return
        for b, n in enumerate(new):
            start = len(self.tokens[b])
            if n and start % self.P and self.c._pages[b][start // self.P] != old_pages[b][start // self.P]:
                self.copies += 1
            if n:                                                                # write the new tokens where the table says
                tids = list(range(self.next_id, self.next_id + n))
                self.next_id += n
                self.tokens[b] += tids
                pages, slot = self.slots(b, start, start + n)
                assert all(self.c._ref[p] == 1 for p in pages), "a sequence writes into a page it does not own alone"
                self.data[pages, :, :, :, slot] = row_bytes(tids, self.data.shape[-1]).reshape(n, L, 2, HKV, -1)
                if self.param is not None:
                    self.param[pages, :, :, :, slot] = param_bits(tids).reshape(n, L, 2, HKV, 2)
        assert self.c.append_indptr.tolist() == np.concatenate([[0], np.cumsum(new)]).tolist()

    def refusal_expected(self, seq, length):
        kept = min(self.c._released[seq], -(-length // self.P))
        return kept * self.P > max(0, length - self.W)

    def fork(self, src, dst, length):
        want = len(self.tokens[src]) if length is None else length
        before = self.state()
        if self.refusal_expected(src, want):
            with pytest.raises(ValueError, match="released"):
                self.c.fork(src, dst, length)
            assert self.state() == before
            self.refused += 1
            return
        self.c.fork(src, dst, length)
        self.tokens[dst] = self.tokens[src][:want]
        assert self.state()[1:] == before[1:], "fork copies nothing"

    def truncate(self, seq, length):
        before = self.state()
        if self.refusal_expected(seq, length):
            with pytest.raises(ValueError, match="released"):
                self.c.truncate(seq, length)
            assert self.state() == before
            self.refused += 1
            return
        self.c.truncate(seq, length)
        del self.tokens[seq][length:]
        assert self.state()[1:] == before[1:], "truncate copies nothing"

    def reset(self, seq):
        self.c.reset(seq)
        self.tokens[seq] = []

    def check(self):
        c, P = self.c, self.P
        count = [0] * c.max_pages
        for b in range(self.B):
            n = len(self.tokens[b])
            assert c.seq_lens[b] == n and len(c._pages[b]) == -(-n // P), "one entry per page_size tokens of the model"
            assert self.table(b) == c._pages[b] and c.last_page_len[b] == (n - (len(c._pages[b]) - 1) * P if n else 0)
            rel = c._released[b]
            assert all(p == -1 for p in c._pages[b][:rel]) and all(0 <= p < c.max_pages for p in c._pages[b][rel:])
            assert rel * P <= max(0, n - self.W) if self.W else rel == 0, "a released page inside the window"
            for p in c._pages[b][rel:]:
                count[p] += 1
        self.most_released = max(self.most_released, *c._released)
        assert c._ref == count, "a page's count is the number of entries that name it"
        assert sorted(c._free) == [p for p in range(c.max_pages) if count[p] == 0] and len(set(c._free)) == len(c._free)
        assert c.pages_in_use == sum(k > 0 for k in count) == c.max_pages - len(c._free)
        # the model's page count: pages whose first tokens differ cannot be one page, and no page is held beyond the entries
        firsts = {(i, self.tokens[b][i * P]) for b in range(self.B) for i in range(c._released[b], len(c._pages[b]))}
        assert len(firsts) <= c.pages_in_use <= sum(len(c._pages[b]) - c._released[b] for b in range(self.B))
        for b in range(self.B):                                                   # each sequence reads back exactly its tokens
            lo, n = c._released[b] * P, len(self.tokens[b])
            if lo < n:
                pages, slot = self.slots(b, lo, n)
                want = row_bytes(self.tokens[b][lo:], self.data.shape[-1]).reshape(n - lo, L, 2, HKV, -1)
                assert np.array_equal(self.data[pages, :, :, :, slot], want), (b, "codes")
                assert self.param is None or np.array_equal(self.param[pages, :, :, :, slot], param_bits(self.tokens[b][lo:]).reshape(n - lo, L, 2, HKV, 2)), (b, "params")


def drive(P, max_pages, window, kind, steps, seed):
    t, rng, B = Twin(P, max_pages, 4, kind, window), np.random.default_rng(seed), 4
    counts = [0, 0, 1, 1, 1, 2, 3, P - 1, P, P + 1, 2 * P + 1]
    for _ in range(steps):
        op = rng.choice(["extend", "extend", "extend", "fork", "fork", "truncate", "reset"], p=[0.2, 0.2, 0.2, 0.12, 0.12, 0.1, 0.06])
        if op == "extend":
            new = [int(rng.choice(counts)) if rng.random() < 0.7 else 0 for _ in range(B)]
            t.extend(new)
        elif op == "fork":
            src, dst = (int(x) for x in rng.choice(B, 2, replace=False))
            n = len(t.tokens[src])
            pick = rng.random()
            length = None if pick < 0.4 else int(rng.integers(0, n + 1)) if pick < 0.8 else (n // P) * P    # full, anywhere (mid-page), page edge
            t.fork(src, dst, length)
        elif op == "truncate":
            seq = int(rng.integers(B))
            n = len(t.tokens[seq])
            t.truncate(seq, n if rng.random() < 0.1 else int(rng.integers(max(0, n - 2 * P), n + 1)))
        else:
            t.reset(int(rng.integers(B)))
        t.check()
    return t


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("P, max_pages", [(1, (40, 16)), (4, (14, 12)), (16, (9, 9))])         # (without, with a window)
def test_allocator_and_contents_against_the_token_model(P, max_pages, window):
    """2 500 random operations; after each one every invariant of Twin.check, with out-of-pages, copies and (with a window) refusals
    all occurring"""
    W = (2 * P + 1 if P > 1 else 5) if window else None
    max_pages = max_pages[window]
    t = drive(P, max_pages, W, "int4" if P != 4 else "bf16", 2500, 1000 * P + bool(window))
    assert t.failed >= 5, "the pool must run out"
    assert t.copies >= 20 or P == 1, "copy-on-write must happen"          # P = 1 has no partly filled page
    assert P > 1 or t.copies == 0
    assert (t.refused >= 5 and t.most_released >= 2) if window else (t.refused == 0 and t.most_released == 0)
    for b in range(4):
        t.reset(b)
    t.check()
    assert sorted(t.c._free) == list(range(max_pages))


def test_errors_of_fork_and_truncate():
    c = PagedKVCache(1, 1, 4, 8, 3, kind="bf16", device="cpu")
    c.extend([6, 0, 0])
    for bad in (lambda: c.fork(0, 0), lambda: c.fork(0, 1, 7), lambda: c.fork(0, 1, -1), lambda: c.truncate(0, 7), lambda: c.truncate(0, -1),
                lambda: c.fork(1, 2, 1)):
        with pytest.raises(ValueError):
            bad()
    assert c._pages == [[0, 1], [], []] and c.pages_in_use == 2
    c.fork(0, 1)
    c.fork(0, 2, 0)                                                   # a reset
    assert c._pages == [[0, 1], [0, 1], []] and c._ref[:2] == [2, 2] and c.pages_in_use == 2 and c.seq_lens == [6, 6, 0]
    c.extend([1, 0, 0])                                               # page 1 is partly filled and shared: seq 0 moves to a fresh page
    assert c._pages == [[0, 2], [0, 1], []] and c._ref[:3] == [2, 1, 1]
    c.extend([0, 1, 0])                                               # seq 1 is now page 1's sole owner: no second copy
    assert c._pages == [[0, 2], [0, 1], []] and c.pages_in_use == 3
    c.reset(0)
    assert c._pages == [[], [0, 1], []] and c._free[-1] == 2 and c._ref[:3] == [1, 1, 0]
    c.truncate(1, 4)
    assert c._pages[1] == [0] and c._free[-2:] == [2, 1]


def test_out_of_pages_counts_the_copies_and_only_pages_that_come_free():
    c = PagedKVCache(1, 1, 4, 3, 2, kind="bf16", device="cpu")
    c.extend([6, 0])
    c.fork(0, 1)
    c.extend([1, 0])                                                  # the copy takes the last page
    assert c.pages_in_use == 3
    c.truncate(0, 6)
    c.fork(1, 0)
    assert c.pages_in_use == 2
    c.extend([2, 0])                                                  # one page for the copy; the two tokens fit it
    state = repr((c._pages, c._free, c._ref, c.seq_lens))
    with pytest.raises(RuntimeError, match="out of pages: 1 needed, 0 free"):
        c.extend([0, 3])                                              # seq 1 owns page 1 alone by now, but needs a third page
    assert repr((c._pages, c._free, c._ref, c.seq_lens)) == state
    # a windowed release of a shared page gains nothing until the last owner releases it
    w = PagedKVCache(1, 1, 4, 4, 2, kind="bf16", device="cpu", window=4)
    w.extend([8, 0])
    w.fork(0, 1, 6)
    w.extend([4, 0])                                                  # seq 0 releases page 0 (still seq 1's) and takes a new page
    assert w._pages == [[-1, 1, 2], [0, 1]] and w._ref[:3] == [1, 2, 1] and w.pages_in_use == 3
    with pytest.raises(RuntimeError, match="out of pages: 2 needed, 1 free"):
        w.extend([8, 0])                                              # releases page 1 as well, which seq 1 holds too: only page 3 is free
    w.reset(1)                                                        # page 0's last owner lets go; page 1 stays seq 0's
    assert w._pages == [[-1, 1, 2], []] and w._free == [3, 0] and w._ref == [0, 1, 1, 0]
    w.extend([8, 0])                                                  # now page 1 comes free with the release, and is handed out again
    assert w._pages == [[-1, -1, 2, 1, 0], []] and w._free == [3]


# ---- windows -----------------------------------------------------------------------------------------------------------------------------
def test_fork_and_truncate_below_a_released_page_are_refused():
    P, W = 4, 6
    c = PagedKVCache(1, 1, P, 16, 3, kind="bf16", device="cpu", window=W)
    c.extend([19, 0, 0])
    c.extend([1, 0, 0])                       # 20 tokens; the decode query at 19 attends from 14: pages 0 .. 2 (positions 0 .. 11) released
    assert c._released[0] == 3 and c._pages[0][:3] == [-1, -1, -1]
    # a sequence of `length` tokens attends from length - W: 3 released pages are fine from length 18 on
    for length in (17, 12, 5, 1):
        with pytest.raises(ValueError, match="released"):
            c.fork(0, 1, length)
        with pytest.raises(ValueError, match="released"):
            c.truncate(0, length)
    c.fork(0, 1, 18)                          # the boundary: 3 * 4 <= 18 - 6
    assert c._pages[1] == c._pages[0][:5] and c._released[1] == 3 and c.seq_lens[1] == 18
    c.fork(0, 2, 0)                           # nothing is kept, so nothing can be masked
    assert c._pages[2] == [] and c._released[2] == 0
    c.truncate(0, 18)
    assert c.seq_lens[0] == 18 and c._released[0] == 3
    with pytest.raises(ValueError, match="released"):
        c.truncate(0, 17)
    c.truncate(0, 0)
    assert c._pages[0] == [] and c._released[0] == 0 and c.pages_in_use == 2      # seq 1 still holds pages 3 and 4
    # without release nothing is ever refused
    k = PagedKVCache(1, 1, P, 16, 2, kind="bf16", device="cpu", window=W, release=False)
    k.extend([20, 0])
    k.fork(0, 1, 3)
    k.truncate(0, 1)
    assert k.pages_in_use == 1 and k._ref[k._pages[0][0]] == 2


# ---- a cache that never forks allocates as it always did -------------------------------------------------------------------------------
def digest(states):
    return hashlib.sha256(repr(states).encode()).hexdigest()[:16]


def basic_trace(cls):
    """the operations of tests/test_kvcache_cpu.py::test_page_allocator_bookkeeping_on_host"""
    c = cls(2, 2, 4, 8, 3, kind="bf16", device="cpu")
    out = []
    for op in (lambda: c.extend([5, 0, 4]), lambda: c.extend(1), lambda: c.reset(0), lambda: c.extend([40, 0, 0]), lambda: c.extend([3, 2, 0])):
        try:
            op()
        except RuntimeError:
            out.append("out of pages")
        out.append(([list(p) for p in c._pages], list(c._free)))
    return out


def window_trace(cls, P, W):
    """the operations of tests/test_kv_window_cpu.py::test_cache_releases_exactly_the_pages_below_the_window"""
    B, rng = 4, np.random.default_rng(P * 1000 + W)
    most = 30
    cache = cls(1, 1, P, B * (-(-(W + most) // P) + 1) + 2, B, kind="bf16", device="cpu", window=W)
    states = []
    for step in range(300):
        if step % 3 == 0:
            new = [1] * B
        elif step % 3 == 1:
            new = [int(n) for n in rng.integers(0, most + 1, B)]
        else:
            new = [0, 1, 0, int(rng.integers(1, most + 1))]
        if step in (120, 200):
            cache.reset(1)
            states.append(([list(p) for p in cache._pages], list(cache._free), list(cache._released)))
        cache.extend(new)
        states.append(([list(p) for p in cache._pages], list(cache._free), list(cache._released), cache.kv_indices.tolist()))
    return digest(states), (cache._pages[0][-2:], cache._free[-3:])


BASIC_TRACE = [([[0, 1], [], [2]], [7, 6, 5, 4, 3]), ([[0, 1], [3], [2, 4]], [7, 6, 5]), ([[], [3], [2, 4]], [7, 6, 5, 1, 0]), 'out of pages',
               ([[], [3], [2, 4]], [7, 6, 5, 1, 0]), ([[0], [3], [2, 4]], [7, 6, 5, 1])]
# (a digest of every step's _pages, _free, _released and kv_indices, the last two entries of sequence 0 and the top of the free list)
WINDOW_TRACES = {(16, 40): ('6bd8a88946b63075', ([3, 4], [13, 14, 2])), (1, 7): ('8a3eef0c27eaccf9', ([93, 110], [105, 57, 77])),
                 (24, 100): ('ebb774c69c438c6b', ([14, 20], [15, 19, 18])), (16, 1): ('0971b7c7eab541ce', ([-1, 3], [9, 7, 10])),
                 (16, 16): ('e01d21977ecd1efb', ([14, 9], [10, 13, 2]))}


def test_no_fork_identity_basic():
    assert basic_trace(PagedKVCache) == BASIC_TRACE


@pytest.mark.parametrize("P, W", [(16, 40), (1, 7), (24, 100), (16, 1), (16, 16)])
def test_no_fork_identity_window_release(P, W):
    assert window_trace(PagedKVCache, P, W) == WINDOW_TRACES[(P, W)]


if __name__ == "__main__":
    print("BASIC_TRACE =", basic_trace(PagedKVCache))
    print("WINDOW_TRACES =", {pw: window_trace(PagedKVCache, *pw) for pw in [(16, 40), (1, 7), (24, 100), (16, 1), (16, 16)]})

"""CPU tests of tree-masked attention over the paged KV cache and of keeping a path: the host side of mm_paged_prefill_tree and
mm_kv_move_rows (symbols, statuses without device work, Python argument errors), PagedKVCache.tree_mask / accept on a CPU cache next to
a twin that only ever saw the accepted tokens, and the numpy oracle itself (tests/kv_tree_oracle.py).  No kernel is launched here."""
import inspect

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_oracle as ko
import kv_prefill_oracle as kpo
import kv_tree_oracle as kto

KINDS = (_lib.MM_KV_INT4, _lib.MM_KV_BF16, _lib.MM_KV_FP8_E4M3)
# the 4-ary tree of depth 3: a root, its 4 children (nodes 1 .. 4) and 4 children of each of them (5 .. 20): 21 nodes, 16 root-to-leaf paths
TREE21 = [-1] + [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4


# ---- the C ABI and the Python ops ----------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported_and_the_version_stays():
    lib = _lib.load()
    header = open(inspect.getsourcefile(_lib).replace("micromix_amd/_lib.py", "include/micromix_hip.h")).read()
    for name in ("mm_paged_prefill_tree", "mm_kv_move_rows"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header, name
    assert lib.mm_version() == 660
    assert "kv_move_rows" in mixedgemm.__all__ and callable(mixedgemm.kv_move_rows)
    assert list(inspect.signature(mixedgemm.kv_move_rows).parameters) == ["kv_data", "kv_param", "kv_indptr", "kv_indices", "move_indptr",
                                                                          "src_pos", "dst_pos"]
    p = inspect.signature(mixedgemm.paged_prefill).parameters["tree_mask"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm", inspect.getsourcefile(_lib).replace("_lib.py", "dropin/mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.kv_move_rows is mixedgemm.kv_move_rows and dropin.paged_prefill is mixedgemm.paged_prefill


def test_tree_prefill_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes (16, 64) or null"""
    lib = _lib.load()
    OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED

    def tree(kind=0, q=16, qo=16, T=5, data=16, param=16, max_pages=4, L=2, layer=1, Hkv=8, P=16, hd=128, indptr=16, indices=16, last=16,
             B=2, Hq=32, msl=100, ws=None, ws_bytes=0, o=16, mask=64):
        return lib.mm_paged_prefill_tree(q, qo, T, data, param, kind, max_pages, L, layer, Hkv, P, hd, indptr, indices, last, B, Hq, msl,
                                         0.0, ws, ws_bytes, o, None, mask)

    assert lib.mm_paged_prefill_workspace_bytes(5, 2, 32, 8, 100) == 0
    for kind in KINDS:
        assert tree(kind, T=0) == OK and tree(kind, B=0) == OK and tree(kind, T=0, mask=None, q=None) == OK     # nothing to do
        for ptr in ("q", "qo", "data", "indptr", "indices", "last", "o", "mask"):
            assert tree(kind, **{ptr: None}) == BAD, ptr
        if kind != _lib.MM_KV_BF16:
            assert tree(kind, param=None) == BAD                                   # int4 and fp8 need their params
        for mask in (65, 66, 68, 60):                                              # the words are read as 64-bit loads
            assert tree(kind, mask=mask) == BAD, mask
        for bad in (dict(max_pages=0), dict(L=0), dict(layer=2), dict(layer=-1), dict(Hkv=0), dict(P=0), dict(hd=0), dict(B=-1), dict(T=-1),
                    dict(Hq=0), dict(Hq=33), dict(msl=-1)):
            assert tree(kind, **bad) == BAD, bad
        assert tree(kind, hd=64) == UNS and tree(kind, Hq=8 * 17) == UNS
        # a bound long enough for the split path: the workspace of mm_paged_prefill_workspace_bytes, present, large enough, aligned
        need = lib.mm_paged_prefill_workspace_bytes(5, 2, 16, 1, 1 << 20)
        assert need > 0
        split = dict(Hkv=1, Hq=16, msl=1 << 20)
        assert tree(kind, **split) == BAD and tree(kind, ws=16, ws_bytes=need - 1, **split) == BAD
        assert tree(kind, ws=24, ws_bytes=need, **split) == BAD
        assert tree(kind, ws=16, ws_bytes=need, mask=None, **split) == BAD
    assert tree(_lib.MM_KV_BF16, param=None, mask=None) == BAD                     # a bf16 cache needs no params, but the words
    for kind in (2, 4, -1):
        assert tree(kind) == BAD


def test_move_rows_statuses_without_device_work():
    lib = _lib.load()
    OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED

    def move(kind=0, data=16, param=16, max_pages=4, L=2, Hkv=8, P=16, hd=128, indptr=16, indices=16, B=2, mptr=16, src=16, dst=16, n=0):
        return lib.mm_kv_move_rows(data, param, kind, max_pages, L, Hkv, P, hd, indptr, indices, B, mptr, src, dst, n, None)

    for kind in KINDS:
        assert move(kind) == OK and move(kind, indptr=None, indices=None, mptr=None, src=None, dst=None) == OK      # no moves
        assert move(kind, n=3, B=0, indptr=None) == OK                                                        # no sequences
        assert move(kind, data=None) == BAD
        assert move(kind, param=None) == (OK if kind == _lib.MM_KV_BF16 else BAD)
        for bad in (dict(max_pages=0), dict(L=0), dict(Hkv=0), dict(P=0), dict(hd=0), dict(L=-1), dict(P=-3), dict(n=-1), dict(B=-1)):
            assert move(kind, **bad) == BAD, bad
        for hd in (64, 127, 256):
            assert move(kind, hd=hd) == UNS and move(kind, hd=hd, n=1, data=None) == UNS
        for ptr in ("indptr", "indices", "mptr", "src", "dst"):
            assert move(kind, n=1, **{ptr: None}) == BAD, ptr
        assert move(kind, data=24) == BAD                                                                     # not 16-byte aligned
        assert move(kind, L=65536) == UNS
    assert move(_lib.MM_KV_INT4, param=18) == BAD                                                             # not 4-byte aligned
    for kind in (2, 4, -1, 255):
        assert move(kind) == BAD


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 8, 16, 64), dtype=torch.uint8)
    param = torch.zeros((4, 2, 2, 8, 16, 2), dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.kv_move_rows(data, param, i32(3), i32(4), i32(3), i32(2), i32(2))
    with pytest.raises(TypeError):
        mixedgemm.kv_move_rows(None, None, i32(3), i32(4), i32(3), i32(2), i32(2))
    q = torch.zeros((5, 32, 128), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="window or tree_mask"):                   # refused before anything is looked at
        mixedgemm.paged_prefill(q, data, param, i32(3), i32(4), i32(2), i32(3), 0, 100, window=8, tree_mask=torch.zeros((5,), dtype=torch.int64))
    c = PagedKVCache(1, 1, 4, 8, 1, kind="bf16", device="cpu", window=8)
    c.extend(3)
    mask, _ = c.tree_mask([[-1, 0, 0]])
    with pytest.raises(ValueError, match="sliding-window"):
        c.attend_new(0, torch.zeros((3, 1, 128), dtype=torch.bfloat16), tree=mask)


# ---- tree_mask -----------------------------------------------------------------------------------------------------------------------
def u64(mask):
    return [int(x) & (1 << 64) - 1 for x in mask.tolist()]


def test_tree_mask_words_and_depths_of_hand_written_trees():
    c = PagedKVCache(1, 1, 16, 32, 4, kind="bf16", device="cpu")
    c.extend([5, 5, 21, 3])
    chain, star = [-1, 0, 1, 2, 3], [-1, -1, -1, -1, -1]
    mask, depths = c.tree_mask([chain, star, TREE21, None])
    assert mask.dtype == torch.int64 and tuple(mask.shape) == (34,) and mask.device.type == "cpu"
    w = u64(mask)
    assert w[0:5] == [0b1, 0b11, 0b111, 0b1111, 0b11111] and depths[0] == [0, 1, 2, 3, 4]
    assert w[5:10] == [1, 2, 4, 8, 16] and depths[1] == [0] * 5
    t = w[10:31]
    assert t[0] == 1 and t[1:5] == [0b11, 0b101, 0b1001, 0b10001]
    assert t[5:9] == [1 << i | 0b11 for i in range(5, 9)]                          # children of node 1: itself, node 1, the root
    assert t[9:13] == [1 << i | 0b101 for i in range(9, 13)]
    assert t[20] == 1 << 20 | 0b10001
    assert depths[2] == [0] + [1] * 4 + [2] * 16
    assert w[31:34] == [1, 3, 7] and depths[3] == [0, 1, 2]                        # None: a causal chain
    assert w == [x for par in (chain, star, TREE21) for x in kto.tree_words(par)[0]] + kto.chain_words(3)
    # 64 nodes use the sign bit; a chain longer than a word is allowed and keeps all-ones words past it
    c2 = PagedKVCache(1, 1, 16, 32, 2, kind="bf16", device="cpu")
    c2.extend([64, 70])
    mask, depths = c2.tree_mask([list(range(-1, 63)), None])
    w = u64(mask)
    assert w[63] == (1 << 64) - 1 and int(mask[63]) == -1 and w[62] == (1 << 63) - 1 and depths[0][63] == 63
    assert w[64:128] == kto.chain_words(64) and w[128:] == [(1 << 64) - 1] * 6 and depths[1] == list(range(70))


def test_tree_mask_errors():
    c = PagedKVCache(1, 1, 16, 32, 2, kind="bf16", device="cpu")
    with pytest.raises(ValueError, match="nothing is announced"):
        c.tree_mask([None, None])
    c.extend([3, 65])
    for bad in ([[-1, 1, 0], None], [[-1, 0, 3], None], [[-2, 0, 0], None], [[0, 0, 0], None],       # a parent >= its index, or < -1
                [[-1, 0], None], [[-1, 0, 0, 0], None], [[-1, 0, 0]],                                # wrong lengths
                [None, [-1] * 65]):                                                                  # a tree of more than 64 nodes
        with pytest.raises(ValueError):
            c.tree_mask(bad)
    c.tree_mask([[-1, 0, 0], None])
    c.truncate(0, 1)
    with pytest.raises(ValueError, match="changed since the last extend"):
        c.tree_mask([[-1], None])


# ---- accept on a CPU cache, next to a twin that was extended by the path's tokens only ------------------------------------------------
def fill_rows(c, b, lo, ids):
    """write rows that name token ids `ids` into positions lo .. of sequence b, every (layer, K / V, head)"""
    data = c.kv_data.view(torch.uint8).numpy()
    param = None if c.kv_param is None else c.kv_param.view(torch.int16).numpy()
    P, segs = c.page_size, data.shape[1] * 2 * data.shape[3]
    for k, tid in enumerate(ids):
        page, slot = c._pages[b][(lo + k) // P], (lo + k) % P
        j, seg = np.arange(data.shape[-1]), np.arange(segs)[:, None]
        data[page, :, :, :, slot] = ((tid * 7 + 37 * seg + j) % 251).astype(np.uint8).reshape(data.shape[1], 2, data.shape[3], -1)
        if param is not None:
            param[page, :, :, :, slot] = np.stack([(tid * 31 + seg[:, 0]) & 0x7FFF, (tid + 5 * seg[:, 0]) & 0x7FFF], -1).astype(np.int16).reshape(
                data.shape[1], 2, data.shape[3], 2)


def logical_rows(c, b):
    data = c.kv_data.view(torch.uint8).numpy()
    param = None if c.kv_param is None else c.kv_param.view(torch.int16).numpy()
    pos = np.arange(c.seq_lens[b])
    pages, slot = np.asarray(c._pages[b], dtype=np.int64)[pos // c.page_size], pos % c.page_size
    return data[pages, :, :, :, slot].tobytes(), None if param is None else param[pages, :, :, :, slot].tobytes()


def bookkeeping(c):
    return repr((c._pages, c._free, c._ref, c._released, c.seq_lens, c.pages_in_use, c.num_new_tokens, c.kv_indptr.tolist(),
                 c.kv_indices.tolist()[: sum(map(len, c._pages))], c.last_page_len.tolist(), c.append_indptr.tolist()))


def canonical(c):
    """the bookkeeping with the pages' names taken out: a draft that took more pages than its path keeps makes the sequences after it
    in the batch take other pages than the twin's do, so page NUMBERS can differ while every count agrees"""
    used = {p for pages in c._pages for p in pages}
    assert sorted(c._free) == [p for p in range(c.max_pages) if p not in used] and all(c._ref[p] == 0 for p in c._free)
    groups = [[[b2 for b2 in range(c.batch) if i < len(c._pages[b2]) and c._pages[b2][i] == p] for i, p in enumerate(pages)] for pages in c._pages]
    return repr((groups, [[c._ref[p] for p in pages] for pages in c._pages], sorted(c._ref), len(c._free), c.pages_in_use, c._released, c.seq_lens,
                 c.num_new_tokens, c.kv_indptr.tolist(), c.last_page_len.tolist(), c.append_indptr.tolist()))


# (prior, fork (src, dst, length), parents, new, paths, literal).  literal: only the last sequence of the batch drafts more pages than
# it keeps, so its surplus pages go back in the order the twin never took them and even the page numbers and the free list's order agree
ACCEPT_CASES = [
    # [0, 1, 6] -> 0, 1, 2; [0, 2, 5]: slot 1 is written while slot 2 is still a source; sequence 3 shares sequence 0's first tokens
    ([6, 0, None, 3], (0, 3, 3), [TREE21, [-1, 0, 0, 1, 1, 2], None, None], [21, 6, 4, 0], [[0, 1, 6], [0, 2, 5], [0, 1], None], False),
    ([6, 0, 0], (0, 2, 3), [None, None, TREE21], [2, 0, 21], [[0, 1], None, [0, 1, 6]], True),
    # a whole draft rejected -- by a sequence that shared no partly filled page: one that did keeps the copy its extend made, which a
    # twin that announced nothing never takes (the rows agree all the same)
    ([6, 0, 0], (0, 2, 3), [None, TREE21, None], [2, 21, 1], [[0, 1], [], [0]], False),
]


@pytest.mark.parametrize("kind", ["int4", "bf16", "fp8_e4m3"])
@pytest.mark.parametrize("P", [1, 4, 16])
@pytest.mark.parametrize("case", range(len(ACCEPT_CASES)))
def test_accept_equals_a_twin_that_saw_only_the_path(kind, P, case):
    prior, (fsrc, fdst, flen), parents, new, paths, literal = ACCEPT_CASES[case]
    prior = [P + 1 if a is None else a for a in prior]
    B = len(prior)
    nxt = [1000 * b for b in range(B)]
    caches = []
    for twin in (False, True):
        c = PagedKVCache(2, 2, P, 64, B, kind=kind, device="cpu")
        c.extend(prior)
        for b in range(B):
            fill_rows(c, b, 0, [nxt[b] + i for i in range(prior[b])])
        c.fork(fsrc, fdst, flen)                             # the draft of a member of the pair: its copy-on-write comes first
        base = list(c.seq_lens)
        c.extend([len(p or []) for p in paths] if twin else new)
        for b in range(B):
            fill_rows(c, b, base[b], [nxt[b] + 100 + i for i in ((paths[b] or []) if twin else range(new[b]))])
        if not twin:
            c.tree_mask(parents)
            other = fsrc if new[fdst] else fdst
            before = logical_rows(c, other)
            c.accept(paths)
            assert logical_rows(c, other) == before, "the other member of the fork changed"
        else:
            c.extend(0)                                      # nothing announced any more, as after accept
        caches.append(c)
    ours, twin = caches
    assert canonical(ours) == canonical(twin)
    if literal:
        assert bookkeeping(ours) == bookkeeping(twin)
    for b in range(B):
        assert logical_rows(ours, b) == logical_rows(twin, b), b
    with pytest.raises(ValueError, match="changed since the last extend"):
        ours.accept([[]] * B)                                # accepted already
    ours.extend(1)                                           # and the sequences go on
    assert ours.seq_lens == [n + 1 for n in twin.seq_lens]


def test_move_list_whose_destinations_are_sources():
    """the oracle and the CPU path agree that path [1, 2, 5] reads slots 1, 2, 5 before it writes slots 0, 1, 2"""
    c = PagedKVCache(1, 1, 4, 8, 1, kind="int4", device="cpu")
    c.extend(3)
    fill_rows(c, 0, 0, [1, 2, 3])
    c.extend(6)
    fill_rows(c, 0, 3, [10, 11, 12, 13, 14, 15])
    c.tree_mask([[-1, -1, 1, 1, 1, 2]])
    data = c.kv_data.view(torch.uint8).numpy().copy()
    param = c.kv_param.view(torch.int16).numpy().copy()
    kto.move_rows(data, param, [0, 3], c._pages[0], [0, 3], [4, 5, 8], [3, 4, 5])
    c.accept([[1, 2, 5]])
    assert c.seq_lens == [6] and c._pages == [[0, 1]] and c._free[-1] == 2
    assert np.array_equal(c.kv_data.view(torch.uint8).numpy(), data) and np.array_equal(c.kv_param.view(torch.int16).numpy(), param)
    t = PagedKVCache(1, 1, 4, 8, 1, kind="int4", device="cpu")
    t.extend(6)
    fill_rows(t, 0, 0, [1, 2, 3, 11, 12, 15])
    assert logical_rows(c, 0) == logical_rows(t, 0)


def test_accept_errors():
    c = PagedKVCache(1, 1, 4, 16, 2, kind="bf16", device="cpu")
    with pytest.raises(ValueError, match="nothing to accept"):
        c.accept([[], []])
    c.extend([6, 0])
    c.tree_mask([[-1, 0, 0, 1, 1, 2], None])
    state = bookkeeping(c)
    for bad in ([[1], None],            # does not start at a root
                [[0, 3, 5], None],      # 5 is a child of 2, not of 3
                [[0, 2, 1], None],      # not ascending: 1 is no child of 2
                [[0, 6], None], [[-1], None], [[0, 0], None],
                [None, None],           # tokens announced, no path
                [[0]]):                 # one path for two sequences
        with pytest.raises(ValueError):
            c.accept(bad)
        assert bookkeeping(c) == state, bad
    c.accept([[0, 2, 5], []])
    assert c.seq_lens == [3, 0]
    # without tree_mask the announced tokens are chains: only a prefix is a path
    c.extend([4, 2])
    with pytest.raises(ValueError):
        c.accept([[0, 2], [0]])
    c.accept([[0, 1], []])
    assert c.seq_lens == [5, 0] and c.pages_in_use == 2
    # fork, truncate, reset and another extend each end the draft
    for change in (lambda: c.fork(0, 1), lambda: c.truncate(0, 5), lambda: c.reset(1), lambda: c.extend(0)):
        c.extend([2, 0])
        change()
        if c._announced is not None:                        # another extend announces its own tokens: the old paths no longer fit
            with pytest.raises(ValueError):
                c.accept([[0, 1], None])
            c.accept([[], None])
        else:
            with pytest.raises(ValueError, match="changed since the last extend"):
                c.accept([[0, 1], []])


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def test_oracle_with_a_chain_mask_is_the_causal_oracle_exactly():
    rng = np.random.default_rng(5)
    Hq, Hkv, P, L = 4, 2, 4, 2
    prior, new = [0, 9, 3, 70], [5, 7, 0, 66]               # 66 > 64: causal whatever the words say
    lens = [a + n for a, n in zip(prior, new)]
    npg = [-(-n // P) for n in lens]
    indptr = np.concatenate([[0], np.cumsum(npg)]).astype(np.int32)
    indices = rng.permutation(sum(npg) + 2)[: sum(npg)].astype(np.int32)
    last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
    qo = np.concatenate([[0], np.cumsum(new)])
    q = rng.integers(0x3C00, 0x4100, (int(qo[-1]), Hq, 128)).astype(np.uint16) | (rng.integers(0, 2, (int(qo[-1]), Hq, 128)) << 15).astype(np.uint16)
    for int4 in (False, True):
        if int4:
            data = rng.integers(0, 256, (sum(npg) + 2, L, 2, Hkv, P, 64)).astype(np.uint8)
            param = np.abs(rng.standard_normal((sum(npg) + 2, L, 2, Hkv, P, 2))).astype(np.float16)
        else:
            data = rng.integers(0x3C00, 0x4000, (sum(npg) + 2, L, 2, Hkv, P, 128)).astype(np.uint16)
            param = None
        words = kto.chain_words(5) + kto.chain_words(7) + [0x1234] * 66
        got = kto.attention(q, data, param, indptr, indices, last, qo, words, 1)
        want = kpo.attention(q, data, param, indptr, indices, last, qo, 1)
        assert np.array_equal(got, want)
        assert np.array_equal(kto.vmax(q.shape, data, param, indptr, indices, last, qo, words, 1),
                              kpo.vmax(q.shape, data, param, indptr, indices, last, qo, 1))
        # and a tree changes it: a star's leaves see the committed tokens and themselves only
        star = [1 << j for j in range(5)] + kto.chain_words(7) + [0] * 66
        o = kto.attention(q, data, param, indptr, indices, last, qo, star, 1)
        K, V = ko.dequantized(data, param, indptr, indices, last, 1, 0)
        assert np.allclose(o[:5], np.repeat(V[:, :5].transpose(1, 0, 2), Hq // Hkv, 1)), "base 0: a star's leaf returns its own V"
        assert np.array_equal(o[5:], want[5:])
        assert not kto.attention(q, data, param, indptr, indices, last, qo, [0] * 5 + words[5:], 1)[:5].any(), "word 0 at base 0: o = 0"


def test_oracle_keep_matrix_follows_the_rule():
    keep = kto.keep_matrix(10, 4, [0b0001, 0b1111, 0b0100, 0b1001])
    assert keep[:, :6].all()                                                      # the committed tokens, all of them
    assert keep[:, 6:].tolist() == [[True, False, False, False],
                                    [True, True, False, False],                   # bits above j are ignored
                                    [False, False, True, False],
                                    [True, False, False, True]]
    assert kto.keep_matrix(3, 5, [31] * 5)[:, :].tolist() == [[False] * 3, [False] * 3, [True, False, False], [True, True, False], [True] * 3]

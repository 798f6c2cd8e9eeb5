"""CPU tests of greedy draft verification: the host side of mm_argmax_rows / mm_verify_greedy (symbols, every status without device
work, Python argument errors), the numpy oracle itself (tests/kv_verify_oracle.py: its argmax against torch.argmax on the CPU, its walk
against hand-written cases) and PagedKVCache.verify on a CPU cache next to a twin that accepts the oracle's paths.  No kernel is
launched here."""
import inspect

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_verify_oracle as kvo
import test_kv_tree_cpu as t_tree

TREE21 = t_tree.TREE21
OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED


# ---- the C ABI and the Python ops ----------------------------------------------------------------------------------------------------
def test_symbols_declared_and_exported_and_the_version_stays():
    lib = _lib.load()
    header = open(inspect.getsourcefile(_lib).replace("micromix_amd/_lib.py", "include/micromix_hip.h")).read()
    for name in ("mm_argmax_rows_workspace_bytes", "mm_argmax_rows", "mm_verify_greedy"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f" {name}(" in header, name
    assert lib.mm_version() == 660
    assert f"#define MM_ARGMAX_CHUNK {_lib.MM_ARGMAX_CHUNK} " in header and _lib.MM_ARGMAX_CHUNK <= 65536
    assert f"#define MM_VERIFY_STRIDE {_lib.MM_VERIFY_STRIDE} " in header and _lib.MM_VERIFY_STRIDE == 66 == kvo.STRIDE
    assert f"#define MM_ARGMAX_MAX_ROWS {_lib.MM_ARGMAX_MAX_ROWS}" in header and _lib.MM_ARGMAX_MAX_ROWS >= 4096
    for name in ("argmax_rows", "argmax_rows_workspace_bytes", "verify_greedy"):
        assert name in mixedgemm.__all__ and callable(getattr(mixedgemm, name))
    sig = inspect.signature(mixedgemm.argmax_rows).parameters
    assert list(sig) == ["logits", "out", "workspace"] and all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("out", "workspace"))
    sig = inspect.signature(mixedgemm.verify_greedy).parameters
    assert list(sig) == ["target_tok", "draft_tok", "root_tok", "qo_indptr", "kv_indptr", "last_page_len", "page_size", "tree_mask", "result",
                         "move_src", "move_dst"]
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY and sig[n].default is None for n in ("tree_mask", "result", "move_src", "move_dst"))
    for name in ("verify_launch", "commit", "verify"):
        assert callable(getattr(PagedKVCache, name))
    assert list(inspect.signature(PagedKVCache.verify_launch).parameters) == ["self", "target_tok", "draft_tok", "root_tok"]
    import importlib.util
    spec = importlib.util.spec_from_file_location("dropin_mixedgemm", inspect.getsourcefile(_lib).replace("_lib.py", "dropin/mixedgemm.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert dropin.argmax_rows is mixedgemm.argmax_rows and dropin.verify_greedy is mixedgemm.verify_greedy


def test_argmax_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes or null"""
    lib = _lib.load()
    C = _lib.MM_ARGMAX_CHUNK

    def arg(logits=16, rows=3, vocab=100, ld=None, out=16, ws=None, ws_bytes=0):
        return lib.mm_argmax_rows(logits, rows, vocab, vocab if ld is None else ld, out, ws, ws_bytes, None)

    assert arg(rows=0) == OK and arg(rows=0, logits=None, out=None) == OK
    assert arg(logits=None) == BAD and arg(out=None) == BAD
    assert arg(rows=-1) == BAD and arg(vocab=0) == BAD and arg(vocab=-5) == BAD and arg(ld=99) == BAD
    for odd in (17, 19, 31):
        assert arg(logits=odd) == BAD, odd                                         # bf16 values lie on even addresses
    assert arg(vocab=(1 << 20) + 1) == UNS and arg(rows=_lib.MM_ARGMAX_MAX_ROWS + 1) == UNS
    # one part: no workspace; more: rows * parts partials of 8 bytes, present, large enough
    assert lib.mm_argmax_rows_workspace_bytes(3, C) == 0 and lib.mm_argmax_rows_workspace_bytes(4096, 1) == 0
    assert lib.mm_argmax_rows_workspace_bytes(3, C + 1) == 3 * 2 * 8
    assert lib.mm_argmax_rows_workspace_bytes(21, 128256) == 21 * -(-128256 // C) * 8
    assert lib.mm_argmax_rows_workspace_bytes(1, 1 << 20) == (1 << 20) // C * 8
    assert lib.mm_argmax_rows_workspace_bytes(0, C + 1) == 0 and lib.mm_argmax_rows_workspace_bytes(3, 0) == 0
    need = lib.mm_argmax_rows_workspace_bytes(3, C + 1)
    assert arg(vocab=C + 1) == BAD and arg(vocab=C + 1, ws=16) == BAD and arg(vocab=C + 1, ws=16, ws_bytes=need - 1) == BAD
    assert arg(vocab=C + 1, ws=None, ws_bytes=need) == BAD
    assert arg(vocab=C + 1, ws=20, ws_bytes=need) == BAD                           # the partials are 8-byte words
    assert arg(vocab=C + 1, rows=0) == OK


def test_verify_statuses_without_device_work():
    lib = _lib.load()

    def ver(target=16, draft=16, root=16, mask=64, qo=16, T=5, indptr=16, last=16, P=16, B=2, result=16, src=16, dst=16):
        return lib.mm_verify_greedy(target, draft, root, mask, qo, T, indptr, last, P, B, result, src, dst, None)

    assert ver(B=0) == OK and ver(B=0, target=None, draft=None, root=None, mask=None, qo=None, indptr=None, last=None, result=None,
                                  src=None, dst=None) == OK
    for ptr in ("target", "draft", "root", "qo", "indptr", "last", "result", "src", "dst"):
        assert ver(**{ptr: None}) == BAD, ptr
        assert ver(mask=None, **{ptr: None}) == BAD, ptr
    for mask in (65, 66, 68, 60):                                                  # the words are read as 64-bit loads
        assert ver(mask=mask) == BAD, mask
    assert ver(T=-1) == BAD and ver(B=-1) == BAD and ver(P=0) == BAD and ver(P=-4) == BAD
    # without tokens the per-token arrays may be absent; the per-sequence ones may not
    for ptr in ("root", "qo", "indptr", "last", "result"):
        assert ver(T=0, target=None, draft=None, src=None, dst=None, **{ptr: None}) == BAD, ptr


def test_python_argument_errors():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.argmax_rows(torch.zeros((3, 100), dtype=torch.bfloat16))
    with pytest.raises(TypeError, match="bfloat16"):
        mixedgemm.argmax_rows(torch.zeros((3, 100), dtype=torch.float32))
    with pytest.raises(TypeError):
        mixedgemm.argmax_rows(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.verify_greedy(i32(5), i32(5), i32(2), i32(3), i32(3), i32(2), 16)
    for bad in range(6):                                                           # int64 ids: told to convert them
        args = [i32(5), i32(5), i32(2), i32(3), i32(3), i32(2)]
        args[bad] = args[bad].to(torch.int64)
        with pytest.raises(TypeError, match=r"convert it with \w+\.to\(torch\.int32\)"):
            mixedgemm.verify_greedy(*args, 16)
    c = PagedKVCache(1, 1, 4, 8, 1, kind="bf16", device="cpu")
    c.extend(3)
    with pytest.raises(RuntimeError, match="device cache"):
        c.verify_launch(i32(3), i32(3), i32(1))
    with pytest.raises(RuntimeError, match="announced"):
        c.verify(i32(2), i32(3), i32(1))
    c.truncate(0, 3)
    with pytest.raises(ValueError, match="changed since the last extend"):
        c.verify(i32(3), i32(3), i32(1))
    with pytest.raises(ValueError, match="changed since the last extend"):
        c.commit(torch.zeros((1, 66), dtype=torch.int32))


# ---- the argmax oracle is torch.argmax on the CPU ------------------------------------------------------------------------------------
def bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)


def special_rows(rng, rows, vocab):
    """bf16 bits of values quantized to 16 levels, so ties are everywhere, with NaNs of both signs, +-inf and +-0 planted"""
    x = np.round(rng.standard_normal((rows, vocab)) * 2.0).clip(-8, 7).astype(np.float32)
    bits = (x.view(np.uint32) >> 16).astype(np.uint16)
    special = np.array([0x7FC0, 0xFFC0, 0x7F81, 0xFFFF, 0x7F80, 0xFF80, 0x0000, 0x8000], dtype=np.uint16)
    for r in range(rows):
        kinds = special[: [0, 8, 4, 6, 2][r % 5]] if r % 5 else special[4:]       # some rows with NaNs, some with none
        cols = rng.integers(0, vocab, size=2 * len(kinds))
        bits[r, cols] = np.tile(kinds, 2)
    return bits


def test_argmax_oracle_equals_torch_argmax_on_the_cpu():
    rng = np.random.default_rng(3)
    bits = special_rows(rng, 40, 97)
    extra = np.stack([np.full(97, 0xFF80), np.full(97, 0x3F80), np.full(97, 0x8000), np.full(97, 0xFFC0),        # all -inf, all equal, -0, -NaN
                      np.where(np.arange(97) % 2, 0x0000, 0x8000), np.where(np.arange(97) % 2, 0x7FC0, 0xFFC1),    # +-0 mixed, +-NaN mixed
                      np.where(np.arange(97) == 50, 0xFFC0, 0x7F80), np.where(np.arange(97) == 96, 0x8000, 0x8001)]).astype(np.uint16)
    bits = np.concatenate([bits, extra])
    want = torch.argmax(bf16_tensor(bits), dim=1).numpy()
    got = kvo.argmax_rows(bits)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert got[40:].tolist() == [0, 0, 0, 0, 0, 0, 50, 96]
    # the rule itself, value by value
    assert kvo.rank([0x0000])[0] == kvo.rank([0x8000])[0]
    assert kvo.rank([0x7FC0])[0] == kvo.rank([0xFFC0])[0] == kvo.rank([0x7F81])[0] == kvo.rank([0xFFFF])[0] > kvo.rank([0x7F80])[0]
    order = [0xFF80, 0xFF7F, 0xC000, 0x8001, 0x8000, 0x0001, 0x3F80, 0x7F7F, 0x7F80, 0x7FC0]
    r = kvo.rank(order)
    assert all(a < b for a, b in zip(r[:4], r[1:5])) and r[4] < r[5] and all(a < b for a, b in zip(r[5:], r[6:]))


# ---- the walk oracle on hand-written cases -------------------------------------------------------------------------------------------
def one(draft, target, root, parents, base=10, P=4):
    """one sequence of len(draft) nodes at `base`"""
    n = len(draft)
    words = None if parents is None else t_tree.kto.tree_words(parents)[0]
    pages = -(-(base + n) // P)
    last = base + n - (pages - 1) * P if pages else 0
    res, src, dst = kvo.verify(target, draft, [root], words, [0, n], [0, pages], [last], P)
    return res[0].tolist(), src.tolist(), dst.tolist()


def test_walk_oracle_on_hand_written_cases():
    pad = lambda xs: xs + [-1] * (66 - len(xs))
    # a chain of 4: the first two match, the third does not
    res, src, dst = one([5, 6, 9, 8], [6, 7, 8, 9], 5, None)
    assert res == pad([2, 7, 0, 1]) and src == [10, 11, -1, -1] and dst == [10, 11, -1, -1]
    # nothing matches: the bonus is the root token
    assert one([5, 6], [6, 7], 4, None)[0] == pad([0, 4])
    # everything matches: the bonus is the target's choice after the last node
    assert one([5, 6, 7], [6, 7, 8], 5, None)[0] == pad([3, 8, 0, 1, 2])
    # two children with the same token: the lower index wins, and the walk goes on below IT (node 1 has a matching child, node 2 does not)
    #        nodes: 0 root(5); 1, 2 children of 0, both token 6; 3 child of 1 (token 7); 4 child of 2 (token 7)
    res, src, dst = one([5, 6, 6, 7, 7], [6, 7, 9, 1, 2], 5, [-1, 0, 0, 1, 2])
    assert res == pad([3, 1, 0, 1, 3]) and src == [10, 11, 13, -1, -1] and dst == [10, 11, 12, -1, -1]
    # the same tokens, but node 1's target differs from its child: the walk stops at node 1 and never looks under node 2
    assert one([5, 6, 6, 7, 7], [6, 8, 7, 1, 2], 5, [-1, 0, 0, 1, 2])[0] == pad([2, 8, 0, 1])
    # several roots (children of the committed token): the one with the wanted token, here node 2
    res, src, dst = one([4, 5, 6, 7], [0, 0, 7, 3], 6, [-1, -1, -1, 2])
    assert res == pad([2, 3, 2, 3]) and src == [12, 13, -1, -1] and dst == [10, 11, -1, -1]
    # a matching token under the WRONG parent is not taken
    assert one([5, 6, 7], [7, 0, 0], 5, [-1, -1, 1])[0] == pad([1, 7, 0])
    # the 21-node tree: root, child 2, its third child (node 11)
    draft = list(range(100, 121))
    target = [0] * 21
    target[0], target[2], target[11] = 102, 111, 77
    res, src, dst = one(draft, target, 100, TREE21, base=7, P=16)
    assert res == pad([3, 77, 0, 2, 11]) and src[:4] == [7, 9, 18, -1] and dst[:4] == [7, 8, 9, -1]
    # bits at i and above are ignored; parents come from the highest bit below
    assert [kvo.parent_of(w, i) for w, i in ((0b1011, 3), (0b1011, 1), (0b1000, 3), (~0 & (1 << 64) - 1, 63), (1 << 63, 63), (0b110, 0))] == [1, 0, -1, 62, -1, -1]
    # keep-all: more than 64 tokens, or a negative root token; and an empty sequence of either sort
    tgt = list(range(70))
    res, src, dst = kvo.verify(tgt + [3, 4], [0] * 72, [1, -1, 9, -1], None, [0, 70, 72, 72, 72], [0, 5, 6, 6, 6], [16, 2, 0], 16)[0:3]
    assert res[0].tolist() == pad([70, 69]) and res[1].tolist() == pad([2, 4]) and res[2].tolist() == pad([0, 9]) and res[3].tolist() == pad([0, -1])
    assert (src == -1).all() and (dst == -1).all()
    assert kvo.paths_of(res, [70, 2, 0, 0]) == [list(range(70)), [0, 1], None, None]


def test_seq_lens_follow_the_page_table():
    assert kvo.seq_lens([0, 0, 1, 3, 6], [0, 4, 1, 99, ], 4)[:3] == [0, 4, 5]
    assert kvo.seq_lens([0, 3], [-2], 4) == [8] and kvo.seq_lens([0, 3], [9], 4) == [12]      # clamped, as the kernels clamp


# ---- PagedKVCache.verify on a CPU cache next to a twin that accepts the oracle's paths -------------------------------------------------
VERIFY_CASES = [
    # (prior, parents, new, draft, target, root)
    ([6, 0, 5], [TREE21, None, None], [21, 4, 0], list(range(100, 121)) + [7, 8, 9, 3], None, [100, 7, 50]),
    ([3, 9, 2], [None, [-1, 0, 0, 1, 1, 2], [-1, -1]], [3, 6, 2], [1, 2, 3, 5, 6, 6, 7, 7, 8, 4, 4], [9, 9, 9, 6, 7, 8, 0, 0, 0, 2, 3], [0, 5, 4]),
    ([1, 1, 70], [None, None, None], [66, 2, 1], [0] * 69, list(range(69)), [0, -1, 5]),       # a prompt chunk, a negative root, a miss
]


@pytest.mark.parametrize("kind", ["int4", "bf16", "fp8_e4m3"])
@pytest.mark.parametrize("case", range(len(VERIFY_CASES)))
def test_verify_on_a_cpu_cache_equals_accept_of_the_oracle_paths(kind, case):
    prior, parents, new, draft, target, root = VERIFY_CASES[case]
    if target is None:                                       # the 21-node tree: accept root, node 1, node 6; the chain: 7, 8 and not 9
        target = [0] * 25
        target[0], target[1], target[6] = 101, 106, 55
        target[21:25] = [8, 1, 1, 1]
    B, P = len(prior), 4
    caches = []
    for twin in (False, True):
        c = PagedKVCache(2, 2, P, 64, B, kind=kind, device="cpu")
        c.extend(prior)
        for b in range(B):
            t_tree.fill_rows(c, b, 0, [1000 * b + i for i in range(prior[b])])
        base = list(c.seq_lens)
        c.extend(new)
        for b in range(B):
            t_tree.fill_rows(c, b, base[b], [1000 * b + 100 + i for i in range(new[b])])
        words = None
        if any(p is not None for p in parents):
            words = [int(w) for w in c.tree_mask(parents)[0].tolist()]
        caches.append((c, words))
    (ours, words), (twin, _) = caches
    want, _, _ = kvo.verify(target, draft, root, words, ours.append_indptr.tolist(), ours.kv_indptr.tolist(), ours.last_page_len.tolist(), P)
    want_paths = kvo.paths_of(want, new)
    i32 = lambda xs: torch.tensor(xs, dtype=torch.int32)
    paths, nxt = ours.verify(i32(target), i32(draft), i32(root))
    assert paths == want_paths and nxt == want[:, 1].tolist()
    twin.accept(want_paths)
    assert t_tree.bookkeeping(ours) == t_tree.bookkeeping(twin)
    for b in range(B):
        assert t_tree.logical_rows(ours, b) == t_tree.logical_rows(twin, b), b
    assert ours.seq_lens == [prior[b] + (len(want_paths[b]) if want_paths[b] is not None else 0) for b in range(B)]
    if case == 0:
        assert paths == [[0, 1, 6], [0, 1], None] and nxt == [55, 1, 50]
    with pytest.raises(ValueError, match="changed since the last extend"):
        ours.verify(i32(target), i32(draft), i32(root))      # verified already


def test_commit_takes_a_result_and_refuses_what_accept_refuses():
    """commit is accept's validation and bookkeeping without the moves, so on a CPU cache it can be driven with the oracle's result"""
    c = PagedKVCache(1, 1, 4, 16, 2, kind="bf16", device="cpu")
    c.extend([6, 3])
    c.tree_mask([[-1, 0, 0, 1, 1, 2], None])
    row = lambda xs: xs + [-1] * (66 - len(xs))
    state = t_tree.bookkeeping(c)
    for bad in ([row([2, 9, 0, 3]), row([1, 4, 0])],         # 3 is a child of 1, not of 0
                [row([6, 9]), row([0, 4])],                  # a tree that kept all: 0, 1, 2, .. is no path of it
                [row([1, 9, 7]), row([0, 4])]):              # not a token of the sequence
        with pytest.raises(ValueError, match="commit"):
            c.commit(torch.tensor(bad, dtype=torch.int32))
        assert t_tree.bookkeeping(c) == state
    paths, nxt = c.commit(torch.tensor([row([2, 9, 0, 2]), row([3, 4])], dtype=torch.int32))      # the chain kept all
    assert paths == [[0, 2], [0, 1, 2]] and nxt == [9, 4] and c.seq_lens == [2, 3]


def test_accept_still_works_through_the_shared_part():
    c = PagedKVCache(1, 1, 4, 16, 1, kind="int4", device="cpu")
    c.extend(6)
    c.tree_mask([[-1, -1, 1, 1, 1, 2]])
    with pytest.raises(ValueError, match="accept: token 5 of sequence 0 does not continue the path"):
        c.accept([[1, 5]])
    c.accept([[1, 2, 5]])
    assert c.seq_lens == [3]

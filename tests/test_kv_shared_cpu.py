"""PagedKVCache.share_groups() -- the grouping attend(shared=True) hands to mm_paged_decode_shared -- on a CPU cache: host bookkeeping
only, no kernel.  The rule (micromix_amd/kvcache.py): sequences in index order; a sequence joins the first group whose leader lists the
same real page in entry 0; a group shares page_size * (leading entries on which all members agree), capped at its shortest member."""
import inspect

import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_shared_oracle as so

P = 4


def cache(batch, page_size=P, max_pages=256, **kw):
    return PagedKVCache(1, 1, page_size, max_pages, batch, kind="bf16", device="cpu", **kw)


def uploaded(c):
    """the three device tensors, as (groups, shared) again: what _upload wrote must be what share_groups() says"""
    ptr, mem, sh = c.group_indptr.tolist(), c.group_members.tolist(), c.shared_len.tolist()
    assert len(ptr) == c.batch + 1 and len(mem) == len(sh) == c.batch and ptr[0] == 0 and ptr[-1] == c.batch
    groups = [mem[a:b] for a, b in zip(ptr, ptr[1:]) if b > a]
    assert ptr == sorted(ptr) and all(x == c.batch for x in ptr[len(groups):]), "the unused trailing groups are empty"
    return groups, sh


def check(c, groups, shared):
    assert c.share_groups() == (groups, shared)
    assert uploaded(c) == (groups, shared)
    assert c._max_shared == max(shared) and c._max_suffix == max(n - s for n, s in zip(c.seq_lens, shared))


def test_n_forks_of_one_prompt_before_and_after_a_copying_extend():
    c = cache(5)
    c.extend([10, 0, 0, 0, 0])
    check(c, [[0], [1], [2], [3], [4]], [0] * 5)
    for dst in (1, 2, 3):
        c.fork(0, dst)
    check(c, [[0, 1, 2, 3], [4]], [10, 10, 10, 10, 0])          # the partly filled third page is shared too
    c.extend([1, 1, 1, 1, 0])                                   # three copies: the shared count falls to the last page edge
    assert len({c._pages[b][2] for b in range(4)}) == 4
    check(c, [[0, 1, 2, 3], [4]], [8, 8, 8, 8, 0])
    c.extend([0, 0, 7, 0, 3])
    check(c, [[0, 1, 2, 3], [4]], [8, 8, 8, 8, 0])


def test_fork_in_the_middle_of_a_page():
    c = cache(3)
    c.extend([14, 0, 0])
    c.fork(0, 1, length=6)
    check(c, [[0, 1], [2]], [6, 6, 0])                          # capped at the shorter member, not a multiple of the page size
    c.fork(0, 2, length=9)
    check(c, [[0, 1, 2]], [6, 6, 6])
    c.extend([0, 1, 0])                                         # sequence 1 takes its own copy of page 1
    check(c, [[0, 1, 2]], [4, 4, 4])


def test_truncate_and_reset_of_the_leader():
    c = cache(3)
    c.extend([12, 0, 0])
    c.fork(0, 1)
    c.fork(0, 2)
    c.truncate(0, 5)
    check(c, [[0, 1, 2]], [5, 5, 5])
    c.truncate(0, 0)                                            # an empty leader leads nobody; 1 leads 2
    check(c, [[0], [1, 2]], [0, 12, 12])
    c.extend([3, 0, 0])
    c.reset(1)
    check(c, [[0], [1], [2]], [0, 0, 0])


def test_two_level_beam_tree_gets_the_depth_common_to_the_whole_group():
    c = cache(4)
    c.extend([8, 0, 0, 0])
    c.fork(0, 1)
    c.extend([8, 8, 0, 0])                                      # 0 and 1 diverge after 8 tokens
    c.fork(0, 2)                                                # 2 shares 16 with 0, 8 with 1
    c.fork(1, 3)
    check(c, [[0, 1, 2, 3]], [8, 8, 8, 8])


def test_nothing_shared_and_an_empty_sequence():
    c = cache(4)
    c.extend([5, 0, 9, 1])
    check(c, [[0], [1], [2], [3]], [0, 0, 0, 0])
    assert c._max_suffix == 9
    e = cache(2)
    check(e, [[0], [1]], [0, 0])


def test_window_cache_refuses_the_shared_path():
    c = cache(2, window=8)
    c.extend([3, 3])
    with pytest.raises(ValueError, match="window"):
        c.attend(0, None, shared=True)
    assert c.share_groups() == ([[0], [1]], [0, 0])             # the bookkeeping itself still answers


def test_random_operations_next_to_a_token_list_model():
    rng = np.random.default_rng(2024)
    B = 6
    c = cache(B, max_pages=400)
    tokens, fresh = [[] for _ in range(B)], 0                   # the model: what each sequence holds, every token a number of its own
    for step in range(1000):
        op = rng.integers(0, 10)
        if op < 4:
            new = [int(rng.integers(0, 4)) if rng.integers(0, 2) else 0 for _ in range(B)]
            new = [n if len(tokens[b]) + n <= 40 else 0 for b, n in enumerate(new)]
            c.extend(new)
            for b, n in enumerate(new):
                tokens[b] += list(range(fresh, fresh + n))
                fresh += n
        elif op < 7:
            src, dst = (int(x) for x in rng.choice(B, 2, replace=False))
            whole = not rng.integers(0, 3)
            length = len(tokens[src]) if whole else int(rng.integers(0, len(tokens[src]) + 1))
            c.fork(src, dst, None if whole else length)
            tokens[dst] = list(tokens[src][:length])
        elif op < 9:
            b = int(rng.integers(0, B))
            length = int(rng.integers(0, len(tokens[b]) + 1))
            c.truncate(b, length)
            del tokens[b][length:]
        else:
            b = int(rng.integers(0, B))
            c.reset(b)
            tokens[b] = []
        assert c.seq_lens == [len(t) for t in tokens]
        groups, shared = c.share_groups()
        assert uploaded(c) == (groups, shared), step
        assert sorted(b for grp in groups for b in grp) == list(range(B)), "group_members is a permutation"
        for grp in groups:
            n = shared[grp[0]]
            for b in grp:
                assert shared[b] == n <= c.seq_lens[b], (step, grp, shared)
                assert c._pages[b][: -(-n // P)] == c._pages[grp[0]][: -(-n // P)], (step, grp, "pages over the shared count")
                assert tokens[b][:n] == tokens[grp[0]][:n], (step, grp, "the shared tokens are the same tokens")
            if len(grp) == 1:
                assert n == 0
        assert c._max_shared == max(shared) and c._max_suffix == max(len(t) - s for t, s in zip(tokens, shared))


def test_gpu_cases_cover_every_shared_count_and_slab_filling():
    """the hand-built groups of tests/test_kv_shared_gpu.py, which no GPU is needed to enumerate: in every case each shared count once,
    a group of one, full slabs, a partly filled last slab, tails that differ within a slab, and the tables mm_paged_decode_shared expects"""
    for g in (1, 3, 4, 8, 16):
        per = 16 // g
        for P in (1, 5, 16):
            groups = so.random_groups(g, 1000 * g + 10 * P + 4)
            assert sorted(s for s, _ in groups[:-1]) == sorted(so.SHARED_COUNTS) and groups[-1] == (0, [0])
            assert sorted({len(t) for _, t in groups}) == sorted(set(so.group_sizes(g)))
            assert all(len(set(t[:per])) == min(len(t), per, 4) for _, t in groups)
            lay = so.layout(P, groups, 1)
            B = lay["B"]
            assert sorted(lay["group_members"].tolist()) == list(range(B)) and lay["group_members"].tolist() != list(range(B))
            assert lay["group_indptr"].shape == (B + 1,) and lay["group_indptr"][len(groups)] == B == lay["group_indptr"][-1]
            for (s, tails), a, b in zip(groups, lay["group_indptr"], lay["group_indptr"][1:]):
                mem = lay["group_members"][a:b]
                assert [lay["lens"][m] - s for m in mem] == tails and all(lay["shared_len"][m] == s for m in mem)
                assert all(lay["pages"][m][: -(-s // P)] == lay["pages"][mem[0]][: -(-s // P)] for m in mem)
            own = [p for pages, s in zip(lay["pages"], lay["shared_len"]) for p in pages[-(-int(s) // P):]]
            assert len(own) == len(set(own)) and 0 not in lay["kv_indices"], "tails on pages of their own; page 0 is nobody's"


# ---- the C ABI and the Python op: no device work ---------------------------------------------------------------------------------------
def test_symbols_declared_and_exported_and_the_version_stays():
    lib = _lib.load()
    header = open(inspect.getsourcefile(_lib).replace("micromix_amd/_lib.py", "include/micromix_hip.h")).read()
    for name in ("mm_paged_decode_shared", "mm_paged_decode_shared_workspace_bytes"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f" {name}(" in header
    assert lib.mm_version() == 660
    assert "paged_decode_shared" in mixedgemm.__all__ and "paged_decode_shared_workspace_bytes" in mixedgemm.__all__
    assert list(inspect.signature(mixedgemm.paged_decode_shared).parameters) == [
        "q", "kv_data", "kv_param", "kv_indptr", "kv_indices", "last_page_len", "layer_idx", "group_indptr", "group_members", "shared_len",
        "max_shared_len", "max_suffix_len", "sm_scale", "workspace", "out"]
    assert list(inspect.signature(PagedKVCache.attend).parameters) == ["self", "layer", "q", "max_seq_len", "sm_scale", "shared", "max_shared_len"]
    assert inspect.signature(PagedKVCache.attend).parameters["shared"].default is False


def chunks(work, bound):
    """kv_chunks of micromix_amd/csrc/mx_kernels.h in plain words: enough chunks to give 512 workgroups, of at least 256 tokens each
    (counted as ceil(bound / 256) chunks at most), the chunk length a multiple of 128"""
    n = max(1, min(-(-512 // work), (bound + 255) // 256))
    length = max(128, -(-(-(-bound // n)) // 128) * 128)
    return -(-bound // length) if bound else 1


def test_workspace_size_follows_the_host_arguments_alone():
    ws = _lib.load().mm_paged_decode_shared_workspace_bytes
    part = (128 + 2) * 4                                        # (o[128], m, l) fp32 of one (sequence, query head, chunk)
    for B, Hq, Hkv in ((1, 8, 2), (8, 32, 8), (64, 32, 8), (5, 4, 1), (3, 32, 2), (7, 6, 2), (67, 2, 2)):
        per = 16 // (Hq // Hkv)
        for shared in (0, 1, 255, 256, 257, 1024, 4096, 1 << 29):
            for tail in (0, 1, 255, 256, 257, 1024, 1 << 29):
                want = B * Hq * (chunks(-(-B // per) * Hkv, shared) + chunks(B * Hkv, tail)) * part
                assert ws(B, Hq, Hkv, shared, tail) == want, (B, Hq, Hkv, shared, tail)
    assert ws(1, 8, 2, 256, 256) == 8 * 2 * part and ws(1, 8, 2, 257, 0) == 8 * 3 * part     # one chunk each; 257 tokens are two
    assert ws(8, 32, 8, 4096, 64) == 8 * 32 * (16 + 1) * part   # 2 slabs x 8 kv heads: every 256 tokens of the prompt a chunk
    assert ws(64, 32, 8, 4096, 64) == 64 * 32 * (4 + 1) * part  # 16 slabs x 8: four chunks reach 512 workgroups
    for bad in ((0, 8, 2, 10, 10), (-1, 8, 2, 10, 10), (65536, 8, 2, 10, 10), (1, 8, 3, 10, 10), (1, 0, 2, 10, 10), (1, 8, 0, 10, 10),
                (1, 8, 2, -1, 10), (1, 8, 2, 10, -1), (1, 8, 2, (1 << 29) + 1, 10), (1, 8, 2, 10, 2 ** 31 - 1), (1, 34, 2, 10, 10)):
        assert ws(*bad) == 0, bad


def test_statuses_without_device_work():
    """every row returns before a launch: the addresses are fakes (16) or null"""
    lib = _lib.load()
    OK, BAD, UNS = _lib.MM_OK, _lib.MM_ERR_BAD_ARG, _lib.MM_ERR_UNSUPPORTED
    need = lib.mm_paged_decode_shared_workspace_bytes(3, 8, 2, 100, 100)

    def call(q=16, data=16, param=16, kind=0, max_pages=4, L=2, layer=1, Hkv=2, P=16, hd=128, indptr=16, indices=16, last=16, B=3, Hq=8,
             gi=16, gm=16, sl=16, ms=100, mt=100, ws=None, ws_bytes=None, o=16):
        return lib.mm_paged_decode_shared(q, data, param, kind, max_pages, L, layer, Hkv, P, hd, indptr, indices, last, B, Hq, gi, gm, sl, ms,
                                          mt, 1.0, ws, need if ws_bytes is None else ws_bytes, o, None)

    assert call(B=0) == OK and call(B=0, q=None, gi=None, ws=None) == OK              # nothing to do
    for null in ("q", "data", "param", "indptr", "indices", "last", "gi", "gm", "sl", "o"):
        assert call(ws=16, **{null: None}) == BAD, null
    assert call(ws=16, kind=_lib.MM_KV_BF16, param=None, q=None) == BAD                # bf16 needs no params; the null q is the backstop
    assert call(ws=None) == BAD and call(ws=16, ws_bytes=need - 1) == BAD and call(ws=24) == BAD and call(ws=16, ws_bytes=0) == BAD
    for bad in (dict(Hq=0), dict(Hq=7), dict(ms=-1), dict(mt=-1), dict(ms=(1 << 29) + 1), dict(mt=2 ** 31 - 1), dict(B=-1), dict(layer=2),
                dict(P=0), dict(kind=2), dict(max_pages=0)):
        assert call(ws=16, **bad) == BAD, bad
    assert call(ws=16, hd=64) == UNS and call(ws=16, Hq=34) == UNS and call(Hq=34, q=None) == UNS


def test_python_argument_errors_without_a_device():
    i32 = lambda n: torch.zeros((n,), dtype=torch.int32)
    data = torch.zeros((4, 2, 2, 2, 16, 128), dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mixedgemm.paged_decode_shared(torch.zeros((3, 8, 128), dtype=torch.bfloat16), data, None, i32(4), i32(4), i32(3), 1, i32(4), i32(3), i32(3), 10, 10)

"""GPU tests of greedy draft verification (mixedgemm.argmax_rows, mixedgemm.verify_greedy, PagedKVCache.verify_launch / commit / verify).
Every comparison is exact equality; the references are tests/kv_verify_oracle.py and a twin cache that runs accept(oracle paths).

1 places  each row's maximum at a chosen column with an equal value planted at a later one (the earlier must win): every column of the
          first and last 300, +-9 around every multiple of MM_ARGMAX_CHUNK, +-1 around every multiple of 2 048; vocab = 2 CHUNK + 5 with
          ld = vocab + 3 (and ld = vocab + 4, odd, so that every row alignment occurs in one call), vocab in {1, 7, 8, 9, 255, 257,
          CHUNK +- 1} with ld == vocab; all of them at pointer offsets of 0 .. 7 elements.  Everything outside the rows is NaN: a read
          past a row's end or in front of its start wins the row
2 values  logits quantized to 16 levels (ties everywhere) with NaNs of both signs, +-inf, +-0, a row of -inf and an all-equal row,
          against the oracle, the workspace filled with NaNs; one row at vocab 32 000, 128 256 and 152 064, maximum first and last
3 verify  random trees over tokens {0, 1, 2} against the oracle: n_b in {0, 1, 2, 21, 63, 64, 65, 70} and a sequence with a negative
          root token; tree words, the same with garbage in bits j and above, and no words (chains); page sizes 1, 16, 24, bases on
          and off a page edge; result, move_src, move_dst compared whole over outputs that were poisoned first
4 class   extend a tree / append_rope / attend_new(tree=) / argmax_rows / verify next to a twin that runs accept(oracle path): paths of
          length 0, 3 and the full depth; cache bytes, tables, seq_lens and the next decode step equal; the fork's other member
          untouched; a chain on a window= cache
5 graph   argmax_rows -> verify_launch captured once, replayed with two trees and logits of the same T, commit after each

No bound here comes from what a kernel produced."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_exact_cases as kc
import kv_tree_oracle as kto
import kv_verify_oracle as kvo
import test_kv_tree_gpu as t_tree
import test_kv_verify_cpu as t_cpu

pytestmark = pytest.mark.gpu

KINDS = ["int4", "bf16", "fp8_e4m3"]
C = _lib.MM_ARGMAX_CHUNK
U64 = (1 << 64) - 1
NAN = float("nan")
i32 = t_tree.i32


# ---- 1. argmax: places -----------------------------------------------------------------------------------------------------------------
def chosen_columns(vocab):
    cols = set(range(min(300, vocab))) | set(range(max(0, vocab - 300), vocab))
    for m in range(0, vocab + 10, C):
        cols |= set(range(m - 9, m + 10))
    for m in range(0, vocab + 2, 2048):
        cols |= {m - 1, m, m + 1}
    return sorted(c for c in cols if 0 <= c < vocab)


def planted(dev, vocab, ld, offset, cols):
    """a [rows, vocab] view, row stride ld, `offset` elements into a NaN-filled buffer: -1 everywhere, 3 at cols[r] and at one later column"""
    rows = len(cols)
    buf = torch.full((offset + rows * ld + 16,), NAN, dtype=torch.bfloat16, device=dev)
    view = buf[offset: offset + rows * ld].view(rows, ld)[:, :vocab]
    view.fill_(-1.0)
    r = torch.arange(rows, device=dev)
    at = torch.tensor(cols, dtype=torch.int64, device=dev)
    room = vocab - 1 - at                                    # columns behind the chosen one
    later = at + torch.where(room > 0, 1 + (r * 7919) % room.clamp(min=1), torch.zeros_like(at))
    view[r, later] = 3.0
    view[r, at] = 3.0
    assert view.data_ptr() % 16 == (buf.data_ptr() + 2 * offset) % 16 and (view.stride(0) == ld or rows == 1)
    return view


def check_places(dev, vocab, ld, offset):
    cols = chosen_columns(vocab) if vocab > 1 else [0] * 9
    view = planted(dev, vocab, ld, offset, cols)
    ws = None
    need = mixedgemm.argmax_rows_workspace_bytes(len(cols), vocab)
    assert (need == 0) == (vocab <= C)
    if need:
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    got = mixedgemm.argmax_rows(view, workspace=ws)
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(cols),)
    got = got.cpu().numpy()
    bad = np.flatnonzero(got != np.array(cols))
    assert not len(bad), (f"vocab {vocab} ld {ld} offset {offset}: {len(bad)} of {len(cols)} rows wrong, first row {bad[0]}: "
                          f"got {got[bad[0]]}, want {cols[bad[0]]}")


@pytest.mark.parametrize("offset", range(8))
def test_argmax_finds_every_chosen_column(dev, offset):
    vocab = 2 * C + 5
    assert len(chosen_columns(vocab)) * (vocab + 4) * 2 <= 256 << 20
    check_places(dev, vocab, vocab + 3, offset)
    check_places(dev, vocab, vocab + 4, offset)              # an odd row distance: the rows of one call start at every alignment
    for small in (1, 7, 8, 9, 255, 257, C - 1, C + 1):
        check_places(dev, small, small, offset)


# ---- 2. argmax: values -----------------------------------------------------------------------------------------------------------------
def run_argmax(dev, bits, ld=None, poison_ws=True):
    rows, vocab = bits.shape
    ld = vocab if ld is None else ld
    full = np.full((rows, ld), 0x7FC0, dtype=np.uint16)
    full[:, :vocab] = bits
    t = torch.from_numpy(full.view(np.int16)).to(dev).view(torch.bfloat16)[:, :vocab]
    need = mixedgemm.argmax_rows_workspace_bytes(rows, vocab)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev) if need and poison_ws else None
    out = mixedgemm.argmax_rows(t, workspace=ws)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("vocab, ld", [(2 * C + 5, 2 * C + 9), (C, C), (1000, 1001), (3 * C, 3 * C)])
def test_argmax_values_against_the_oracle(dev, vocab, ld):
    rng = np.random.default_rng(vocab)
    bits = t_cpu.special_rows(rng, 45, vocab)
    col = np.arange(vocab)
    extra = np.stack([np.full(vocab, 0xFF80), np.full(vocab, 0x3F80), np.full(vocab, 0x8000), np.full(vocab, 0xFFC0),
                      np.where(col % 2, 0x0000, 0x8000), np.where(col % 2, 0x7FC0, 0xFFC1),
                      np.where(col == vocab - 1, 0xFFC0, 0x7F80), np.where(col == vocab - 1, 0x8000, 0x8001),
                      np.where(col == vocab - 1, 0xFF80 + 1, 0xFF80)]).astype(np.uint16)      # -inf but for a -NaN in the last column
    bits = np.concatenate([bits, extra])
    want = kvo.argmax_rows(bits)
    assert want[45:].tolist() == [0, 0, 0, 0, 0, 0, vocab - 1, vocab - 1, vocab - 1]
    got = run_argmax(dev, bits, ld)
    assert np.array_equal(got, want), f"rows {np.flatnonzero(got != want)[:8]}: got {got[got != want][:8]}, want {want[got != want][:8]}"
    assert np.array_equal(run_argmax(dev, bits, ld, poison_ws=False), want)                # the op's own workspace


@pytest.mark.parametrize("vocab", [32000, 128256, 152064])
def test_argmax_of_one_long_row(dev, vocab):
    rng = np.random.default_rng(vocab)
    for where in (0, vocab - 1):
        bits = t_cpu.special_rows(rng, 1, vocab)             # row 0: no NaN; +inf somewhere in it
        bits[bits == 0x7F80] = 0x4000
        bits[0, where] = 0x7F80
        assert kvo.argmax_rows(bits)[0] == where
        assert run_argmax(dev, bits)[0] == where
        bits[0, where] = 0x40E0                              # 7, a tie with the 16-level values: the oracle says which one
        assert run_argmax(dev, bits)[0] == kvo.argmax_rows(bits)[0]


# ---- 3. verify against the oracle ----------------------------------------------------------------------------------------------------------
COUNTS = [21, 0, 1, 2, 63, 64, 65, 70, 21]                   # the last one gets a negative root token


@pytest.mark.parametrize("P", [1, 16, 24])
@pytest.mark.parametrize("mode", ["words", "garbage", "chains"])
def test_verify_greedy_against_the_oracle(dev, P, mode):
    B, T = len(COUNTS), sum(COUNTS)
    qo = kc.indptr_of(COUNTS)
    for seed in range(6):
        rng = np.random.default_rng(100 * P + seed)
        # bases on a page edge (a multiple of P, 0 included) and off it
        base = [int(rng.integers(0, 5)) * P + (int(rng.integers(1, P)) if P > 1 and b % 2 else 0) for b in range(B)]
        lens = [a + n for a, n in zip(base, COUNTS)]
        npg = [-(-n // P) for n in lens]
        kv_indptr = kc.indptr_of(npg)
        last = np.array([n - (k - 1) * P if k else 0 for n, k in zip(lens, npg)], dtype=np.int32)
        draft, target = rng.integers(0, 3, T), rng.integers(0, 3, T)
        root = rng.integers(0, 3, B)
        root[-1] = -1 - int(rng.integers(0, 5))
        words = None
        if mode != "chains":
            words = []
            for n in COUNTS:
                if n <= 64:                                  # parents biased towards -1 and low nodes: siblings with equal tokens are common
                    words += kto.tree_words([int(rng.integers(-1, max(0, min(i, 1 + i // 3)))) if i else -1 for i in range(n)])[0]
                else:
                    words += [int(x) for x in rng.integers(0, 1 << 62, n)]
            if mode == "garbage":                            # bits j and above of node j's word, its own bit included, are random
                at = [j for n in COUNTS for j in range(n)]
                words = [w if j >= 64 else w & ((1 << j) - 1) | (int(rng.integers(0, 1 << 62)) << j) & U64 for w, j in zip(words, at)]
        want = kvo.verify(target, draft, root, words, qo, kv_indptr, last, P)
        if mode == "garbage":                                # precondition of the case: the bits at j and above change nothing
            clean = [w & ((1 << j) - 1) if j < 64 else w for w, j in zip(words, at)]
            assert all(np.array_equal(a, b) for a, b in zip(want, kvo.verify(target, draft, root, clean, qo, kv_indptr, last, P)))
        outs = [torch.full(shape, 12345, dtype=torch.int32, device=dev) for shape in ((B, 66), (T,), (T,))]
        mask = None if words is None else t_tree.words_tensor(words, dev)
        got = mixedgemm.verify_greedy(i32(target, dev), i32(draft, dev), i32(root, dev), i32(qo, dev), i32(kv_indptr, dev), i32(last, dev), P,
                                      tree_mask=mask, result=outs[0], move_src=outs[1], move_dst=outs[2])
        torch.cuda.synchronize()
        assert all(g is o for g, o in zip(got, outs))
        for name, g, w in zip(("result", "move_src", "move_dst"), got, want):
            g = g.cpu().numpy()
            assert np.array_equal(g, w), f"P={P} {mode} seed {seed}: {name} differs at {np.argwhere(g != w)[:4].tolist()}"
        k = want[0][:, 0]
        assert k[1] == 0 and k[6] == 65 and k[7] == 70 and k[8] == 21 and (want[0][8, 2:] == -1).all()
    fresh = mixedgemm.verify_greedy(i32(target, dev), i32(draft, dev), i32(root, dev), i32(qo, dev), i32(kv_indptr, dev), i32(last, dev), P,
                                    tree_mask=mask)          # the op's own outputs
    torch.cuda.synchronize()
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(fresh, want))


def test_verify_greedy_paths_are_long_enough_to_mean_something():
    """the random cases above must reach paths of several nodes, or a walk that stops after one step would pass them (host only)"""
    rng = np.random.default_rng(1)
    most = 0
    for _ in range(6):
        words = kto.tree_words([int(rng.integers(-1, max(0, min(i, 1 + i // 3)))) if i else -1 for i in range(63)])[0]
        res = kvo.verify(rng.integers(0, 3, 63), rng.integers(0, 3, 63), [1], words, [0, 63], [0, 63], [1], 1)[0]
        most = max(most, int(res[0, 0]))
    assert most >= 3


# ---- 4. the class, end to end ------------------------------------------------------------------------------------------------------------
# 21 nodes: node 0 the root, nodes 2 k - 1 and 2 k children of node 2 (k - 1): a spine 0, 2, 4, .. 20 of depth 11 with a leaf beside each node
SPINE = [-1] + [2 * ((i - 1) // 2) for i in range(1, 21)]
V = C + 40                                                   # two parts: the class test goes through the finishing launch too


def draft_step(rng, counts, paths, dev, bonus=7):
    """(draft_tok, root_tok, logits) in which sequence b's walk takes paths[b] (checked against the oracle by the caller): node i of every
    sequence holds token 100 + i, the row of a path's node carries 60 in the column of the next node's token, its last row in `bonus`"""
    T = sum(counts)
    draft = np.concatenate([100 + np.arange(n) for n in counts]).astype(np.int32) if T else np.zeros(0, np.int32)
    logits = rng.standard_normal((T, V)).astype(np.float32)
    root, q0 = [], 0
    for n, path in zip(counts, paths):
        path = path or []
        root.append(100 + path[0] if path else 5)
        for i, p in enumerate(path):
            logits[q0 + p, 100 + path[i + 1] if i + 1 < len(path) else bonus] = 60.0
        q0 += n
    return i32(draft, dev), i32(root, dev), t_tree.bf(logits, dev)


def whole_cache(c):
    return (c.kv_data.cpu().view(torch.uint8), None if c.kv_param is None else c.kv_param.cpu().view(torch.int16), c.kv_indptr.cpu(),
            c.kv_indices.cpu(), c.last_page_len.cpu(), c.append_indptr.cpu(), c.group_indptr.cpu(), c.group_members.cpu(), c.shared_len.cpu())


def same_cache(a, b, what):
    assert a.seq_lens == b.seq_lens and a._pages == b._pages and a._ref == b._ref and a._free == b._free, what
    for i, (x, y) in enumerate(zip(whole_cache(a), whole_cache(b))):
        assert (x is None and y is None) or torch.equal(x, y), f"{what}: cache tensor {i} differs"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("path", [[], [0, 2, 4], list(range(0, 21, 2))], ids=["none", "three", "full"])
def test_verify_equals_a_twin_that_accepts_the_oracle_path(dev, kind, path):
    """sequence 2 is a fork of sequence 0 (20 tokens, P = 16: a partly filled shared page) and verifies the 21-node tree, sequence 1 a
    chain of 3 of which 2 match, sequence 0 announces nothing"""
    Hq, Hkv, P, B, Lyr = 8, 2, 16, 3, 2
    rng = np.random.default_rng(80)
    rnd = lambda n, h: t_tree.bf(rng.standard_normal((n, h, 128)), dev)
    new, parents, paths = [0, 3, 21], [None, None, SPINE], [None, [0, 1], path]
    prompt = [rnd(27, h) for h in (Hq, Hkv, Hkv)]
    draft_rows = [rnd(24, h) for h in (Hq, Hkv, Hkv)]
    step = [rnd(3, h) for h in (Hq, Hkv, Hkv)]
    draft, root, logits = draft_step(rng, new, paths, dev)
    outs = []
    for twin in (False, True):
        c = PagedKVCache(Lyr, Hkv, P, 32, B, kind=kind, device=dev)
        c.extend([20, 7, 0])
        cos, sin = t_tree.rope_rows(list(range(20)) + list(range(7)), dev)
        for layer in range(Lyr):
            c.append_rope(layer, *prompt, cos, sin)
        c.fork(0, 2)
        base = list(c.seq_lens)
        c.extend(new)
        before = t_tree.logical_rows(c, 0)
        mask, depths = c.tree_mask(parents)
        cos, sin = t_tree.rope_rows([base[b] + d for b in range(B) for d in depths[b]], dev)
        for layer in range(Lyr):
            c.attend_new(layer, c.append_rope(layer, *draft_rows, cos, sin), tree=mask)
        if twin:
            target = kvo.argmax_rows(t_tree.bits(logits))
            want = kvo.verify(target, draft.cpu().numpy(), root.cpu().numpy(), [int(w) for w in mask.tolist()], c.append_indptr.cpu().numpy(),
                              c.kv_indptr.cpu().numpy(), c.last_page_len.cpu().numpy(), P)[0]
            assert kvo.paths_of(want, new) == paths, "precondition: the logits must make the chosen path win"
            assert want[:, 1].tolist() == [5, 7, 7 if path else 5]
            c.accept(paths)
            got = (paths, want[:, 1].tolist())
        else:
            got = c.verify(mixedgemm.argmax_rows(logits), draft, root)
            assert c._announced is None
        after = t_tree.logical_rows(c, 0)
        assert torch.equal(before[0], after[0]) and (before[1] is None or torch.equal(before[1], after[1])), "the fork's other member changed"
        snapshot = [t if t is None else t.clone() for t in whole_cache(c)]
        c.extend(1)
        for layer in range(Lyr):
            c.append(layer, step[1], step[2])
        outs.append((c, got, snapshot, [c.attend(layer, step[0]) for layer in range(Lyr)]))
    torch.cuda.synchronize()
    (ours, got, snap, o_ours), (twin, want, snap_twin, o_twin) = outs
    assert got == want and got[0] == paths
    assert ours.seq_lens == twin.seq_lens == [21, 10, 21 + len(path)]
    for i, (x, y) in enumerate(zip(snap, snap_twin)):
        assert (x is None and y is None) or torch.equal(x, y), f"after verify: cache tensor {i} differs from the twin's after accept"
    same_cache(ours, twin, "after the next step")
    for layer in range(Lyr):
        t_tree.same_bits(o_ours[layer], o_twin[layer], f"{kind} layer {layer}")


@pytest.mark.parametrize("kind", KINDS)
def test_verify_a_chain_on_a_windowed_cache(dev, kind):
    Hkv, P, B = 2, 4, 2
    rng = np.random.default_rng(81)
    rnd = lambda n: t_tree.bf(rng.standard_normal((n, Hkv, 128)), dev)
    rows = [rnd(30), rnd(30), rnd(9), rnd(9)]
    # at least one node each: a window cache that releases pages cannot go back below what its extend let go (accept refuses it)
    new, paths = [5, 4], [[0, 1, 2], [0]]
    draft, root, logits = draft_step(rng, new, paths, dev)
    caches = []
    for twin in (False, True):
        c = PagedKVCache(1, Hkv, P, 32, B, kind=kind, device=dev, window=8)
        c.extend([19, 11])
        c.append(0, rows[0], rows[1])
        c.extend(new)
        c.append(0, rows[2], rows[3])
        if twin:
            c.accept(paths)
        else:
            assert c.verify(mixedgemm.argmax_rows(logits), draft, root) == (paths, [7, 7])
        caches.append(c)
    torch.cuda.synchronize()
    same_cache(*caches, "window")
    assert caches[0].seq_lens == [22, 12]
    c = PagedKVCache(1, Hkv, P, 32, 1, kind=kind, device=dev, window=8)
    c.extend(3)
    c.tree_mask([[-1, 0, 0]])
    with pytest.raises(ValueError, match="sliding-window"):
        c.verify_launch(i32([0] * 3, dev), i32([0] * 3, dev), i32([0], dev))


# ---- 5. one graph, two trees -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_graph_of_argmax_and_verify_replays_with_another_tree(dev, kind):
    B, Hkv, n = 2, 2, 12
    rng = np.random.default_rng(90)
    rnd = lambda m: t_tree.bf(rng.standard_normal((m, Hkv, 128)), dev)
    trees = [[[-1, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 7], None], [[-1, -1, 0, 1, 2, 2, 4, 5, 5, 8, 8, 10], [-1] + [0] * 11]]
    chosen = [[[0, 2, 5], [0, 1, 2, 3]], [[1, 3], [0, 7]]]
    prior = [rnd(79), rnd(79)]
    steps = [(rnd(B * n), rnd(B * n)) for _ in trees]
    ours, twin = (PagedKVCache(1, Hkv, 16, 64, B, kind=kind, device=dev) for _ in range(2))
    for c in (ours, twin):
        c.extend([70, 9])
        c.append(0, *prior)
    # the tensors the graph reads and writes; the first launches, outside capture, see a root token nothing matches: no rows move
    logits = torch.zeros((B * n, V), dtype=torch.bfloat16, device=dev)
    draft, root, target = i32([0] * (B * n), dev), i32([-1] * B, dev), i32([0] * (B * n), dev)
    ws = torch.full((mixedgemm.argmax_rows_workspace_bytes(B * n, V),), 0xFF, dtype=torch.uint8, device=dev)
    ours.extend(n)
    ours.tree_mask(trees[0])
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mixedgemm.argmax_rows(logits, out=target, workspace=ws)
        result = ours.verify_launch(target, draft, root)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert result[:, 0].tolist() == [n, n]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        mixedgemm.argmax_rows(logits, out=target, workspace=ws)
        assert ours.verify_launch(target, draft, root) is result
    for step, (tree, paths) in enumerate(zip(trees, chosen)):
        d, r, lg = draft_step(rng, [n, n], paths, dev)
        for c in (ours, twin):
            if step or c is twin:
                c.extend(n)
            mask = c.tree_mask(tree)[0]
            c.append(0, *steps[step])
        draft.copy_(d), root.copy_(r), logits.copy_(lg)
        graph.replay()
        got = ours.commit(result)
        want = kvo.verify(kvo.argmax_rows(t_tree.bits(lg)), d.cpu().numpy(), r.cpu().numpy(), [int(w) for w in mask.tolist()],
                          twin.append_indptr.cpu().numpy(), twin.kv_indptr.cpu().numpy(), twin.last_page_len.cpu().numpy(), 16)
        assert kvo.paths_of(want[0], [n, n]) == paths, "precondition: the logits must make the chosen paths win"
        assert np.array_equal(result.cpu().numpy(), want[0]) and got == (paths, [7, 7])
        twin.accept(paths)
        torch.cuda.synchronize()
        same_cache(ours, twin, f"replay {step}")
    assert ours.seq_lens == [70 + 3 + 2, 9 + 4 + 2]

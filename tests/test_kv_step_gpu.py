"""GPU tests of the device steps of the paged KV cache (mixedgemm.kv_step, PagedKVCache.step_launch / sync).  Every comparison is exact
equality; the references are a twin PagedKVCache that runs today's accept + extend on the host and tests/kv_step_oracle.py.

1 tables    step by step against a CPU twin, sync() only at the end: batch 1, 63, 64, 65, 130 (a lane, a wave, across waves) x page size
            1, 16, 24; next_counts mix 0, 1, 5, 21 and a 70-token chunk; keep drawn per step over 0 .. n, with the planted edges: base + k
            a multiple of P, k = 0 where base % P == 0 (every new page goes back), an empty sequence that announces nothing, a sequence
            that drops at least 3 pages while its neighbour takes at least 3; keep as [B] and as [B, 66]; token_pos with and without depths
2 forks     8 samples of one prompt after the host extend that copies the shared last page: shared pages are never pushed, the counts after
            sync() are the twin's, a later host extend gives equal tables
3 statuses  each MM_KV_STEP_* condition (BAD_STATE in its three forms) next to the nearest step that succeeds; state and tables byte-equal but for the two status
            words; a second call does nothing; sync() names the step and the status.  These are status returns: no buffer is too small
            for the step that was asked for
            replay, sync(), replay, sync() of one graph with host calls in between, the host methods refusing after every replay
4 decode    keep = None: 8 plain decode steps in one hipGraph against 8 host extend(1)
5 graph     one hipGraph of 4 speculative steps (append x 2 layers, attend_new(tree=), verify_launch, step_launch), all three cache kinds,
            against a device twin that runs verify() + extend() on the host between the steps; replayed once more with new inputs
6 refusals  a stale state under capture, a cache that releases pages, host methods while the device is ahead
1024 sequences, the limit of one workgroup, go through mixedgemm.kv_step directly against the oracle."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_step_oracle as ko
import test_kv_tree_gpu as t_tree

pytestmark = pytest.mark.gpu

KINDS = ["int4", "bf16", "fp8_e4m3"]
i32 = t_tree.i32


def cache(P, max_pages, batch, device, kind="bf16", **kw):
    return PagedKVCache(num_layers=2, num_kv_heads=1, page_size=P, max_pages=max_pages, batch=batch, kind=kind, device=device, **kw)


def tables(c):
    indptr = c.kv_indptr.cpu().tolist()
    return indptr, c.kv_indices.cpu().tolist()[:indptr[-1]], c.last_page_len.cpu().tolist(), c.append_indptr.cpu().tolist()


def same_host_state(a, b, what):
    assert a._pages == b._pages, what
    assert a._free == b._free, f"{what}: the free list, order included"
    assert a._ref == b._ref and a.seq_lens == b.seq_lens and a.num_new_tokens == b.num_new_tokens, what
    assert (a._announced[0], a._announced[1]) == (b._announced[0], b._announced[1]), what


# ---- 1. the tables against a CPU twin -------------------------------------------------------------------------------------------------------
def step_counts(B, P):
    """0, 1, 5, 21 and one 70-token chunk; sequence 3, the chunk's neighbour, takes at least 3 pages a step too"""
    counts = [70 if b == 2 else (70 if P > 1 else 5) if b == 3 else 5 if b % 16 == 4 else 21 if b == 0 else b % 2 for b in range(B)]
    if B > 6:
        assert counts[6] == 0
    return counts


def plan(B, P, seed, max_len=560, steps=5):
    """the steps of one case on a CPU twin: [(keep, depths, tables, token_pos)], the twin, and what was planted (host only)"""
    rng = np.random.default_rng(seed)
    counts = step_counts(B, P)
    twin = cache(P, 600, B, "cpu")
    prompt = [0 if b == 6 else (b * 7) % (2 * P + 3) for b in range(B)]
    twin.extend(prompt)
    twin.extend(counts)
    out, seen = [], set()
    for s in range(steps):
        announced, bases = twin._announced
        keep = [int(rng.integers(0, n + 1)) for n in announced]
        if s == 1:                                           # base + k an exact multiple of P
            keep = [min(n, -base % P) for n, base in zip(announced, bases)]
        if s == 2:                                           # base % P == 0 and k = 0: every page of the draft goes back
            keep = [0 if base % P == 0 else k for k, base in zip(keep, bases)]
        if s == 0 and B > 3:                                 # sequence 2 drops its pages, its neighbour keeps all and takes new ones
            keep[2], keep[3] = 0, announced[3]
        for b in range(B):
            if announced[b] and (bases[b] + keep[b]) % P == 0:
                seen.add("edge")
            if announced[b] and bases[b] % P == 0 and keep[b] == 0:
                seen.add("all back")
            if not twin.seq_lens[b] and not counts[b]:
                seen.add("empty")
        if s == 0 and B > 3:
            dropped = len(twin._pages[2]) - -(-(bases[2]) // P)
            taken = -(-(twin.seq_lens[3] + counts[3]) // P) - len(twin._pages[3])
            if dropped >= 3 and taken >= 3:
                seen.add("drop 3 take 3")
        depths = None if s % 2 == 0 else [int(x) for x in rng.integers(0, 12, sum(counts))]
        st = ko.from_cache(twin, max_len)
        want = ko.step(st, P, max_len, keep, counts, sum(counts), 600, depths)
        if want is None:                                     # the pool of 600 pages is used up: the case ends here
            assert st.status == ko.OUT_OF_PAGES
            break
        twin.accept([list(range(k)) if n else None for k, n in zip(keep, announced)])
        twin.extend(counts)
        n = int(twin.kv_indptr[-1])
        tbl = (twin.kv_indptr.tolist(), twin.kv_indices[:n].tolist(), twin.last_page_len.tolist(), twin.append_indptr.tolist())
        assert want[:4] == tbl and (st.pages, st.free) == (twin._pages, twin._free), "the oracle and the twin disagree"
        out.append((keep, depths, tbl, want[4]))
    return out, twin, counts, prompt, seen


@pytest.mark.parametrize("P", [1, 16, 24])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_tables_equal_the_cpu_twin_step_by_step(dev, B, P):
    max_len = 560
    todo, twin, counts, prompt, seen = plan(B, P, 1000 * B + P)
    assert len(todo) >= 3
    if B >= 63:
        assert {"edge", "all back", "empty", "drop 3 take 3"} <= seen, seen
    c = cache(P, 600, B, dev)
    c.extend(prompt)
    c.extend(counts)
    first = None
    for s, (keep, depths, tbl, pos) in enumerate(todo):
        k = i32(keep, dev)
        if s % 2:                                            # as verify_launch hands it over: column 0 of [B, 66]
            wide = torch.full((B, _lib.MM_VERIFY_STRIDE), -7, dtype=torch.int32, device=dev)
            wide[:, 0] = k
            k = wide
        got = c.step_launch(k, counts, max_seq_len=max_len, depths=depths)
        first = got if first is None else first
        assert got is first and got.dtype is torch.int32 and got.numel() == sum(counts)
        assert tables(c) == tbl, f"step {s}"
        assert got.cpu().tolist() == pos, f"step {s}: token_pos"
    with pytest.raises(RuntimeError, match=r"sync\(\)"):
        c.seq_lens
    c.sync()
    same_host_state(c, twin, "after sync()")
    # the host goes on from there: equal tables after the same host calls
    paths = [list(range(n)) if n else None for n in counts]
    c.accept(paths), twin.accept(paths)
    more = [int(b < 8) for b in range(B)]
    c.extend(more), twin.extend(more)
    n = int(twin.kv_indptr[-1])
    assert tables(c) == (twin.kv_indptr.tolist(), twin.kv_indices[:n].tolist(), twin.last_page_len.tolist(), twin.append_indptr.tolist())


def test_1024_sequences_against_the_oracle(dev):
    """the limit of one workgroup, 16 waves, through mixedgemm.kv_step: sequence b announces b % 3 tokens, every 4th is empty"""
    B, P, M, max_len = 1024, 4, 2000, 32
    pps = max_len // P
    rng = np.random.default_rng(5)
    lens = [0 if b % 4 == 0 else int(rng.integers(1, 9)) for b in range(B)]
    announced = [min(n, b % 3) for b, n in enumerate(lens)]
    perm = [int(x) for x in rng.permutation(M)]
    pages, at = [], 0
    for n in lens:
        pages.append(perm[at:at + -(-n // P)])
        at += len(pages[-1])
    st = ko.State(lens, announced, pages, perm[at:], M, pps)
    state = i32(st.pack(), dev)
    assert state.numel() == mixedgemm.kv_step_state_ints(B, M, pps)
    nxt = [b % 3 for b in range(B)]
    T = sum(nxt)
    out = [torch.full((n,), -9, dtype=torch.int32, device=dev) for n in (B + 1, M, B, B + 1, T)]
    for s in range(3):
        keep = [int(rng.integers(0, a + 1)) for a in st.announced]
        want = ko.step(st, P, max_len, keep, nxt, T, M)
        assert want is not None
        mixedgemm.kv_step(state, M, pps, P, max_len, i32(nxt, dev), T, *out[:4], keep=i32(keep, dev), token_pos=out[4])
        got = [t.cpu().tolist() for t in out]
        got[1] = got[1][:want[0][-1]]
        assert got == list(want), f"step {s}"
        flat = state.cpu().tolist()
        back = ko.State.unpack(flat, B, M, pps)
        assert flat[:4] == [0, s + 1, len(st.free), 0]
        assert (back.seq_len, back.announced, back.pages, back.free) == (st.seq_len, st.announced, st.pages, st.free)


# ---- 2. forked sequences ----------------------------------------------------------------------------------------------------------------------
def test_forked_samples_keep_their_shared_pages(dev):
    B, P, max_len = 8, 16, 256
    rng = np.random.default_rng(2)
    c, twin = cache(P, 100, B, dev), cache(P, 100, B, "cpu")
    for x in (c, twin):
        x.extend([37] + [0] * (B - 1))
        for b in range(1, B):
            x.fork(0, b)
        x.extend(5)                                          # seven copies of the partly filled page 2
    shared = [p for p in range(100) if twin._ref[p] > 1]
    assert shared == twin._pages[0][:2] and all(twin._ref[p] == B for p in shared)
    for s in range(4):
        keep = [int(rng.integers(0, 6)) for _ in range(B)]
        if s == 1:
            keep = [0] * B                                   # back to the prompt: the copied page stays, nothing below it goes
        c.step_launch(i32(keep, dev), 5, max_seq_len=max_len)
        twin.accept([list(range(k)) for k in keep])           # today's host code, not the CPU form of step_launch
        twin.extend(5)
        assert tables(c) == tables(twin)
    c.sync()
    same_host_state(c, twin, "after sync()")
    assert all(c._ref[p] == B and p not in c._free for p in shared)
    c.extend(3), twin.extend(3)
    assert tables(c) == tables(twin) and c._pages == twin._pages and c._free == twin._free


# ---- 3. each status -----------------------------------------------------------------------------------------------------------------------------
def direct(dev, st, P, max_len, keep, nxt, T=None, capacity=None, total=64):
    """one mixedgemm.kv_step call on the packed oracle state `st` with tables of `total` entries that hold a pattern; returns what the
    device left: (state, [kv_indptr, kv_indices, last_page_len, append_indptr, token_pos]) as lists, before and after, and the tensors"""
    B = len(nxt)
    T = sum(nxt) if T is None else T
    state = i32(st.pack(), dev)
    room = max(T, sum(max(n, 0) for n in nxt), 1)             # token_pos has room for the tokens whatever T claims
    out = [torch.arange(n, dtype=torch.int32, device=dev) + 1000 * (i + 1) for i, n in enumerate((B + 1, total, B, B + 1, room))]
    indices = out[1] if capacity is None else out[1][:capacity]
    before = (state.cpu().tolist(), [t.cpu().tolist() for t in out])

    def call():
        mixedgemm.kv_step(state, st.max_pages, st.pages_per_seq, P, max_len, i32(nxt, dev), T, out[0], indices, out[2], out[3],
                          keep=None if keep is None else i32(keep, dev), token_pos=out[4][:T] if T else None)
        return state.cpu().tolist(), [t.cpu().tolist() for t in out]
    return before, call


def two_sequences(max_pages, P=4, max_len=16, pps=None):
    """[4, 4] committed and [2, 2] announced on pages 0 .. 3, the rest free (host only); pps: list entries per sequence, if not those of max_len"""
    twin = cache(P, max_pages, 2, "cpu")
    twin.extend([4, 4])
    twin.extend([2, 2])
    st = ko.from_cache(twin, max_len)
    st.pages_per_seq = pps or st.pages_per_seq
    return st


FAILS = [  # name, max_pages, max_len, keep, next_new, T (None: their sum), kv_indices capacity (None: all 64), the status
    ("one page short", 5, 16, None, [4, 4], None, None, ko.OUT_OF_PAGES),
    ("one token too long", 6, 9, None, [4, 4], None, None, ko.TOO_LONG),
    ("k = n + 1", 6, 16, [2, 3], [4, 4], None, None, ko.BAD_KEEP),
    ("k = -1", 6, 16, [-1, 2], [4, 4], None, None, ko.BAD_KEEP),
    ("a negative count", 6, 16, None, [4, -1], 3, None, ko.BAD_NEXT),
    ("the sum one off", 6, 16, None, [4, 4], 9, None, ko.BAD_SUM),
    ("the sum one off, below", 6, 16, None, [4, 4], 7, None, ko.BAD_SUM),
    ("kv_indices one short", 6, 16, None, [4, 4], None, 5, ko.INDICES_CAPACITY),
    ("a sequence's list too short", 6, 16, None, [4, 4], None, None, ko.SEQ_PAGES),        # with 2 list entries a sequence
]


@pytest.mark.parametrize("case", FAILS, ids=[f[0] for f in FAILS])
def test_a_step_that_cannot_be_taken_changes_two_words(dev, case):
    _, max_pages, max_len, keep, nxt, T, capacity, status = case
    pps = 2 if status == ko.SEQ_PAGES else None
    st, check = two_sequences(max_pages, max_len=max_len, pps=pps), two_sequences(max_pages, max_len=max_len, pps=pps)
    T = sum(nxt) if T is None else T
    assert ko.step(check, 4, max_len, keep, nxt, T, 64 if capacity is None else capacity) is None and check.status == status
    (state0, out0), call = direct(dev, st, 4, max_len, keep, nxt, T, capacity)
    for again in range(2):                                   # the second call finds the status and does nothing
        state, out = call()
        assert state[0] == status and state[3] == 0 and state[1] == 0, (state[:4], ko.NAMES[status])
        assert state[1:3] + state[4:] == state0[1:3] + state0[4:] and out == out0, "a failed step wrote something"
    # ... and also a step that could be taken does nothing behind it: sticky
    good = i32([0, 0], dev)
    tbl = [torch.full((n,), 77, dtype=torch.int32, device=dev) for n in (3, 64, 2, 3)]
    mixedgemm.kv_step(i32(state, dev), max_pages, st.pages_per_seq, 4, max_len, good, 0, *tbl)
    assert all(t.eq(77).all() for t in tbl)


SUCCEEDS = [("exactly enough pages", 6, 16, None, [4, 4], None), ("len + n == max_seq_len", 6, 10, None, [4, 4], None),
            ("k = n", 6, 16, [2, 2], [4, 4], None), ("k = 0", 6, 16, [0, 0], [4, 4], None), ("kv_indices exactly enough", 6, 16, None, [4, 4], 6)]


@pytest.mark.parametrize("case", SUCCEEDS, ids=[f[0] for f in SUCCEEDS])
def test_the_nearest_step_that_can_be_taken(dev, case):
    _, max_pages, max_len, keep, nxt, capacity = case
    st = two_sequences(max_pages, max_len=max_len)
    want = ko.step(st, 4, max_len, keep, nxt, 8, 64 if capacity is None else capacity)
    assert want is not None
    (state0, out0), call = direct(dev, two_sequences(max_pages, max_len=max_len), 4, max_len, keep, nxt, 8, capacity)
    state, out = call()
    assert state[:4] == [0, 1, len(st.free), 0]
    back = ko.State.unpack(state, 2, max_pages, st.pages_per_seq)
    assert (back.seq_len, back.announced, back.pages, back.free) == (st.seq_len, st.announced, st.pages, st.free)
    n = want[0][-1]
    assert [out[0], out[1][:n], out[2], out[3], out[4]] == list(want) and out[1][n:] == out0[1][n:], "entries past kv_indptr[B] were touched"


def test_sync_names_the_step_and_the_status(dev):
    c, twin = cache(4, 7, 2, dev), cache(4, 7, 2, "cpu")
    for x in (c, twin):
        x.extend([4, 4])
        x.extend([2, 2])
    assert twin.steps_guaranteed(4, 32) == 1                 # 6 + 4 tokens take the 3 pages left; the next 4 have none
    for s in range(4):                                       # steps 0 good, 1 fails, 2 and 3 find the status
        c.step_launch(None, 4, max_seq_len=32)
    twin.step_launch(None, 4, max_seq_len=32)
    good = tables(twin)
    assert tables(c) == good
    with pytest.raises(RuntimeError, match=r"step 1 .*MM_KV_STEP_OUT_OF_PAGES \(7\)"):
        c.sync()
    same_host_state(c, twin, "the last good step")
    assert tables(c) == good
    c.truncate(0, 3), twin.truncate(0, 3)                    # the host works again, and so does the next step: the state is uploaded anew
    c.extend(1), twin.extend(1)
    c.step_launch(i32([0, 1], dev), 2, max_seq_len=32), twin.step_launch(torch.tensor([0, 1], dtype=torch.int32), 2, max_seq_len=32)
    assert tables(c) == tables(twin)
    c.sync()
    same_host_state(c, twin, "after the recovery")


def _long(flat):
    flat[4] = 9                                              # seq_len[0] = 9 on 2 pages of 4


def _negative(flat):
    flat[2] = -1                                             # free_count


def _overfull(flat):
    flat[2] = 6                                              # free_count = max_pages, and the step pushes 2 more


@pytest.mark.parametrize("tweak, keep", [(_long, None), (_negative, None), (_overfull, [0, 0])], ids=["a sequence", "free_count < 0", "the stack overflows"])
def test_a_state_the_rule_does_not_leave_is_refused(dev, tweak, keep):
    """MM_KV_STEP_BAD_STATE in its three forms; nothing is read or written outside the buffers, nothing changes but the two words"""
    st = two_sequences(6)
    flat = st.pack()
    tweak(flat)
    state = i32(flat, dev)
    tbl = [torch.full((n,), 77, dtype=torch.int32, device=dev) for n in (3, 64, 2, 3, 8)]
    for again in range(2):
        mixedgemm.kv_step(state, 6, st.pages_per_seq, 4, 16, i32([4, 4], dev), 8, *tbl[:4], keep=None if keep is None else i32(keep, dev),
                          token_pos=tbl[4])
        got = state.cpu().tolist()
        assert got[0] == ko.BAD_STATE and got[3] == 0 and got[1:3] + got[4:] == flat[1:3] + flat[4:]
        assert all(t.eq(77).all() for t in tbl)


def test_replay_sync_replay_sync(dev):
    """the Python of a captured step_launch does not run at a replay: sync() has to find what the graph did every time, and the host
    methods have to refuse in between.  The first step_launch of this cache is the captured one (upload_state prepares it)"""
    warm = cache(4, 8, 2, dev)
    warm.step_launch(None, 1, max_seq_len=64)                # the kernels are loaded, by another cache
    c, twin = cache(4, 60, 2, dev), cache(4, 60, 2, "cpu")
    for x in (c, twin):
        x.extend([7, 2])
        x.extend(3)
    keep = i32([0, 0], dev)
    c.upload_state(64, 3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(2):
            c.step_launch(keep, 3, max_seq_len=64)
    c.sync()                                                 # nothing ran yet
    same_host_state(c, twin, "after capture")
    for r, ks in enumerate([[1, 3], [2, 0], [3, 3], [0, 1]]):
        keep.copy_(i32(ks, dev))
        graph.replay()
        torch.cuda.synchronize()
        for what, call in (("seq_lens", lambda: c.seq_lens), ("extend", lambda: c.extend(1)), ("pages_in_use", lambda: c.pages_in_use),
                           ("commit", lambda: c.commit(c._verify_result)), ("truncate", lambda: c.truncate(0, 1))):
            with pytest.raises(RuntimeError, match=r"sync\(\)"):
                call()
        c.sync()
        for _ in range(2):
            twin.accept([list(range(k)) for k in ks])
            twin.extend(3)
        same_host_state(c, twin, f"round {r}")
        assert tables(c) == tables(twin) and c.pages_in_use == twin.pages_in_use
        c.sync()                                             # a second one finds nothing new
        same_host_state(c, twin, f"round {r}, synced twice")
        if r == 1:                                           # host calls in between: the state goes up again before the next replay
            for x in (c, twin):
                x.truncate(0, 5)
                x.extend(3)
            c.upload_state(64, 3)
            assert c.seq_lens == twin.seq_lens               # nothing ran since: the host lists are current
    assert c.seq_lens == twin.seq_lens


# ---- 4. plain decode in one graph ---------------------------------------------------------------------------------------------------------------
def test_eight_decode_steps_in_one_graph(dev):
    B, P, max_len = 3, 4, 64
    c, twin = cache(P, 60, B, dev), cache(P, 60, B, "cpu")
    for x in (c, twin):
        x.extend([7, 0, 12])
        x.extend(1)
    pos = c.step_launch(None, 1, max_seq_len=max_len)       # outside capture: the state, the counts, token_pos; the kernels are loaded
    twin.extend(1)
    torch.cuda.synchronize()
    assert tables(c) == tables(twin) and pos.cpu().tolist() == [8, 1, 13]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(8):
            assert c.step_launch(None, 1, max_seq_len=max_len) is pos
    assert tables(c) == tables(twin), "capture must not run anything"
    for replay in range(2):
        graph.replay()
        for _ in range(8):
            twin.extend(1)
        torch.cuda.synchronize()
        assert tables(c) == tables(twin), f"replay {replay}"
        assert pos.cpu().tolist() == [n - 1 for n in twin.seq_lens]
    c.sync()
    same_host_state(c, twin, "after sync()")
    assert c.seq_lens == [25, 18, 30]


# ---- 5. one graph of four speculative steps -----------------------------------------------------------------------------------------------------
TREE6 = [-1, 0, 0, 1, 1, 2]


@pytest.mark.parametrize("kind", KINDS)
def test_four_speculative_steps_in_one_graph(dev, kind):
    B, Hq, P, MSL, S = 2, 4, 16, 128, 4
    counts, parents = [6, 3], [TREE6, None]
    T = sum(counts)
    rng = np.random.default_rng(7)
    rnd = lambda *shape: t_tree.bf(rng.standard_normal(shape), dev)
    prompt = (rnd(27, 1, 128), rnd(27, 1, 128))

    def inputs():
        # tokens over {0, 1}: paths of several nodes are common, and so are rejections
        return (rnd(S, T, 1, 128), rnd(S, T, 1, 128), rnd(S, T, Hq, 128), i32(rng.integers(0, 2, (S, T)), dev), i32(rng.integers(0, 2, (S, T)), dev))

    ours, twin = cache(P, 64, B, dev, kind), cache(P, 64, B, dev, kind)
    for c in (ours, twin):
        c.extend([20, 7])
        for layer in range(2):
            c.append(layer, *prompt)
        c.extend(counts)
        mask, depths = c.tree_mask(parents)
    mask = ours.tree_mask(parents)[0]
    K, V, Q, target, draft = inputs()
    root = i32([1, 0], dev)

    def device_steps(steps):
        outs = []
        for s in steps:
            for layer in range(2):
                ours.append(layer, K[s], V[s])
                outs.append(ours.attend_new(layer, Q[s], max_seq_len=MSL, tree=mask))
            result = ours.verify_launch(target[s], draft[s], root)
            ours.step_launch(result, counts, max_seq_len=MSL, depths=depths)
            root.copy_(result[:, 1])
        return outs

    def host_steps(steps, root_twin):
        outs, kept = [], []
        for s in steps:
            m = twin.tree_mask(parents)[0]
            for layer in range(2):
                twin.append(layer, K[s], V[s])
                outs.append(twin.attend_new(layer, Q[s], max_seq_len=MSL, tree=m))
            paths, nxt = twin.verify(target[s], draft[s], root_twin)
            kept.append([len(p) for p in paths])
            twin.extend(counts)
            root_twin = i32(nxt, dev)
        return outs, root_twin, kept

    def compare(o_ours, o_twin, root_twin, what):
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(o_ours, o_twin)):
            t_tree.same_bits(a, b, f"{what}: step {i // 2} layer {i % 2}")
        assert torch.equal(root, root_twin) and tables(ours) == tables(twin), what
        live = sorted({p for pages in twin._pages for p in pages})
        assert torch.equal(ours.kv_data[live].view(torch.uint8), twin.kv_data[live].view(torch.uint8)), f"{what}: the live pages"
        assert ours.kv_param is None or torch.equal(ours.kv_param[live].view(torch.int16), twin.kv_param[live].view(torch.int16)), what

    # one step outside capture: the state goes up, every buffer is allocated, every kernel loaded
    o_twin, root_twin, kept = host_steps([0], root.clone())
    compare(device_steps([0]), o_twin, root_twin, "the eager step")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_ours = device_steps(range(S))
    all_kept = []
    for replay in range(2):
        if replay:                                           # new inputs where the graph reads them
            for old, new in zip((K, V, Q, target, draft), inputs()):
                old.copy_(new)
        graph.replay()
        o_twin, root_twin, kept = host_steps(range(S), root_twin)
        all_kept += kept
        compare(o_ours, o_twin, root_twin, f"replay {replay}")
    assert any(0 < k[0] < 6 for k in all_kept) and any(k[1] < 3 for k in all_kept), f"precondition: drafts are partly rejected: {all_kept}"
    ours.sync()
    same_host_state(ours, twin, "after sync()")


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(dev, monkeypatch):
    with pytest.raises(ValueError, match="window"):
        cache(4, 50, 2, dev, window=8).step_launch(None, 1, max_seq_len=64)
    c = cache(4, 50, 2, dev)
    c.extend([6, 3])
    # under capture the state has to be current already, and so have the counts (the capture state is faked: nothing is launched)
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="stale device state"):
            c.step_launch(None, 1, max_seq_len=64)
        c.upload_state(64)                                   # the state alone: the counts are still to be uploaded
        with pytest.raises(RuntimeError, match="new next_counts"):
            c.step_launch(None, 1, max_seq_len=64)
        assert not c._ahead and c.seq_lens == [6, 3]
        c.upload_state(64, 1)                                # ... and with them, and token_pos: the first call passes
        c.step_launch(None, 1, max_seq_len=64)
    q = torch.zeros((2, 4, 128), dtype=torch.bfloat16, device=dev)
    k = torch.zeros((2, 1, 128), dtype=torch.bfloat16, device=dev)
    for what, call in (("extend", lambda: c.extend(1)), ("fork", lambda: c.fork(0, 1)), ("truncate", lambda: c.truncate(0, 1)),
                       ("reset", lambda: c.reset(0)), ("accept", lambda: c.accept([[0], [0]])), ("commit", lambda: c.commit(c._verify_result)),
                       ("share_groups", c.share_groups), ("pages_in_use", lambda: c.pages_in_use), ("seq_lens", lambda: c.seq_lens),
                       ("steps_guaranteed", lambda: c.steps_guaranteed(1, 64)), ("upload_state", lambda: c.upload_state(64)),
                       ("attend", lambda: c.attend(0, q)), ("attend_new", lambda: c.attend_new(0, q)),
                       ("attend(shared=True)", lambda: c.attend(0, q, 64, shared=True)),
                       ("max_seq_len", lambda: c.step_launch(None, 1, max_seq_len=128))):
        with pytest.raises(RuntimeError, match=r"sync\(\)"):
            call()
    # what works while the device is ahead
    c.append(0, k, k)
    c.attend(0, q, 64), c.attend_new(0, q, 64), c.attend(0, q, 64, shared=True, max_shared_len=16)
    c.tree_mask([None, None])
    c.verify_launch(i32([0, 0], dev), i32([0, 0], dev), i32([0, 0], dev))
    torch.cuda.synchronize()
    c.sync()
    assert c.seq_lens == [7, 4] and c.pages_in_use == 3

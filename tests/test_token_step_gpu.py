"""GPU tests of the token half of a decode step (mixedgemm.ngram_draft, mixedgemm.token_step; include/micromix_tokens.h).  Both are integer
functions of their inputs alone, so every comparison is equality against tests/token_oracle.py:
1 search    ngram_draft on seeded histories over an alphabet of 3 at the lengths around the start, max_n and the part edge, rows whose
            starts are not 16-byte aligned, one, 63 and 65 sequences; the slots at and past N hold a copy of the suffix that would win
            if it were read; every output array and every element of tokens is compared
2 planted   histories of distinct tokens with n-grams planted: longer earlier against shorter later, two equal, across and at a part
            edge, cut short by the start, e = N - 2, a constant history, a best match of min_n - 1; 0, 1, 2 and 64 nodes
3 far       129 histories of 2^24 tokens: the last row starts past 2^31 elements, its match ends near 2^24
4 commit    token_step: every case of the rule, the sticky kv_state, a tree-shaped path
5 loop      one hipGraph of 8 steps ngram_draft -> f -> verify_greedy -> token_step for 5 requests against the plain rollout, replayed
            after everything was rewritten in place; and with a PagedKVCache (verify_launch, step_launch, kv_state) in the same graph,
            also on a pool that runs out"""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
from micromix_amd.kvcache import PagedKVCache
import token_oracle as to
import test_kv_tree_gpu as t_tree
import test_token_step_cpu as t_cpu

pytestmark = pytest.mark.gpu

i32 = t_tree.i32
CHUNK = _lib.TOKENS["MM_NGRAM_CHUNK"]
NODES = (5, 0, 1, 2, 64, 7)


def indptr_of(counts):
    out = [0]
    for n in counts:
        out.append(out[-1] + n)
    return out


def draft_and_compare(dev, rows, total, counts, min_n, max_n, what):
    """rows: int32 numpy [B, ld].  Runs ngram_draft on the device and the oracle on lists; compares all six outputs (entries nothing
    writes keep -7) and the whole of tokens.  Returns the oracle's outputs"""
    B, indptr = len(rows), indptr_of(counts)
    T = indptr[-1]
    want_rows = rows.tolist()
    want = to.ngram_draft(want_rows, total, indptr, T, min_n, max_n)
    tokens = i32(rows, dev)
    outs = {k: torch.full((B if k in ("root_tok", "match_len") else T,), -7, dtype=torch.int32, device=dev) for k in want}
    got = mixedgemm.ngram_draft(tokens, i32(total, dev), i32(indptr, dev), T, min_n=min_n, max_n=max_n, **outs)
    torch.cuda.synchronize()
    for k, v in want.items():
        assert getattr(got, k) is outs[k]
        assert outs[k].cpu().tolist() == [-7 if x is None else x for x in v], f"{what}: {k}"
    assert torch.equal(tokens.cpu(), torch.tensor(want_rows, dtype=torch.int32)), f"{what}: tokens outside the slack changed, or the slack is wrong"
    return want


def winning_slack(rows, total, max_n):
    """the slots at and past N hold the suffix over and over: an end position there would match max_n tokens"""
    for row, N in zip(rows, total):
        w = min(max_n, N)
        if w and N < len(row):
            row[N:] = np.resize(row[N - w:N], len(row) - N)


# ---- 1. seeded histories ---------------------------------------------------------------------------------------------------------------------
def lengths(max_n):
    return [0, 1, 2, max_n, max_n + 1, CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + max_n - 1, 16389]


@pytest.mark.parametrize("ld, B, min_n, max_n", [(16400, 65, 1, 4), (16401, 63, 2, 16), (16403, 65, 3, 5), (16401, 65, 1, 16), (16403, 63, 1, 2),
                                                 (16400, 63, 4, 4)])
def test_seeded_histories_equal_the_oracle(dev, ld, B, min_n, max_n):
    rng = np.random.default_rng(ld * 131 + B)
    rows = rng.integers(0, 3, (B, ld)).astype(np.int32)
    Ns = lengths(max_n)
    total = [Ns[(b + B) % len(Ns)] for b in range(B)]
    winning_slack(rows, total, max_n)
    want = draft_and_compare(dev, rows, total, [NODES[b % len(NODES)] for b in range(B)], min_n, max_n, f"ld {ld} B {B}")
    assert max(want["match_len"]) >= min(max_n, 7) and min(want["match_len"]) == 0


@pytest.mark.parametrize("ld", [16400, 16401, 16403])
def test_one_sequence_at_every_length(dev, ld):
    """batch 1: the row start is aligned, the lengths are not"""
    rng = np.random.default_rng(ld)
    for min_n, max_n in ((1, 3), (2, 16)):
        for at, N in enumerate(lengths(max_n)):
            rows = rng.integers(0, 3, (1, ld)).astype(np.int32)
            winning_slack(rows, [N], max_n)
            draft_and_compare(dev, rows, [N], [NODES[at % len(NODES)]], min_n, max_n, f"ld {ld} N {N} max_n {max_n}")


def test_padding_ids_and_lengths_outside_the_buffer(dev):
    """tokens are compared as 32-bit integers (a padding id matches itself); total_len is clamped to [0, ld_tok]; a sequence of more
    than 64 nodes gets none written; at N = ld_tok there is no slack"""
    rng = np.random.default_rng(5)
    rows = rng.choice(np.array([-1, 0, -2 ** 31, 2 ** 31 - 1], dtype=np.int64), (6, 50)).astype(np.int32)
    draft_and_compare(dev, rows, [-4, 50, 57, 49, 48, 30], [3, 4, 4, 4, 65, 4], 1, 6, "edges")


# ---- 2. planted matches -------------------------------------------------------------------------------------------------------------------------
def planted_cases(ld):
    """(name, N, {position: tokens planted}, (m, e) of the match with min_n = 2, max_n = 8): distinct tokens everywhere else, and the
    suffix 5 6 7 8 at the end of every history unless the case says otherwise"""
    N, suf = 16389, [5, 6, 7, 8]
    end = lambda n: {n - 4: suf}
    return [
        ("a longer earlier match against a shorter later one", N, {100: suf, 9000: [7, 8], **end(N)}, (4, 103)),
        ("two matches of equal length", N, {100: suf, 9000: suf, **end(N)}, (4, 9003)),
        ("an n-gram that straddles the part edge", N, {CHUNK - 2: suf, **end(N)}, (4, CHUNK + 1)),
        ("the first end position of a part", N, {CHUNK - 3: suf, **end(N)}, (4, CHUNK)),
        ("the last end position of a part", N, {CHUNK - 4: suf, **end(N)}, (4, CHUNK - 1)),
        ("the halo of the third part", 16400, {2 * CHUNK - 1: suf, 40: [6, 7, 8], **end(16400)}, (4, 2 * CHUNK + 2)),
        ("cut short by the start of the history", N, {0: [6, 7, 8], **end(N)}, (3, 2)),
        ("the start beats a shorter later match", N, {0: [6, 7, 8], 12000: [7, 8], **end(N)}, (3, 2)),
        ("e = N - 2", N, {N - 3: [9, 9, 9]}, (2, N - 2)),
        ("a constant history", 300, {0: [3] * 300}, (8, 298)),
        ("a constant history over two parts", CHUNK + 9, {0: [3] * (CHUNK + 9)}, (8, CHUNK + 7)),
        ("a best match of min_n - 1", N, {500: [8], 9000: [8], **end(N)}, (0, None)),
        ("no token repeats", N, {}, (0, None)),
        ("the match ends where the suffix begins", N, {N - 8: suf, **end(N)}, (4, N - 5)),
        ("the suffix overlaps its match", 40, {30: [1, 2, 1, 2, 1, 2, 1, 2, 1, 2]}, (8, 37)),
    ]


@pytest.mark.parametrize("min_n, max_n", [(2, 8), (5, 16), (1, 3)])
def test_planted_matches(dev, min_n, max_n):
    ld = 16401
    cases = planted_cases(ld)
    rows = np.tile(np.arange(1000, 1000 + ld, dtype=np.int32), (len(cases), 1))
    for row, (_, N, plants, _) in zip(rows, cases):
        for at, toks in plants.items():
            row[at:at + len(toks)] = toks
    total = [c[1] for c in cases]
    winning_slack(rows, total, max_n)
    counts = [(0, 1, 2, 64, 6)[b % 5] for b in range(len(cases))]
    before = rows.copy()
    want = draft_and_compare(dev, rows, total, counts, min_n, max_n, f"planted {min_n} {max_n}")
    if (min_n, max_n) == (2, 8):                                 # the oracle itself, against the answers worked out by hand
        indptr = indptr_of(counts)
        for b, (name, N, _, (m, e)) in enumerate(cases):
            assert want["match_len"][b] == m, name
            nodes = want["draft_tok"][indptr[b]:indptr[b + 1]]
            h = before[b].tolist()
            assert nodes == ([h[N - 1]] + [h[e + 1 + i % (N - 1 - e)] if m else h[N - 1] for i in range(counts[b] - 1)])[:counts[b]], name
    if min_n == 5:                                               # every planted 4-gram is now a best match of min_n - 1
        assert want["match_len"] == [0] * 9 + [16, 16, 0, 0, 0, 8]


# ---- 3. past 2^31 elements ---------------------------------------------------------------------------------------------------------------------
def test_a_history_of_two_to_the_24_behind_two_to_the_31_elements(dev):
    B, ld = 129, _lib.TOKENS["MM_TOKENS_MAX_LD"]
    need = B * ld * 4 + (1 << 30)
    if torch.cuda.mem_get_info(dev)[0] < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory")
    assert (B - 1) * ld >= 2 ** 31
    tokens = torch.empty((B, ld), dtype=torch.int32, device=dev)
    last = tokens[B - 1]
    torch.arange(1000, 1000 + ld, dtype=torch.int32, device=dev, out=last)
    e, suf = ld - 700, i32([5, 6, 7, 8], dev)
    last[e - 3:e + 1] = suf
    last[100:104] = suf                                          # an equal match at a low position must lose
    last[ld - 4:] = suf
    total = torch.zeros(B, dtype=torch.int32, device=dev)
    total[B - 1] = ld
    total[0] = -1
    counts = [0] * (B - 1) + [6]
    got = mixedgemm.ngram_draft(tokens, total, i32(indptr_of(counts), dev), 6, min_n=2, max_n=16)
    torch.cuda.synchronize()
    assert got.match_len.cpu().tolist() == [0] * (B - 1) + [4] and got.root_tok.cpu().tolist() == [-1] * (B - 1) + [8]
    assert got.draft_tok.cpu().tolist() == [8] + [1000 + e + 1 + i for i in range(5)] and got.cand_tok.cpu().tolist()[-2:] == [1000 + e + 5, -1]
    assert got.row_total_len.cpu().tolist() == [ld] * 6 and got.row_seq.cpu().tolist() == [B - 1] * 6
    assert last[ld - 4:].cpu().tolist() == [5, 6, 7, 8]          # N == ld_tok: no slack
    # the commit at the far end: room for 3 of 5 tokens
    total[B - 1] = ld - 3
    finished = torch.zeros(B, dtype=torch.int32, device=dev)
    result = torch.full((B, 66), -1, dtype=torch.int32, device=dev)
    result[:, :2] = 0
    result[B - 1, :7] = i32([5, 44, 0, 1, 2, 3, 4], dev)
    emitted = mixedgemm.token_step(tokens, total, finished, result, i32([40, 41, 42, 43, 44, 45], dev), i32(indptr_of(counts), dev),
                                   i32([0] * (B - 1) + [8], dev), torch.full((B,), 2 ** 31 - 1, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert emitted.cpu().tolist() == [0] * (B - 1) + [3] and total.cpu().tolist() == [-1] + [0] * (B - 2) + [ld]
    assert finished.cpu().tolist() == [0] * (B - 1) + [to.LENGTH] and last[ld - 5:].cpu().tolist() == [1000 + ld - 5, 5, 40, 41, 42]


# ---- 4. the commit ------------------------------------------------------------------------------------------------------------------------------
def commit_cases():
    """(name, n, root, k, path, generated tokens along the path, total_len, max_total, stop set, finished before) -> checked by the
    oracle; ld = 40.  The tokens a path names are target_tok[q0 + node]"""
    return [
        ("k = 0", 5, 3, 0, [], [], 10, 40, [], 0),
        ("k = n", 5, 3, 5, [0, 1, 2, 3, 4], [11, 12, 13, 14, 15], 10, 40, [], 0),
        ("a stop token at the first generated position", 5, 3, 4, [0, 1, 2, 3], [7, 12, 13, 14], 10, 40, [7, -1], 0),
        ("a stop token at the last generated position", 5, 3, 4, [0, 1, 2, 3], [11, 12, 13, 7], 10, 40, [-1, 7], 0),
        ("the cap cuts in front of a stop token", 5, 3, 4, [0, 1, 2, 3], [11, 12, 7, 14], 10, 12, [7, 7], 0),
        ("cap = 0", 5, 3, 3, [0, 1, 2], [11, 12, 13], 12, 12, [11, -1], 0),
        ("finished is sticky", 5, 3, 3, [0, 1, 2], [11, 12, 13], 10, 40, [], 1),
        ("finished by length is sticky", 5, 3, 3, [0, 1, 2], [11, 12, 13], 10, 40, [], 2),
        ("a prompt chunk", 70, 3, 70, [], [], 10, 200, [], 0),
        ("a prompt chunk by its root", 5, -1, 5, [], [], 10, 40, [], 0),
        ("a tree-shaped path", 6, 3, 3, [0, 2, 5], [11, 13, 16], 10, 40, [], 0),
        ("n = 0", 0, 3, 0, [], [], 10, 40, [], 0),
        ("the buffer ends before max_total", 5, 3, 5, [0, 1, 2, 3, 4], [11, 12, 13, 14, 15], 37, 1000, [], 0),
        ("the limit is reached exactly", 5, 3, 2, [0, 1], [11, 12], 10, 12, [], 0),
        ("a stop token on the last slot", 5, 3, 2, [0, 1], [11, 7], 10, 12, [7, -1], 0),
        ("64 nodes, all kept", 64, 3, 64, list(range(64)), list(range(100, 164)), 0, 1000, [130, -1], 0),
        ("a stop token past the path does not count", 5, 3, 2, [0, 1], [11, 12], 10, 40, [13, 14], 0),
    ]


def test_token_step_cases(dev):
    cases, ld = commit_cases(), 40
    B = len(cases)
    qo = indptr_of([c[1] for c in cases])
    target = list(range(2000, 2000 + qo[-1]))                    # rows no path names hold tokens that are in no stop set
    result = []
    for b, (_, n, root, k, path, made, *_rest) in enumerate(cases):
        for node, tok in zip(path, made):
            target[qo[b] + node] = tok
        if n == 5 and k == 2:
            target[qo[b] + 2], target[qo[b] + 3] = 13, 14        # "past the path": the tokens of nodes that were not accepted
        result.append([k, made[-1] if made else root] + path + [-1] * (64 - len(path)))
    rows = np.arange(B * ld, dtype=np.int32).reshape(B, ld) + 5000
    total, most = [c[6] for c in cases], [c[7] for c in cases]
    stops = [(c[8] + [-1, -1])[:2] for c in cases]
    finished, roots = [c[9] for c in cases], [c[2] for c in cases]

    w_rows, w_total, w_fin = rows.tolist(), total[:], finished[:]
    want = to.token_step(w_rows, w_total, w_fin, result, target, qo, roots, most, stops)
    by_name = {c[0]: (want[b], w_total[b], w_fin[b]) for b, c in enumerate(cases)}
    assert by_name["k = n"] == (5, 15, 0) and by_name["a stop token at the first generated position"] == (1, 11, 1)
    assert by_name["a stop token at the last generated position"] == (4, 14, 1) and by_name["the cap cuts in front of a stop token"] == (2, 12, 2)
    assert by_name["cap = 0"] == (0, 12, 2) and by_name["finished is sticky"] == (0, 10, 1) and by_name["a prompt chunk"] == (0, 10, 0)
    assert by_name["a tree-shaped path"] == (3, 13, 0) and w_rows[10][10:13] == [11, 13, 16]
    assert by_name["the buffer ends before max_total"] == (3, 40, 2) and by_name["the limit is reached exactly"] == (2, 12, 2)
    assert by_name["a stop token on the last slot"] == (2, 12, 1) and by_name["64 nodes, all kept"] == (31, 31, 1)
    assert by_name["a stop token past the path does not count"] == (2, 12, 0)

    args = [i32(x, dev) for x in (result, target, qo, roots, most)]
    state = lambda: (i32(rows, dev), i32(total, dev), i32(finished, dev))
    # a failed kv_step in front: nothing at all is written
    tokens, tl, fin = state()
    emitted = torch.full((B,), -7, dtype=torch.int32, device=dev)
    kv = i32([_lib.KV_STEP["MM_KV_STEP_OUT_OF_PAGES"], 3, 0, 3], dev)
    assert mixedgemm.token_step(tokens, tl, fin, *args, stop_tok=i32(stops, dev), kv_state=kv, emitted=emitted) is emitted
    torch.cuda.synchronize()
    assert emitted.cpu().tolist() == [-7] * B and tl.cpu().tolist() == total and fin.cpu().tolist() == finished
    assert torch.equal(tokens.cpu(), torch.from_numpy(rows))
    # status 0, and no state at all: the rule
    for kv in (i32([0, 3, 0, 0], dev), None):
        tokens, tl, fin = state()
        emitted = mixedgemm.token_step(tokens, tl, fin, *args, stop_tok=i32(stops, dev), kv_state=kv)
        torch.cuda.synchronize()
        assert emitted.cpu().tolist() == want and tl.cpu().tolist() == w_total and fin.cpu().tolist() == w_fin
        assert tokens.cpu().tolist() == w_rows
    # without a stop list nothing stops
    tokens, tl, fin = state()
    w2 = (rows.tolist(), total[:], finished[:])
    want2 = to.token_step(*w2, result, target, qo, roots, most, None)
    assert mixedgemm.token_step(tokens, tl, fin, *args).cpu().tolist() == want2 and want2 != want
    assert (tokens.cpu().tolist(), tl.cpu().tolist(), fin.cpu().tolist()) == w2


@pytest.mark.parametrize("seed", range(2))
def test_token_step_random_cases_equal_the_oracle(dev, seed):
    import random
    rng = random.Random(500 + seed)
    for case in range(12):
        B, ld = rng.choice((1, 63, 65, 130)), rng.choice((1, 3, 12, 30))
        tokens, total, finished, result, target, qo, root, most, stop = t_cpu.random_step_case(rng, B, ld)
        t, tl, fin = i32(np.array(tokens).reshape(B, ld), dev), i32(total, dev), i32(finished, dev)
        want = to.token_step(tokens, total, finished, result, target, qo, root, most, stop)      # in place: the lists become the expectation
        got = mixedgemm.token_step(t, tl, fin, i32(np.array(result).reshape(B, 66), dev), i32(target, dev), i32(qo, dev), i32(root, dev), i32(most, dev),
                                   stop_tok=None if stop is None else i32(stop, dev))
        torch.cuda.synchronize()
        assert got.cpu().tolist() == want and tl.cpu().tolist() == total and fin.cpu().tolist() == finished, (seed, case)
        assert t.cpu().tolist() == tokens, (seed, case)


# ---- 5. the loop ------------------------------------------------------------------------------------------------------------------------------------
class Loop:
    """the buffers of one captured loop and its steps; with a cache, verify_launch and step_launch are part of every step"""

    def __init__(self, dev, cache=None, max_seq_len=None):
        self.dev, self.cache, self.max_seq_len = dev, cache, max_seq_len
        self.f = i32(to.model_table(), dev)
        self.counts = to.LOOP_NODES
        self.indptr = indptr_of(self.counts)
        self.T, B = self.indptr[-1], len(self.counts)
        self.qo = i32(self.indptr, dev)
        self.tokens, self.total_len, self.finished, self.max_total, self.stops = t_cpu.loop_state(0, dev)
        z = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
        self.outs = dict(draft_tok=z(self.T), root_tok=z(B), cand_tok=z(self.T), match_len=z(B), row_seq=z(self.T), row_total_len=z(self.T))
        self.target, self.result, self.moves = z(self.T), z(B * 66).view(B, 66), (z(self.T), z(self.T))
        self.emitted = [z(B) for _ in range(to.LOOP_STEPS)]
        # verify_greedy wants a page table for its move table: one page of 4096 slots a sequence, holding the announced tokens
        self.kv_indptr, self.last_page_len = i32(list(range(B + 1)), dev), i32(self.counts, dev)

    def load(self, variant):
        for old, new in zip((self.tokens, self.total_len, self.finished, self.max_total, self.stops), t_cpu.loop_state(variant, self.dev)):
            old.copy_(new)

    def step(self, s):
        c = self.cache
        qo = self.qo if c is None else c.append_indptr
        d = mixedgemm.ngram_draft(self.tokens, self.total_len, qo, self.T, min_n=1, max_n=4, **self.outs)
        torch.index_select(self.f, 0, d.draft_tok, out=self.target)
        if c is None:
            result = mixedgemm.verify_greedy(self.target, d.draft_tok, d.root_tok, qo, self.kv_indptr, self.last_page_len, 4096,
                                             result=self.result, move_src=self.moves[0], move_dst=self.moves[1])[0]
        else:
            result = c.verify_launch(self.target, d.draft_tok, d.root_tok)
        mixedgemm.token_step(self.tokens, self.total_len, self.finished, result, self.target, qo, d.root_tok, self.max_total,
                             stop_tok=self.stops, kv_state=None if c is None else c.step_state, emitted=self.emitted[s])
        if c is not None:
            c.step_launch(result, self.counts, max_seq_len=self.max_seq_len)

    def emitted_lists(self):
        return [e.cpu().tolist() for e in self.emitted]


def test_eight_steps_in_one_graph_are_the_plain_rollout(dev):
    loop = Loop(dev)
    loop.step(0)                                                 # every kernel is loaded; the state is written again below
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for s in range(to.LOOP_STEPS):
            loop.step(s)
    seen = []
    for variant in (0, 1, 0):                                    # prompts, limits and stop sets rewritten in place
        loop.load(variant)
        graph.replay()
        torch.cuda.synchronize()
        seen.append(t_cpu.check_loop(variant, loop.tokens, loop.total_len, loop.finished, loop.emitted_lists()))
    assert seen[0] == seen[2] and {0, 1, 2} <= set(seen[0][1])
    # the same loop on CPU tensors leaves the same history, slack included
    cpu = t_cpu.loop_state(0)
    for _ in range(to.LOOP_STEPS):
        d = mixedgemm.ngram_draft(cpu[0], cpu[1], i32(loop.indptr, "cpu"), loop.T, min_n=1, max_n=4)
        target = loop.f.cpu()[d.draft_tok.long()]
        result = i32(to.chain_verify(target.tolist(), d.draft_tok.tolist(), d.root_tok.tolist(), loop.indptr), "cpu")
        mixedgemm.token_step(cpu[0], cpu[1], cpu[2], result, target, i32(loop.indptr, "cpu"), d.root_tok, cpu[3], stop_tok=cpu[4])
    assert torch.equal(cpu[0], loop.tokens.cpu()) and torch.equal(cpu[1], loop.total_len.cpu()) and torch.equal(cpu[2], loop.finished.cpu())


def paged_loop(dev, max_pages):
    P, MSL = 16, 256
    prompts = to.loop_requests(0)[0]

    def new_cache():
        c = PagedKVCache(num_layers=1, num_kv_heads=1, page_size=P, max_pages=max_pages, batch=len(prompts), kind="int4", device=dev)
        c.extend([len(p) - 1 for p in prompts])                  # the cache holds every token but the last one picked
        c.extend(to.LOOP_NODES)
        c.upload_state(MSL, to.LOOP_NODES)
        return c

    warm = Loop(dev, PagedKVCache(num_layers=1, num_kv_heads=1, page_size=P, max_pages=64, batch=len(prompts), kind="int4", device=dev), MSL)
    warm.cache.extend([len(p) - 1 for p in prompts])
    warm.cache.extend(to.LOOP_NODES)
    warm.step(0)                                                 # the kernels are loaded, by another cache
    loop = Loop(dev, new_cache(), MSL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for s in range(to.LOOP_STEPS):
            loop.step(s)
    for e in loop.emitted:
        e.fill_(0)
    graph.replay()
    torch.cuda.synchronize()
    return loop


def test_the_loop_with_a_paged_cache(dev):
    loop = paged_loop(dev, 64)
    total, fin = t_cpu.check_loop(0, loop.tokens, loop.total_len, loop.finished, loop.emitted_lists())
    c = loop.cache
    c.sync()
    for b, (n, f) in enumerate(zip(total, fin)):
        if not f:
            assert c.seq_lens[b] - c._announced[0][b] == n - 1, f"sequence {b}: the cache holds every committed token but the bonus"
    assert 0 in fin and c._announced[0] == to.LOOP_NODES


def test_the_history_stops_where_the_page_table_did(dev):
    """a pool too small for the last steps: the failed step still commits its verified tokens, no later one does"""
    loop = paged_loop(dev, 9)
    state = loop.cache.step_state.cpu().tolist()
    status, done, failed = state[0], state[1], state[3]
    assert status == _lib.KV_STEP["MM_KV_STEP_OUT_OF_PAGES"] and done == failed and 0 < failed < to.LOOP_STEPS - 1, state[:4]
    emitted = loop.emitted_lists()
    assert all(sum(e) > 0 for e in emitted[:failed + 1]) and all(sum(e) == 0 for e in emitted[failed + 1:]), emitted
    t_cpu.check_loop(0, loop.tokens, loop.total_len, loop.finished, emitted, steps=failed + 1, accepted=False)
    with pytest.raises(RuntimeError, match="OUT_OF_PAGES"):
        loop.cache.sync()

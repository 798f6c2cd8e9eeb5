"""GPU tests of the seeded uniform numbers (mixedgemm.uniform_rows; include/micromix_random.h).  The numbers are an integer function of
(seed, sub, pos, domain), so every comparison is equality against tests/random_oracle.py:
1 vectors     the interface vectors of tests/test_random_cpu.py, bit for bit
2 oracle      bits and out for 1 .. 4097 rows, every n that ends inside, at and past a block, a dense out and views with slack (whose
              sentinel stays), row_seq absent and given with entries at -1 and at batch, negative positions, the extreme seeds and 64
              seeds that differ in one bit, both ends of the domain; out == (bits >> 8) * 2^-24 exactly
3 far         2^24 rows of 16 streams, and a stream that starts past 2^31 elements
4 invariance  the numbers of (seed, sub, pos) in a batch of 1 at row 0 and in a batch of 65 at a shuffled row
5 loop        one hipGraph of 8 steps ngram_draft -> uniform_rows -> table lookup -> spec_sample_rows -> verify_greedy -> token_step over
              rows of one finite value (on which the sampler is exact), predicted token for token by random_oracle + spec_oracle +
              token_oracle: the same seeds give the same histories on a replay, a request samples the same tokens alone and among
              others, another seed changes that request and no other"""
import functools
import random

import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
import random_oracle as ro
import spec_oracle as sp
import token_oracle as to
import test_random_cpu as t_cpu

pytestmark = pytest.mark.gpu

i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
i64 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(dev)
SENTINEL = -5


def reference(bits):
    """(out, bits) as CPU tensors fp32 / int32 [n, rows] from the oracle's words"""
    w = np.array(bits, dtype=np.uint32).reshape(len(bits), -1)
    return torch.from_numpy((w >> 8).astype(np.float32) * np.float32(2.0 ** -24)), torch.from_numpy(w.view(np.int32).copy())


def run(dev, seed, pos, n, sub=None, row_seq=None, domain=0, ld=None):
    """uniform_rows into sentinel-filled stores of n + 1 streams, ld apart; returns (out, bits) on the CPU after checking that nothing
    outside [n, rows] was written"""
    rows = len(pos)
    ld = rows if ld is None else ld
    store = torch.full((n + 1, ld), float(SENTINEL), dtype=torch.float32, device=dev)
    wstore = torch.full((n + 1, ld), SENTINEL, dtype=torch.int32, device=dev)
    got = mixedgemm.uniform_rows(i64(seed, dev), i32(pos, dev), n=n, sub=None if sub is None else i32(sub, dev),
                                 row_seq=None if row_seq is None else i32(row_seq, dev), domain=domain, out=store[:n, :rows], bits=wstore[:n, :rows])
    torch.cuda.synchronize()
    assert rows == 0 or (got[0].data_ptr() == store.data_ptr() and got[1].data_ptr() == wstore.data_ptr())
    store, wstore = store.cpu(), wstore.cpu()
    assert bool((store[n] == SENTINEL).all()) and bool((wstore[n] == SENTINEL).all()), "a stream past n was written"
    assert bool((store[:, rows:] == SENTINEL).all()) and bool((wstore[:, rows:] == SENTINEL).all()), "the slack of ld_out was written"
    return store[:n, :rows], wstore[:n, :rows]


# ---- 1. the interface vectors ---------------------------------------------------------------------------------------------------------------
def test_the_interface_vectors(dev):
    for seed, pos, sub, domain, n, bits, u24 in t_cpu.INTERFACE_VECTORS:
        out, got = run(dev, [seed], [pos], n, [sub], None, domain)
        assert got[:, 0].tolist() == [ro.as_int32(w) for w in bits]
        assert (out[:, 0].double() * 2 ** 24).tolist() == [float(w >> 8) for w in bits]
        assert u24 is None or (out[:, 0].double() * 2 ** 24).tolist() == [float(x) for x in u24]
        fresh = mixedgemm.uniform_rows(i64([seed], dev), i32([pos], dev), n=n, sub=i32([sub], dev), domain=domain)      # allocated, dense, no bits
        assert isinstance(fresh, torch.Tensor) and fresh.is_contiguous() and torch.equal(fresh.cpu(), out)


# ---- 2. the oracle ---------------------------------------------------------------------------------------------------------------------------
SPECIAL_SEEDS = [0, -1, 2 ** 63 - 1, -2 ** 63] + [0x0123456789ABCDEF ^ (1 << b) for b in range(64)]
for _s in range(4, len(SPECIAL_SEEDS)):
    SPECIAL_SEEDS[_s] -= (SPECIAL_SEEDS[_s] >> 63) << 64                                      # as int64


def case_inputs(rows, with_seq, rng):
    """(seed, sub, row_seq, pos): without row_seq the batch is one short of the rows, so the last row is outside it"""
    pick_pos = lambda: rng.choice((0, -1, -2 ** 31, 2 ** 31 - 1, -rng.randrange(1, 100000), rng.randrange(0, 200000), rng.randrange(0, 200000)))
    pos = [pick_pos() for _ in range(rows)]
    if with_seq:
        seed = SPECIAL_SEEDS + [rng.randrange(-2 ** 63, 2 ** 63)]
        batch = len(seed)
        row_seq = [rng.randrange(0, batch) for _ in range(rows)]
        if rows >= 3:
            row_seq[rows // 2], row_seq[rows - 1] = -1, batch                                   # outside, on both sides
        sub = None
    else:
        batch = max(1, rows - 1)
        seed = (SPECIAL_SEEDS * (batch // len(SPECIAL_SEEDS) + 1))[:batch]                      # equal seeds: the positions and sub differ
        row_seq = None
        sub = [rng.choice((0, 1, -1, rng.randrange(-2 ** 31, 2 ** 31))) for _ in range(batch)]
    return seed, sub, row_seq, pos


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_bits_and_numbers_equal_the_oracle(dev, rows):
    rng = random.Random(rows)
    configs = [(False, 0xFFFFFFFF), (True, 0)] + ([(False, 0), (True, 0xFFFFFFFF)] if rows <= 257 else [])
    for with_seq, domain in configs:
        seed, sub, row_seq, pos = case_inputs(rows, with_seq, rng)
        want_u, want_bits = ro.uniform_rows(seed, pos, 16, sub, row_seq, domain)               # once: n streams are the first n of 16
        ref_out, ref_bits = reference(want_bits)
        assert ref_out.double().mul(2 ** 24).tolist() == [[float(x) for x in s] for s in want_u] and float(ref_out.max()) < 1.0
        outside = [r for r in range(rows) if not 0 <= (r if row_seq is None else row_seq[r]) < len(seed)]
        assert rows < 3 or outside, "precondition: a row outside the batch"
        assert all(want_bits[i][r] == 0 for i in range(16) for r in outside)
        for n in (1, 2, 3, 4, 5, 8, 15, 16):
            for ld in (rows, rows + 1, rows + 3):
                out, bits = run(dev, seed, pos, n, sub, row_seq, domain, ld)
                what = (rows, with_seq, hex(domain), n, ld)
                assert torch.equal(bits, ref_bits[:n]), what
                assert torch.equal(out, ref_out[:n]), what
                assert torch.equal(out, ((bits >> 8) & 0xFFFFFF).float() * 2.0 ** -24), what


def test_seeds_that_differ_in_one_bit_share_no_word(dev):
    seed, pos = SPECIAL_SEEDS, [12345] * len(SPECIAL_SEEDS)
    _, bits = run(dev, seed, pos, 16)
    assert bits.tolist() == [[ro.as_int32(w) for w in s] for s in ro.uniform_rows(seed, pos, 16)[1]]
    assert len(set(bits.flatten().tolist())) == bits.numel()


# ---- 3. far ------------------------------------------------------------------------------------------------------------------------------------
def test_two_to_the_24_rows(dev):
    rows, n = ro.MAX_ROWS, 16
    pos = torch.arange(-5, rows - 5, dtype=torch.int32, device=dev)
    seed = torch.arange(rows, dtype=torch.int64, device=dev) * 0x1E3779B97F4A7C15 - 2 ** 62      # wraps: seeds all over int64
    out, bits = mixedgemm.uniform_rows(seed, pos, n=n, domain=3, bits=True)
    torch.cuda.synchronize()
    assert torch.equal(out, ((bits >> 8) & 0xFFFFFF).float() * 2.0 ** -24) and float(out.max()) < 1.0
    at = [0, 1, 63, 64, 255, 256, 2 ** 16, 2 ** 23 - 1, 2 ** 23, rows - 257, rows - 2, rows - 1]
    seeds, got = seed[at].tolist(), bits[:, at].cpu()
    for c, r in enumerate(at):
        assert got[:, c].tolist() == [ro.as_int32(w) for w in ro.words(seeds[c], r - 5, 0, 3, n)], r
    with pytest.raises(RuntimeError, match="at most"):
        mixedgemm.uniform_rows(seed[:1], torch.zeros(rows + 1, dtype=torch.int32, device=dev))


def test_a_stream_behind_two_to_the_31_elements(dev):
    rows, n, ld = 300, 5, 2 ** 29 + 3
    need = n * ld * 4 + (1 << 30)
    if torch.cuda.mem_get_info(dev)[0] < need:
        pytest.skip(f"needs {need / 2 ** 30:.1f} GiB of device memory")
    assert (n - 1) * ld >= 2 ** 31
    store = torch.empty((n, ld), dtype=torch.float32, device=dev)       # out and bits are stored at one index: out alone, half the memory
    store[:, :rows + 8] = SENTINEL
    seed, pos = list(range(7, 7 + rows)), list(range(1000, 1000 + rows))
    out = mixedgemm.uniform_rows(i64(seed, dev), i32(pos, dev), n=n, out=store[:, :rows])
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), reference(ro.uniform_rows(seed, pos, n)[1])[0])
    assert bool((store[:, rows:rows + 8] == SENTINEL).all())


# ---- 4. batch invariance ------------------------------------------------------------------------------------------------------------------------
def test_the_numbers_do_not_depend_on_the_batch_or_the_row(dev):
    rng = random.Random(65)
    seed, sub, pos = -0x123456789ABCDEF, 3, 4321
    alone = mixedgemm.uniform_rows(i64([seed], dev), i32([pos], dev), n=16, sub=i32([sub], dev), domain=9, bits=True)
    seeds, subs = [rng.randrange(-2 ** 63, 2 ** 63) for _ in range(65)], [rng.randrange(0, 8) for _ in range(65)]
    slot = 41
    seeds[slot], subs[slot] = seed, sub
    order = list(range(65))
    rng.shuffle(order)                                           # row r holds sequence order[r]
    positions = [pos if s == slot else rng.randrange(0, 10000) for s in order]
    among = mixedgemm.uniform_rows(i64(seeds, dev), i32(positions, dev), n=16, sub=i32(subs, dev), row_seq=i32(order, dev), domain=9, bits=True)
    torch.cuda.synchronize()
    row = order.index(slot)
    assert row != 0 and torch.equal(among[1][:, row], alone[1][:, 0]) and torch.equal(among[0][:, row], alone[0][:, 0])
    assert alone[1][:, 0].tolist() == [ro.as_int32(w) for w in ro.words(seed, pos, sub, 9, 16)]
    same_row = mixedgemm.uniform_rows(i64(seeds, dev), i32([positions[order.index(s)] for s in range(65)], dev), n=16, sub=i32(subs, dev), domain=9, bits=True)
    assert torch.equal(same_row[1][:, slot], alone[1][:, 0])     # without row_seq: row 41 is sequence 41


# ---- 5. the sampled loop --------------------------------------------------------------------------------------------------------------------------
V, LD, STEPS, DOMAIN, TEMPERATURE = 64, 96, 8, 5, 0.8
ALPHABET, SET_SIZES = 6, (2, 2, 2, 3, 2, 2, 4, 5)


@functools.lru_cache(maxsize=None)
def successor_sets():
    """token t is followed by one of 2 to 5 tokens, all among the first ALPHABET: histories soon repeat, so the lookup drafts tokens
    that are accepted with probability 1 / (the size of the set)"""
    rng = random.Random(2)
    return tuple(tuple(sorted(rng.sample(range(ALPHABET), SET_SIZES[t % len(SET_SIZES)]))) for t in range(V))


@functools.lru_cache(maxsize=None)
def table_bits():
    """bf16 [V, V]: row t holds 1.5 on t's successors and -inf elsewhere, the rows on which test_spec_sample_gpu.py shows the rule exact"""
    return np.stack([sp.uniform_row(V, cols) for cols in successor_sets()])


def requests(variant):
    """five requests: (prompt, seed, sub, max_total, stop tokens); request 3 is the one the tests single out.  Variant 1 rewrites
    everything; variant 2 is variant 0 with another seed for request 2"""
    if variant == 1:
        return [([9, 8, 7, 9, 8], 77, 1, 40, [-1, -1]), ([1], -2 ** 63, 0, 9, [-1, -1]), ([5, 5, 5, 5, 5, 5, 5, 5, 5], 2 ** 63 - 1, 2, 96, [0, -1]),
                ([2, 3], 123456789, 0, 96, [-1, 4]), ([60, 61, 62], 0, 9, 30, [-1, -1])]
    base = [([3, 1, 4, 1, 5, 9, 2, 6], 0x5EED0001, 0, 96, [-1, -1]), ([7, 0, 7], 0x5EED0002, 0, 14, [-1, -1]),
            ([2, 7, 1, 8, 2, 8, 1, 8, 2, 8], -0x5EED0003, 0, 96, [-1, -1]), ([6, 2, 6, 3], 0x0123456789ABCDEF, 4, 30, [-1, -1]),
            ([33, 5], 0x5EED0005, 1, 96, [5, -1])]
    if variant == 2:
        base[2] = base[2][:1] + (0x5EED0033,) + base[2][2:]
    return base


NODES = (4, 3, 5, 4, 2)


@functools.lru_cache(maxsize=None)
def rollout(reqs_key, nodes):
    """the loop in Python integers: (tokens, total_len, finished, emitted per step) of `STEPS` steps"""
    reqs = reqs_key
    tokens = [list(p) + [-1] * (LD - len(p)) for p, *_ in reqs]
    total, finished = [len(r[0]) for r in reqs], [0] * len(reqs)
    seeds, subs, most, stops = [r[1] for r in reqs], [r[2] for r in reqs], [r[3] for r in reqs], [r[4] for r in reqs]
    indptr = [0]
    for n in nodes:
        indptr.append(indptr[-1] + n)
    T, emitted, bits = indptr[-1], [], table_bits()
    for _ in range(STEPS):
        d = to.ngram_draft(tokens, total, indptr, T, 1, 4)
        u24, _ = ro.uniform_rows(seeds, d["row_total_len"], 2, subs, d["row_seq"], DOMAIN)
        target = [sp.spec_row(bits[d["draft_tok"][t]], None, d["cand_tok"][t], u24[0][t] * 2.0 ** -24, u24[1][t] * 2.0 ** -24, TEMPERATURE)[0]
                  for t in range(T)]
        result = to.chain_verify(target, d["draft_tok"], d["root_tok"], indptr)
        emitted.append(to.token_step(tokens, total, finished, result, target, indptr, d["root_tok"], most, stops))
    return tokens, total, finished, emitted


def freeze(reqs):
    return tuple((tuple(p), seed, sub, most, tuple(stops)) for p, seed, sub, most, stops in reqs)


class Loop:
    """the buffers of one captured loop of STEPS sampled steps for len(nodes) requests, and the graph"""

    def __init__(self, dev, nodes):
        self.dev, self.nodes = dev, tuple(nodes)
        B = len(nodes)
        indptr = [0]
        for n in nodes:
            indptr.append(indptr[-1] + n)
        self.T = T = indptr[-1]
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        self.qo = i32(indptr, dev)
        self.table = torch.from_numpy(table_bits().view(np.int16)).to(dev).view(torch.bfloat16)
        self.tokens, self.total_len, self.finished, self.max_total, self.stops = z(B, LD), z(B), z(B), z(B), z(B, 2)
        self.seed, self.sub = torch.zeros(B, dtype=torch.int64, device=dev), z(B)
        self.outs = dict(draft_tok=z(T), root_tok=z(B), cand_tok=z(T), match_len=z(B), row_seq=z(T), row_total_len=z(T))
        self.u = torch.zeros((2, T), dtype=torch.float32, device=dev)
        self.logits = torch.zeros((T, V), dtype=torch.bfloat16, device=dev)
        self.temperature = torch.full((T,), TEMPERATURE, dtype=torch.float32, device=dev)
        self.target, self.accepted = z(T), z(T)
        self.ws = torch.empty(max(1, mixedgemm.spec_sample_rows_workspace_bytes(T, V)), dtype=torch.uint8, device=dev)
        self.result, self.moves = z(B, 66), (z(T), z(T))
        self.kv_indptr, self.last_page_len = i32(list(range(B + 1)), dev), i32(nodes, dev)      # one page of 4096 slots a sequence
        self.emitted = [z(B) for _ in range(STEPS)]
        self.load(requests(0)[:B])
        self.step(0)                                             # every kernel is loaded; the state is written again before a replay
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            for s in range(STEPS):
                self.step(s)

    def load(self, reqs):
        dev = self.dev
        rows = np.full((len(reqs), LD), -1, dtype=np.int32)
        for b, (p, *_rest) in enumerate(reqs):
            rows[b, :len(p)] = p
        self.tokens.copy_(i32(rows, dev))
        self.total_len.copy_(i32([len(r[0]) for r in reqs], dev))
        self.finished.zero_()
        self.seed.copy_(i64([r[1] for r in reqs], dev))
        self.sub.copy_(i32([r[2] for r in reqs], dev))
        self.max_total.copy_(i32([r[3] for r in reqs], dev))
        self.stops.copy_(i32([r[4] for r in reqs], dev))

    def step(self, s):
        d = mixedgemm.ngram_draft(self.tokens, self.total_len, self.qo, self.T, min_n=1, max_n=4, **self.outs)
        mixedgemm.uniform_rows(self.seed, d.row_total_len, n=2, sub=self.sub, row_seq=d.row_seq, domain=DOMAIN, out=self.u)
        torch.index_select(self.table, 0, d.draft_tok, out=self.logits)
        mixedgemm.spec_sample_rows(self.logits, None, d.cand_tok, self.u[0], self.u[1], temperature=self.temperature, out=self.target,
                                   accepted=self.accepted, workspace=self.ws)
        mixedgemm.verify_greedy(self.target, d.draft_tok, d.root_tok, self.qo, self.kv_indptr, self.last_page_len, 4096, result=self.result,
                                move_src=self.moves[0], move_dst=self.moves[1])
        mixedgemm.token_step(self.tokens, self.total_len, self.finished, self.result, self.target, self.qo, d.root_tok, self.max_total,
                             stop_tok=self.stops, emitted=self.emitted[s])

    def replay(self, reqs):
        """load, replay, and compare everything the loop commits with the oracle's rollout; returns the committed histories"""
        self.load(reqs)
        for e in self.emitted:
            e.fill_(-9)
        self.graph.replay()
        torch.cuda.synchronize()
        tokens, total, finished, emitted = rollout(freeze(reqs), self.nodes)
        got_total = self.total_len.cpu().tolist()
        assert got_total == total and self.finished.cpu().tolist() == finished
        assert [e.cpu().tolist() for e in self.emitted] == emitted
        got = self.tokens.cpu().tolist()
        histories = [row[:n] for row, n in zip(got, got_total)]
        assert histories == [row[:n] for row, n in zip(tokens, total)]
        return histories


@functools.lru_cache(maxsize=None)
def loop_of_five(dev):
    return Loop(dev, NODES)


def test_the_rollouts_the_loop_tests_rely_on():
    """on the oracle alone: drafts are accepted and rejected, sequences stop and run out, and the seed of request 2 matters to it"""
    base, other = rollout(freeze(requests(0)), NODES), rollout(freeze(requests(2)), NODES)
    emitted = base[3]
    per_request = [sum(e[b] for e in emitted) for b in range(5)]
    assert max(per_request) > STEPS, "no draft was ever accepted"
    assert any(0 < e[b] < NODES[b] for e in emitted for b in range(5)), "no draft was ever rejected"
    assert {0, to.STOPPED, to.LENGTH} <= set(base[2]), base[2]
    history = lambda r, b: r[0][b][:r[1][b]]
    assert history(base, 2) != history(other, 2) and all(history(base, b) == history(other, b) for b in (0, 1, 3, 4))
    for b, (prompt, *_rest) in enumerate(requests(0)):             # every committed token is a successor of the one before it
        h = history(base, b)
        assert all(h[i + 1] in successor_sets()[h[i]] for i in range(len(prompt) - 1, len(h) - 1))


def test_a_replay_with_the_same_seeds_leaves_the_same_histories(dev):
    loop = loop_of_five(dev)
    first = loop.replay(requests(0))
    rewritten = loop.replay(requests(1))                         # every prompt, seed, sub, limit and stop set rewritten in place
    again = loop.replay(requests(0))
    assert first == again and rewritten != first


def test_a_request_alone_and_among_others_commits_the_same_tokens(dev):
    among = loop_of_five(dev).replay(requests(0))[3]
    alone_loop = Loop(dev, NODES[3:4])
    alone = alone_loop.replay(requests(0)[3:4])[0]
    assert alone == among and len(alone) > len(requests(0)[3][0]) + STEPS // 2
    neighbours = requests(1)
    neighbours[3] = requests(0)[3]
    assert loop_of_five(dev).replay(neighbours)[3] == alone        # other neighbours at the same slot


def test_another_seed_changes_that_request_and_no_other(dev):
    loop = loop_of_five(dev)
    base, other = loop.replay(requests(0)), loop.replay(requests(2))
    assert base[2] != other[2] and all(base[b] == other[b] for b in (0, 1, 3, 4))

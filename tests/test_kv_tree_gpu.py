"""GPU tests of tree-masked attention over the paged KV cache and of keeping a path (mixedgemm.paged_prefill(tree_mask=),
mixedgemm.kv_move_rows, PagedKVCache.tree_mask / attend_new(tree=) / accept), for the three cache kinds.

1 chain   words (2 << j) - 1 give the BITS of the causal call: g in {1, 4, 16}, P in {1, 16, 24}, n_b in {1, 5, 63, 64}, a sequence of
          65 tokens whose words are garbage (it is causal whatever they say), and once through the split path with a workspace
2 oracle  random trees against tests/kv_tree_oracle.py within test_kvprefill_gpu.check's budget (2 bf16 ulps + 2^-8 max|V| over the
          attended tokens: the arithmetic is mm_paged_prefill's, so the bound is): the new region starting at, straddling and
          following a 64-token kv tile edge; g = 16 (a tree over several query tiles); a tree across a split-KV chunk edge with a
          NaN-filled workspace; bits above j set (they change nothing, bit for bit); word 0 at base 0 (o == 0)
3 exact   every head of every query names the one token it must return, |o - V[target]| <= 2^-20 as in tests/kv_exact_cases.py, while a
          non-ancestor in a LOWER slot carries a key that scores 45 nats higher: the causal call returns that one (asserted too)
4 moves   kv_move_rows against the numpy oracle over a whole cache of random bytes
5 class   extend / append_rope at depth positions / attend_new(tree=) / accept / extend(1) / append / attend, bit-equal to a twin
          cache that only ever saw the accepted tokens; one member of a forked pair verifies a tree, the other stays untouched
6 graph   append + attend_new(tree=) captured once, replayed with two trees of the same T

No bound here comes from what a kernel produced."""
import numpy as np
import pytest
import torch

from micromix_amd import mixedgemm
from micromix_amd.kvcache import PagedKVCache
import kv_exact_cases as kc
import kv_fp8_oracle as fo
import kv_oracle as ko
import kv_tree_oracle as kto
import test_kvprefill_gpu as t_pre

pytestmark = pytest.mark.gpu

KINDS = ["int4", "bf16", "fp8_e4m3"]
L, LAYER = 2, 1
U64 = (1 << 64) - 1
TREE21 = [-1] + [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4


def i32(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)


def words_tensor(words, dev):
    return torch.tensor([w - (1 << 64) if w >> 63 else w for w in words], dtype=torch.int64).to(dev)


def bits(t):
    return t.detach().contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def bf(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).to(dev)


def empty_cache(kind, max_pages, Hkv, P, dev, layers=L):
    shape = (max_pages, layers, 2, Hkv, P)
    if kind == "bf16":
        return torch.zeros(shape + (128,), dtype=torch.bfloat16, device=dev), None
    return (torch.zeros(shape + (64 if kind == "int4" else 128,), dtype=torch.uint8, device=dev),
            torch.zeros(shape + (2,), dtype=torch.float16, device=dev))


def build(kind, prior, new, Hq, Hkv, P, dev, seed, K=None, V=None, q=None):
    """a cache whose layer LAYER holds prior[b] + new[b] tokens per sequence (kv_append; Gaussian unless K, V are given), shuffled pages"""
    rng = np.random.default_rng(seed)
    lens = [a + n for a, n in zip(prior, new)]
    indptr, indices, last, max_pages = kc.page_table(lens, P, seed)
    data, param = empty_cache(kind, max_pages, Hkv, P, dev)
    tbl = [i32(a, dev) for a in (indptr, indices, last)]
    T = sum(lens)
    k = bf(rng.standard_normal((T, Hkv, 128)) if K is None else K, dev)
    v = bf(rng.standard_normal((T, Hkv, 128)) * 0.5 if V is None else V, dev)
    mixedgemm.kv_append(data, param, *tbl, k, v, i32(kc.indptr_of(lens), dev), LAYER)
    qo = kc.indptr_of(new)
    qq = bf(rng.standard_normal((int(qo[-1]), Hq, 128)) * 2.0 if q is None else q, dev)
    return dict(kind=kind, data=data, param=param, tbl=tbl, tbl_h=(indptr, indices, last), qo=qo, qo_d=i32(qo, dev), q=qq, msl=max(lens),
                prior=list(prior), new=list(new))


def host(c):
    """the cache as the oracles take it: int4 codes + params, or bf16 bits (fp8: the bits of its dequantized values)"""
    if c["kind"] == "bf16":
        return c["data"].cpu().view(torch.int16).numpy().view(np.uint16).copy(), None
    data, param = c["data"].cpu().numpy().copy(), c["param"].cpu().numpy().copy()
    return (data, param) if c["kind"] == "int4" else (fo.dequantize(data, param), None)


def tree_call(c, words, msl=None, workspace=None):
    return mixedgemm.paged_prefill(c["q"], c["data"], c["param"], *c["tbl"], c["qo_d"], LAYER, c["msl"] if msl is None else msl,
                                   workspace=workspace, tree_mask=words_tensor(words, c["q"].device))


def causal_call(c, msl=None, workspace=None):
    return mixedgemm.paged_prefill(c["q"], c["data"], c["param"], *c["tbl"], c["qo_d"], LAYER, c["msl"] if msl is None else msl,
                                   workspace=workspace)


def same_bits(a, b, what):
    a, b = bits(a).astype(np.int64), bits(b).astype(np.int64)
    bad = a != b
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {tuple(int(i) for i in np.argwhere(bad)[0])}: "
                           f"{int(a[bad][0]):#06x} vs {int(b[bad][0]):#06x}")


def against_oracle(c, o, words, what):
    hd, hp = host(c)
    qb = bits(c["q"])
    want = kto.attention(qb, hd, hp, *c["tbl_h"], c["qo"], words, LAYER)
    vm = kto.vmax(qb.shape, hd, hp, *c["tbl_h"], c["qo"], words, LAYER)
    t_pre.check(o, want, vm, what)
    return want


def random_words(rng, new):
    out = []
    for n in new:
        out += kto.tree_words([int(rng.integers(-1, i)) for i in range(n)])[0] if n <= 64 else [int(x) for x in rng.integers(0, 1 << 62, n)]
    return out


# ---- 1. a chain is the causal mask, bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_chain_words_give_the_bits_of_the_causal_call(dev, kind):
    prior, new = [0, 37, 64, 100, 7, 0], [1, 5, 63, 64, 65, 64]
    rng = np.random.default_rng(1)
    words = [w for n in new for w in (kto.chain_words(n) if n <= 64 else [int(x) for x in rng.integers(0, 1 << 62, n)])]
    for g, Hkv in ((1, 4), (4, 2), (16, 1)):
        for P in (1, 16, 24):
            c = build(kind, prior, new, g * Hkv, Hkv, P, dev, seed=10 * g + P)
            assert mixedgemm.paged_prefill_workspace_bytes(sum(new), len(new), g * Hkv, Hkv, c["msl"]) == 0
            got, want = tree_call(c, words), causal_call(c)
            torch.cuda.synchronize()
            same_bits(got, want, f"{kind} g={g} P={P}")
            assert int(torch.count_nonzero(want.float())) > 0


@pytest.mark.parametrize("kind", KINDS)
def test_chain_words_through_the_split_path(dev, kind):
    """Hkv = 1 and a large bound: several kv chunks, the partials in a workspace of mm_paged_prefill_workspace_bytes, the merge launch"""
    prior, new, Hq, Hkv, bound = [700, 0, 300], [64, 5, 65], 4, 1, 1 << 16
    c = build(kind, prior, new, Hq, Hkv, 16, dev, seed=77)
    need = mixedgemm.paged_prefill_workspace_bytes(sum(new), len(new), Hq, Hkv, bound)
    assert need > 0, "must take the split path"
    ws = [torch.full((need,), 0xFF, dtype=torch.uint8, device=dev) for _ in range(2)]
    words = kto.chain_words(64) + kto.chain_words(5) + [0xDEADBEEF] * 65
    got, want = tree_call(c, words, bound, ws[0]), causal_call(c, bound, ws[1])
    torch.cuda.synchronize()
    same_bits(got, want, kind)
    against_oracle(c, got, words, kind)


# ---- 2. random trees against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_random_trees_against_the_oracle(dev, kind):
    """n = 9 new tokens at base 0, 60, 64 and 1000 (the new region starts at, straddles and follows a kv tile edge), a 65-token chain
    and a 40-node tree next to them; then g = 16, where a query tile holds 4 tokens and the 40-node tree spans ten of them"""
    rng = np.random.default_rng(21)
    prior, new = [0, 60, 64, 1000, 3, 100], [9, 9, 9, 9, 65, 40]
    for g, Hkv, P in ((4, 2, 16), (16, 1, 24)):
        c = build(kind, prior, new, g * Hkv, Hkv, P, dev, seed=30 + g)
        words = random_words(rng, new)
        o = tree_call(c, words)
        # bits above j change nothing: the kernel ANDs them away
        high = [w | (U64 << (j + 1) & U64) for n, a0 in zip(new, c["qo"]) for j, w in enumerate(words[a0:a0 + n])]
        o_high = tree_call(c, high)
        torch.cuda.synchronize()
        against_oracle(c, o, words, f"{kind} g={g}")
        same_bits(o_high, o, f"{kind} g={g}: bits above j")
        assert not torch.equal(o, causal_call(c)), "the trees must differ from chains"


@pytest.mark.parametrize("kind", KINDS)
def test_word_zero_at_base_zero_gives_zeros(dev, kind):
    c = build(kind, [0, 5], [6, 6], 8, 2, 16, dev, seed=41)
    words = [0, 1, 0, 0b101, 0, 0b100000] + [0] * 6
    o = tree_call(c, words)
    torch.cuda.synchronize()
    for j in (0, 2, 4):
        assert int(torch.count_nonzero(o[j].float())) == 0, j               # attends nothing: o = 0, not NaN
    assert int(torch.count_nonzero(o[1].float())) > 0 and int(torch.count_nonzero(o[6:].float())) > 0     # base 5: the committed tokens
    against_oracle(c, o, words, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_tree_across_a_split_chunk_edge_with_a_nan_workspace(dev, kind):
    """bound 1024 with little other work gives 4 chunks of 256 tokens (asserted from the workspace size): the trees at base 252, 508
    and 764 have nodes on both sides of a chunk edge, the one at base 256 starts on it"""
    prior, new, Hq, Hkv, bound = [252, 508, 764, 256], [9, 9, 9, 9], 4, 1, 1024
    c = build(kind, prior, new, Hq, Hkv, 16, dev, seed=51)
    need = mixedgemm.paged_prefill_workspace_bytes(sum(new), len(new), Hq, Hkv, bound)
    tiles = sum(new) // (64 // (Hq // Hkv)) + len(new)
    assert need == tiles * Hkv * 4 * 64 * 130 * 4, "expected 4 chunks (of 256 tokens)"
    words = random_words(np.random.default_rng(52), new)
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)           # every float a NaN
    o = tree_call(c, words, bound, ws)
    torch.cuda.synchronize()
    against_oracle(c, o, words, kind)


# ---- 3. exact answers --------------------------------------------------------------------------------------------------------------
def caterpillar(m):
    """2 m + 1 nodes: slot 0 the root; for k = 1 .. m slot 2 k - 1 a leaf (the decoy) and slot 2 k the next spine node, both children of
    spine node k - 1.  The decoy sits in the LOWER slot, is no ancestor of anything, and carries its sibling's key times 1.5"""
    parents = [-1]
    for k in range(1, m + 1):
        parents += [2 * (k - 1), 2 * (k - 1)]
    return parents


def exact_case(g, Hkv, P, bases, m):
    """K, V, q, the expected rows and the rows a causal kernel gets wrong.  Committed and spine tokens hold the code u(pos) as K, decoy
    2 k - 1 holds 1.5 u(pos of spine node 2 k); V names (sequence, position, head).  A head's query is 8 u(its target): spine node k
    asks, head by head, for itself, its parent, the root (the first new slot), the last committed token and then ancestors and
    committed tokens at random; a decoy asks for itself (through its sibling's code), then the same list from its parent on"""
    Hq, n, rng = g * Hkv, 2 * m + 1, np.random.default_rng(900 + g)
    parents = caterpillar(m)
    lens = [a + n for a in bases]
    starts = np.concatenate([[0], np.cumsum(lens)])
    code = np.concatenate([np.arange(ln) for ln in lens])                   # the position whose code a token's K holds ...
    gain = np.ones(len(code), dtype=np.float32)                             # ... and times what
    target = np.zeros((len(bases) * n, Hq), dtype=np.int64)                 # the position each (query, head) must return
    fooled = np.zeros((len(bases) * n, Hq), dtype=bool)
    for b, a in enumerate(bases):
        for k in range(1, m + 1):
            code[starts[b] + a + 2 * k - 1], gain[starts[b] + a + 2 * k - 1] = a + 2 * k, 1.5
        for j in range(n):
            up = [2 * i for i in range((j - 1) // 2 if j % 2 else j // 2 - 1, -1, -1)]          # up the spine to the root
            want = [a + j, a + (up[0] if up else j), a] + ([a - 1] if a else [a])
            while len(want) < Hq:
                want.append(a + int(rng.choice([j] + up)) if rng.random() < 0.5 or not a else int(rng.integers(0, a)))
            target[b * n + j] = want[:Hq]
            # a causal kernel sees the decoy one slot below every spine node but the root
            fooled[b * n + j] = [w - a >= 2 and (w - a) % 2 == 0 for w in want[:Hq]]
    seq = np.repeat(np.arange(len(bases)), lens)
    K = np.stack([kc.codebook(h)[code] for h in range(Hkv)], 1).astype(np.float32) * gain[:, None, None]
    V = np.concatenate([kc.v_grid(b, np.arange(ln)[:, None], np.arange(Hkv)[None, :]) for b, ln in enumerate(lens)])
    kvh = np.arange(Hq) // g
    tok = starts[np.repeat(np.arange(len(bases)), n)][:, None] + target     # flat token index of each target
    q = np.stack([8.0 * kc.codebook(h)[code[tok[:, hq]]] for hq, h in enumerate(kvh)], 1).astype(np.float32)
    expect = V[tok, kvh[None, :]].astype(np.float64)
    words = [w for _ in bases for w in kto.tree_words(parents)[0]]
    return dict(K=K, V=V, q=q, expect=expect, fooled=fooled, words=words, new=[n] * len(bases), lens=lens, Hq=Hq, target=target)


def lead_nats(c, case, causal):
    """the least lead, in nats, of each (query, head)'s target over every other token it attends, from the cache's own (dequantized)
    values in fp64; causal: under the causal mask instead, -inf where the target does not lead"""
    hd, hp = host(c)
    q = kc.to_bf16(case["q"]).astype(np.float64)
    g = case["Hq"] // hd.shape[3]
    words = kto.chain_words(case["new"][0]) * len(case["new"]) if causal else case["words"]
    out, n = np.zeros(q.shape[:2]), case["new"][0]
    for b in range(len(case["new"])):
        Kd, _ = ko.dequantized(hd, hp, *c["tbl_h"], LAYER, b)
        keep = kto.keep_matrix(case["lens"][b], n, words[b * n:(b + 1) * n])
        for j in range(n):
            for hq in range(case["Hq"]):
                s = Kd[hq // g] @ q[b * n + j, hq] / np.sqrt(128.0)
                tgt = case["target"][b * n + j, hq]
                assert keep[j, tgt], "a target the query does not attend"
                others = keep[j].copy()
                others[tgt] = False
                out[b * n + j, hq] = s[tgt] - (s[others].max() if others.any() else -np.inf)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("g, Hkv, P, m", [(4, 2, 16, 16), (16, 1, 24, 16), (1, 4, 1, 31)])
def test_every_head_returns_the_ancestor_it_names(dev, kind, g, Hkv, P, m):
    """bases 0, 50, 64 and 1000 with 33 (63) nodes: targets and decoys on the first and the last new slot, on both sides of the kv tile
    edge at 64 (base 50: decoy 63, spine 64) and of page edges (P = 16: 64 | 80; P = 24: 72 | 1008)"""
    bases = [0, 50, 64, 1000]
    case = exact_case(g, Hkv, P, bases, m)
    c = build(kind, bases, case["new"], g * Hkv, Hkv, P, dev, seed=60 + g, K=case["K"], V=case["V"], q=case["q"])
    lead = lead_nats(c, case, causal=False)
    assert lead.min() >= kc.MARGIN_NATS, f"precondition: a target leads by only {lead.min():.1f} nats"
    lost = lead_nats(c, case, causal=True)
    assert case["fooled"].any() and lost[case["fooled"]].max() <= -kc.MARGIN_NATS, "precondition: the decoy must win under the causal mask"
    o, o_causal = tree_call(c, case["words"]), causal_call(c)
    torch.cuda.synchronize()
    n, Hq = case["new"][0], case["Hq"]
    label = lambda i: f"seq {i // (n * Hq)} (base {bases[i // (n * Hq)]}) node {i // Hq % n} head {i % Hq}"
    got = o.float().cpu().numpy().astype(np.float64)
    msg = kc.describe_mismatch(got.reshape(-1, 128), case["expect"].reshape(-1, 128), label, kc.EXACT_BOUND)
    assert msg is None, f"{kind} g={g} P={P}: {msg}"
    wrong = np.abs(o_causal.float().cpu().numpy().astype(np.float64) - case["expect"]).max(-1) > 0.25
    assert wrong[case["fooled"]].all(), "the causal call must return the decoy on these rows: the test would not see a causal kernel"


# ---- 4. moves ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("P", [1, 16, 24])
def test_move_rows_against_the_oracle_over_a_poisoned_cache(dev, kind, P):
    rng = np.random.default_rng(70 + P)
    Hkv, layers = 2, 3
    lens = [40, 150, 30, 60, 20]
    npg = [-(-n // P) for n in lens]
    max_pages = sum(npg) + 2
    indptr = kc.indptr_of(npg)
    indices = rng.permutation(max_pages)[: sum(npg)].astype(np.int32)
    indices[indptr[3] + npg[3] - 1] = -1                                    # the last page of sequence 3: released
    width = {"int4": 64, "bf16": 256, "fp8_e4m3": 128}[kind]
    raw = rng.integers(0, 256, (max_pages, layers, 2, Hkv, P, width), dtype=np.uint8)          # every byte of the cache is poison
    praw = rng.integers(0, 1 << 16, (max_pages, layers, 2, Hkv, P, 2)).astype(np.uint16)
    if kind == "bf16":
        data, param = torch.from_numpy(raw.copy()).to(dev).view(torch.bfloat16), None
    else:
        data, param = torch.from_numpy(raw.copy()).to(dev), torch.from_numpy(praw.view(np.int16).copy()).to(dev).view(torch.float16)
    moves = [
        # packing a path down: every destination but the first is another move's source; then a swap and a rotation
        [(s, d) for d, s in enumerate([1, 2, 5, 9, 10, 17, 33, 39])] + [(20, 21), (21, 20)] + [(25, 26), (26, 27), (27, 25)],
        [(149 - i, i) for i in range(70)],                                  # 70 moves: those past the 64th are skipped
        [],                                                                 # a sequence without moves
        [(3, 4), (-1, 5), (6, -2), (60, 7), (8, 1 << 20), (59, 9), (10, 59), (11, 11), (12, 13)],   # out of range, a released page, src == dst
        [(19, 0)],
    ]
    mptr = kc.indptr_of([len(m) for m in moves])
    src = np.array([s for m in moves for s, _ in m], dtype=np.int32)
    dst = np.array([d for m in moves for _, d in m], dtype=np.int32)
    want, pwant = raw.copy(), praw.copy()
    kto.move_rows(want, None if kind == "bf16" else pwant, indptr, indices, mptr, src, dst)
    assert (want != raw).any() and not np.array_equal(want[indices[indptr[1]]], raw[indices[indptr[1]]])
    mixedgemm.kv_move_rows(data, param, i32(indptr, dev), i32(indices, dev), i32(mptr, dev), i32(src, dev), i32(dst, dev))
    torch.cuda.synchronize()
    got = data.view(torch.uint8).cpu().numpy().reshape(raw.shape)
    assert np.array_equal(got, want), f"{int((got != want).sum())} code bytes differ"
    if param is not None:
        assert np.array_equal(param.view(torch.int16).cpu().numpy().view(np.uint16), pwant), "params differ"
    # nothing outside the destination rows changed, and the skipped moves left their destinations alone
    touched = np.zeros((max_pages, P), dtype=bool)
    for b, m in enumerate(moves):
        for s, d in m[:64]:
            if s != d and min(s, d) >= 0 and max(s, d) < npg[b] * P and indices[indptr[b] + s // P] >= 0 and indices[indptr[b] + d // P] >= 0:
                touched[indices[indptr[b] + d // P], d % P] = True
    changed = (got != raw).any(axis=(1, 2, 3, 5))
    assert not (changed & ~touched).any() and int(touched.sum()) == 13 + 64 + 2 + 1
    # an empty call and a call whose every move is skipped are fine
    mixedgemm.kv_move_rows(data, param, i32(indptr, dev), i32(indices, dev), i32(np.zeros(6), dev), i32([], dev), i32([], dev))
    torch.cuda.synchronize()
    assert np.array_equal(data.view(torch.uint8).cpu().numpy().reshape(raw.shape), want)


# ---- 5. the class, end to end ------------------------------------------------------------------------------------------------------------
def rope_rows(positions, dev):
    inv = 1.0 / (500000.0 ** (torch.arange(0, 128, 2).float() / 128))
    ang = torch.tensor(positions, dtype=torch.float32)[:, None] * inv
    return (torch.cat([ang.cos(), ang.cos()], -1).to(torch.bfloat16).to(dev), torch.cat([ang.sin(), ang.sin()], -1).to(torch.bfloat16).to(dev))


def logical_rows(cache, b):
    pos = torch.arange(cache.seq_lens[b])
    pages, slot = torch.tensor(cache._pages[b])[pos // cache.page_size], pos % cache.page_size
    data = cache.kv_data.cpu().view(torch.uint8).reshape(*cache.kv_data.shape[:5], -1)[pages, :, :, :, slot]
    param = None if cache.kv_param is None else cache.kv_param.cpu().view(torch.int16)[pages, :, :, :, slot]
    return data, param


@pytest.mark.parametrize("kind", KINDS)
def test_verify_a_tree_accept_a_path_and_go_on_like_a_twin(dev, kind):
    """sequence 2 is a fork of sequence 0 (20 tokens, P = 16: a partly filled shared page) and verifies the 21-node tree, sequence 1 a
    chain of 3, sequence 0 nothing.  After accept([..]) both caches decode one more token: same bits, same rows, same page counts"""
    Hq, Hkv, P, B = 8, 2, 16, 3
    rng = np.random.default_rng(80)
    rnd = lambda n, h: bf(rng.standard_normal((n, h, 128)), dev)
    new, paths, parents = [0, 3, 21], [None, [0, 1], [0, 1, 6]], [None, None, TREE21]
    prompt = [rnd(27, h) for h in (Hq, Hkv, Hkv)]
    draft = [rnd(24, h) for h in (Hq, Hkv, Hkv)]
    step = [rnd(3, h) for h in (Hq, Hkv, Hkv)]
    picked = [0, 1] + [3 + i for i in paths[2]]                             # the accepted tokens' rows of `draft`
    outs = []
    for twin in (False, True):
        c = PagedKVCache(L, Hkv, P, 32, B, kind=kind, device=dev)
        c.extend([20, 7, 0])
        cos, sin = rope_rows(list(range(20)) + list(range(7)), dev)
        for layer in range(L):
            c.append_rope(layer, *prompt, cos, sin)
        c.fork(0, 2)
        base = list(c.seq_lens)
        if twin:
            c.extend([0, 2, 3])
            cos, sin = rope_rows([7, 8, 20, 21, 22], dev)
            for layer in range(L):
                c.attend_new(layer, c.append_rope(layer, *(t[picked] for t in draft), cos, sin))
        else:
            c.extend(new)
            assert c._pages[2][-2] != c._pages[0][-1] and c._ref[c._pages[0][-1]] == 1, "the copy-on-write comes first"
            before = logical_rows(c, 0)
            mask, depths = c.tree_mask(parents)
            assert depths[2] == [0] + [1] * 4 + [2] * 16
            cos, sin = rope_rows([base[b] + d for b in range(B) for d in depths[b]], dev)
            for layer in range(L):
                o = c.attend_new(layer, c.append_rope(layer, *draft, cos, sin), tree=mask)
            c.accept(paths)
            after = logical_rows(c, 0)
            assert torch.equal(before[0], after[0]) and (before[1] is None or torch.equal(before[1], after[1])), "the other member changed"
        c.extend(1)
        for layer in range(L):
            c.append(layer, step[1], step[2])
        outs.append((c, [c.attend(layer, step[0]) for layer in range(L)]))
    torch.cuda.synchronize()
    (ours, o_ours), (twin, o_twin) = outs
    assert ours.seq_lens == twin.seq_lens == [21, 10, 24]
    assert ours.pages_in_use == twin.pages_in_use and sorted(ours._ref) == sorted(twin._ref) and ours._pages == twin._pages
    for layer in range(L):
        same_bits(o_ours[layer], o_twin[layer], f"{kind} layer {layer}")
    for b in range(B):
        (d0, p0), (d1, p1) = logical_rows(ours, b), logical_rows(twin, b)
        assert torch.equal(d0, d1) and (p0 is None or torch.equal(p0, p1)), f"rows of sequence {b}"


# ---- 6. one graph, two trees -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_graph_replays_with_another_tree_in_the_same_tensor(dev, kind):
    B, Hq, Hkv, n, bound = 2, 8, 2, 12, 512
    cache = PagedKVCache(1, Hkv, 16, 64, B, kind=kind, device=dev)
    rng = np.random.default_rng(90)
    rnd = lambda m, h: bf(rng.standard_normal((m, h, 128)), dev)
    cache.extend([70, 9])
    cache.append(0, rnd(79, Hkv), rnd(79, Hkv))
    sq, sk, sv = rnd(B * n, Hq), rnd(B * n, Hkv), rnd(B * n, Hkv)
    cache.extend(n)
    trees = [[[-1, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6, 7], None], [[-1, -1, 0, 1, 2, 2, 4, 5, 5, 8, 8, 10], [-1] + [0] * 11]]
    mask = cache.tree_mask(trees[0])[0]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        cache.append(0, sk, sv)
        cache.attend_new(0, sq, max_seq_len=bound, tree=mask)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cache.append(0, sk, sv)
        out = cache.attend_new(0, sq, max_seq_len=bound, tree=mask)
    got = []
    for step, tree in enumerate(trees):
        if step:
            cache.accept([[0, 2, 5], [0, 1]])                             # a path of the first tree; then the next draft
            cache.extend(n)
        mask.copy_(cache.tree_mask(tree)[0])
        for t in (sq, sk, sv):
            t.copy_(rnd(*t.shape[:2]))
        graph.replay()
        torch.cuda.synchronize()
        got.append(out.clone())
        eager = cache.attend_new(0, sq, max_seq_len=bound, tree=mask)
        torch.cuda.synchronize()
        same_bits(got[-1], eager, f"replay {step}")
        c = dict(kind=kind, data=cache.kv_data, param=cache.kv_param, q=sq, qo=cache.append_indptr.cpu().numpy(),
                 tbl_h=(cache.kv_indptr.cpu().numpy(), cache.kv_indices.cpu().numpy(), cache.last_page_len.cpu().numpy()))
        hd, hp = host(c)
        words = [int(x) & U64 for x in mask.tolist()]
        want = kto.attention(bits(sq), hd, hp, *c["tbl_h"], c["qo"], words, 0)
        t_pre.check(got[-1], want, kto.vmax(sq.shape, hd, hp, *c["tbl_h"], c["qo"], words, 0), f"replay {step}")
    assert cache.seq_lens == [70 + 3 + n, 9 + 2 + n]

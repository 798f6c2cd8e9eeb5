"""GPU tests of mixedgemm.spec_sample_rows and chain_candidates.  The reference is tests/spec_oracle.py: the rule of
include/micromix_spec.h in Python integers, and for Gaussian rows the set of answers that sample_oracle.py's bound on a mass admits.
Every comparison is exact unless said otherwise; tests/test_spec_sample_cpu.py proves the preconditions from the oracle alone.

1 exact      rows that hold one finite value and -inf: the target uniform on a set A, the draft on a set B, |A|, |B| in {4, 8}, two
             tokens shared, members on both sides of every part edge: the boundary pair of u_accept, what is always accepted and always
             rejected, and the distribution test -- every x of B against a grid of (u_accept, u_resample) returns every token of A
             equally often
2 one-hot    draft_logits=None and a draft row in the greedy case
3 equalities rows without a candidate equal sample_rows, greedy rows equal argmax_rows, the draft being the target accepts every
             candidate the target keeps, out= and accepted= are written in place
4 layout     pointer offsets 0 .. 7 and odd row distances of the two matrices independently, NaN outside the rows, a workspace of 0xFF
             bytes, and the same bits per row from another grid of rows
5 Gaussian   vocab 20 000, the draft the target plus noise: every decision and every token is admissible
6 chains     chain_candidates -> spec_sample_rows -> verify_greedy equals the oracle's walk, eagerly and as one replayed hipGraph

No bound here comes from what a kernel produced."""
import numpy as np
import pytest
import torch

from micromix_amd import _lib, mixedgemm
import sample_oracle as so
import spec_oracle as sp

pytestmark = pytest.mark.gpu

C = _lib.MM_ARGMAX_CHUNK
ROWS = 16                                                    # the most rows of one call here
TOP = 1.0 - 2.0 ** -24
i32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
f32 = lambda a, dev: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def poisoned_ws(rows, vocab, dev):
    return torch.full((mixedgemm.spec_sample_rows_workspace_bytes(rows, vocab),), 0xFF, dtype=torch.uint8, device=dev)


def from_bits(bits, dev, ld=None, offset=0):
    """bf16 [rows, vocab] on the device at `offset` elements into its buffer, rows ld apart; every element outside the rows is NaN"""
    rows, vocab = bits.shape
    ld = vocab if ld is None else ld
    full = np.full(offset + rows * ld + 8, 0x7FC0, dtype=np.uint16)
    body = full[offset: offset + rows * ld].reshape(rows, ld)
    body[:, :vocab] = bits
    buf = torch.from_numpy(full.view(np.int16)).to(dev).view(torch.bfloat16)
    return buf[offset: offset + rows * ld].view(rows, ld)[:, :vocab]


def opt(a, kind, dev):
    return None if a is None else kind(a, dev)


def call(dev, bits, draft, cand, ua, ur, T=None, k=None, p=None, q=None, ld=None, dld=None, offset=0, doffset=0):
    """(out, accepted) as lists, over a workspace of 0xFF bytes"""
    rows, vocab = bits.shape
    x = from_bits(bits, dev, ld, offset)
    d = None if draft is None else from_bits(draft, dev, dld, doffset)
    out, acc = mixedgemm.spec_sample_rows(x, d, i32(cand, dev), f32(ua, dev), f32(ur, dev), temperature=opt(T, f32, dev), top_k=opt(k, i32, dev),
                                          top_p=opt(p, f32, dev), min_p=opt(q, f32, dev), workspace=poisoned_ws(rows, vocab, dev))
    torch.cuda.synchronize()
    assert out.dtype == acc.dtype == torch.int32 and tuple(out.shape) == tuple(acc.shape) == (rows,)
    return out.tolist(), acc.tolist()


def oracle(bits, draft, cand, ua, ur, T=None, k=None, p=None, q=None):
    pick = lambda a, r, default: default if a is None else a[r]
    rows = [sp.spec_row(bits[r], None if draft is None else draft[r], int(cand[r]), ua[r], ur[r], pick(T, r, 1.0), pick(k, r, None),
                        pick(p, r, None), pick(q, r, None)) for r in range(len(bits))]
    return [o for o, _ in rows], [a for _, a in rows]


def in_chunks(cases, n=ROWS):
    return [cases[i:i + n] for i in range(0, len(cases), n)]


# ---- 1. the exact family -----------------------------------------------------------------------------------------------------------------
def exact_cases(A, B):
    """(x, u_accept, u_resample): the boundary pair and the ends of u for every token of B, then the distribution grid"""
    cases = [(x, ua, ur) for x in B for ua, ur in ((0.5 - 2.0 ** -24, 0.3), (0.5, 0.3), (0.0, 0.0), (TOP, TOP), (1.0, 1.0))]
    n, n2 = 2, 6                                             # tests/test_spec_sample_cpu.py: DIST_GRID
    grid = [(x, (j + 0.5) / n, (k + 0.5) / n2) for x in B for j in range(n) for k in range(n2)]
    return cases, grid


@pytest.mark.parametrize("vocab", [C - 1, C, C + 1, 2 * C + 5])
@pytest.mark.parametrize("a, b", [(8, 4), (4, 8), (4, 4), (8, 8)])
def test_the_exact_family(dev, vocab, a, b):
    A, B = sp.exact_sets(vocab, a, b)
    tb, db = sp.uniform_row(vocab, A), sp.uniform_row(vocab, B)
    shared, only_b = set(A) & set(B), set(B) - set(A)
    cases, grid = exact_cases(A, B)
    tokens = []
    for which, chunk in enumerate(in_chunks(cases + grid)):
        n = len(chunk)
        bits, draft = np.tile(tb, (n, 1)), np.tile(db, (n, 1))
        cand, ua, ur = [c[0] for c in chunk], np.float32([c[1] for c in chunk]), np.float32([c[2] for c in chunk])
        # every other call under filters that keep the one class whole: the select runs, the answers do not move
        par = dict(T=np.float32([0.7] * n), k=[2] * n, p=np.float32([0.5] * n), q=np.float32([0.5] * n)) if which % 2 else {}
        got = call(dev, bits, draft, cand, ua, ur, ld=vocab + 3, dld=vocab + 5, offset=which % 8, doffset=(3 * which + 1) % 8, **par)
        want = oracle(bits, draft, cand, ua, ur, **par)
        assert got == want, (vocab, a, b, which, [(c, g, w) for c, g, w in zip(chunk, zip(*got), zip(*want)) if g != w][:4])
        for (x, u_a, _), tok, acc in zip(chunk, *got):
            if x in only_b:
                assert acc == 0, "a token the target gives no mass is always rejected"
            if x in shared and b >= a:
                assert (tok, acc) == (x, 1), "p >= q: accepted at every u"
            if x in shared and (a, b) == (8, 4):
                assert acc == int(u_a < 0.5), "p / q = 1 / 2: the boundary pair 0.5 - 2^-24 and 0.5 is among the cases"
            assert tok in A and (acc == 1) == (tok == x)
        tokens += got[0]
    # the distribution test on the device's own outputs: the grid alone, every x of B weighted by q(x) = 1 / |B|
    counts = np.bincount(tokens[len(cases):], minlength=vocab)
    assert sorted(np.flatnonzero(counts).tolist()) == A and set(counts[A].tolist()) == {len(grid) // a}, counts[A].tolist()


# ---- 2. the one-hot form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vocab", [1, 7, C + 1, 2 * C + 5])
def test_the_one_hot_form(dev, vocab):
    A = [0] if vocab == 1 else [1, 3, 4, 6] if vocab == 7 else sp.exact_sets(vocab, 4, 4)[0]
    tb = sp.uniform_row(vocab, A)
    outside = [c for c in range(vocab) if c not in A][:1]
    # accept iff mulshift(Zp, U) < P_x: u < 1 / |A|; the residual is P with x removed
    edge = 1.0 / len(A)
    cases = [(x, ua, ur) for x in A + outside for ua, ur in ((edge - 2.0 ** -24, 0.0), (edge, 0.0), (0.0, 0.5), (0.6, 0.1), (0.6, 0.5), (TOP, TOP))]
    cases = cases[:ROWS * 2]
    nan_row, inf_row = np.full(vocab, 0x7FC0, dtype=np.uint16), sp.uniform_row(vocab, A[:1])
    inf_row[A[0]] = 0x7F80
    for chunk in in_chunks(cases):
        n = len(chunk)
        bits = np.tile(tb, (n, 1))
        cand, ua, ur = [c[0] for c in chunk], np.float32([c[1] for c in chunk]), np.float32([c[2] for c in chunk])
        want = oracle(bits, None, cand, ua, ur)
        got = call(dev, bits, None, cand, ua, ur)
        assert got == want, (vocab, [(c, g, w) for c, g, w in zip(chunk, zip(*got), zip(*want)) if g != w][:4])
        for (x, u_a, _), tok, acc in zip(chunk, *got):
            if x in A:
                assert acc == int(u_a < edge or len(A) == 1) and (tok == x) == (acc == 1) and tok in A
            else:
                assert acc == 0 and tok in A
        # a draft row in the greedy case -- NaN, +inf, or the temperature -- gives the same answers as None
        greedy_draft = np.stack([nan_row if r % 2 else inf_row for r in range(n)])
        assert call(dev, bits, greedy_draft, cand, ua, ur, dld=vocab + 1, doffset=3) == want


def test_a_target_that_is_one_hot_at_the_candidate_always_accepts(dev):
    vocab = C + 9
    cols = [0, 7, 8, C - 1, C, C + 8, vocab - 1, 4097]
    bits = np.stack([sp.uniform_row(vocab, [c]) for c in cols])
    n = len(cols)
    for ua in (0.0, 0.5, TOP, float("nan")):
        out, acc = call(dev, bits, None, cols, np.float32([ua] * n), np.float32([0.5] * n))
        assert out == cols and acc == [1] * n
    # ... and with a draft row that spreads its mass: q(x) < 1 = p(x)
    draft = np.stack([sp.uniform_row(vocab, cols) for _ in cols])
    assert call(dev, bits, draft, cols, np.float32([TOP] * n), np.float32([0.5] * n)) == (cols, [1] * n)


# ---- 3. bit equalities -------------------------------------------------------------------------------------------------------------------
def gaussian_rows(vocab, rows, seed):
    bits, par = so.gaussian_case(vocab, rows, seed)
    return bits, dict(T=par["T"], k=par["k"], p=par["p"], q=par["q"])


@pytest.mark.parametrize("vocab", [7, C + 1, 2 * C + 5])
def test_rows_without_a_candidate_equal_sample_rows(dev, vocab):
    bits, par = gaussian_rows(vocab, ROWS, vocab)
    x = from_bits(bits, dev, vocab + 3, 1)
    nan_draft = torch.full((ROWS, vocab), float("nan"), dtype=torch.bfloat16, device=dev)
    cand = i32([-1, vocab, -5, vocab + 100, -(1 << 31), (1 << 31) - 1, -1, vocab] * 2, dev)
    ur, ua = f32((np.arange(ROWS) * 0.6180339887 + 0.05) % 1.0, dev), f32(np.zeros(ROWS), dev)
    for kw in ({}, dict(temperature=f32(par["T"], dev)),
               dict(temperature=f32(par["T"], dev), top_k=i32(par["k"], dev), top_p=f32(par["p"], dev), min_p=f32(par["q"], dev))):
        want = mixedgemm.sample_rows(x, ur, **kw)
        for draft in (None, nan_draft, x):
            out, acc = mixedgemm.spec_sample_rows(x, draft, cand, ua, ur, workspace=poisoned_ws(ROWS, vocab, dev), **kw)
            assert torch.equal(out, want) and acc.tolist() == [-1] * ROWS, (vocab, sorted(kw))


@pytest.mark.parametrize("vocab", [97, 2 * C + 5])
def test_greedy_rows_equal_argmax_rows(dev, vocab):
    rng = np.random.default_rng(vocab)
    bits = so.bf16_bits(np.round(rng.standard_normal((12, vocab)) * 2.0))            # ties everywhere: the lowest index must win
    bits[3, vocab - 2] = 0x7FC0                              # NaN
    bits[4, vocab // 2] = 0x7F80                             # +inf
    bits[5, :] = 0xFF80                                      # only -inf
    bits[6, 1] = 0xFFC0                                      # -NaN
    bits[7, [2, vocab - 1]] = 0x7F80                         # +inf twice
    T = np.array([0.0, -1.0, float("nan"), 1.0, 1.0, 1.0, 1.0, 0.7, -0.0, 0.0, float("nan"), float("-inf")], dtype=np.float32)
    assert all(so.is_greedy(bits[r], T[r]) for r in range(12))
    x = from_bits(bits, dev, vocab + 1)
    best = mixedgemm.argmax_rows(x)
    want = best.tolist()
    assert want == [so.argmax(bits[r]) for r in range(12)]
    cand = [want[r] if r % 3 == 0 else -1 if r % 3 == 1 else (want[r] + 1) % vocab for r in range(12)]
    u = f32([0.99] * 12, dev)
    draft = from_bits(so.bf16_bits(rng.standard_normal((12, vocab))), dev, vocab + 2, 5)
    for d in (None, draft, x):
        for kw in ({}, dict(top_k=i32([5] * 12, dev), top_p=f32([0.5] * 12, dev), min_p=f32([0.1] * 12, dev))):
            out, acc = mixedgemm.spec_sample_rows(x, d, i32(cand, dev), u, u, temperature=f32(T, dev), workspace=poisoned_ws(12, vocab, dev), **kw)
            assert torch.equal(out, best) and acc.tolist() == [1, -1, 0] * 4


@pytest.mark.parametrize("vocab", [8, 2 * C + 5])
def test_a_draft_that_is_the_target_accepts_whatever_the_target_keeps(dev, vocab):
    bits, par = gaussian_rows(vocab, ROWS, vocab + 1)
    bits[:, vocab - 1] = 0xFF80                              # a token without mass in every row
    x = from_bits(bits, dev, vocab + 1, 3)
    kw = dict(temperature=f32(par["T"], dev), top_k=i32(par["k"], dev), top_p=f32(par["p"], dev), min_p=f32(par["q"], dev))
    u = f32((np.arange(ROWS) * 0.6180339887 + 0.05) % 1.0, dev)
    cand = mixedgemm.sample_rows(x, u, **kw)                 # drawn from the kept set: P_x > 0
    for ua in (0.0, 0.5, TOP, 7.0):
        out, acc = mixedgemm.spec_sample_rows(x, x, cand, f32([ua] * ROWS, dev), u, **kw)
        assert torch.equal(out, cand) and acc.tolist() == [1] * ROWS
    # the same bits in another tensor are the same distribution
    copy = from_bits(bits, dev, vocab + 2, 6)
    assert mixedgemm.spec_sample_rows(x, copy, cand, f32([TOP] * ROWS, dev), u, **kw)[1].tolist() == [1] * ROWS
    # a candidate neither side gives any mass: rejected, no residual (P is Q), so the target's argmax
    none = i32([vocab - 1] * ROWS, dev)
    out, acc = mixedgemm.spec_sample_rows(x, x, none, f32([0.0] * ROWS, dev), u, **kw)
    assert acc.tolist() == [0] * ROWS and torch.equal(out, mixedgemm.argmax_rows(x))


def test_out_and_accepted_views_are_written_in_place(dev):
    vocab = C + 1
    A, B = sp.exact_sets(vocab, 8, 4)
    n = 6
    bits, draft = np.tile(sp.uniform_row(vocab, A), (n, 1)), np.tile(sp.uniform_row(vocab, B), (n, 1))
    cand, ua, ur = B[:4] + [-1, B[0]], np.float32([0.2, 0.7, 0.2, 0.7, 0.5, 0.9]), np.float32([0.1, 0.3, 0.5, 0.7, 0.9, 0.95])
    want = oracle(bits, draft, cand, ua, ur)
    box = torch.full((2, 16), 77, dtype=torch.int32, device=dev)
    out_view, acc_view = box[0, 3:3 + n], box[1, 5:5 + n]
    ws = poisoned_ws(n, vocab, dev)
    out, acc = mixedgemm.spec_sample_rows(from_bits(bits, dev), from_bits(draft, dev), i32(cand, dev), f32(ua, dev), f32(ur, dev), out=out_view,
                                          accepted=acc_view, workspace=ws)
    assert out is out_view and acc is acc_view
    assert box[0].tolist() == [77] * 3 + want[0] + [77] * (13 - n) and box[1].tolist() == [77] * 5 + want[1] + [77] * (11 - n)
    assert mixedgemm.spec_sample_rows_workspace_bytes(n, vocab) == ws.numel()
    with pytest.raises(RuntimeError, match="workspace"):
        mixedgemm.spec_sample_rows(from_bits(bits, dev), None, i32(cand, dev), f32(ua, dev), f32(ur, dev), workspace=ws[:-8])
    with pytest.raises(RuntimeError, match=r"draft_logits must be bf16 \[6, 8193\]"):
        mixedgemm.spec_sample_rows(from_bits(bits, dev), from_bits(draft[:5], dev), i32(cand, dev), f32(ua, dev), f32(ur, dev))
    with pytest.raises(TypeError, match="cand_tok must be torch.int32"):
        mixedgemm.spec_sample_rows(from_bits(bits, dev), None, i32(cand, dev).long(), f32(ua, dev), f32(ur, dev))
    with pytest.raises(TypeError, match="u_accept must be"):
        mixedgemm.spec_sample_rows(from_bits(bits, dev), None, i32(cand, dev), 0.5, f32(ur, dev))
    none = mixedgemm.spec_sample_rows(from_bits(bits, dev)[:0], None, i32(cand, dev)[:0], f32(ua, dev)[:0], f32(ur, dev)[:0])
    assert none[0].numel() == 0 and none[1].numel() == 0


# ---- 4. layout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", range(8))
def test_every_alignment_of_the_two_matrices(dev, offset):
    vocab = 2 * C + 5
    A, B = sp.exact_sets(vocab, 8, 4)
    tb, db = sp.uniform_row(vocab, A), sp.uniform_row(vocab, B)
    chunk = [(x, ua, ur) for x in B for ua in (0.25, 0.75) for ur in (0.3, 0.8)]
    chunk = [(x, ua, (ur + 0.11 * i) % 1.0) for i, (x, ua, ur) in enumerate(chunk)]
    n = len(chunk)
    assert n == ROWS
    bits, draft = np.tile(tb, (n, 1)), np.tile(db, (n, 1))
    cand, ua, ur = [c[0] for c in chunk], np.float32([c[1] for c in chunk]), np.float32([c[2] for c in chunk])
    want = oracle(bits, draft, cand, ua, ur)
    assert len(set(want[0])) >= 5 and 0 in want[1] and 1 in want[1]
    # odd row distances: the rows of one call start at every 2-byte alignment, and differently in the two matrices
    for doffset, ld, dld in (((3 * offset + 1) % 8, vocab + 3, vocab + 4), (offset, vocab + 1, vocab), (7 - offset, vocab, vocab + 7)):
        assert call(dev, bits, draft, cand, ua, ur, ld=ld, dld=dld, offset=offset, doffset=doffset) == want, (offset, doffset, ld, dld)


def test_another_grid_of_rows_gives_the_same_bits_per_row(dev):
    bits, draft, cand, par = sp.gaussian_case(True)
    kw = dict(T=par["T"], k=par["k"], p=par["p"], q=par["q"])
    whole = call(dev, bits, draft, cand, par["ua"], par["ur"], **kw)
    for rows in (slice(3, 9), slice(15, 16), slice(0, 16, 5)):
        part = call(dev, bits[rows], draft[rows], cand[rows], par["ua"][rows], par["ur"][rows], **{n: v[rows] for n, v in kw.items()})
        assert part == (whole[0][rows], whole[1][rows]), rows
    # the same call over a workspace of zeros
    x, d = from_bits(bits, dev), from_bits(draft, dev)
    out, acc = mixedgemm.spec_sample_rows(x, d, i32(cand, dev), f32(par["ua"], dev), f32(par["ur"], dev), temperature=f32(par["T"], dev),
                                          top_k=i32(par["k"], dev), top_p=f32(par["p"], dev), min_p=f32(par["q"], dev),
                                          workspace=torch.zeros_like(poisoned_ws(*bits.shape, dev)))
    assert (out.tolist(), acc.tolist()) == whole


# ---- 5. Gaussian rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filters", [False, True], ids=["temperature", "all-filters"])
def test_gaussian_rows_give_admissible_decisions_and_tokens(dev, filters):
    """a row whose admissible set holds more than one outcome is checked for membership only; test_spec_sample_cpu.py asserts from the
    oracle that at most one row in sixteen is such, for the decision and for the token separately"""
    bits, draft, cand, par = sp.gaussian_case(filters)
    sets = sp.gaussian_admissible(filters)
    out, acc = call(dev, bits, draft, cand, par["ua"], par["ur"], T=par["T"], k=par["k"], p=par["p"], q=par["q"])
    print(f"filters {filters}: decisions {acc}, {sum(len(d) > 1 for d, _, _ in sets)} rows with two admissible decisions, "
          f"{sum(len(t) > 1 for _, t, _ in sets)} with more than one admissible token")
    bad = [(r, acc[r], out[r], sorted(d), sorted(t)[:4]) for r, (d, t, kept) in enumerate(sets)
           if acc[r] not in d or out[r] not in t or not kept[out[r]] or (acc[r] == 1) != (out[r] == int(cand[r]))]
    assert not bad, bad


# ---- 6. chains: candidates -> spec_sample_rows -> verify_greedy -----------------------------------------------------------------------------
VOCAB6 = C + 1


def chain_step(variant):
    """5 sequences over 16 rows of the exact family: three drafts of 4 nodes, an empty sequence and a prompt chunk of 4 rows.  Returns
    the numpy inputs and the oracle's walk.  variant 0: |A| = 8, |B| = 4 (a shared token survives u < 1 / 2); variant 1: other sets,
    other tokens, u and temperatures, and a root that does not match"""
    a, b = (8, 4) if variant == 0 else (4, 8)
    A, B = sp.exact_sets(VOCAB6, a, b)
    if variant:
        A, B = sorted((c + 2) % VOCAB6 for c in A), sorted((c + 2) % VOCAB6 for c in B)
    shared, only_b = sorted(set(A) & set(B)), sorted(set(B) - set(A))
    qo = [0, 4, 4, 8, 12, 16]
    s0, s1, o0 = shared[0], shared[1], only_b[0]
    # draft tokens per node; a node's token is the candidate of the row before it
    draft = [s0, s1, s0, s1,   s1, s0, s0, s1,   s0, s1, s1, s0,   s1, o0, s0, s1] if variant == 0 else \
            [s1, o0, s0, s1,   s0, s0, s1, s1,   s1, s0, o0, s1,   s0, s1, s0, s1]
    root = [s0, 5, s1, -1, s1] if variant == 0 else [s1, 9, s1, -1, s0]
    ua = np.float32([0.25, 0.30, 0.75, 0.1,   0.2, 0.4, 0.45, 0.9,   0.6, 0.7, 0.1, 0.3,   0.1, 0.2, 0.3, 0.4])
    ur = np.float32((np.arange(16) * 0.6180339887 + 0.11 + 0.3 * variant) % 1.0)
    T = np.float32(0.5 + 0.1 * np.arange(16) + variant)
    bits, dbits = np.tile(sp.uniform_row(VOCAB6, A), (16, 1)), np.tile(sp.uniform_row(VOCAB6, B), (16, 1))
    row = lambda t, x: sp.spec_row(bits[t], dbits[t], -1 if x is None else x, ua[t], ur[t], T[t])
    return dict(bits=bits, dbits=dbits, draft=draft, root=root, qo=qo, ua=ua, ur=ur, T=T, walk=sp.chain_walk(row, draft, root, qo))


def test_chain_step_inputs_cover_the_walk():
    """precondition, from the oracle: the two steps hold a rejection by u, a rejection by the token, a fully accepted chain whose
    bonus is the plain sample, the prompt chunk, the empty sequence and a root that does not match"""
    w0, w1 = chain_step(0)["walk"], chain_step(1)["walk"]
    assert [k for k, _ in w0] == [3, 0, 4, 4, 1] and w0[1][1] == 5
    assert [k for k, _ in w1] == [1, 0, 0, 4, 4] and w1[1][1] == 9 and w1[2][1] == chain_step(1)["root"][2]
    assert all(tok >= 0 for _, tok in w0 + w1)


def check_result(result, step):
    got = result.cpu().numpy()
    for b, (k, bonus) in enumerate(step["walk"]):
        prompt = step["root"][b] < 0
        assert (got[b, 0], got[b, 1]) == (k, bonus), (b, got[b, :6].tolist(), k, bonus)
        assert got[b, 2:2 + k].tolist() == ([-1] * k if prompt else list(range(k))) and (got[b, 2 + k:] == -1).all(), b


def test_candidates_spec_sample_and_verify_equal_the_oracles_walk_eagerly_and_replayed(dev):
    step = chain_step(0)
    T, B = 16, 5
    logits, dlogits = from_bits(step["bits"], dev, VOCAB6 + 3, 1), from_bits(step["dbits"], dev, VOCAB6 + 1, 2)
    draft, root, qo = i32(step["draft"], dev), i32(step["root"], dev), i32(step["qo"], dev)
    ua, ur, temp = f32(step["ua"], dev), f32(step["ur"], dev), f32(step["T"], dev)
    # one page of 16 rows per sequence, the new tokens at its end: base = last_page_len - n
    kv_indptr, last_page_len = i32(np.arange(B + 1), dev), i32([10, 3, 12, 4, 16], dev)
    cand, target, acc = (torch.full((T,), 77, dtype=torch.int32, device=dev) for _ in range(3))
    result = torch.empty((B, _lib.MM_VERIFY_STRIDE), dtype=torch.int32, device=dev)
    src, dst = torch.empty_like(cand), torch.empty_like(cand)
    ws = poisoned_ws(T, VOCAB6, dev)

    def run():
        mixedgemm.chain_candidates(draft, qo, out=cand)
        mixedgemm.spec_sample_rows(logits, dlogits, cand, ua, ur, temperature=temp, out=target, accepted=acc, workspace=ws)
        mixedgemm.verify_greedy(target, draft, root, qo, kv_indptr, last_page_len, 16, result=result, move_src=src, move_dst=dst)

    run()
    torch.cuda.synchronize()
    assert cand.tolist() == sp.chain_candidates(step["draft"], step["qo"])
    check_result(result, step)
    eager = [t.clone() for t in (cand, target, acc, result, src, dst)]

    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t in (cand, target, acc, result, src, dst):
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, (cand, target, acc, result, src, dst))), "the replay on the same inputs"

    # everything rewritten in place: the logits, the draft (so the candidates), the roots, the u's and the temperatures
    step = chain_step(1)
    logits.copy_(from_bits(step["bits"], dev)), dlogits.copy_(from_bits(step["dbits"], dev))
    draft.copy_(i32(step["draft"], dev)), root.copy_(i32(step["root"], dev))
    ua.copy_(f32(step["ua"], dev)), ur.copy_(f32(step["ur"], dev)), temp.copy_(f32(step["T"], dev))
    graph.replay()
    torch.cuda.synchronize()
    replayed = [t.clone() for t in (cand, target, acc, result, src, dst)]
    check_result(result, step)
    run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(replayed, (cand, target, acc, result, src, dst))), "the replay and the eager call"
    assert cand.tolist() == sp.chain_candidates(step["draft"], step["qo"])
